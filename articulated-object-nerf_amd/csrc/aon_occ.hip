// Occupancy-grid accelerated inference (aon_occupancy_build, aon_render_fwd_occ / aon_art_render_fwd_occ): a bitfield of the cells of a
// density grid that may hold matter, and per render level the list of samples that fall into occupied cells.  The MLP then runs only on
// that list (the GATHER instances of mlp_fwd_kernel / art_mlp_fwd_kernel); every other sample gets the sentinel record below.  No atomics:
// the same bits on every run.  An optional ray mask: the samples of a ray whose `ray_live` byte is 0 are EMPTY
// whatever the grid says; the grid itself may be null (every cell occupied: the mask alone decides).
//
// Convention (tests/_occ_ref.py is an independent numpy copy):
//   * the grid is built from a density grid of (nx, ny, nz) points x_a = lo_a + idx_a step_a (ops.grid_points); it has (nx-1, ny-1, nz-1)
//     cells, cell (i, j, k) named by its lowest corner, bit c = (i (ny-1) + j) (nz-1) + k of a C-order bitfield, 32 cells per uint32 word
//     (bit c is bit c & 31 of word c >> 5);
//   * a cell is occupied iff one of its 8 corner densities is above `threshold` or NaN, then dilated by `dilate` cells (Chebyshev max
//     filter).  Both steps in one: the dilated bit of cell c is set iff a grid point of the corner box of the cells within `dilate` of c
//     is above the threshold or NaN;
//   * sample x (o + t d, multiply then add: the MLP kernel's own bits) lies in cell floor((x_a - lo_a) / step_a) per axis (fp32 subtraction,
//     IEEE division, floor), clamped to cells_a - 1 (x_a == hi_a); hi_a = lo_a + cells_a step_a, multiply then add (the last grid point).
//     A coordinate outside [lo_a, hi_a], or NaN, is EMPTY;
//   * an empty sample's raw record is (0, 0, 0, -inf): relu(-inf) = 0 and softplus(-inf + sigma_bias) = 0 exactly (softplus_f32 takes
//     exp2(-inf) = 0), so its density is exactly zero under both activations and its weight is exactly zero.
//
// Per level and render chunk, three launches over tiles of kOccTile = 1024 consecutive samples (256 threads x 4), as aon_mesh.hip:
//   (a) mark: look every sample up, write the sentinel record of the empty ones, count the occupied ones of the tile;
//   (b) scan: ONE workgroup turns the tile counts into exclusive offsets and the total, which it writes to the device counter the gather
//       MLP launch reads its pass count from (no host synchronisation) and adds to the caller's per-level tally;
//   (c) emit: the lookup again, and the ascending list of occupied sample indices at the scanned offsets.
#include "aon_launch.h"
#include "aon_occ_lookup.h"

namespace aon {

constexpr int kOccTile = 1024;
constexpr int kOccThreads = 256;

// ---- build: density grid -> dilated bitfield, one launch, one thread per cell, a wave's 64 bits packed with one ballot ----
__global__ __launch_bounds__(kOccThreads) void occ_build_kernel(const float* __restrict__ dens, int64_t nx, int64_t ny, int64_t nz, float thr, int r,
                                                                uint32_t* __restrict__ bits, int64_t ncells, int64_t nwords) {
  const int64_t cx = nx - 1, cy = ny - 1, cz = nz - 1;
  const int64_t c = (int64_t)blockIdx.x * kOccThreads + threadIdx.x;
  bool occ = false;
  if (c < ncells) {
    const int64_t i = c / (cy * cz), rem = c - i * (cy * cz), j = rem / cz, k = rem - j * cz;
    // grid points of the corner box of the cells within r of (i, j, k), clamped to the grid
    const int64_t i0 = i - r > 0 ? i - r : 0, i1 = (i + r < cx - 1 ? i + r : cx - 1) + 1;
    const int64_t j0 = j - r > 0 ? j - r : 0, j1 = (j + r < cy - 1 ? j + r : cy - 1) + 1;
    const int64_t k0 = k - r > 0 ? k - r : 0, k1 = (k + r < cz - 1 ? k + r : cz - 1) + 1;
    for (int64_t pi = i0; pi <= i1 && !occ; ++pi)
      for (int64_t pj = j0; pj <= j1 && !occ; ++pj) {
        const float* row = dens + (pi * ny + pj) * nz;
        for (int64_t pk = k0; pk <= k1; ++pk)
          if (!(row[pk] <= thr)) { occ = true; break; }   // above the threshold, or NaN
      }
  }
  const uint64_t b = __ballot(occ);
  const int lane = threadIdx.x & 63;
  const int64_t word = (c - lane) / 32 + (lane >> 5);   // the wave's first cell is a multiple of 64
  if ((lane & 31) == 0 && word < nwords) bits[word] = (uint32_t)(lane ? b >> 32 : b);
}

hipError_t launch_occ_build(const float* dens, const int64_t* dims, float thr, int dilate, uint32_t* bits, hipStream_t stream) {
  const int64_t ncells = (dims[0] - 1) * (dims[1] - 1) * (dims[2] - 1);
  const int64_t nwords = (ncells + 31) / 32;
  const int64_t blocks = (ncells + kOccThreads - 1) / kOccThreads;
  occ_build_kernel<<<dim3((unsigned)blocks), dim3(kOccThreads), 0, stream>>>(dens, dims[0], dims[1], dims[2], thr, dilate, bits, ncells, nwords);
  return hipGetLastError();
}

// ---- per-level sample marking and compaction (the lookup itself: occ_lookup, aon_occ_lookup.h) ----
struct OccSamples {
  const float* rays_o; const float* rays_d; const float* t_vals;   // (n,3), (n,3), (n,S)
  int64_t total; int S;                                             // n * S <= INT32_MAX (the caller's chunking)
  const uint8_t* ray_live;                                          // (n,) or null: a dead ray's samples are EMPTY
};

__device__ __forceinline__ int occ_tile_flags(const OccGrid& G, const OccSamples& s, int64_t g0, bool (&occ)[4]) {
  int n = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t g = g0 + r;
    occ[r] = false;
    if (g >= s.total) continue;
    const int64_t ray = g / s.S;
    if (s.ray_live && !s.ray_live[ray]) continue;   // dead ray
    if (G.bits) {
      const float t = s.t_vals[g];
      float x[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) x[a] = __fadd_rn(s.rays_o[ray * 3 + a], __fmul_rn(t, s.rays_d[ray * 3 + a]));   // helper.cast_rays
      occ[r] = occ_lookup(G, x);
    } else {
      occ[r] = true;   // a null grid: every cell occupied
    }
    n += occ[r] ? 1 : 0;
  }
  return n;
}

// (a) the sentinel record of every empty sample; the tile's occupied count
__global__ __launch_bounds__(kOccThreads) void occ_mark_kernel(OccGrid G, OccSamples s, f32x4* __restrict__ raw, int* __restrict__ tile_counts) {
  __shared__ int red[kOccThreads / 64];
  const int64_t g0 = (int64_t)blockIdx.x * kOccTile + 4 * threadIdx.x;
  bool occ[4];
  const int n = occ_tile_flags(G, s, g0, occ);
  f32x4 sentinel;
  sentinel[0] = 0.f; sentinel[1] = 0.f; sentinel[2] = 0.f; sentinel[3] = -__builtin_huge_valf();
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (g0 + r < s.total && !occ[r]) raw[g0 + r] = sentinel;
  int tot;
  block_excl_scan<int>(n, tot, red);
  if (threadIdx.x == 0) tile_counts[blockIdx.x] = tot;
}

// (b) one workgroup: exclusive offsets of the tile counts in tile order; *count = total; tally[0] += total when tally is given
__global__ __launch_bounds__(kOccThreads) void occ_scan_kernel(const int* __restrict__ tile_counts, int64_t ntiles, int* __restrict__ offs,
                                                               int64_t* __restrict__ count, int64_t* __restrict__ tally) {
  __shared__ int64_t red[kOccThreads / 64];
  constexpr int kPer = 8;
  int64_t carry = 0;
  for (int64_t base = 0; base < ntiles; base += (int64_t)kOccThreads * kPer) {
    const int64_t t0 = base + (int64_t)threadIdx.x * kPer;
    int cv[kPer];
    int64_t sv = 0;
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
      cv[r] = t0 + r < ntiles ? tile_counts[t0 + r] : 0;
      sv += cv[r];
    }
    int64_t tv;
    int64_t run = carry + block_excl_scan<int64_t>(sv, tv, red);
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
      if (t0 + r < ntiles) offs[t0 + r] = (int)run;
      run += cv[r];
    }
    carry += tv;
  }
  if (threadIdx.x == 0) {
    *count = carry;
    if (tally) *tally += carry;
  }
}

// (c) the occupied sample indices of a tile at its scanned offset, ascending
__global__ __launch_bounds__(kOccThreads) void occ_emit_kernel(OccGrid G, OccSamples s, const int* __restrict__ offs, int* __restrict__ idx) {
  __shared__ int red[kOccThreads / 64];
  const int64_t g0 = (int64_t)blockIdx.x * kOccTile + 4 * threadIdx.x;
  bool occ[4];
  const int n = occ_tile_flags(G, s, g0, occ);
  int tot;
  int run = offs[blockIdx.x] + block_excl_scan<int>(n, tot, red);
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (occ[r]) idx[run++] = (int)(g0 + r);
}

int64_t occ_list_bytes(int64_t total) {   // per chunk and level: sample list, tile counts, tile offsets, the device counter
  const int64_t tiles = (total + kOccTile - 1) / kOccTile;
  return ((total * 4 + 255) / 256 + (tiles * 4 + 255) / 256 * 2 + 1) * 256;
}

// raw: (total, 4) records; ws: occ_list_bytes(total) bytes, 256-byte aligned -> idx (total int32) and the counter (int64) for the gather launch
hipError_t launch_occ_compact(const OccGrid& G, const float* rays_o, const float* rays_d, const float* t_vals, int64_t n, int S, float* raw,
                              char* ws, int64_t* tally, const int** idx_out, const int64_t** count_out, hipStream_t stream,
                              const uint8_t* ray_live) {
  const OccSamples s{rays_o, rays_d, t_vals, n * S, S, ray_live};
  const int64_t tiles = (s.total + kOccTile - 1) / kOccTile;
  int* idx = reinterpret_cast<int*>(ws);
  int* counts = reinterpret_cast<int*>(ws + (s.total * 4 + 255) / 256 * 256);
  int* offs = counts + (tiles * 4 + 255) / 256 * 64;
  int64_t* count = reinterpret_cast<int64_t*>(offs + (tiles * 4 + 255) / 256 * 64);
  *idx_out = idx; *count_out = count;
  if (tiles == 0) return hipMemsetAsync(count, 0, 8, stream);
  occ_mark_kernel<<<dim3((unsigned)tiles), dim3(kOccThreads), 0, stream>>>(G, s, reinterpret_cast<f32x4*>(raw), counts);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  occ_scan_kernel<<<dim3(1), dim3(kOccThreads), 0, stream>>>(counts, tiles, offs, count, tally);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  occ_emit_kernel<<<dim3((unsigned)tiles), dim3(kOccThreads), 0, stream>>>(G, s, offs, idx);
  return hipGetLastError();
}

// ---- early ray termination (tests/_stop_ref.py is an independent numpy copy) ----
// A level is evaluated front to back in rounds of R consecutive sample indices; round k covers [kR, min(S, (k+1)R)) of every ray.  Per ray:
// tau (fp32, 0 at the start of the level) and stop (int32, S at the start).  After round k's MLP launch a ray with stop == S adds
// sigma_i * delta_i of the round's samples to tau in ascending i -- one sequential fp32 chain, every multiply and add rounded -- with
// sigma_i / delta_i as composite_kernel (aon_render.hip) forms them, and stops (stop = (k+1)R) when tau >= tau_stop = fp32(-ln eps).
// In a later round a sample i >= stop[ray] is DEAD: the sentinel record, not listed.  The last round decides nothing (no depth launch).
struct OccRound {
  const int* stop;   // (n,)
  int s0, s1;        // the round's sample indices [s0, s1) of every ray
  int64_t count;     // n * (s1 - s0)
};

// tile slot q -> ray q / (s1 - s0), sample s0 + q % (s1 - s0); a null grid: every cell occupied
__device__ __forceinline__ int occ_round_flags(const OccGrid& G, const OccSamples& s, const OccRound& rd, int64_t q0, bool (&occ)[4], int64_t (&gi)[4]) {
  const int w = rd.s1 - rd.s0;
  int n = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t q = q0 + r;
    occ[r] = false;
    gi[r] = -1;
    if (q >= rd.count) continue;
    const int64_t ray = q / w;
    const int i = rd.s0 + (int)(q - ray * w);
    const int64_t g = ray * s.S + i;
    gi[r] = g;
    if (rd.stop[ray] <= i) continue;   // dead: behind the ray's stop
    if (s.ray_live && !s.ray_live[ray]) continue;   // dead ray
    if (G.bits) {
      const float t = s.t_vals[g];
      float x[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) x[a] = __fadd_rn(s.rays_o[ray * 3 + a], __fmul_rn(t, s.rays_d[ray * 3 + a]));
      occ[r] = occ_lookup(G, x);
    } else {
      occ[r] = true;
    }
    n += occ[r] ? 1 : 0;
  }
  return n;
}

__global__ __launch_bounds__(kOccThreads) void occ_mark_round_kernel(OccGrid G, OccSamples s, OccRound rd, f32x4* __restrict__ raw,
                                                                     int* __restrict__ tile_counts) {
  __shared__ int red[kOccThreads / 64];
  const int64_t q0 = (int64_t)blockIdx.x * kOccTile + 4 * threadIdx.x;
  bool occ[4];
  int64_t gi[4];
  const int n = occ_round_flags(G, s, rd, q0, occ, gi);
  f32x4 sentinel;
  sentinel[0] = 0.f; sentinel[1] = 0.f; sentinel[2] = 0.f; sentinel[3] = -__builtin_huge_valf();
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (gi[r] >= 0 && !occ[r]) raw[gi[r]] = sentinel;
  int tot;
  block_excl_scan<int>(n, tot, red);
  if (threadIdx.x == 0) tile_counts[blockIdx.x] = tot;
}

__global__ __launch_bounds__(kOccThreads) void occ_emit_round_kernel(OccGrid G, OccSamples s, OccRound rd, const int* __restrict__ offs,
                                                                     int* __restrict__ idx) {
  __shared__ int red[kOccThreads / 64];
  const int64_t q0 = (int64_t)blockIdx.x * kOccTile + 4 * threadIdx.x;
  bool occ[4];
  int64_t gi[4];
  const int n = occ_round_flags(G, s, rd, q0, occ, gi);
  int tot;
  int run = offs[blockIdx.x] + block_excl_scan<int>(n, tot, red);
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (occ[r]) idx[run++] = (int)gi[r];   // ascending: q ascends with (ray, i)
}

// tau[ray] = 0, stop[ray] = S
__global__ __launch_bounds__(kOccThreads) void occ_stop_init_kernel(float* __restrict__ tau, int* __restrict__ stop, int64_t n, int S) {
  const int64_t ray = (int64_t)blockIdx.x * kOccThreads + threadIdx.x;
  if (ray < n) { tau[ray] = 0.f; stop[ray] = S; }
}

// dst[ray * stride] = src ? src[ray] : value (the caller's (n_rays, 2) stop map, one level's column)
__global__ __launch_bounds__(kOccThreads) void occ_stop_store_kernel(const int* __restrict__ src, int value, int* __restrict__ dst, int64_t n, int stride) {
  const int64_t ray = (int64_t)blockIdx.x * kOccThreads + threadIdx.x;
  if (ray < n) dst[ray * stride] = src ? src[ray] : value;
}

// The optical depth of a round: one wavefront per live ray.  The lanes fetch the round's records (one contiguous 16 B x (s1 - s0) run per
// ray) and t values and form sigma_i * delta_i in parallel; the sum is then taken in ascending i by one lane-by-lane chain, the bits of a
// sequential loop.  A stopped ray's wave leaves at once, so the cost follows the live rays.
__global__ __launch_bounds__(kOccThreads) void occ_depth_kernel(const f32x4* __restrict__ raw, const float* __restrict__ t_vals,
                                                                const float* __restrict__ dirs, int64_t n, int S, int s0, int s1, ActParams ap,
                                                                float tau_stop, float* __restrict__ tau, int* __restrict__ stop) {
  const int lane = threadIdx.x & 63;
  const int64_t ray = (int64_t)blockIdx.x * (kOccThreads / 64) + (threadIdx.x >> 6);
  if (ray >= n) return;              // wave-uniform
  if (stop[ray] != S) return;        // stopped in an earlier round
  const float dn = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(dirs[ray * 3], dirs[ray * 3]), __fmul_rn(dirs[ray * 3 + 1], dirs[ray * 3 + 1])),
                                        __fmul_rn(dirs[ray * 3 + 2], dirs[ray * 3 + 2])));
  const float* tv = t_vals + ray * S;
  float acc = tau[ray];
  for (int base = s0; base < s1; base += 64) {
    const int i = base + lane;
    float p = 0.f;
    if (i < s1) {
      float sg = raw[ray * S + i][3];
      if (ap.act == 1) sg = __builtin_fmaxf(sg, 0.f);
      else if (ap.act == 2) sg = softplus_f32(__fadd_rn(sg, ap.sigma_bias));
      const float dist = i < S - 1 ? __fmul_rn(__fsub_rn(tv[i + 1], tv[i]), dn) : __fmul_rn(1e10f, dn);
      p = __fmul_rn(sg, dist);
    }
    const int cnt = s1 - base < 64 ? s1 - base : 64;
    for (int j = 0; j < cnt; ++j) acc = __fadd_rn(acc, __shfl(p, j));
  }
  if (lane == 0) {
    tau[ray] = acc;
    if (acc >= tau_stop) stop[ray] = s1;   // NaN compares false: never stops
  }
}

// the per-level tally of a render that lists every sample (eps == 0 without a grid)
__global__ void occ_tally_set_kernel(int64_t* __restrict__ tally, int64_t v0, int64_t v1) {
  if (threadIdx.x == 0 && blockIdx.x == 0) { tally[0] = v0; tally[1] = v1; }
}
hipError_t launch_occ_tally_set(int64_t* tally, int64_t v0, int64_t v1, hipStream_t stream) {
  occ_tally_set_kernel<<<dim3(1), dim3(64), 0, stream>>>(tally, v0, v1);
  return hipGetLastError();
}

int64_t occ_stop_state_bytes(int64_t n) { return (n * 4 + 255) / 256 * 256 * 2; }   // tau, stop

hipError_t launch_occ_stop_init(char* state, int64_t n, int S, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  float* tau = reinterpret_cast<float*>(state);
  int* stop = reinterpret_cast<int*>(state + (n * 4 + 255) / 256 * 256);
  occ_stop_init_kernel<<<dim3((unsigned)((n + kOccThreads - 1) / kOccThreads)), dim3(kOccThreads), 0, stream>>>(tau, stop, n, S);
  return hipGetLastError();
}

// state == nullptr: fill with `value`
hipError_t launch_occ_stop_store(const char* state, int value, int* dst, int64_t n, int stride, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const int* stop = state ? reinterpret_cast<const int*>(state + (n * 4 + 255) / 256 * 256) : nullptr;
  occ_stop_store_kernel<<<dim3((unsigned)((n + kOccThreads - 1) / kOccThreads)), dim3(kOccThreads), 0, stream>>>(stop, value, dst, n, stride);
  return hipGetLastError();
}

// launch_occ_compact over the sub-range [s0, s1) of every ray, minus the dead samples.  G.bits == nullptr: no grid.
hipError_t launch_occ_compact_round(const OccGrid& G, const float* rays_o, const float* rays_d, const float* t_vals, int64_t n, int S, int s0, int s1,
                                    const char* state, float* raw, char* ws, int64_t* tally, const int** idx_out, const int64_t** count_out,
                                    hipStream_t stream, const uint8_t* ray_live) {
  const OccSamples s{rays_o, rays_d, t_vals, n * S, S, ray_live};
  const OccRound rd{reinterpret_cast<const int*>(state + (n * 4 + 255) / 256 * 256), s0, s1, n * (s1 - s0)};
  const int64_t tiles = (rd.count + kOccTile - 1) / kOccTile;
  const int64_t full_tiles = (s.total + kOccTile - 1) / kOccTile;   // the buffers keep launch_occ_compact's layout
  int* idx = reinterpret_cast<int*>(ws);
  int* counts = reinterpret_cast<int*>(ws + (s.total * 4 + 255) / 256 * 256);
  int* offs = counts + (full_tiles * 4 + 255) / 256 * 64;
  int64_t* count = reinterpret_cast<int64_t*>(offs + (full_tiles * 4 + 255) / 256 * 64);
  *idx_out = idx; *count_out = count;
  if (tiles == 0) return hipMemsetAsync(count, 0, 8, stream);
  occ_mark_round_kernel<<<dim3((unsigned)tiles), dim3(kOccThreads), 0, stream>>>(G, s, rd, reinterpret_cast<f32x4*>(raw), counts);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  occ_scan_kernel<<<dim3(1), dim3(kOccThreads), 0, stream>>>(counts, tiles, offs, count, tally);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  occ_emit_round_kernel<<<dim3((unsigned)tiles), dim3(kOccThreads), 0, stream>>>(G, s, rd, offs, idx);
  return hipGetLastError();
}

hipError_t launch_occ_depth(const float* raw, const float* t_vals, const float* dirs, int64_t n, int S, int s0, int s1, const ActParams& ap,
                            float tau_stop, char* state, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  float* tau = reinterpret_cast<float*>(state);
  int* stop = reinterpret_cast<int*>(state + (n * 4 + 255) / 256 * 256);
  constexpr int kRays = kOccThreads / 64;
  occ_depth_kernel<<<dim3((unsigned)((n + kRays - 1) / kRays)), dim3(kOccThreads), 0, stream>>>(reinterpret_cast<const f32x4*>(raw), t_vals, dirs, n, S,
                                                                                               s0, s1, ap, tau_stop, tau, stop);
  return hipGetLastError();
}

}  // namespace aon
