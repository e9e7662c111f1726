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
// Per level and render chunk (or round, section 4.10; or scene level, section 4.17), three launches over tiles of kOccTile = 1024 samples:
//   (a) mark: look every sample up, write the sentinel record of the empty ones, count the occupied ones of the tile;
//   (b) scan: ONE workgroup turns the tile counts into exclusive offsets and the total, which it writes to the device counter the gather
//       MLP launch reads its pass count from (no host synchronisation) and adds to the caller's tally;
//   (c) emit: the lookup again, and the ascending list of occupied sample indices at the scanned offsets.
#include "aon_launch.h"
#include "../../include/aon_hip_scene.h"
#include "aon_occ_lookup.h"
#include "aon_ray_core.h"

namespace aon {

constexpr int kOccTile = 1024;
constexpr int kOccThreads = 256;
constexpr int kOccPer = kOccTile / kOccThreads;
constexpr int kOccWaves = kOccThreads / 64;

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

// ---- sample marking and compaction (the lookup itself: occ_lookup, aon_occ_lookup.h) ----
// ONE mark / scan / emit for K segments of rows, each against its own grid, over the sample window [s0, s1) of every row: a render level is
// one segment and the window [0, S) (section 4.9), a round of early termination a narrower window and the rays' stop map (section 4.10), a
// scene level its K objects' pair rows (section 4.17).  A tile is kOccTile consecutive window slots of ONE segment and finds its segment
// from the K + 1 first-tile numbers.  The record travels by value in the kernel arguments (no device copy to keep alive, nothing for the
// host to wait for): KMAX = 1 keeps it at 152 bytes for the single-object renders, KMAX = AON_SCENE_MAX_OBJECTS takes 1.4 KB.
// A segment without a grid to which neither a ray mask nor a stop map applies is DENSE: there is nothing to decide, so it has no tiles, its
// rows of `raw` and of the list are not touched, and its count is all of its samples (the caller runs the ordinary MLP launch on it).
template <int KMAX>
struct OccArgs {
  OccGrid g[KMAX];          // bits == nullptr: every cell occupied
  int64_t row0[KMAX + 1];   // segment starts in rows; row0[K] = the number of rows
  int tile0[KMAX + 1];      // first tile of each segment, ascending; tile0[K] = the number of tiles
  int K, S, s0, s1;         // rows * S <= INT32_MAX (the entry points' checks): slots, records and list entries fit 32 bits
  const float* o; const float* d; const float* t_vals;   // (rows,3), (rows,3), (rows,S)
  const uint8_t* ray_live;  // (rows,) or null: a dead ray's samples are EMPTY
  const int* stop;          // (rows,) or null: sample i >= stop[row] is DEAD (section 4.10)
};

template <int KMAX>
__host__ __device__ __forceinline__ bool occ_dense(const OccArgs<KMAX>& a, int k) { return !a.g[k].bits && !a.ray_live && !a.stop; }

// Slot q of segment k's window -> row q / (s1 - s0), sample i = s0 + q % (s1 - s0).  rec: the sample's index in `raw` and `t_vals` (-1: the
// slot lies past the segment's end); local: its listed, SEGMENT-LOCAL index row_local * S + i.  Returns whether the sample is occupied.
template <int KMAX>
__device__ __forceinline__ bool occ_flag(const OccArgs<KMAX>& a, int k, uint32_t q, int64_t& rec, int& local) {
  const uint32_t w = a.s1 - a.s0;
  rec = -1;
  if (q >= (uint32_t)(a.row0[k + 1] - a.row0[k]) * w) return false;
  const uint32_t row_local = q / w;
  const int i = a.s0 + (int)(q - row_local * w);
  const int64_t row = a.row0[k] + row_local;
  local = (int)row_local * a.S + i;
  rec = a.row0[k] * a.S + local;
  if (a.stop && a.stop[row] <= i) return false;       // dead: behind the ray's stop
  if (a.ray_live && !a.ray_live[row]) return false;   // dead ray
  if (!a.g[k].bits) return true;
  const float t = a.t_vals[rec];
  float x[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) x[c] = __fadd_rn(a.o[row * 3 + c], __fmul_rn(t, a.d[row * 3 + c]));   // helper.cast_rays
  return occ_lookup(a.g[k], x);
}

// A workgroup's tile: thread t takes slots t, t + 256, t + 512, t + 768 (coalesced t_vals reads), so slot r * 256 + 64 * wave + lane
// ascends with (r, wave, lane).  Counts by wave ballots: cnt[r][wave] = the occupied slots of quarter r in that wave, after a barrier.
struct OccTile {
  int k;                     // the tile's segment: the last k with tile0[k] <= tile (segments without tiles lose to their successor)
  int64_t rec[kOccPer];
  int local[kOccPer];
  uint64_t bal[kOccPer];     // the wave's ballot of quarter r
  bool occ[kOccPer];
};

template <int KMAX>
__device__ __forceinline__ void occ_tile_flags(const OccArgs<KMAX>& a, OccTile& s, int (&cnt)[kOccPer][kOccWaves]) {
  s.k = 0;
  for (int j = 1; j < a.K; ++j)   // (uniform)
    if ((int)blockIdx.x >= a.tile0[j]) s.k = j;
  const uint32_t q0 = (uint32_t)((int)blockIdx.x - a.tile0[s.k]) * kOccTile + threadIdx.x;
#pragma unroll
  for (int r = 0; r < kOccPer; ++r) {
    s.occ[r] = occ_flag(a, s.k, q0 + r * kOccThreads, s.rec[r], s.local[r]);
    s.bal[r] = __builtin_amdgcn_ballot_w64(s.occ[r]);
    if ((threadIdx.x & 63) == 0) cnt[r][threadIdx.x >> 6] = __builtin_popcountll(s.bal[r]);
  }
  __syncthreads();
}

// (a) the sentinel record of every empty sample; the tile's occupied count
template <int KMAX>
__global__ __launch_bounds__(kOccThreads) void occ_mark_kernel(OccArgs<KMAX> a, f32x4* __restrict__ raw, int* __restrict__ tile_counts) {
  __shared__ int cnt[kOccPer][kOccWaves];
  OccTile s;
  occ_tile_flags(a, s, cnt);
  f32x4 sentinel;
  sentinel[0] = 0.f; sentinel[1] = 0.f; sentinel[2] = 0.f; sentinel[3] = -__builtin_huge_valf();
#pragma unroll
  for (int r = 0; r < kOccPer; ++r)
    if (raw && s.rec[r] >= 0 && !s.occ[r]) raw[s.rec[r]] = sentinel;   // (raw null: the records are the caller's, the deferred view branch)
  if (threadIdx.x == 0) {
    int tot = 0;
#pragma unroll
    for (int r = 0; r < kOccPer; ++r)
#pragma unroll
      for (int w = 0; w < kOccWaves; ++w) tot += cnt[r][w];
    tile_counts[blockIdx.x] = tot;
  }
}

// (b) one workgroup, per segment: offs[tile] = the occupied samples of the segment's earlier tiles; counts[k] = the segment's total (dense:
// all of its samples); tally[k] += counts[k] when tally is given.  Integers: exact, the order of the sums does not matter.
template <int KMAX>
__global__ __launch_bounds__(kOccThreads) void occ_scan_kernel(OccArgs<KMAX> a, const int* __restrict__ tile_counts, int* __restrict__ offs,
                                                               int64_t* __restrict__ counts, int64_t* __restrict__ tally) {
  __shared__ int64_t red[kOccWaves];
  for (int k = 0; k < a.K; ++k) {   // (uniform)
    const int64_t total = (occ_dense(a, k) ? (a.row0[k + 1] - a.row0[k]) * (a.s1 - a.s0) : 0) +
                          block_scan_counts(tile_counts + a.tile0[k], a.tile0[k + 1] - a.tile0[k], offs + a.tile0[k], red);
    if (threadIdx.x == 0) {
      counts[k] = total;
      if (tally) tally[k] += total;
    }
  }
}

// (c) the occupied samples of a tile at its scanned offset in the segment's list (idx + row0[k] * S), ascending: the rank of a slot is the
// tile's offset + the earlier quarters + the earlier waves of its quarter + the earlier lanes of its ballot
template <int KMAX>
__global__ __launch_bounds__(kOccThreads) void occ_emit_kernel(OccArgs<KMAX> a, const int* __restrict__ offs, int* __restrict__ idx) {
  __shared__ int cnt[kOccPer][kOccWaves];
  OccTile s;
  occ_tile_flags(a, s, cnt);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  int* list = idx + a.row0[s.k] * a.S;
  int run = offs[blockIdx.x];
#pragma unroll
  for (int r = 0; r < kOccPer; ++r) {
    int before = run;
#pragma unroll
    for (int w = 0; w < kOccWaves; ++w) {
      if (w < wave) before += cnt[r][w];
      run += cnt[r][w];
    }
    if (s.occ[r]) list[before + __builtin_popcountll(s.bal[r] & below)] = s.local[r];
  }
}

// The workspace of a compaction, 256-byte aligned parts: the lists (`total` int32), tile counts and tile offsets (`tile_cap` int32 each)
// and the K counters (int64).  ws == nullptr: the size alone.
struct OccLists {
  int* idx; int* tile_counts; int* offs; int64_t* counts;
  int64_t bytes;
};
static OccLists occ_carve(char* ws, int64_t total, int64_t tile_cap, int K) {
  auto up = [](int64_t b) { return (b + 255) / 256 * 256; };
  const int64_t o1 = up(total * 4), o2 = o1 + up(tile_cap * 4), o3 = o2 + up(tile_cap * 4);
  return {reinterpret_cast<int*>(ws), reinterpret_cast<int*>(ws + o1), reinterpret_cast<int*>(ws + o2), reinterpret_cast<int64_t*>(ws + o3),
          o3 + up((int64_t)K * 8)};
}
static int64_t occ_tiles(int64_t samples) { return (samples + kOccTile - 1) / kOccTile; }
int64_t occ_list_bytes(int64_t total) { return occ_carve(nullptr, total, occ_tiles(total), 1).bytes; }   // per chunk and level
int64_t scene_occ_tile_cap(int64_t pairs, int K, int S) { return pairs * S / kOccTile + K; }              // >= sum_k ceil(P_k S / 1024)
int64_t scene_occ_list_bytes(int64_t pairs, int K, int S) {
  return occ_carve(nullptr, (pairs > 0 ? pairs : 1) * S, scene_occ_tile_cap(pairs, K, S), K).bytes;
}

template <int KMAX>
static hipError_t occ_compact(const OccCompact& c, float* raw, const OccLists& L, int64_t* tally, hipStream_t stream) {
  OccArgs<KMAX> a{};
  a.K = c.K; a.S = c.S; a.s0 = c.s0; a.s1 = c.s1;
  a.o = c.rays_o; a.d = c.rays_d; a.t_vals = c.t_vals; a.ray_live = c.ray_live; a.stop = c.stop;
  for (int k = 0; k < c.K; ++k) a.g[k] = c.grids[k];
  int64_t tiles = 0;
  for (int k = 0; k <= c.K; ++k) {
    a.row0[k] = c.starts[k];
    a.tile0[k] = (int)tiles;
    if (k < c.K && !occ_dense(a, k)) tiles += occ_tiles((c.starts[k + 1] - c.starts[k]) * (c.s1 - c.s0));
  }
  const dim3 grid((unsigned)tiles), block(kOccThreads);
  if (tiles > 0) {
    occ_mark_kernel<KMAX><<<grid, block, 0, stream>>>(a, reinterpret_cast<f32x4*>(raw), L.tile_counts);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  if (tiles > 0 || tally) {   // (every segment dense or empty: the dense launches read no counter, the tally is all the scan writes)
    occ_scan_kernel<KMAX><<<dim3(1), block, 0, stream>>>(a, L.tile_counts, L.offs, L.counts, tally);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  if (tiles > 0) occ_emit_kernel<KMAX><<<grid, block, 0, stream>>>(a, L.offs, L.idx);
  return hipGetLastError();
}

hipError_t launch_occ_compact(const OccCompact& c, float* raw, char* ws, int64_t tile_cap, int64_t* tally, const int** idx_out,
                              const int64_t** counts_out, hipStream_t stream) {
  const OccLists L = occ_carve(ws, c.starts[c.K] * c.S, tile_cap, c.K);
  *idx_out = L.idx; *counts_out = L.counts;
  if (c.starts[c.K] == 0) return hipMemsetAsync(L.counts, 0, (size_t)c.K * 8, stream);   // no rows: empty lists, nothing to launch
  return c.K == 1 ? occ_compact<1>(c, raw, L, tally, stream) : occ_compact<AON_SCENE_MAX_OBJECTS>(c, raw, L, tally, stream);
}

// ---- early ray termination (tests/_stop_ref.py is an independent numpy copy) ----
// A level is evaluated front to back in rounds of R consecutive sample indices; round k covers [kR, min(S, (k+1)R)) of every ray.  Per ray:
// tau (fp32, 0 at the start of the level) and stop (int32, S at the start).  After round k's MLP launch a ray with stop == S adds
// sigma_i * delta_i of the round's samples to tau in ascending i -- one sequential fp32 chain, every multiply and add rounded -- with
// sigma_i / delta_i as composite_kernel (aon_render.hip) forms them, and stops (stop = (k+1)R) when tau >= tau_stop = fp32(-ln eps).
// In a later round a sample i >= stop[ray] is DEAD: the sentinel record, not listed (occ_flag).  The last round decides nothing (no depth launch).
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
  const float dn = ray_norm_f32(dirs, ray);
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
OccStopState occ_stop_state(char* state, int64_t n) {
  if (!state) return {nullptr, nullptr};
  return {reinterpret_cast<float*>(state), reinterpret_cast<int*>(state + occ_stop_state_bytes(n) / 2)};
}

hipError_t launch_occ_stop_init(char* state, int64_t n, int S, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const OccStopState st = occ_stop_state(state, n);
  occ_stop_init_kernel<<<dim3((unsigned)((n + kOccThreads - 1) / kOccThreads)), dim3(kOccThreads), 0, stream>>>(st.tau, st.stop, n, S);
  return hipGetLastError();
}

// state == nullptr: fill with `value`
hipError_t launch_occ_stop_store(char* state, int value, int* dst, int64_t n, int stride, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  occ_stop_store_kernel<<<dim3((unsigned)((n + kOccThreads - 1) / kOccThreads)), dim3(kOccThreads), 0, stream>>>(occ_stop_state(state, n).stop, value, dst,
                                                                                                                n, stride);
  return hipGetLastError();
}

hipError_t launch_occ_depth(const float* raw, const float* t_vals, const float* dirs, int64_t n, int S, int s0, int s1, const ActParams& ap,
                            float tau_stop, char* state, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const OccStopState st = occ_stop_state(state, n);
  constexpr int kRays = kOccThreads / 64;
  occ_depth_kernel<<<dim3((unsigned)((n + kRays - 1) / kRays)), dim3(kOccThreads), 0, stream>>>(reinterpret_cast<const f32x4*>(raw), t_vals, dirs, n, S,
                                                                                               s0, s1, ap, tau_stop, st.tau, st.stop);
  return hipGetLastError();
}

}  // namespace aon
