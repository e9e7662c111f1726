// Occupancy-grid accelerated inference (aon_occupancy_build, aon_render_fwd_occ / aon_art_render_fwd_occ): a bitfield of the cells of a
// density grid that may hold matter, and per render level the list of samples that fall into occupied cells.  The MLP then runs only on
// that list (the GATHER instances of mlp_fwd_kernel / art_mlp_fwd_kernel); every other sample gets the sentinel record below.  No atomics:
// the same bits on every run.
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
#include "aon_common.h"

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

// ---- per-level sample marking and compaction ----
__device__ __forceinline__ bool occ_lookup(const OccGrid& G, const float (&x)[3]) {
  int64_t c[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (!(x[a] >= G.lo[a] && x[a] <= G.hi[a])) return false;   // outside the box, or NaN
    const int64_t q = (int64_t)__builtin_floorf(__fdiv_rn(__fsub_rn(x[a], G.lo[a]), G.step[a]));
    c[a] = q < G.cells[a] - 1 ? q : G.cells[a] - 1;
  }
  const int64_t lin = (c[0] * G.cells[1] + c[1]) * G.cells[2] + c[2];
  return (G.bits[lin >> 5] >> (lin & 31)) & 1u;
}

struct OccSamples {
  const float* rays_o; const float* rays_d; const float* t_vals;   // (n,3), (n,3), (n,S)
  int64_t total; int S;                                             // n * S <= INT32_MAX (the caller's chunking)
};

__device__ __forceinline__ int occ_tile_flags(const OccGrid& G, const OccSamples& s, int64_t g0, bool (&occ)[4]) {
  int n = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t g = g0 + r;
    occ[r] = false;
    if (g >= s.total) continue;
    const int64_t ray = g / s.S;
    const float t = s.t_vals[g];
    float x[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) x[a] = __fadd_rn(s.rays_o[ray * 3 + a], __fmul_rn(t, s.rays_d[ray * 3 + a]));   // helper.cast_rays
    occ[r] = occ_lookup(G, x);
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
                              char* ws, int64_t* tally, const int** idx_out, const int64_t** count_out, hipStream_t stream) {
  const OccSamples s{rays_o, rays_d, t_vals, n * S, S};
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

}  // namespace aon
