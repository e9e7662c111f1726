// Occupancy grids for scenes (include/aon_hip_scene_occ.h is the contract, tests/_scene_occ_ref.py the yardstick):
// aon_occ.hip's mark / scan / emit for the K object segments of a scene's pair rows at once, each segment against its own object's grid, and
// the stage call that drives them and the GATHER instance of art_mlp_fwd_kernel.  Three launches per level whatever K is, no atomics: the
// same bits on every run.
//
// A pair's ray is already in its object's frame, so a grid built in that frame applies verbatim: x = o' + t d' (multiply, then add: the MLP
// kernel's own bits), looked up by occ_lookup (aon_occ_lookup.h) -- the device function occ_mark_kernel uses.  A tile is kSceneOccTile = 1024
// consecutive samples of ONE object: object k has ceil(P_k S / 1024) tiles when it has a grid and none otherwise, and a tile finds its
// object from the K + 1 first-tile numbers in the kernel arguments, beside the K grid records (by value, as aon_scene_pairs' object records
// travel: no device copy to keep alive, nothing for the host to wait for).  Thread t of a tile takes samples t, t + 256, t + 512, t + 768.
//   scene_occ_mark_kernel  the sentinel record (0, 0, 0, -inf) of every empty sample; the tile's occupied count (wave ballots + an LDS sum);
//   scene_occ_scan_kernel  ONE workgroup: per object the exclusive prefix of its tiles' counts and the object's total -> K device counters
//                          (a dense object's: all of its samples), added to the caller's tally when given;
//   scene_occ_emit_kernel  the lookup again; object k's ascending list of SEGMENT-LOCAL sample indices row_local * S + i at idx + starts[k] S,
//                          so each segment feeds launch_art_mlp_fwd_gather unchanged with its own ray / t / raw pointers.
#include "../../include/aon_hip_scene_occ.h"
#include "aon_capi_util.h"
#include "aon_occ_lookup.h"

using namespace aon::capi;

namespace aon {
namespace {

constexpr int kSceneOccTile = 1024;
constexpr int kSceneOccThreads = 256;
constexpr int kSceneOccPer = kSceneOccTile / kSceneOccThreads;
constexpr int kSceneOccWaves = kSceneOccThreads / 64;
constexpr int kMaxObj = AON_SCENE_MAX_OBJECTS;

struct SceneOccArgs {   // by value in the kernel arguments (1.4 KB)
  OccGrid g[kMaxObj];          // bits == nullptr: a dense object (no tiles)
  int64_t row0[kMaxObj + 1];   // segment starts in rows; row0[K] = P
  int tile0[kMaxObj + 1];      // first tile of each object, ascending; tile0[K] = the number of tiles
  int K, S;
  const float* pair_o; const float* pair_d; const float* t_vals;   // (P,3), (P,3), (P,S)
};

// the object of a tile: the last k with tile0[k] <= tile (objects without tiles share their successor's first tile and lose to it)
__device__ __forceinline__ int scene_occ_object(const SceneOccArgs& a, int tile) {
  int k = 0;
  for (int j = 1; j < a.K; ++j)   // (uniform)
    if (tile >= a.tile0[j]) k = j;
  return k;
}

// the tile's four samples of this thread: segment-local indices g[r] (-1 past the segment's end) and whether they are occupied
__device__ __forceinline__ void scene_occ_flags(const SceneOccArgs& a, int k, int64_t (&g)[kSceneOccPer], bool (&occ)[kSceneOccPer]) {
  const int64_t total = (a.row0[k + 1] - a.row0[k]) * a.S;   // <= INT32_MAX (the entry point's check)
  const int64_t g0 = (int64_t)((int)blockIdx.x - a.tile0[k]) * kSceneOccTile + threadIdx.x;
#pragma unroll
  for (int r = 0; r < kSceneOccPer; ++r) {
    g[r] = g0 + r * kSceneOccThreads;
    occ[r] = false;
    if (g[r] >= total) { g[r] = -1; continue; }
    const int64_t row = a.row0[k] + (int64_t)((uint32_t)g[r] / (uint32_t)a.S);
    const float t = a.t_vals[a.row0[k] * a.S + g[r]];
    float x[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c] = __fadd_rn(a.pair_o[row * 3 + c], __fmul_rn(t, a.pair_d[row * 3 + c]));   // helper.cast_rays
    occ[r] = occ_lookup(a.g[k], x);
  }
}

__global__ __launch_bounds__(kSceneOccThreads) void scene_occ_mark_kernel(SceneOccArgs a, f32x4* __restrict__ raw, int* __restrict__ tile_counts) {
  __shared__ int cnt[kSceneOccPer][kSceneOccWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k = scene_occ_object(a, blockIdx.x);
  int64_t g[kSceneOccPer];
  bool occ[kSceneOccPer];
  scene_occ_flags(a, k, g, occ);
  f32x4 sentinel;
  sentinel[0] = 0.f; sentinel[1] = 0.f; sentinel[2] = 0.f; sentinel[3] = -__builtin_huge_valf();
#pragma unroll
  for (int r = 0; r < kSceneOccPer; ++r) {
    if (g[r] >= 0 && !occ[r]) raw[a.row0[k] * a.S + g[r]] = sentinel;
    const int c = __builtin_popcountll(__builtin_amdgcn_ballot_w64(occ[r]));
    if (lane == 0) cnt[r][wave] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0;
#pragma unroll
    for (int r = 0; r < kSceneOccPer; ++r)
#pragma unroll
      for (int w = 0; w < kSceneOccWaves; ++w) tot += cnt[r][w];
    tile_counts[blockIdx.x] = tot;
  }
}

// per object: offs[tile] = the occupied samples of the object's earlier tiles; counts[k] = the object's total (dense: all of its samples);
// tally[k] += counts[k] when tally is given.  Integers: exact, the order of the sums does not matter.
__global__ __launch_bounds__(kSceneOccThreads) void scene_occ_scan_kernel(SceneOccArgs a, const int* __restrict__ tile_counts, int* __restrict__ offs,
                                                                          int64_t* __restrict__ counts, int64_t* __restrict__ tally) {
  __shared__ int64_t red[kSceneOccWaves];
  constexpr int kPer = 8;
  for (int k = 0; k < a.K; ++k) {   // (uniform)
    const int64_t b0 = a.tile0[k], b1 = a.tile0[k + 1];
    int64_t carry = a.g[k].bits ? 0 : (a.row0[k + 1] - a.row0[k]) * a.S;
    for (int64_t base = b0; base < b1; base += (int64_t)kSceneOccThreads * kPer) {
      const int64_t t0 = base + (int64_t)threadIdx.x * kPer;
      int cv[kPer];
      int64_t sv = 0;
#pragma unroll
      for (int r = 0; r < kPer; ++r) {
        cv[r] = t0 + r < b1 ? tile_counts[t0 + r] : 0;
        sv += cv[r];
      }
      int64_t tv;
      int64_t run = carry + block_excl_scan<int64_t>(sv, tv, red);
#pragma unroll
      for (int r = 0; r < kPer; ++r) {
        if (t0 + r < b1) offs[t0 + r] = (int)run;
        run += cv[r];
      }
      carry += tv;
    }
    if (threadIdx.x == 0) {
      counts[k] = carry;
      if (tally) tally[k] += carry;
    }
  }
}

__global__ __launch_bounds__(kSceneOccThreads) void scene_occ_emit_kernel(SceneOccArgs a, const int* __restrict__ offs, int* __restrict__ idx) {
  __shared__ int cnt[kSceneOccPer][kSceneOccWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k = scene_occ_object(a, blockIdx.x);
  int64_t g[kSceneOccPer];
  bool occ[kSceneOccPer];
  scene_occ_flags(a, k, g, occ);
  uint64_t bal[kSceneOccPer];
#pragma unroll
  for (int r = 0; r < kSceneOccPer; ++r) {
    bal[r] = __builtin_amdgcn_ballot_w64(occ[r]);
    if (lane == 0) cnt[r][wave] = __builtin_popcountll(bal[r]);
  }
  __syncthreads();
  const uint64_t below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  int* list = idx + a.row0[k] * a.S;
  int run = offs[blockIdx.x];   // ascending: sample = r * 256 + 64 * wave + lane
#pragma unroll
  for (int r = 0; r < kSceneOccPer; ++r) {
    int before = run;
#pragma unroll
    for (int w = 0; w < kSceneOccWaves; ++w) {
      if (w < wave) before += cnt[r][w];
      run += cnt[r][w];
    }
    if (occ[r]) list[before + __builtin_popcountll(bal[r] & below)] = (int)g[r];
  }
}

int64_t scene_occ_tile_cap(int64_t pairs, int K, int S) { return pairs * S / kSceneOccTile + K; }   // >= sum_k ceil(P_k S / 1024)
int64_t scene_occ_idx_bytes(int64_t pairs, int S) { return align_up((pairs > 0 ? pairs : 1) * S * 4, 256); }
int64_t scene_occ_tile_bytes(int64_t pairs, int K, int S) { return align_up(scene_occ_tile_cap(pairs, K, S) * 4, 256); }

}  // namespace

int64_t scene_occ_list_bytes(int64_t pairs, int K, int S) {   // the lists, tile counts, tile offsets, K counters
  return scene_occ_idx_bytes(pairs, S) + 2 * scene_occ_tile_bytes(pairs, K, S) + align_up((int64_t)K * 8, 256);
}

hipError_t launch_scene_occ_compact(const OccGrid* grids, const int64_t* starts, int K, int S, const float* pair_o, const float* pair_d,
                                    const float* t_vals, float* raw, char* ws, int64_t* tally, const int** idx_out, const int64_t** counts_out,
                                    hipStream_t stream) {
  const int64_t pairs = starts[K];
  SceneOccArgs a;
  std::memset(&a, 0, sizeof(a));
  int64_t tiles = 0;
  for (int k = 0; k < K; ++k) {
    a.g[k] = grids[k];
    a.row0[k] = starts[k];
    a.tile0[k] = (int)tiles;
    if (grids[k].bits) tiles += ((starts[k + 1] - starts[k]) * S + kSceneOccTile - 1) / kSceneOccTile;
  }
  a.row0[K] = pairs;
  a.tile0[K] = (int)tiles;
  a.K = K; a.S = S;
  a.pair_o = pair_o; a.pair_d = pair_d; a.t_vals = t_vals;
  int* idx = reinterpret_cast<int*>(ws);
  int* tile_counts = reinterpret_cast<int*>(ws + scene_occ_idx_bytes(pairs, S));
  int* offs = reinterpret_cast<int*>(ws + scene_occ_idx_bytes(pairs, S) + scene_occ_tile_bytes(pairs, K, S));
  int64_t* counts = reinterpret_cast<int64_t*>(ws + scene_occ_idx_bytes(pairs, S) + 2 * scene_occ_tile_bytes(pairs, K, S));
  *idx_out = idx; *counts_out = counts;
  const dim3 grid((unsigned)tiles), block(kSceneOccThreads);
  if (tiles > 0) {
    scene_occ_mark_kernel<<<grid, block, 0, stream>>>(a, reinterpret_cast<f32x4*>(raw), tile_counts);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  if (tiles > 0 || tally) {   // (no grid on any object with rows: the dense launches read no counter, the tally is all the scan writes)
    scene_occ_scan_kernel<<<dim3(1), block, 0, stream>>>(a, tile_counts, offs, counts, tally);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  if (tiles > 0) {
    scene_occ_emit_kernel<<<grid, block, 0, stream>>>(a, offs, idx);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace aon

extern "C" {

int64_t aon_scene_occ_workspace_bytes(int64_t pairs, int k, int s) {
  if (pairs < 0 || k < 1 || k > AON_SCENE_MAX_OBJECTS || s < 1 || pairs > (int64_t)0x7fffffff / s) return 0;
  return aon::scene_occ_list_bytes(pairs, k, s);
}

int aon_scene_art_mlp_fwd_occ(const void* packed, const void* const* smalls_host, const aon_occupancy* const* grids_host, const int64_t* starts_host,
                              const float* pair_o, const float* pair_d, const float* pair_v, const float* t_vals, int k, int s, float* raw,
                              int64_t* occupied_dev, void* workspace, int64_t workspace_bytes, void* stream_) {
  auto bad = [&](const std::string& what) { return fail(AON_E_INVALID, ("aon_scene_art_mlp_fwd_occ: " + what).c_str()); };
  if (k < 1 || k > AON_SCENE_MAX_OBJECTS || s < 1) return bad("bad object count / sample count (1 <= k <= 16, s >= 1)");
  bool ascending = starts_host && starts_host[0] == 0;
  for (int j = 0; ascending && j < k; ++j) ascending = starts_host[j + 1] >= starts_host[j];
  if (!ascending) return bad("starts_host must ascend from starts_host[0] = 0");
  const int64_t pairs = starts_host[k];
  if (pairs > (int64_t)0x7fffffff / s) return bad("more than 2^31 - 1 samples (starts_host[k] * s)");
  if (pairs == 0) return AON_OK;
  bool null = !packed || !smalls_host || !grids_host || !pair_o || !pair_d || !pair_v || !t_vals || !raw || !workspace;
  for (int j = 0; !null && j < k; ++j) null = starts_host[j + 1] > starts_host[j] && !smalls_host[j];
  if (null) return bad("null pointer");
  aon::OccGrid grids[AON_SCENE_MAX_OBJECTS];
  std::memset(grids, 0, sizeof(grids));
  for (int j = 0; j < k; ++j)
    if (grids_host[j])
      if (const char* msg = occ_grid_bad(grids_host[j], grids[j])) return bad("object " + std::to_string(j) + ": " + msg);
  if ((reinterpret_cast<uintptr_t>(raw) & 15) || (reinterpret_cast<uintptr_t>(workspace) & 255))
    return bad("raw must be 16-byte aligned and the workspace 256-byte aligned");
  for (int j = 0; j < k; ++j)
    if (starts_host[j + 1] > starts_host[j] && forms_differ(packed, smalls_host[j])) return fail(AON_E_INVALID, kFormsMsg);
  if (workspace_bytes < aon_scene_occ_workspace_bytes(pairs, k, s))
    return fail(AON_E_WORKSPACE, "aon_scene_art_mlp_fwd_occ: workspace smaller than aon_scene_occ_workspace_bytes()");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const int* idx = nullptr;
  const int64_t* counts = nullptr;
  if (int rc = check(aon::launch_scene_occ_compact(grids, starts_host, k, s, pair_o, pair_d, t_vals, raw, static_cast<char*>(workspace), occupied_dev,
                                                   &idx, &counts, stream), "aon_scene_art_mlp_fwd_occ (compact)"))
    return rc;
  // one MLP launch per object with rows, as aon_art_mlp_fwd makes it (no per-ray view bias): on the object's list, or dense
  for (int j = 0; j < k; ++j) {
    const int64_t r0 = starts_host[j], rows = starts_host[j + 1] - r0;
    if (rows == 0) continue;
    MlpTimer timer(stream, rows * s);
    const char* pk = static_cast<const char*>(packed);
    const float* sm = static_cast<const float*>(smalls_host[j]);
    const hipError_t e = grids[j].bits ? aon::launch_art_mlp_fwd_gather(pk, sm, pair_o + r0 * 3, pair_d + r0 * 3, pair_v + r0 * 3, t_vals + r0 * s, rows, s,
                                                                        raw + r0 * s * 4, stream, nullptr, idx + r0 * s, counts + j, rows * s)
                                       : aon::launch_art_mlp_fwd(pk, sm, pair_o + r0 * 3, pair_d + r0 * 3, pair_v + r0 * 3, t_vals + r0 * s, rows, s,
                                                                 raw + r0 * s * 4, stream);
    if (int rc = check(e, "aon_scene_art_mlp_fwd_occ")) return rc;
  }
  return AON_OK;
}

}  // extern "C"
