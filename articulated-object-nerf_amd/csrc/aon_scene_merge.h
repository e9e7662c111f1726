// The order in which a ray's merged samples are composited, for scene_composite_kernel (aon_scene.hip) and
// scene_composite_bwd_kernel (aon_scene_grad.hip).  One wavefront per ray.  A ray's LIVE lists are the entries of slot[ray, 0..K) that name a
// row of the pairs' arrays; list j (in object order) has S samples with ascending t.  The merged order is by the key (t, object, i): a
// sample's rank is its own index plus, in every other list, the number of keys below its own -- t <= mine in a list of a lower object,
// t < mine in a list of a higher one.
//
// Per wave in LDS: a 256-byte head (the live lists' rows, objects, first and last t), then the kernel's own per-sample arrays, of which
// the t in list layout (`tl`, L * S floats) is staged here.
#pragma once
#include "../../include/aon_hip_scene.h"
#include "aon_ray_core.h"

namespace aon {

constexpr int kMaxObj = AON_SCENE_MAX_OBJECTS;
constexpr int kHeadBytes = 256;

struct SceneLists {
  int* lp;      // row of live list j
  int* lk;      // its object
  float* llo;   // its first and last t
  float* lhi;
  __device__ __forceinline__ explicit SceneLists(char* head)
      : lp(reinterpret_cast<int*>(head)), lk(lp + kMaxObj), llo(reinterpret_cast<float*>(lk + kMaxObj)), lhi(llo + kMaxObj) {}
};
static_assert(4 * kMaxObj * 4 <= kHeadBytes, "the head holds four words per object");

// The head from slot[ray, 0..K) -> L, the number of live lists (wave-uniform); `live`: lane k's entry names a row.  With L == 0 nothing is
// written.  (a row past `pairs` is nobody's: treated as dead, never dereferenced)
__device__ __forceinline__ int scene_live_lists(const SceneLists& h, const int32_t* slot, const float* t_vals, int64_t ray, int K, int64_t pairs,
                                                int S, int lane, bool& live) {
  int p = -1;
  if (lane < K) p = slot[ray * K + lane];
  live = p >= 0 && p < pairs;
  const uint64_t m = __builtin_amdgcn_ballot_w64(live);
  if (live) {
    const int j = __builtin_popcountll(m & (lane == 0 ? 0ull : (~0ull >> (64 - lane))));
    h.lp[j] = p;
    h.lk[j] = lane;
    h.llo[j] = t_vals[(int64_t)p * S];
    h.lhi[j] = t_vals[(int64_t)p * S + S - 1];
  }
  return __builtin_popcountll(m);
}

// tl[j * S + i] <- t of sample i of live list j; the head and tl are readable by every lane afterwards
__device__ __forceinline__ void scene_stage_t(const SceneLists& h, float* tl, const float* t_vals, int L, int S, int lane) {
  wave_lds_sync();
  for (int j = 0; j < L; ++j) {
    const float* tv = t_vals + (int64_t)h.lp[j] * S;
    for (int i = lane; i < S; i += 64) tl[j * S + i] = tv[i];
  }
  wave_lds_sync();
}

// rank of sample i (at t) of list j.  0 <= rank <= L * S - 1 whatever the t hold (each count is at most S).
__device__ __forceinline__ int scene_rank(const SceneLists& h, const float* tl, float t, int i, int j, int L, int S) {
  const int kj = h.lk[j];
  int rank = i;
  for (int b = 0; b < L; ++b) {
    if (b == j) continue;
    if (t < h.llo[b]) continue;                  // wholly behind this sample
    if (t > h.lhi[b]) { rank += S; continue; }   // wholly in front of it
    const bool le = h.lk[b] < kj;
    const float* x = tl + b * S;
    int lo = 0, hi = S;                          // the lists are sorted already: a binary search
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      const float xm = x[mid];
      if (le ? xm <= t : xm < t) lo = mid + 1; else hi = mid;
    }
    rank += lo;
  }
  return rank;
}

}  // namespace aon
