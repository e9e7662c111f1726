// Backward of the per-list merged scene composite (include/aon_hip_scene_lists_grad.h is the contract and
// tests/_scene_lists_grad_ref.py an independent torch fp64 restatement): d(rgb, acc, depth, obj_acc) -> d raw per sample of every live
// list, each list read by its own record -- what a scene with a vanilla NeRF as the backdrop needs to be learned from.
//
//   scene_composite_lists_bwd_kernel  scene_composite_bwd_kernel's shape (aon_scene_grad.hip), a second kernel BESIDE it: one wavefront per
//                                     ray, the aon_scene_merge.h head and ranks, three sweeps through one loop body, the fp64 product scan
//                                     in rank order in blocks of 64 with a carry, the suffix sum from the far end, 22 B of LDS per merged
//                                     sample.  The k list records travel by value in the kernel arguments, as in
//                                     scene_composite_lists_kernel (aon_scene_lists.hip); the list loop is outermost, a list's record is
//                                     read once per list through a wave-uniform index, and the branch on its act stands OUTSIDE the
//                                     per-sample body (list_samples<ACT>): inside it the activation is a template argument, as in the
//                                     homogeneous kernel, so the sample record stays in registers.
//
// The per-sample expressions are aon_composite_grad.h's, in scene_composite_bwd_kernel's order: with k closed lists of one act and one set of
// scalars every bit of d_raw is that kernel's.  The one new piece is the last interval of an open list: 1e10f * dn, formed as the forward
// forms it.
#include "../../include/aon_hip_scene_lists_grad.h"
#include "aon_capi_util.h"
#include "aon_composite_grad.h"
#include "aon_scene_merge.h"

using namespace aon::capi;

namespace aon {
namespace {

// Per wave in LDS, as scene_composite_bwd_kernel: the 256-byte head and 22 bytes per merged sample (two doubles in RANK order, t and the
// 16-bit rank in list layout).  90,368 B at the limit of 4,096 merged samples.
constexpr int kListGradSampleBytes = 22;
constexpr int kListGradLdsBudget = 160 * 1024;

struct SceneListGradRecs {   // by value in the kernel arguments (16 x 20 B)
  aon_scene_list r[kMaxObj];
};

struct SceneCompositeListsBwdArgs {
  const float4* raw; const float* t_vals; const int32_t* slot; const float* dirs;
  const float* g_rgb; const float* g_acc; const float* g_depth; const float* g_obj_acc;
  int64_t n; int K; int64_t pairs; int S; int white_bkgd;
  float4* d_raw;
  int wave_bytes;
  SceneListGradRecs lists;
};

// What the sweeps share: the wave's LDS arrays and the ray's upstream gradients
struct ListSweep {
  double* fT; double* gS; float* tl; unsigned short* rk;
  int L, S, lane;
  float dn;
};

// The samples of live list j in one sweep (scene_composite_bwd_kernel's loop body, `last` for the list's last interval):
//   sweep 0  rank by counting, f in rank order
//   sweep 1  w gw in rank order
//   sweep 2  dL/dalpha_j = T_j gw_j - Sfx_j / f_j, and one float4 per sample; a factor that is exactly zero gives +0
template <int ACT>
__device__ __forceinline__ void list_samples(int sweep, const ListSweep& q, const SceneLists& h, const CompositeUpstream& up, const ActParams& ap,
                                             int j, float last, double gO, const float4* raw_row, float4* d_row) {
  const int S = q.S;
  for (int i = q.lane; i < S; i += 64) {
    const int e = j * S + i;
    const float t = q.tl[e];
    const float dist = i < S - 1 ? __fmul_rn(__fsub_rn(q.tl[e + 1], t), q.dn) : last;
    const float4 r = raw_row[i];
    CompositeSample s;
    density<ACT>(ap, r.w, dist, s);
    if (sweep == 0) {
      const int rank = scene_rank(h, q.tl, t, i, j, q.L, S);
      q.fT[rank] = s.f;
      q.rk[e] = (unsigned short)rank;
      continue;
    }
    colours<ACT>(ap, r, s);
    const int rank = q.rk[e];
    const double T = q.fT[rank];
    const double gw = up.gw(s, t) + gO;
    const double w = s.alpha * T;
    if (sweep == 1) {
      q.gS[rank] = w * gw;
      continue;
    }
    const double dalpha = T * gw - q.gS[rank] / s.f;
    float4 o;
    o.x = w == 0.0 ? 0.f : (float)(w * up.gC0 * s.d0);
    o.y = w == 0.0 ? 0.f : (float)(w * up.gC1 * s.d1);
    o.z = w == 0.0 ? 0.f : (float)(w * up.gC2 * s.d2);
    o.w = s.kf == 0.0 ? 0.f : (float)(dalpha * s.kf);
    d_row[i] = o;
  }
}

__global__ __launch_bounds__(256) void scene_composite_lists_bwd_kernel(SceneCompositeListsBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) char scene_lists_grad_lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t ray = (int64_t)blockIdx.x * (blockDim.x >> 6) + wv;
  if (ray >= a.n) return;   // wave-uniform; no block-level barrier below
  const int K = a.K, S = a.S, MS = K * S;
  char* base = scene_lists_grad_lds + (size_t)wv * a.wave_bytes;
  const SceneLists h(base);
  ListSweep q;
  q.fT = reinterpret_cast<double*>(base + kHeadBytes);   // RANK order: f, then T
  q.gS = q.fT + MS;                                      // RANK order: w gw, then Sfx
  q.tl = reinterpret_cast<float*>(q.gS + MS);            // list layout
  q.rk = reinterpret_cast<unsigned short*>(q.tl + MS);
  q.S = S; q.lane = lane;

  bool live;
  const int L = scene_live_lists(h, a.slot, a.t_vals, ray, K, a.pairs, S, lane, live);
  if (L == 0) return;   // no list: no row of d_raw is this ray's
  scene_stage_t(h, q.tl, a.t_vals, L, S, lane);
  q.L = L;
  q.dn = ray_norm_f32(a.dirs, ray);
  const int M = L * S;
  const CompositeUpstream up(a.g_rgb, a.g_acc, a.g_depth, a.white_bkgd, ray);

#pragma nounroll
  for (int sweep = 0; sweep < 3; ++sweep) {
    for (int j = 0; j < L; ++j) {
      const int64_t row = (int64_t)h.lp[j] * S;
      // the list's record: h.lk[j] is the same in every lane (0 <= lk < K <= 16), so this is a scalar read of the kernel arguments
      const int kj = __builtin_amdgcn_readfirstlane(h.lk[j]) & (kMaxObj - 1);
      const aon_scene_list& rec = a.lists.r[kj];
      const ActParams ap{rec.act, rec.rgb_scale, rec.rgb_shift, rec.sigma_bias, nullptr, 0.f};
      const float last = rec.open_end ? __fmul_rn(1e10f, q.dn) : 0.f;
      // dL/dw_j takes g_obj_acc[ray, list of j] too
      const double gO = a.g_obj_acc ? (double)a.g_obj_acc[ray * K + kj] : 0.0;
      const float4* raw_row = a.raw + row;
      float4* d_row = a.d_raw + row;
      // wave-uniform: one branch per list, none per sample
      if (ap.act == 1) list_samples<1>(sweep, q, h, up, ap, j, last, gO, raw_row, d_row);
      else if (ap.act == 2) list_samples<2>(sweep, q, h, up, ap, j, last, gO, raw_row, d_row);
      else list_samples<0>(sweep, q, h, up, ap, j, last, gO, raw_row, d_row);
    }
    wave_lds_sync();
    if (sweep == 0) {   // T_j = prod_{m < j} f_m: 64 at a time, the carry is everything before the block
      double carry = 1.0;
      for (int b0 = 0; b0 < M; b0 += 64) {
        const int j = b0 + lane;
        const double T = wave_exclusive_product_f64(j < M ? q.fT[j] : 1.0, lane, carry);
        if (j < M) q.fT[j] = T;
      }
    } else if (sweep == 1) {   // Sfx_j = sum_{m > j} w_m gw_m, scanned from the far end
      double sfx_carry = 0.0;
      for (int b0 = ((M - 1) >> 6) << 6; b0 >= 0; b0 -= 64) {
        const int j = b0 + lane;
        const double sfx = wave_exclusive_suffix_sum_f64(j < M ? q.gS[j] : 0.0, lane, sfx_carry);
        if (j < M) q.gS[j] = sfx;
      }
    }
    wave_lds_sync();
  }
}

DeviceOnce g_scene_lists_grad_lds;

}  // namespace

int64_t scene_composite_lists_bwd_wave_bytes(int K, int S) { return (kHeadBytes + (int64_t)K * S * kListGradSampleBytes + 15) / 16 * 16; }

hipError_t launch_scene_composite_lists_bwd(const float* raw, const float* t_vals, const int32_t* slot, const float* dirs, const float* g_rgb,
                                            const float* g_acc, const float* g_depth, const float* g_obj_acc, int64_t n, int K, int64_t pairs,
                                            int S, int white_bkgd, const aon_scene_list* lists_host, float* d_raw, hipStream_t stream) {
  if (n <= 0 || pairs <= 0) return hipSuccess;
  if (K < 1 || K > kMaxObj) return hipErrorInvalidValue;
  const int64_t wave_bytes = scene_composite_lists_bwd_wave_bytes(K, S);
  int waves = (int)(kListGradLdsBudget / wave_bytes);
  if (waves < 1) return hipErrorInvalidValue;   // (K * S <= 4096: 90,368 B)
  waves = waves > 4 ? 4 : waves;
  if (hipError_t e = set_max_lds(scene_composite_lists_bwd_kernel, kListGradLdsBudget, g_scene_lists_grad_lds); e != hipSuccess) return e;
  SceneCompositeListsBwdArgs a{reinterpret_cast<const float4*>(raw), t_vals, slot, dirs, g_rgb, g_acc, g_depth, g_obj_acc, n, K, pairs, S, white_bkgd,
                               reinterpret_cast<float4*>(d_raw), (int)wave_bytes, {}};
  std::memset(&a.lists, 0, sizeof(a.lists));
  std::memcpy(a.lists.r, lists_host, sizeof(aon_scene_list) * K);
  const int64_t grid = (n + waves - 1) / waves;
  scene_composite_lists_bwd_kernel<<<dim3((unsigned)grid), dim3(64 * waves), (size_t)(wave_bytes * waves), stream>>>(a);
  return hipGetLastError();
}

}  // namespace aon

extern "C" {

int aon_scene_composite_lists_bwd(const float* raw, const float* t_vals, const int32_t* slot, const float* rays_d, const float* g_rgb,
                                  const float* g_acc, const float* g_depth, const float* g_obj_acc, int64_t n, int k, int64_t pairs, int s,
                                  int white_bkgd, const aon_scene_list* lists_host, float* d_raw, void* stream) {
  if (n < 0 || pairs < 0 || k < 1 || k > AON_SCENE_MAX_OBJECTS || s < 2 || (int64_t)k * s > AON_SCENE_MAX_MERGED)
    return fail(AON_E_INVALID, "aon_scene_composite_lists_bwd: bad size / list count (1 <= k <= 16, s >= 2, k * s <= 4096)");
  if (!raw || !t_vals || !slot || !rays_d || !g_rgb || !lists_host || !d_raw)
    return fail(AON_E_INVALID, "aon_scene_composite_lists_bwd: null pointer");
  for (int j = 0; j < k; ++j)
    if (lists_host[j].act < 0 || lists_host[j].act > 2 || lists_host[j].open_end < 0 || lists_host[j].open_end > 1)
      return fail(AON_E_INVALID, "aon_scene_composite_lists_bwd: bad list record (act in [0, 2], open_end 0 or 1)");
  if (reinterpret_cast<uintptr_t>(raw) & 15) return fail(AON_E_INVALID, "aon_scene_composite_lists_bwd: raw must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_raw) & 15) return fail(AON_E_INVALID, "aon_scene_composite_lists_bwd: d_raw must be 16-byte aligned");
  if (n == 0 || pairs == 0) return AON_OK;
  return check(aon::launch_scene_composite_lists_bwd(raw, t_vals, slot, rays_d, g_rgb, g_acc, g_depth, g_obj_acc, n, k, pairs, s, white_bkgd, lists_host,
                                                     d_raw, static_cast<hipStream_t>(stream)), "aon_scene_composite_lists_bwd");
}

}  // extern "C"
