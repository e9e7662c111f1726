// Backward of the merged scene composite (include/aon_hip_scene_grad.h is the contract and tests/_scene_grad_ref.py an
// independent torch fp64 restatement): d(rgb, acc, depth, obj_acc) -> d raw per sample of every live pair.
//
//   scene_composite_bwd_kernel  one wavefront per ray, as scene_composite_kernel (csrc/aon_scene.hip): the t of its live lists staged in LDS and
//                               every sample ranked by counting (aon_scene_merge.h: the forward's own rule and code),
//                               f = 1 - alpha + 1e-10 placed in RANK order and turned into T by a multiplicative scan in blocks of 64 with a
//                               carry, w gw placed in rank order and turned into Sfx by an additive scan from the far end, then every sample
//                               fetches its T and Sfx by rank and writes one float4.
//
// The function and its arithmetic are aon_composite_grad.h's (fp64 on the fp32 inputs, one rounding per output), with the scene's own pieces:
// the last interval of a list is 0, dL/dw takes g_obj_acc[ray, object] too, and an exactly zero factor gives +0.  Both scans run in a
// fixed order over the ray's own merged list; no atomics: a ray's d_raw rows are a function of its own lists only.  alpha, the colours and
// the derivatives are recomputed from raw and t in each of the three sweeps rather than stored: per sample the kernel reads 20 bytes (its
// record three times, from the cache after the first) and writes 16.
#include "../../include/aon_hip_scene_grad.h"
#include "aon_capi_util.h"
#include "aon_composite_grad.h"
#include "aon_scene_merge.h"

using namespace aon::capi;

namespace aon {
namespace {

// Per wave in LDS: the head of the live lists (aon_scene_merge.h) and 22 bytes per sample of the K * S the call admits:
// two doubles in RANK order (f -> T;  w gw -> Sfx), t and the rank (16 bits: K * S <= 4096) in list layout.  90,368 B at the limit: above
// the 64 KiB a kernel gets by default, below the 160 KiB a workgroup may use on gfx950 (set_max_lds, aon_common.h).
constexpr int kSampleBytes = 22;
constexpr int kLdsBudget = 160 * 1024;

struct SceneCompositeBwdArgs {
  const float4* raw; const float* t_vals; const int32_t* slot; const float* dirs;
  const float* g_rgb; const float* g_acc; const float* g_depth; const float* g_obj_acc;
  int64_t n; int K; int64_t pairs; int S; int white_bkgd; ActParams ap;
  float4* d_raw;
  int wave_bytes;
};

template <int ACT>
__global__ __launch_bounds__(256) void scene_composite_bwd_kernel(SceneCompositeBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) char scene_grad_lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t ray = (int64_t)blockIdx.x * (blockDim.x >> 6) + wv;
  if (ray >= a.n) return;   // wave-uniform; no block-level barrier below
  const int K = a.K, S = a.S, MS = K * S;
  char* base = scene_grad_lds + (size_t)wv * a.wave_bytes;
  const SceneLists h(base);
  double* fT = reinterpret_cast<double*>(base + kHeadBytes);   // RANK order: f, then T
  double* gS = fT + MS;                                        // RANK order: w gw, then Sfx
  float* tl = reinterpret_cast<float*>(gS + MS);               // list layout
  unsigned short* rk = reinterpret_cast<unsigned short*>(tl + MS);
  const ActParams ap = a.ap;

  bool live;
  const int L = scene_live_lists(h, a.slot, a.t_vals, ray, K, a.pairs, S, lane, live);
  if (L == 0) return;   // no pair: no row of d_raw is this ray's
  scene_stage_t(h, tl, a.t_vals, L, S, lane);
  const float dn = ray_norm_f32(a.dirs, ray);
  const int M = L * S;
  // dL/dw_j takes g_obj_acc[ray, object of j] too
  const CompositeUpstream up(a.g_rgb, a.g_acc, a.g_depth, a.white_bkgd, ray);

  // Three sweeps over the samples in list layout, one loop body (so that the fp64 exp / log1p code exists once): alpha, the colours and the
  // derivatives are recomputed from raw and t in each.
  //   sweep 0  rank by counting (scene_rank), f in rank order; then T_j = prod_{m < j} f_m: 64 at a time, the carry is everything before the block
  //   sweep 1  w gw in rank order; then Sfx_j = sum_{m > j} w_m gw_m, scanned from the far end
  //   sweep 2  dL/dalpha_j = T_j gw_j - Sfx_j / f_j, and one float4 per sample.  A factor that is exactly zero (w: alpha = 0 at the last
  //            sample of a list and at a sentinel record; d alpha / d raw_sigma likewise) gives +0, not the -0 or NaN of 0 x (something
  //            negative or not finite).
#pragma nounroll
  for (int sweep = 0; sweep < 3; ++sweep) {
    for (int j = 0; j < L; ++j) {
      const int64_t row = (int64_t)h.lp[j] * S;
      const double gO = a.g_obj_acc ? (double)a.g_obj_acc[ray * K + h.lk[j]] : 0.0;
      for (int i = lane; i < S; i += 64) {
        const int e = j * S + i;
        const float t = tl[e];
        const float dist = i < S - 1 ? __fmul_rn(__fsub_rn(tl[e + 1], t), dn) : 0.f;
        const float4 r = a.raw[row + i];
        CompositeSample s;
        density<ACT>(ap, r.w, dist, s);
        if (sweep == 0) {
          const int rank = scene_rank(h, tl, t, i, j, L, S);
          fT[rank] = s.f;
          rk[e] = (unsigned short)rank;
          continue;
        }
        colours<ACT>(ap, r, s);
        const int rank = rk[e];
        const double T = fT[rank];
        const double gw = up.gw(s, t) + gO;
        const double w = s.alpha * T;
        if (sweep == 1) {
          gS[rank] = w * gw;
          continue;
        }
        const double dalpha = T * gw - gS[rank] / s.f;
        float4 o;
        o.x = w == 0.0 ? 0.f : (float)(w * up.gC0 * s.d0);
        o.y = w == 0.0 ? 0.f : (float)(w * up.gC1 * s.d1);
        o.z = w == 0.0 ? 0.f : (float)(w * up.gC2 * s.d2);
        o.w = s.kf == 0.0 ? 0.f : (float)(dalpha * s.kf);
        a.d_raw[row + i] = o;
      }
    }
    wave_lds_sync();
    if (sweep == 0) {
      double carry = 1.0;
      for (int b0 = 0; b0 < M; b0 += 64) {
        const int j = b0 + lane;
        const double T = wave_exclusive_product_f64(j < M ? fT[j] : 1.0, lane, carry);
        if (j < M) fT[j] = T;
      }
    } else if (sweep == 1) {
      double sfx_carry = 0.0;
      for (int b0 = ((M - 1) >> 6) << 6; b0 >= 0; b0 -= 64) {
        const int j = b0 + lane;
        const double sfx = wave_exclusive_suffix_sum_f64(j < M ? gS[j] : 0.0, lane, sfx_carry);
        if (j < M) gS[j] = sfx;
      }
    }
    wave_lds_sync();
  }
}

DeviceOnce g_scene_grad_lds[3];

template <int ACT>
hipError_t launch_act(const SceneCompositeBwdArgs& a, int64_t grid, int waves, hipStream_t stream) {
  if (hipError_t e = set_max_lds(scene_composite_bwd_kernel<ACT>, kLdsBudget, g_scene_grad_lds[ACT]); e != hipSuccess) return e;
  scene_composite_bwd_kernel<ACT><<<dim3((unsigned)grid), dim3(64 * waves), (size_t)a.wave_bytes * waves, stream>>>(a);
  return hipGetLastError();
}

}  // namespace

int64_t scene_composite_bwd_wave_bytes(int K, int S) { return (kHeadBytes + (int64_t)K * S * kSampleBytes + 15) / 16 * 16; }

hipError_t launch_scene_composite_bwd(const float* raw, const float* t_vals, const int32_t* slot, const float* dirs, const float* g_rgb,
                                      const float* g_acc, const float* g_depth, const float* g_obj_acc, int64_t n, int K, int64_t pairs, int S,
                                      int white_bkgd, const ActParams& ap, float* d_raw, hipStream_t stream) {
  if (n <= 0 || pairs <= 0) return hipSuccess;
  const int64_t wave_bytes = scene_composite_bwd_wave_bytes(K, S);
  int waves = (int)(kLdsBudget / wave_bytes);
  if (waves < 1) return hipErrorInvalidValue;   // (K * S <= 4096: 90,368 B)
  waves = waves > 4 ? 4 : waves;
  SceneCompositeBwdArgs a{reinterpret_cast<const float4*>(raw), t_vals, slot, dirs, g_rgb, g_acc, g_depth, g_obj_acc, n, K, pairs, S, white_bkgd, ap,
                          reinterpret_cast<float4*>(d_raw), (int)wave_bytes};
  const int64_t grid = (n + waves - 1) / waves;
  return ap.act == 1 ? launch_act<1>(a, grid, waves, stream) : ap.act == 2 ? launch_act<2>(a, grid, waves, stream) : launch_act<0>(a, grid, waves, stream);
}

}  // namespace aon

extern "C" {

int aon_scene_composite_bwd(const float* raw, const float* t_vals, const int32_t* slot, const float* rays_d, const float* g_rgb, const float* g_acc,
                            const float* g_depth, const float* g_obj_acc, int64_t n, int k, int64_t pairs, int s, int white_bkgd, int act,
                            const aon_render_opts* opts, float* d_raw, void* stream) {
  if (n < 0 || pairs < 0 || k < 1 || k > AON_SCENE_MAX_OBJECTS || s < 2 || (int64_t)k * s > AON_SCENE_MAX_MERGED || act < 0 || act > 2)
    return fail(AON_E_INVALID, "aon_scene_composite_bwd: bad size / object count / act (1 <= k <= 16, s >= 2, k * s <= 4096)");
  if (!raw || !t_vals || !slot || !rays_d || !g_rgb || !d_raw) return fail(AON_E_INVALID, "aon_scene_composite_bwd: null pointer");
  if (reinterpret_cast<uintptr_t>(raw) & 15) return fail(AON_E_INVALID, "aon_scene_composite_bwd: raw must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_raw) & 15) return fail(AON_E_INVALID, "aon_scene_composite_bwd: d_raw must be 16-byte aligned");
  if (n == 0 || pairs == 0) return AON_OK;
  aon::ActParams ap = aon::default_act(act);
  if (opts) { ap.rgb_scale = opts->rgb_scale; ap.rgb_shift = opts->rgb_shift; ap.sigma_bias = opts->sigma_bias; }
  return check(aon::launch_scene_composite_bwd(raw, t_vals, slot, rays_d, g_rgb, g_acc, g_depth, g_obj_acc, n, k, pairs, s, white_bkgd, ap, d_raw,
                                               static_cast<hipStream_t>(stream)), "aon_scene_composite_bwd");
}

}  // extern "C"
