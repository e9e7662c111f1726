// The merged composite of a scene whose lists each carry their own activation and end rule (DESIGN.md section 4.21;
// include/aon_hip_scene_lists.h is the contract and tests/_scene_lists_ref.py an independent numpy copy): a vanilla NeRF behind the
// articulated objects reads relu / sigmoid and keeps the one-object composite's open last interval.
//
//   scene_composite_lists_kernel  scene_composite_kernel's shape (aon_scene.hip), a second kernel BESIDE it: one wavefront per ray, the t of
//                                 its live lists staged in LDS and every sample ranked by counting (aon_scene_merge.h), 1 - alpha + 1e-10
//                                 placed in rank order, the 64-wide product scan in rank order with a carry, the sums in a fixed order.
//                                 The k list records travel by value in the kernel arguments; the list loop is outermost and a list's
//                                 record is read once per list through a wave-uniform index, so the branches on act / open_end never
//                                 diverge inside a wave.
//
// Operation order of a sample's interval, as composite_kernel (aon_render.hip) has it: dn = ray_norm_f32 (aon_ray_core.h), then
// dist = (t_{i+1} - t_i) * dn, or for the last sample of an open list 1e10f * dn, or 0 for a closed one; then sigma * dist.
#include "../../include/aon_hip_scene_lists.h"
#include "aon_capi_util.h"
#include "aon_scene_merge.h"

using namespace aon::capi;

namespace aon {
namespace {

// Per wave in LDS, as scene_composite_kernel: the 256-byte head and 14 bytes per merged sample.
constexpr int kListSampleBytes = 14;
constexpr int kListLdsBudget = 64 * 1024;
int64_t lists_wave_bytes(int K, int S) { return align_up(kHeadBytes + (int64_t)K * S * kListSampleBytes, 16); }

struct SceneListRecs {   // by value in the kernel arguments (16 x 20 B): no device copy to keep alive, nothing for the host to wait for
  aon_scene_list r[kMaxObj];
};

struct SceneCompositeListsArgs {
  const float4* raw; const float* t_vals; const int32_t* slot; const float* dirs;
  int64_t n; int K; int64_t pairs; int S; int white_bkgd;
  float* rgb; float* acc; float* depth; float* obj_acc; float* weights;
  int wave_bytes;
  SceneListRecs lists;
};

__device__ __forceinline__ float list_sigma(int act, float sigma_bias, float sg) {
  if (act == 1) return __builtin_fmaxf(sg, 0.f);
  if (act == 2) return softplus_f32(__fadd_rn(sg, sigma_bias));
  return sg;
}
__device__ __forceinline__ float list_rgb(int act, float rgb_scale, float rgb_shift, float c) {
  if (act == 1) return sigmoid_f32(c);
  if (act == 2) return __fsub_rn(__fmul_rn(sigmoid_f32(c), rgb_scale), rgb_shift);
  return c;
}

__global__ __launch_bounds__(256) void scene_composite_lists_kernel(SceneCompositeListsArgs a) {
  extern __shared__ __attribute__((aligned(16))) char scene_lists_lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t ray = (int64_t)blockIdx.x * (blockDim.x >> 6) + wv;
  if (ray >= a.n) return;   // wave-uniform; no block-level barrier below
  const int K = a.K, S = a.S, MS = K * S;
  char* base = scene_lists_lds + (size_t)wv * a.wave_bytes;
  const SceneLists h(base);
  float* tl = reinterpret_cast<float*>(base + kHeadBytes);
  float* fT = tl + MS;
  float* al = fT + MS;
  unsigned short* rk = reinterpret_cast<unsigned short*>(al + MS);

  bool live;
  const int L = scene_live_lists(h, a.slot, a.t_vals, ray, K, a.pairs, S, lane, live);
  if (a.obj_acc && lane < K && !live) a.obj_acc[ray * K + lane] = 0.f;
  if (L == 0) {
    if (lane == 0) {
      const float bg = a.white_bkgd ? 1.0f : 0.f;
      a.rgb[ray * 3 + 0] = bg; a.rgb[ray * 3 + 1] = bg; a.rgb[ray * 3 + 2] = bg;
      a.acc[ray] = 0.f;
      a.depth[ray] = 0.f;
    }
    return;
  }
  scene_stage_t(h, tl, a.t_vals, L, S, lane);
  const float dn = ray_norm_f32(a.dirs, ray);
  const int M = L * S;
  for (int j = 0; j < L; ++j) {
    const int64_t row = (int64_t)h.lp[j] * S;
    // the list's record: h.lk[j] is the same in every lane (0 <= lk < K <= 16), so this is a scalar read of the kernel arguments
    const aon_scene_list& rec = a.lists.r[__builtin_amdgcn_readfirstlane(h.lk[j]) & (kMaxObj - 1)];
    const int act = rec.act;
    const float sigma_bias = rec.sigma_bias;
    const float last = rec.open_end ? __fmul_rn(1e10f, dn) : 0.f;
    for (int i = lane; i < S; i += 64) {
      const float t = tl[j * S + i];
      const float dist = i < S - 1 ? __fmul_rn(__fsub_rn(tl[j * S + i + 1], t), dn) : last;
      const float sg = list_sigma(act, sigma_bias, a.raw[row + i].w);
      const float alpha = __fsub_rn(1.0f, expf(-__fmul_rn(sg, dist)));
      const int rank = scene_rank(h, tl, t, i, j, L, S);
      fT[rank] = __fadd_rn(__fsub_rn(1.0f, alpha), 1e-10f);
      al[j * S + i] = alpha;
      rk[j * S + i] = (unsigned short)rank;
    }
  }
  wave_lds_sync();
  // T_j = prod_{m < j} (1 - alpha_m + 1e-10) in rank order: 64 at a time, the carry is everything before the block
  float carry = 1.0f;
  for (int b0 = 0; b0 < M; b0 += 64) {
    const int j = b0 + lane;
    const float f = j < M ? fT[j] : 1.0f;
    const float incl = wave_inclusive_scan<true>(f, lane);
    const float excl = dpp_f32<0x138, 0xf>(1.0f, incl);   // wave_shr:1, lane 0 keeps 1
    if (j < M) fT[j] = __fmul_rn(carry, excl);
    carry = __fmul_rn(carry, __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, incl), 63)));
  }
  wave_lds_sync();
  // the sums: per lane over (list, i) ascending, then one fixed tree over the lanes
  float s_r = 0.f, s_g = 0.f, s_b = 0.f, s_w = 0.f, s_d = 0.f;
  for (int j = 0; j < L; ++j) {
    const int64_t row = (int64_t)h.lp[j] * S;
    const int kj = __builtin_amdgcn_readfirstlane(h.lk[j]) & (kMaxObj - 1);
    const aon_scene_list& rec = a.lists.r[kj];
    const int act = rec.act;
    const float rgb_scale = rec.rgb_scale, rgb_shift = rec.rgb_shift;
    float s_o = 0.f;
    for (int i = lane; i < S; i += 64) {
      const int e = j * S + i;
      const float w = __fmul_rn(al[e], fT[rk[e]]);
      const float4 r = a.raw[row + i];
      s_r = __fadd_rn(s_r, __fmul_rn(w, list_rgb(act, rgb_scale, rgb_shift, r.x)));
      s_g = __fadd_rn(s_g, __fmul_rn(w, list_rgb(act, rgb_scale, rgb_shift, r.y)));
      s_b = __fadd_rn(s_b, __fmul_rn(w, list_rgb(act, rgb_scale, rgb_shift, r.z)));
      s_w = __fadd_rn(s_w, w);
      s_d = __fadd_rn(s_d, __fmul_rn(w, tl[e]));
      s_o = __fadd_rn(s_o, w);
      if (a.weights) a.weights[row + i] = w;
    }
    s_o = wave_sum(s_o);
    if (a.obj_acc && lane == 0) a.obj_acc[ray * K + kj] = s_o;
  }
  s_r = wave_sum(s_r); s_g = wave_sum(s_g); s_b = wave_sum(s_b); s_w = wave_sum(s_w); s_d = wave_sum(s_d);
  if (lane == 0) {
    if (a.white_bkgd) {   // rgb + (1 - acc)
      const float bg = __fsub_rn(1.0f, s_w);
      s_r = __fadd_rn(s_r, bg); s_g = __fadd_rn(s_g, bg); s_b = __fadd_rn(s_b, bg);
    }
    a.rgb[ray * 3 + 0] = s_r; a.rgb[ray * 3 + 1] = s_g; a.rgb[ray * 3 + 2] = s_b;
    a.acc[ray] = s_w;
    a.depth[ray] = s_d;
  }
}

}  // namespace
}  // namespace aon

extern "C" {

int aon_scene_composite_lists(const float* raw, const float* t_vals, const int32_t* slot, const float* rays_d, int64_t n, int k, int64_t pairs,
                              int s, int white_bkgd, const aon_scene_list* lists_host, float* rgb, float* acc, float* depth, float* obj_acc,
                              float* weights, void* stream) {
  if (n < 0 || pairs < 0 || k < 1 || k > AON_SCENE_MAX_OBJECTS || s < 2 || (int64_t)k * s > AON_SCENE_MAX_MERGED)
    return fail(AON_E_INVALID, "aon_scene_composite_lists: bad size / list count (1 <= k <= 16, s >= 2, k * s <= 4096)");
  if (!slot || !rays_d || !rgb || !acc || !depth || !lists_host || (pairs > 0 && (!raw || !t_vals)))
    return fail(AON_E_INVALID, "aon_scene_composite_lists: null pointer");
  for (int j = 0; j < k; ++j)
    if (lists_host[j].act < 0 || lists_host[j].act > 2 || lists_host[j].open_end < 0 || lists_host[j].open_end > 1)
      return fail(AON_E_INVALID, "aon_scene_composite_lists: bad list record (act in [0, 2], open_end 0 or 1)");
  if (reinterpret_cast<uintptr_t>(raw) & 15) return fail(AON_E_INVALID, "aon_scene_composite_lists: raw must be 16-byte aligned");
  if (n == 0) return AON_OK;
  const int64_t wave_bytes = aon::lists_wave_bytes(k, s);
  int waves = (int)(aon::kListLdsBudget / wave_bytes);
  waves = waves > 4 ? 4 : waves;   // (>= 1: 256 + 4096 * 14 = 57,600 B)
  aon::SceneCompositeListsArgs a{reinterpret_cast<const float4*>(raw), t_vals, slot, rays_d, n, k, pairs, s, white_bkgd, rgb, acc, depth, obj_acc, weights,
                                 (int)wave_bytes, {}};
  std::memset(&a.lists, 0, sizeof(a.lists));
  std::memcpy(a.lists.r, lists_host, sizeof(aon_scene_list) * k);
  const int64_t grid = (n + waves - 1) / waves;
  aon::scene_composite_lists_kernel<<<dim3((unsigned)grid), dim3(64 * waves), (size_t)(wave_bytes * waves), static_cast<hipStream_t>(stream)>>>(a);
  return check(hipGetLastError(), "aon_scene_composite_lists");
}

}  // extern "C"
