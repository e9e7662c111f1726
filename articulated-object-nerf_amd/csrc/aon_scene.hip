// Scenes of several posed articulated objects in one frame (include/aon_hip_scene.h is the contract and
// tests/_scene_ref.py an independent numpy copy): the two per-ray stages around the unchanged samplers and MLP kernels.
//
//   scene_pair_classify_kernel  one thread per ray: the K object-frame rays and slab tests -> a K-bit live mask per ray (4 B written) and per
//                               block of 256 rays one count per object (wave ballots + an LDS sum: no atomics);
//   scene_pair_scan_kernel      ONE workgroup: exclusive prefix over the (object, block) counts in object-major order -> each block's first
//                               row per object (in place) and the K + 1 segment starts;
//   scene_pair_emit_kernel      one thread per ray again: row = block base + rank among the block's live rays of that object (ballot ranks),
//                               so an object's rows ascend with the ray index; writes slot and the pair's ray, o', d', v', near, far.
//   scene_composite_kernel      one wavefront per ray: the t of its live lists staged in LDS and every sample ranked by counting
//                               (aon_scene_merge.h, shared with the backward), 1 - alpha + 1e-10 placed in rank order,
//                               a multiplicative wave scan in rank order in blocks of 64 with a carry, then the sums in a fixed order.
//
// Arithmetic of the pairs, operation by operation: R^T x as ((R[0][a] x_0) + R[1][a] x_1) + R[2][a] x_2 with separately rounded operations,
// then ray_box_kernel's slab test (csrc/aon_bounds.hip) restated on its torch_max / torch_min (aon_common.h) and ray_limits_finish_kernel's
// clamp-and-live rule without the set-wide patching.
#include "../../include/aon_hip_scene.h"
#include "aon_capi_util.h"
#include "aon_scene_merge.h"

using namespace aon::capi;

namespace aon {
namespace {

constexpr int kPairThreads = 256;

struct SceneObjects {   // by value in the kernel arguments (1152 B): no device copy to keep alive, nothing for the host to wait for
  aon_scene_object o[kMaxObj];
};

// component a of R^T x
__device__ __forceinline__ float rot_t(const float* R, int a, float x0, float x1, float x2) {
  return __fadd_rn(__fadd_rn(__fmul_rn(R[a], x0), __fmul_rn(R[3 + a], x1)), __fmul_rn(R[6 + a], x2));
}

// the object-frame origin and direction of a world ray, its clamped near / far; -> live
__device__ __forceinline__ bool object_ray(const aon_scene_object& ob, const float (&o)[3], const float (&d)[3], float (&oo)[3], float (&od)[3],
                                           float& near_, float& far_) {
  const float s0 = __fsub_rn(o[0], ob.centre[0]), s1 = __fsub_rn(o[1], ob.centre[1]), s2 = __fsub_rn(o[2], ob.centre[2]);
  float t0[3], t1[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    oo[a] = rot_t(ob.rot, a, s0, s1, s2);
    od[a] = rot_t(ob.rot, a, d[0], d[1], d[2]);
    const float inv = __fdiv_rn(1.0f, od[a]);
    const bool neg = inv < 0.f;
    t0[a] = __fmul_rn(__fsub_rn(neg ? ob.hi[a] : ob.lo[a], oo[a]), inv);
    t1[a] = __fmul_rn(__fsub_rn(neg ? ob.lo[a] : ob.hi[a], oo[a]), inv);
  }
  bool valid = !(t0[0] > t1[1] || t0[1] > t1[0]);
  float tmin = torch_max(t0[0], t0[1]), tmax = torch_min(t1[0], t1[1]);
  if (tmin > t1[2] || t0[2] > tmax) valid = false;
  tmin = torch_max(tmin, t0[2]);
  tmax = torch_min(tmax, t1[2]);
  if (!valid) { tmin = -1.0f; tmax = -2.0f; }
  const bool hit = tmax > tmin;   // (false for a NaN)
  if (tmin < 0.f) tmin = 0.f;
  if (tmax < 0.f) tmax = 0.f;
  near_ = tmin;
  far_ = tmax;
  return hit && tmax > tmin;
}

__global__ __launch_bounds__(kPairThreads) void scene_pair_classify_kernel(const float* __restrict__ rays_o, const float* __restrict__ rays_d, int64_t n,
                                                                           SceneObjects objs, int K, int64_t blocks, uint32_t* __restrict__ mask,
                                                                           int32_t* __restrict__ counts) {
  __shared__ int cnt[kPairThreads / 64][kMaxObj];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t ray = (int64_t)blockIdx.x * kPairThreads + threadIdx.x;
  const bool in = ray < n;
  float o[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 0.f};
  if (in) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { o[a] = rays_o[ray * 3 + a]; d[a] = rays_d[ray * 3 + a]; }
  }
  uint32_t bits = 0;
  for (int k = 0; k < K; ++k) {   // (uniform)
    float oo[3], od[3], nr, fr;
    const bool live = in && object_ray(objs.o[k], o, d, oo, od, nr, fr);
    if (live) bits |= 1u << k;
    const int c = __builtin_popcountll(__builtin_amdgcn_ballot_w64(live));
    if (lane == 0) cnt[wave][k] = c;
  }
  if (in) mask[ray] = bits;
  __syncthreads();
  if ((int)threadIdx.x < K) {
    int c = 0;
#pragma unroll
    for (int w = 0; w < kPairThreads / 64; ++w) c += cnt[w][threadIdx.x];
    counts[(int64_t)threadIdx.x * blocks + blockIdx.x] = c;
  }
}

// counts[k * blocks + b] -> the exclusive prefix over all entries in that order (in place); offsets[k] = the prefix at entry k * blocks,
// offsets[K] = the total
__global__ __launch_bounds__(kPairThreads) void scene_pair_scan_kernel(int32_t* __restrict__ counts, int64_t blocks, int K, int64_t* __restrict__ offsets) {
  __shared__ int64_t part[kPairThreads];
  const int64_t total = blocks * K;
  const int64_t per = (total + kPairThreads - 1) / kPairThreads;
  const int64_t e0 = (int64_t)threadIdx.x * per, e1 = e0 + per < total ? e0 + per : total;
  int64_t sum = 0;
  for (int64_t e = e0; e < e1; ++e) sum += counts[e];
  part[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {   // 256 additions: the order is the index order, the same on every run
    int64_t run = 0;
    for (int i = 0; i < kPairThreads; ++i) { const int64_t c = part[i]; part[i] = run; run += c; }
    offsets[K] = run;
  }
  __syncthreads();
  int64_t run = part[threadIdx.x];
  for (int64_t e = e0; e < e1; ++e) {
    const int32_t c = counts[e];
    counts[e] = (int32_t)run;
    if (e % blocks == 0) offsets[e / blocks] = run;
    run += c;
  }
}

__global__ __launch_bounds__(kPairThreads) void scene_pair_emit_kernel(const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                                       const float* __restrict__ viewdirs, int64_t n, SceneObjects objs, int K,
                                                                       int64_t blocks, const uint32_t* __restrict__ mask, const int32_t* __restrict__ bases,
                                                                       int32_t* __restrict__ slot, int32_t* __restrict__ pair_ray, float* __restrict__ pair_o,
                                                                       float* __restrict__ pair_d, float* __restrict__ pair_v, float* __restrict__ pair_near,
                                                                       float* __restrict__ pair_far) {
  __shared__ int cnt[kPairThreads / 64][kMaxObj];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t ray = (int64_t)blockIdx.x * kPairThreads + threadIdx.x;
  const bool in = ray < n;
  const uint32_t bits = in ? mask[ray] : 0u;
  for (int k = 0; k < K; ++k) {
    const int c = __builtin_popcountll(__builtin_amdgcn_ballot_w64((bits >> k) & 1u));
    if (lane == 0) cnt[wave][k] = c;
  }
  __syncthreads();
  if (!in) return;   // (no barrier below)
  float o[3], d[3], v[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) { o[a] = rays_o[ray * 3 + a]; d[a] = rays_d[ray * 3 + a]; v[a] = viewdirs[ray * 3 + a]; }
  const uint64_t below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  for (int k = 0; k < K; ++k) {
    const bool live = (bits >> k) & 1u;
    // (the ballot is taken by every lane still here: the lanes past n left with bits = 0 and count as dead)
    const uint64_t bal = __builtin_amdgcn_ballot_w64(live);
    int32_t row = -1;
    if (live) {
      int before = __builtin_popcountll(bal & below);
      for (int w = 0; w < wave; ++w) before += cnt[w][k];
      row = bases[(int64_t)k * blocks + blockIdx.x] + before;
      float oo[3], od[3], nr, fr;
      object_ray(objs.o[k], o, d, oo, od, nr, fr);
      pair_ray[row] = (int32_t)ray;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        pair_o[(int64_t)row * 3 + a] = oo[a];
        pair_d[(int64_t)row * 3 + a] = od[a];
        pair_v[(int64_t)row * 3 + a] = rot_t(objs.o[k].rot, a, v[0], v[1], v[2]);
      }
      pair_near[row] = nr;
      pair_far[row] = fr;
    }
    slot[ray * K + k] = row;
  }
}

int64_t pair_blocks(int64_t n) { return (n + kPairThreads - 1) / kPairThreads; }
int64_t pair_mask_bytes(int64_t n) { return align_up((n > 0 ? n : 1) * 4, 256); }
int64_t pair_count_bytes(int64_t n, int k) { return align_up((n > 0 ? pair_blocks(n) : 1) * k * 4, 256); }

// ---------------------------------------------------------------------------------------------
// the merged composite
// ---------------------------------------------------------------------------------------------
// Per wave in LDS: the head of the live lists (aon_scene_merge.h) and, per sample of the K * S the call admits, 14 bytes:
// t in list layout, 1 - alpha + 1e-10 -> T in RANK order, alpha and the rank (16 bits: K * S <= 4096) in list layout.
constexpr int kSampleBytes = 14;
constexpr int kLdsBudget = 64 * 1024;
int64_t composite_wave_bytes(int K, int S) { return align_up(kHeadBytes + (int64_t)K * S * kSampleBytes, 16); }

struct SceneCompositeArgs {
  const float4* raw; const float* t_vals; const int32_t* slot; const float* dirs;
  int64_t n; int K; int64_t pairs; int S; int white_bkgd; ActParams ap;
  float* rgb; float* acc; float* depth; float* obj_acc; float* weights;
  int wave_bytes;
};

__device__ __forceinline__ float scene_sigma(const ActParams& ap, float sg) {
  if (ap.act == 1) return __builtin_fmaxf(sg, 0.f);
  if (ap.act == 2) return softplus_f32(__fadd_rn(sg, ap.sigma_bias));
  return sg;
}
__device__ __forceinline__ float scene_rgb(const ActParams& ap, float c) {
  if (ap.act == 1) return sigmoid_f32(c);
  if (ap.act == 2) return __fsub_rn(__fmul_rn(sigmoid_f32(c), ap.rgb_scale), ap.rgb_shift);
  return c;
}

__global__ __launch_bounds__(256) void scene_composite_kernel(SceneCompositeArgs a) {
  extern __shared__ __attribute__((aligned(16))) char scene_lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t ray = (int64_t)blockIdx.x * (blockDim.x >> 6) + wv;
  if (ray >= a.n) return;   // wave-uniform; no block-level barrier below
  const int K = a.K, S = a.S, MS = K * S;
  char* base = scene_lds + (size_t)wv * a.wave_bytes;
  const SceneLists h(base);
  float* tl = reinterpret_cast<float*>(base + kHeadBytes);
  float* fT = tl + MS;
  float* al = fT + MS;
  unsigned short* rk = reinterpret_cast<unsigned short*>(al + MS);
  const ActParams ap = a.ap;

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
    for (int i = lane; i < S; i += 64) {
      const float t = tl[j * S + i];
      const float dist = i < S - 1 ? __fmul_rn(__fsub_rn(tl[j * S + i + 1], t), dn) : 0.f;
      const float sg = scene_sigma(ap, a.raw[row + i].w);
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
    float s_o = 0.f;
    for (int i = lane; i < S; i += 64) {
      const int e = j * S + i;
      const float w = __fmul_rn(al[e], fT[rk[e]]);
      const float4 r = a.raw[row + i];
      s_r = __fadd_rn(s_r, __fmul_rn(w, scene_rgb(ap, r.x)));
      s_g = __fadd_rn(s_g, __fmul_rn(w, scene_rgb(ap, r.y)));
      s_b = __fadd_rn(s_b, __fmul_rn(w, scene_rgb(ap, r.z)));
      s_w = __fadd_rn(s_w, w);
      s_d = __fadd_rn(s_d, __fmul_rn(w, tl[e]));
      s_o = __fadd_rn(s_o, w);
      if (a.weights) a.weights[row + i] = w;
    }
    s_o = wave_sum(s_o);
    if (a.obj_acc && lane == 0) a.obj_acc[ray * K + h.lk[j]] = s_o;
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

int64_t aon_scene_pairs_workspace_bytes(int64_t n, int k) {
  if (n < 0 || k < 1 || k > AON_SCENE_MAX_OBJECTS) return 0;
  return aon::pair_mask_bytes(n) + aon::pair_count_bytes(n, k);
}

int aon_scene_pairs(const float* rays_o, const float* rays_d, const float* viewdirs, int64_t n, const aon_scene_object* objects_host, int k,
                    void* workspace, int64_t workspace_bytes, int64_t* offsets, int32_t* slot, int32_t* pair_ray, float* pair_o, float* pair_d,
                    float* pair_v, float* pair_near, float* pair_far, void* stream_) {
  if (n < 0 || k < 1 || k > AON_SCENE_MAX_OBJECTS || n > (int64_t)0x7fffffff / k) return fail(AON_E_INVALID, "aon_scene_pairs: bad size / object count");
  if (!rays_o || !rays_d || !viewdirs || !objects_host || !workspace || !offsets || !slot || !pair_ray || !pair_o || !pair_d || !pair_v || !pair_near ||
      !pair_far)
    return fail(AON_E_INVALID, "aon_scene_pairs: null pointer");
  if (reinterpret_cast<uintptr_t>(workspace) & 255) return fail(AON_E_INVALID, "aon_scene_pairs: workspace must be 256-byte aligned");
  if (workspace_bytes < aon_scene_pairs_workspace_bytes(n, k)) return fail(AON_E_WORKSPACE, "aon_scene_pairs: workspace smaller than aon_scene_pairs_workspace_bytes()");
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (n == 0) return check(hipMemsetAsync(offsets, 0, sizeof(int64_t) * (k + 1), stream), "aon_scene_pairs");
  aon::SceneObjects objs;
  std::memset(&objs, 0, sizeof(objs));
  std::memcpy(objs.o, objects_host, sizeof(aon_scene_object) * k);
  const int64_t blocks = aon::pair_blocks(n);
  uint32_t* mask = static_cast<uint32_t*>(workspace);
  int32_t* counts = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + aon::pair_mask_bytes(n));
  const dim3 grid((unsigned)blocks), block(aon::kPairThreads);
  aon::scene_pair_classify_kernel<<<grid, block, 0, stream>>>(rays_o, rays_d, n, objs, k, blocks, mask, counts);
  if (int rc = check(hipGetLastError(), "aon_scene_pairs (classify)")) return rc;
  aon::scene_pair_scan_kernel<<<dim3(1), block, 0, stream>>>(counts, blocks, k, offsets);
  if (int rc = check(hipGetLastError(), "aon_scene_pairs (scan)")) return rc;
  aon::scene_pair_emit_kernel<<<grid, block, 0, stream>>>(rays_o, rays_d, viewdirs, n, objs, k, blocks, mask, counts, slot, pair_ray, pair_o, pair_d,
                                                         pair_v, pair_near, pair_far);
  return check(hipGetLastError(), "aon_scene_pairs (emit)");
}

int aon_scene_composite(const float* raw, const float* t_vals, const int32_t* slot, const float* rays_d, int64_t n, int k, int64_t pairs, int s,
                        int white_bkgd, int act, const aon_render_opts* opts, float* rgb, float* acc, float* depth, float* obj_acc, float* weights,
                        void* stream) {
  if (n < 0 || pairs < 0 || k < 1 || k > AON_SCENE_MAX_OBJECTS || s < 2 || (int64_t)k * s > AON_SCENE_MAX_MERGED || act < 0 || act > 2)
    return fail(AON_E_INVALID, "aon_scene_composite: bad size / object count / act (1 <= k <= 16, s >= 2, k * s <= 4096)");
  if (!slot || !rays_d || !rgb || !acc || !depth || (pairs > 0 && (!raw || !t_vals))) return fail(AON_E_INVALID, "aon_scene_composite: null pointer");
  if (reinterpret_cast<uintptr_t>(raw) & 15) return fail(AON_E_INVALID, "aon_scene_composite: raw must be 16-byte aligned");
  if (n == 0) return AON_OK;
  aon::ActParams ap = aon::default_act(act);
  if (opts) { ap.rgb_scale = opts->rgb_scale; ap.rgb_shift = opts->rgb_shift; ap.sigma_bias = opts->sigma_bias; }
  const int64_t wave_bytes = aon::composite_wave_bytes(k, s);
  int waves = (int)(aon::kLdsBudget / wave_bytes);
  waves = waves > 4 ? 4 : waves;   // (>= 1: 256 + 4096 * 14 = 57,600 B)
  aon::SceneCompositeArgs a{reinterpret_cast<const float4*>(raw), t_vals, slot, rays_d, n, k, pairs, s, white_bkgd, ap, rgb, acc, depth, obj_acc, weights,
                            (int)wave_bytes};
  const int64_t grid = (n + waves - 1) / waves;
  aon::scene_composite_kernel<<<dim3((unsigned)grid), dim3(64 * waves), (size_t)(wave_bytes * waves), static_cast<hipStream_t>(stream)>>>(a);
  return check(hipGetLastError(), "aon_scene_composite");
}

}  // extern "C"
