// Backward of the merged scene composite (include/aon_hip_scene_grad.h is the contract and tests/_scene_grad_ref.py an
// independent torch fp64 restatement): d(rgb, acc, depth, obj_acc) -> d raw per sample of every live pair.
//
//   scene_composite_bwd_kernel  one wavefront per ray, as scene_composite_kernel (csrc/aon_scene.hip): the t of its live lists staged in LDS,
//                               every sample ranked by counting with the forward's rule (restated here: aon_scene.hip stays untouched, and
//                               tests/test_hip_scene_grad.py pins the two against one another through ties, duplicates and the bit tests),
//                               f = 1 - alpha + 1e-10 placed in RANK order and turned into T by a multiplicative scan in blocks of 64 with a
//                               carry, w gw placed in rank order and turned into Sfx by an additive scan from the far end, then every sample
//                               fetches its T and Sfx by rank and writes one float4.
//
// Arithmetic as composite_bwd_kernel (csrc/aon_train.hip, whose header says why): everything in fp64 on the fp32 inputs, the fp32 operations
// that are part of the function (the interval lengths, the norm, raw + sigma_bias) in fp32, one rounding per output.  Both scans run in a
// fixed order over the ray's own merged list; no atomics: a ray's d_raw rows are a function of its own lists only.  alpha, the colours and
// the derivatives are recomputed from raw and t in each of the three sweeps rather than stored: per sample the kernel reads 20 bytes (its
// record three times, from the cache after the first) and writes 16.
#include "../../include/aon_hip_scene_grad.h"
#include "aon_capi_util.h"
#include "aon_ray_core.h"

using namespace aon::capi;

namespace aon {
namespace {

constexpr int kMaxObj = AON_SCENE_MAX_OBJECTS;
// Per wave in LDS: a 256-byte head (the live lists' rows, objects, first and last t) and 22 bytes per sample of the K * S the call admits:
// two doubles in RANK order (f -> T;  w gw -> Sfx), t and the rank (16 bits: K * S <= 4096) in list layout.  90,368 B at the limit: above
// the 64 KiB a kernel gets by default, below the 160 KiB a workgroup may use on gfx950 (set_max_lds, aon_common.h).
constexpr int kHeadBytes = 256;
constexpr int kSampleBytes = 22;
constexpr int kLdsBudget = 160 * 1024;

struct SceneCompositeBwdArgs {
  const float4* raw; const float* t_vals; const int32_t* slot; const float* dirs;
  const float* g_rgb; const float* g_acc; const float* g_depth; const float* g_obj_acc;
  int64_t n; int K; int64_t pairs; int S; int white_bkgd; ActParams ap;
  float4* d_raw;
  int wave_bytes;
};

__device__ __forceinline__ double sigmoid_f64(double x) { return 1.0 / (1.0 + exp(-x)); }

// One sample, recomputed from its record: the activations and their derivatives exactly as composite_bwd_kernel takes them
struct SampleD {
  double alpha, f, kf;      // 1 - exp(-sigma delta);  1 - alpha + 1e-10;  d alpha / d raw_sigma
  double c0, c1, c2;        // the colours
  double d0, d1, d2;        // d colour / d raw
};

// (ACT is a template argument: with `act` read at run time the compiler kept a three-entry table of the branches' results in scratch)
template <int ACT>
__device__ __forceinline__ void density(const ActParams& ap, float rw, float dist32, SampleD& s) {
  double sg, dsg;
  if constexpr (ACT == 1) {
    sg = rw > 0.f ? (double)rw : 0.0; dsg = rw > 0.f ? 1.0 : 0.0;
  } else if constexpr (ACT == 2) {
    const float xs = __fadd_rn(rw, ap.sigma_bias);   // (an fp32 add in the forward: part of the function)
    sg = xs > 20.0f ? (double)xs : log1p(exp((double)xs)); dsg = xs > 20.0f ? 1.0 : sigmoid_f64(xs);   // torch Softplus, threshold 20
  } else {
    sg = rw; dsg = 1.0;
  }
  const double dist = dist32;
  const double ex = exp(-sg * dist);
  s.alpha = 1.0 - ex;
  s.f = (1.0 - s.alpha) + 1e-10;
  s.kf = dist * ex * dsg;
}

template <int ACT>
__device__ __forceinline__ void colours(const ActParams& ap, const float4& r, SampleD& s) {
  if constexpr (ACT == 1) {
    s.c0 = sigmoid_f64(r.x); s.c1 = sigmoid_f64(r.y); s.c2 = sigmoid_f64(r.z);
    s.d0 = s.c0 * (1.0 - s.c0); s.d1 = s.c1 * (1.0 - s.c1); s.d2 = s.c2 * (1.0 - s.c2);
  } else if constexpr (ACT == 2) {
    const double s0 = sigmoid_f64(r.x), s1 = sigmoid_f64(r.y), s2 = sigmoid_f64(r.z);
    const double sc = ap.rgb_scale, sh = ap.rgb_shift;
    s.c0 = s0 * sc - sh; s.c1 = s1 * sc - sh; s.c2 = s2 * sc - sh;
    s.d0 = sc * s0 * (1.0 - s0); s.d1 = sc * s1 * (1.0 - s1); s.d2 = sc * s2 * (1.0 - s2);
  } else {
    s.c0 = r.x; s.c1 = r.y; s.c2 = r.z; s.d0 = s.d1 = s.d2 = 1.0;
  }
}

template <int ACT>
__global__ __launch_bounds__(256) void scene_composite_bwd_kernel(SceneCompositeBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) char scene_grad_lds[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t ray = (int64_t)blockIdx.x * (blockDim.x >> 6) + wv;
  if (ray >= a.n) return;   // wave-uniform; no block-level barrier below
  const int K = a.K, S = a.S, MS = K * S;
  char* base = scene_grad_lds + (size_t)wv * a.wave_bytes;
  int* lp = reinterpret_cast<int*>(base);        // row of live list j
  int* lk = lp + kMaxObj;                         // its object
  float* llo = reinterpret_cast<float*>(lk + kMaxObj);   // its first and last t
  float* lhi = llo + kMaxObj;
  double* fT = reinterpret_cast<double*>(base + kHeadBytes);   // RANK order: f, then T
  double* gS = fT + MS;                                        // RANK order: w gw, then Sfx
  float* tl = reinterpret_cast<float*>(gS + MS);               // list layout
  unsigned short* rk = reinterpret_cast<unsigned short*>(tl + MS);
  const ActParams ap = a.ap;

  // the head: scene_composite_kernel's, word for word
  int p = -1;
  if (lane < K) p = a.slot[ray * K + lane];
  const bool live = p >= 0 && p < a.pairs;   // (a row past `pairs` is nobody's: treated as dead, never dereferenced)
  const uint64_t m = __builtin_amdgcn_ballot_w64(live);
  const int L = __builtin_popcountll(m);
  if (L == 0) return;   // no pair: no row of d_raw is this ray's
  if (live) {
    const int j = __builtin_popcountll(m & (lane == 0 ? 0ull : (~0ull >> (64 - lane))));
    lp[j] = p;
    lk[j] = lane;
    llo[j] = a.t_vals[(int64_t)p * S];
    lhi[j] = a.t_vals[(int64_t)p * S + S - 1];
  }
  wave_lds_sync();
  for (int j = 0; j < L; ++j) {
    const float* tv = a.t_vals + (int64_t)lp[j] * S;
    for (int i = lane; i < S; i += 64) tl[j * S + i] = tv[i];
  }
  wave_lds_sync();
  // ||d|| as the forward takes it (fp32): the interval lengths are INPUTS of the function being differentiated
  const float dn = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(a.dirs[ray * 3], a.dirs[ray * 3]), __fmul_rn(a.dirs[ray * 3 + 1], a.dirs[ray * 3 + 1])),
                                        __fmul_rn(a.dirs[ray * 3 + 2], a.dirs[ray * 3 + 2])));
  const int M = L * S;
  const double gC0 = a.g_rgb[ray * 3], gC1 = a.g_rgb[ray * 3 + 1], gC2 = a.g_rgb[ray * 3 + 2];
  const double gA = a.g_acc ? (double)a.g_acc[ray] : 0.0, gD = a.g_depth ? (double)a.g_depth[ray] : 0.0;
  // dL/dw_j = gC.c_j + g_acc - [white] sum(gC) + t_j g_depth + g_obj_acc[ray, object of j]      (rgb += 1 - acc)
  const double gw_const = gA - (a.white_bkgd ? (gC0 + gC1 + gC2) : 0.0);

  // Three sweeps over the samples in list layout, one loop body (so that the fp64 exp / log1p code exists once): alpha, the colours and the
  // derivatives are recomputed from raw and t in each.
  //   sweep 0  rank by counting, the forward's rule: own index + in every other list the number of keys (t, object, i) below this one,
  //            t <= mine in a list of a lower object, t < mine in a list of a higher one.  0 <= rank <= M - 1 whatever the t hold.
  //            f in rank order; then T_j = prod_{m < j} f_m: 64 at a time, the carry is everything before the block
  //   sweep 1  w gw in rank order; then Sfx_j = sum_{m > j} w_m gw_m, scanned from the far end
  //   sweep 2  dL/dalpha_j = T_j gw_j - Sfx_j / f_j, and one float4 per sample.  A factor that is exactly zero (w: alpha = 0 at the last
  //            sample of a list and at a sentinel record; d alpha / d raw_sigma likewise) gives +0, not the -0 or NaN of 0 x (something
  //            negative or not finite).
#pragma nounroll
  for (int sweep = 0; sweep < 3; ++sweep) {
    for (int j = 0; j < L; ++j) {
      const int64_t row = (int64_t)lp[j] * S;
      const int kj = lk[j];
      const double gO = a.g_obj_acc ? (double)a.g_obj_acc[ray * K + kj] : 0.0;
      for (int i = lane; i < S; i += 64) {
        const int e = j * S + i;
        const float t = tl[e];
        const float dist = i < S - 1 ? __fmul_rn(__fsub_rn(tl[e + 1], t), dn) : 0.f;
        const float4 r = a.raw[row + i];
        SampleD s;
        density<ACT>(ap, r.w, dist, s);
        if (sweep == 0) {
          int rank = i;
          for (int b = 0; b < L; ++b) {
            if (b == j) continue;
            if (t < llo[b]) continue;                  // wholly behind this sample
            if (t > lhi[b]) { rank += S; continue; }   // wholly in front of it
            const bool le = lk[b] < kj;
            const float* x = tl + b * S;
            int lo = 0, hi = S;
            while (lo < hi) {
              const int mid = (lo + hi) >> 1;
              const float xm = x[mid];
              if (le ? xm <= t : xm < t) lo = mid + 1; else hi = mid;
            }
            rank += lo;
          }
          fT[rank] = s.f;
          rk[e] = (unsigned short)rank;
          continue;
        }
        colours<ACT>(ap, r, s);
        const int rank = rk[e];
        const double T = fT[rank];
        const double gw = gC0 * s.c0 + gC1 * s.c1 + gC2 * s.c2 + gw_const + (double)t * gD + gO;
        const double w = s.alpha * T;
        if (sweep == 1) {
          gS[rank] = w * gw;
          continue;
        }
        const double dalpha = T * gw - gS[rank] / s.f;
        float4 o;
        o.x = w == 0.0 ? 0.f : (float)(w * gC0 * s.d0);
        o.y = w == 0.0 ? 0.f : (float)(w * gC1 * s.d1);
        o.z = w == 0.0 ? 0.f : (float)(w * gC2 * s.d2);
        o.w = s.kf == 0.0 ? 0.f : (float)(dalpha * s.kf);
        a.d_raw[row + i] = o;
      }
    }
    wave_lds_sync();
    if (sweep == 0) {
      double carry = 1.0;
      for (int b0 = 0; b0 < M; b0 += 64) {
        const int j = b0 + lane;
        double incl = j < M ? fT[j] : 1.0;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const double o = __shfl_up(incl, off);
          if (lane >= off) incl = incl * o;
        }
        double excl = __shfl_up(incl, 1);
        if (lane == 0) excl = 1.0;
        if (j < M) fT[j] = carry * excl;
        carry = carry * __shfl(incl, 63);
      }
    } else if (sweep == 1) {
      double sfx_carry = 0.0;
      for (int b0 = ((M - 1) >> 6) << 6; b0 >= 0; b0 -= 64) {
        const int j = b0 + lane;
        double incl = j < M ? gS[j] : 0.0;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const double o = __shfl_down(incl, off);
          if (lane + off < 64) incl = incl + o;
        }
        double excl = __shfl_down(incl, 1);
        if (lane == 63) excl = 0.0;
        if (j < M) gS[j] = excl + sfx_carry;
        sfx_carry = sfx_carry + __shfl(incl, 0);
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
