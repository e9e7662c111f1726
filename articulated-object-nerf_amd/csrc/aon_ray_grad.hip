// Ray gradients of a FROZEN articulated network: dL/d rays_o, dL/d rays_d and dL/d viewdirs from what the backward
// chain (aon_train_art.hip) already leaves behind -- d x' per sample (ChainSeg::dxp) and the pre-activation gradients of
// deformations_linear.0 and views_linear.0 in the gradient planes.  Two ordinary launches on the caller's stream, both levels in each; no
// MFMA, no atomics, nothing that depends on the launch geometry.
//
//   x_i = o + t_i d (t is data: the coarse t depends on near / far only, the fine t is detached, helper.py:249):
//     g_x_i = dxp_i + W_d0[:, 0:3]^T dZ_d0,i          g_o = sum_i g_x_i          g_d = sum_i t_i g_x_i + g_n d / |d|
//   viewdirs enters through pos_enc(viewdirs, 0, deg_view), a constant of the ray:
//     g_ve = sum_i W_v0[:, view-encoding columns]^T dZ_v0,i   g_viewdirs = g_ve pulled back through the encoding at the forward's rounded arguments
//   |d| scales the interval lengths of the compositing (helper.py:167):
//     g_n = sum_i dL/dalpha_i (1 - alpha_i) sigma_i delta_i     (fp64 from raw, t, dirs and the upstream gradients: aon_composite_grad.h)
//
//   ray_grad_sample_kernel   lane = sample.  A sample's 128 values of a layer are 32 units of 16 B, 512 B apart inside its step; the 32
//                            samples of a step sit side by side, so a wave's load is two whole 512-byte runs.  3 + 27 fused multiply-add
//                            chains over the 128 features in ascending order against weight columns held in LDS; one 128-byte record
//                            {g_x (3), view-encoding partials (27), 0, 0} per sample.
//   ray_grad_reduce_kernel   one wavefront per ray.  Lane c < 32 sums component c of the ray's records in fp64, sample after sample in
//                            ascending order; lane 32 + c the same values times t_i.  Then the norm term (aon_composite_grad.h with d alpha / d |d|)
//                            and the view encoding's backward; every output is rounded to fp32 once.
//   ray_grad_reduce_plain_kernel   the same reduce without the norm term, for ONE level of one block of rays from the stage calls (DESIGN.md
//                            section 4.20: a scene's pair segments, whose interval lengths come from the WORLD direction).
//   vanilla_ray_grad_sample_kernel   the frozen VANILLA network's records for the same reduce kernel (described at the kernel).
#include "aon_art_common.h"
#include "aon_composite_grad.h"
#include "aon_launch.h"

namespace aon {

namespace {

constexpr int kRecFloats = 32;    // g_x at 0..2, the view-encoding partials at 3..29
constexpr int kRecView = 3;
constexpr int kWvCols = 28;       // 27 view-encoding columns padded to whole float4s

struct RgSampleSeg {
  const float* dplanes;   // the level's gradient planes (chain output)
  const float* dxp;       // (Np,4)
  const float* Wd0;       // deformations_linear.0.weight (128, kApDeform0Ld)
  const float* Wv0;       // views_linear.0.weight (128, ap_view0_ld(V))
  float* rec;             // (n * S, 32)
  int64_t nvalid;         // n * S: padding samples are neither read nor written
  int blk_begin;
};
struct RgSampleArgs {
  RgSampleSeg seg[2];
  int nsegs, V;
};

__global__ void __launch_bounds__(256) ray_grad_sample_kernel(RgSampleArgs a) {
  __shared__ __attribute__((aligned(16))) float wd[128 * 4];
  __shared__ __attribute__((aligned(16))) float wv[128 * kWvCols];
  const int tid = (int)threadIdx.x;
  const int si = (a.nsegs > 1 && (int)blockIdx.x >= a.seg[1].blk_begin) ? 1 : 0;
  const RgSampleSeg& S = a.seg[si];
  const int ldv = ap_view0_ld(a.V);
  for (int i = tid; i < 128 * 4; i += 256) wd[i] = (i & 3) < 3 ? S.Wd0[(i >> 2) * kApDeform0Ld + (i & 3)] : 0.f;
  for (int i = tid; i < 128 * kWvCols; i += 256) {
    const int f = i / kWvCols, c = i % kWvCols;
    wv[i] = c < a.V ? S.Wv0[(int64_t)f * ldv + kView0EncCol + c] : 0.f;
  }
  __syncthreads();
  const int64_t n = (int64_t)((int)blockIdx.x - S.blk_begin) * 256 + tid;
  if (n >= S.nvalid) return;
  // feature row f of sample n: ((n >> 5) * (rows / 4) + (f >> 2)) * 128 + (n & 31) * 4 + (f & 3)   (aon_mlp_core.h)
  const float* base = S.dplanes + (n >> 5) * ((int64_t)kAPlRows * 32) + (int)(n & 31) * 4;
  const float* pd = base + (aplane_d(0) / 4) * 128;
  const float* pv = base + (aplane_v(0) / 4) * 128;
  float out[kRecFloats];
#pragma unroll
  for (int k = 0; k < kRecFloats; ++k) out[k] = 0.f;
#pragma unroll 4
  for (int u = 0; u < 32; ++u) {
    const f32x4 z = *reinterpret_cast<const f32x4*>(pd + u * 128);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 w = *reinterpret_cast<const f32x4*>(wd + (4 * u + j) * 4);
#pragma unroll
      for (int k = 0; k < 3; ++k) out[k] = __builtin_fmaf(w[k], z[j], out[k]);
    }
  }
#pragma unroll 2
  for (int u = 0; u < 32; ++u) {
    const f32x4 z = *reinterpret_cast<const f32x4*>(pv + u * 128);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int q = 0; q < kWvCols / 4; ++q) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(wv + (4 * u + j) * kWvCols + 4 * q);
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (4 * q + k < 27) out[kRecView + 4 * q + k] = __builtin_fmaf(w[k], z[j], out[kRecView + 4 * q + k]);
      }
    }
  }
  const f32x4 dx = *reinterpret_cast<const f32x4*>(S.dxp + n * 4);   // x' = deformation_layer(..) + x: the identity path
#pragma unroll
  for (int k = 0; k < 3; ++k) out[k] = __fadd_rn(dx[k], out[k]);
  f32x4* dst = reinterpret_cast<f32x4*>(S.rec + n * kRecFloats);
#pragma unroll
  for (int q = 0; q < kRecFloats / 4; ++q) {
    f32x4 v; v[0] = out[4 * q]; v[1] = out[4 * q + 1]; v[2] = out[4 * q + 2]; v[3] = out[4 * q + 3];
    dst[q] = v;
  }
}

struct RgReduceLevel {
  const float* rec; const float* t; const float* raw;
  const float* g_rgb; const float* g_acc; const float* g_depth;
  ActParams ap;
  int S;
};
struct RgReduceArgs {
  RgReduceLevel lvl[2];
  int nlevels, white_bkgd, Lv;
  int64_t n_rays;
  const float* rays_d; const float* viewdirs;
  float* g_o; float* g_d; float* g_v;
};

// g_n of one ray at one level: the compositing backward (aon_composite_grad.h) with dalpha_i / d|d| = (1 - alpha_i) sigma_i delta_i in the
// place of dalpha_i / d raw_sigma_i.  fp64 on the forward's fp32 inputs; the same value in every lane.
template <int NB>
__device__ __forceinline__ double rg_norm_term(const RgReduceLevel& L, const int64_t ray, const int lane, const float dn, const int white_bkgd) {
  const int S = L.S;
  const ActParams ap = L.ap;
  const int nblk = (S + 63) >> 6;
  const float* tv = L.t + ray * S;
  const CompositeUpstream up(L.g_rgb, L.g_acc, L.g_depth, white_bkgd, ray);
  double tgw[NB], f[NB], kn[NB], wgw[NB];   // T_i gw_i;  1 - alpha_i + 1e-10;  d alpha_i / d |d|;  w_i gw_i
  double carry = 1.0;
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    tgw[b] = 0.0; f[b] = 1.0; kn[b] = 0.0; wgw[b] = 0.0;
    if (b < nblk) {
      const int s = b * 64 + lane;
      const bool in = s < S;
      double alpha = 0.0, gw = 0.0;
      if (in) {
        const int64_t g = ray * S + s;
        const float t = tv[s];
        const float delta = s == S - 1 ? 1e10f : __fsub_rn(tv[s + 1], t);
        float4 r = reinterpret_cast<const float4*>(L.raw)[g];
        if (ap.noise) r.w = __fadd_rn(r.w, __fmul_rn(ap.noise[g], ap.noise_std));
        CompositeSample m;
        composite_sample(ap, r, __fmul_rn(delta, dn), m);
        alpha = m.alpha; f[b] = m.f;
        kn[b] = m.ex * m.sg * (double)delta;
        gw = up.gw(m, t);
      }
      const double T = wave_exclusive_product_f64(f[b], lane, carry);
      tgw[b] = T * gw;
      wgw[b] = in ? alpha * T * gw : 0.0;
    }
  }
  double part = 0.0, sfx_carry = 0.0;
#pragma unroll
  for (int b = NB - 1; b >= 0; --b) {
    if (b < nblk) {
      const double sfx = wave_exclusive_suffix_sum_f64(wgw[b], lane, sfx_carry);
      if (b * 64 + lane < S) part += (tgw[b] - sfx / f[b]) * kn[b];   // dL/dalpha_i * dalpha_i/d|d|
    }
  }
  return wsum64d(part);
}

// The record loop both reduce kernels share: `rec` the ray's first record at this lane's component (a record is one 128-byte line: lanes
// 0..31 read it whole), `tv` its S sample positions; acc += r_i (weighted: t_i r_i) in fp64, sample after sample in ascending order.
__device__ __forceinline__ void rg_sum_records(const float* rec, const float* tv, const int S, const bool weighted, double& acc) {
  int i = 0;
  for (; i + 8 <= S; i += 8) {
    float r[8], t[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { r[k] = rec[(i + k) * kRecFloats]; t[k] = tv[i + k]; }
#pragma unroll
    for (int k = 0; k < 8; ++k) acc += weighted ? (double)t[k] * (double)r[k] : (double)r[k];
  }
  for (; i < S; ++i) {
    const float r = rec[i * kRecFloats], t = tv[i];
    acc += weighted ? (double)t * (double)r : (double)r;
  }
}

// The view encoding, backwards (both reduce kernels): lane kRecView + ci of `acc` holds the summed partial of column ci; columns
// [v ; sin(2^l v) (level-major, xyz-minor) ; sin(2^l v + fp32(pi/2))] in ascending order, at the forward's rounded arguments.  Every lane
// of the wave calls it and gets the same gv.
__device__ __forceinline__ void rg_view_backward(const double acc, const float (&vd)[3], const int Lv, double (&gv)[3]) {
  gv[0] = 0.0; gv[1] = 0.0; gv[2] = 0.0;
  const int V = enc_width(Lv);
  for (int ci = 0; ci < V; ++ci) {
    const double g = __shfl(acc, kRecView + ci);
    int ax = ci;
    double coef = 1.0;
    if (ci >= 3) {
      const int e = ci - 3, second = e >= 3 * Lv ? 1 : 0;
      const int e2 = second ? e - 3 * Lv : e;
      ax = e2 % 3;
      const float scale = (float)(1 << (e2 / 3));
      const float v = ax == 0 ? vd[0] : (ax == 1 ? vd[1] : vd[2]);
      const float arg = __fadd_rn(__fmul_rn(v, scale), second ? AON_HALF_PI_F32 : 0.f);
      coef = (double)scale * (double)cos_f32(arg);
    }
    const double term = coef * g;
    gv[0] += ax == 0 ? term : 0.0;
    gv[1] += ax == 1 ? term : 0.0;
    gv[2] += ax == 2 ? term : 0.0;
  }
}

template <int NB>
__global__ void __launch_bounds__(256) ray_grad_reduce_kernel(RgReduceArgs a) {
  const int lane = (int)threadIdx.x & 63;
  const int64_t ray = (int64_t)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (ray >= a.n_rays) return;
  const float d0 = a.rays_d[ray * 3], d1 = a.rays_d[ray * 3 + 1], d2 = a.rays_d[ray * 3 + 2];
  const float dn = ray_norm_f32(a.rays_d, ray);
  const int c = lane & 31;
  const bool weighted = lane >= 32;
  double acc = 0.0, gn = 0.0;
  for (int l = 0; l < a.nlevels; ++l) {
    const RgReduceLevel& L = a.lvl[l];
    const int S = L.S;
    rg_sum_records(L.rec + ray * S * kRecFloats + c, L.t + ray * S, S, weighted, acc);
    gn += rg_norm_term<NB>(L, ray, lane, dn, a.white_bkgd);
  }
  const float vd[3] = {a.viewdirs[ray * 3], a.viewdirs[ray * 3 + 1], a.viewdirs[ray * 3 + 2]};
  double gv[3];
  rg_view_backward(acc, vd, a.Lv, gv);
  const double tsum = __shfl(acc, (lane + 32) & 63);   // lanes 0..2: sum_i t_i g_x_i
  if (lane < 3) {
    const double dd = lane == 0 ? (double)d0 : (lane == 1 ? (double)d1 : (double)d2);
    const double n64 = sqrt((double)d0 * d0 + (double)d1 * d1 + (double)d2 * d2);
    a.g_o[ray * 3 + lane] = (float)acc;
    a.g_d[ray * 3 + lane] = (float)(tsum + (n64 > 0.0 ? gn * dd / n64 : 0.0));
    a.g_v[ray * 3 + lane] = (float)(lane == 0 ? gv[0] : (lane == 1 ? gv[1] : gv[2]));
  }
}

// The stage-level reduce of ONE level of one block of rays (include/aon_hip_scene_pose.h): ray_grad_reduce_kernel
// without the norm term -- it reads no raw, no directions and no upstream gradients, and S has no limit of its own.
struct RgPlainArgs {
  const float* rec; const float* t; const float* viewdirs;
  float* g_o; float* g_d; float* g_v;
  int64_t n_rays;
  int S, Lv;
};

__global__ void __launch_bounds__(256) ray_grad_reduce_plain_kernel(RgPlainArgs a) {
  const int lane = (int)threadIdx.x & 63;
  const int64_t ray = (int64_t)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (ray >= a.n_rays) return;
  double acc = 0.0;
  rg_sum_records(a.rec + ray * a.S * kRecFloats + (lane & 31), a.t + ray * a.S, a.S, lane >= 32, acc);
  const float vd[3] = {a.viewdirs[ray * 3], a.viewdirs[ray * 3 + 1], a.viewdirs[ray * 3 + 2]};
  double gv[3];
  rg_view_backward(acc, vd, a.Lv, gv);
  const double tsum = __shfl(acc, (lane + 32) & 63);   // lanes 0..2: sum_i t_i g_x_i
  if (lane < 3) {
    a.g_o[ray * 3 + lane] = (float)acc;
    a.g_d[ray * 3 + lane] = (float)tsum;
    a.g_v[ray * 3 + lane] = (float)(lane == 0 ? gv[0] : (lane == 1 ? gv[1] : gv[2]));
  }
}

// ---- the vanilla network ----
// Position enters NeRFMLP twice -- the encoding is the input of pts_linears.0 and rides behind h into pts_linears.5 (model.py:95-103) --
// and the chain leaves dZ0, dZ5 and dZ_v0 in the gradient planes for the weight-gradient stage.  Per sample, in row-vector notation:
//   g_enc = dZ0 . W0 + dZ5 . W5[:, encoding columns]   (P = 3 + 6 (max_deg - min_deg) columns from kTrunk5EncCol, each ONE fmaf chain from 0 over dZ0's 256
//                                                      features in ascending order, then dZ5's 256 on the same accumulator)
//   view partial = dZ_v0 . W_v0[:, view-encoding columns]   (V columns from kView0EncCol; one chain over 128 features, as ray_grad_sample_kernel's)
//   g_x[a] = g_enc[a] + sum_l 2^l cos(arg) g_enc[..]  at the forward's rounded arguments, x = o + t d in cast_rays' bits; fp64 in ascending
//                                                      column order, rounded once.
// The weights are uniform across a wave: W0, then W5's slice, then W_v0's slice are staged through ONE 64 KiB LDS buffer from the network's
// own nn.Linear storages (their own leading dimensions; columns beyond P / V are zero weights, so a chain there stays 0).  A lane carries
// kVrgSpl samples, 256 apart: every 16-byte LDS read feeds 4 * kVrgSpl multiply-adds.
constexpr int kVrgCols = 64;      // 63 position-encoding columns padded to whole float4s
constexpr int kVrgSpl = 2;        // samples per lane (measured against 1: DESIGN.md section 4.15)
constexpr int kVrgBlock = 256 * kVrgSpl;

struct VrgSeg {
  const float* dplanes;   // the level's gradient planes (chain output)
  const float* W0;        // pts_linears.0.weight (256, P)
  const float* W5;        // pts_linears.5.weight (256, vp_trunk5_ld(P))
  const float* Wv0;       // views_linear.0.weight (128, vp_view0_ld(V))
  const float* t;         // (n, S)
  float* rec;             // (n * S, 32)
  int64_t nvalid;         // n * S: padding samples are neither read nor written
  int S, blk_begin;
};
struct VrgArgs {
  VrgSeg seg[2];
  const float* rays_o; const float* rays_d;
  int nsegs, min_deg, Lp, V;
};

// w[f * LD + c] <- W[f * ld + col0 + c] for c < ncols, 0 beyond: `rows` features
template <int LD>
__device__ __forceinline__ void vrg_stage(float* w, const float* W, int rows, int ld, int col0, int ncols, int tid) {
  for (int i = tid; i < rows * LD; i += 256) {
    const int f = i / LD, c = i % LD;
    w[i] = c < ncols ? W[(int64_t)f * ld + col0 + c] : 0.f;
  }
}

// acc[s][c] <- fmaf(w[f][c], z_s[f], acc[s][c]) over the `units` * 4 features of a layer, ascending
template <int NQ, int LD>
__device__ __forceinline__ void vrg_accum(const float* w, const float* const (&pz)[kVrgSpl], int units, float (&acc)[kVrgSpl][kVrgCols]) {
#pragma unroll 2
  for (int u = 0; u < units; ++u) {
    f32x4 z[kVrgSpl];
#pragma unroll
    for (int s = 0; s < kVrgSpl; ++s) z[s] = *reinterpret_cast<const f32x4*>(pz[s] + u * 128);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const f32x4 wq = *reinterpret_cast<const f32x4*>(w + (4 * u + j) * LD + 4 * q);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
          for (int s = 0; s < kVrgSpl; ++s) acc[s][4 * q + k] = __builtin_fmaf(wq[k], z[s][j], acc[s][4 * q + k]);
        }
      }
    }
  }
}

__global__ void __launch_bounds__(256) vanilla_ray_grad_sample_kernel(VrgArgs a) {
  __shared__ __attribute__((aligned(16))) float w[256 * kVrgCols];
  const int tid = (int)threadIdx.x;
  const int si = (a.nsegs > 1 && (int)blockIdx.x >= a.seg[1].blk_begin) ? 1 : 0;
  const VrgSeg& S = a.seg[si];
  const int P = enc_width(a.Lp);
  int64_t n[kVrgSpl];
  bool valid[kVrgSpl];
  const float* base[kVrgSpl];
#pragma unroll
  for (int s = 0; s < kVrgSpl; ++s) {
    n[s] = (int64_t)((int)blockIdx.x - S.blk_begin) * kVrgBlock + s * 256 + tid;
    valid[s] = n[s] < S.nvalid;
    const int64_t m = valid[s] ? n[s] : S.nvalid - 1;   // a lane without a sample follows the level's last one and stores nothing
    // feature row f of sample m: ((m >> 5) * (rows / 4) + (f >> 2)) * 128 + (m & 31) * 4 + (f & 3)   (aon_mlp_core.h)
    base[s] = S.dplanes + (m >> 5) * ((int64_t)kPlRows * 32) + (int)(m & 31) * 4;
    n[s] = m;
  }
  float acc[kVrgSpl][kVrgCols];
#pragma unroll
  for (int s = 0; s < kVrgSpl; ++s) {
#pragma unroll
    for (int c = 0; c < kVrgCols; ++c) acc[s][c] = 0.f;
  }
  const float* pz[kVrgSpl];
  vrg_stage<kVrgCols>(w, S.W0, 256, vp_trunk0_ld(P), 0, P, tid);
  __syncthreads();
#pragma unroll
  for (int s = 0; s < kVrgSpl; ++s) pz[s] = base[s] + (plane_h(0) / 4) * 128;
  vrg_accum<kVrgCols / 4, kVrgCols>(w, pz, 64, acc);
  __syncthreads();
  vrg_stage<kVrgCols>(w, S.W5, 256, vp_trunk5_ld(P), kTrunk5EncCol, P, tid);
  __syncthreads();
#pragma unroll
  for (int s = 0; s < kVrgSpl; ++s) pz[s] = base[s] + (plane_h(5) / 4) * 128;
  vrg_accum<kVrgCols / 4, kVrgCols>(w, pz, 64, acc);
  __syncthreads();
  vrg_stage<kWvCols>(w, S.Wv0, 128, vp_view0_ld(a.V), kView0EncCol, a.V, tid);
  // the encoding, backwards: columns [x ; sin(2^l x) (level-major, xyz-minor) ; sin(2^l x + fp32(pi/2))] in ascending order
  float gx[kVrgSpl][3];
#pragma unroll
  for (int s = 0; s < kVrgSpl; ++s) {
    const int64_t ray = n[s] / S.S;
    const float t = S.t[n[s]];
    float x[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = __fadd_rn(a.rays_o[ray * 3 + k], __fmul_rn(t, a.rays_d[ray * 3 + k]));
    double g[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int ci = 0; ci < kPosEnc; ++ci) {
      if (ci < P) {
        int ax = ci;
        double coef = 1.0;
        if (ci >= 3) {
          const int e = ci - 3, second = e >= 3 * a.Lp ? 1 : 0;
          const int e2 = second ? e - 3 * a.Lp : e;
          ax = e2 % 3;
          const float scale = __builtin_ldexpf(1.0f, a.min_deg + e2 / 3);
          const float xa = ax == 0 ? x[0] : (ax == 1 ? x[1] : x[2]);
          const float arg = __fadd_rn(__fmul_rn(xa, scale), second ? AON_HALF_PI_F32 : 0.f);
          coef = (double)scale * (double)cos_f32(arg);
        }
        const double term = coef * (double)acc[s][ci];
        g[0] += ax == 0 ? term : 0.0;
        g[1] += ax == 1 ? term : 0.0;
        g[2] += ax == 2 ? term : 0.0;
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) gx[s][k] = (float)g[k];
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < kVrgSpl; ++s) {
#pragma unroll
    for (int c = 0; c < kWvCols; ++c) acc[s][c] = 0.f;
    pz[s] = base[s] + (kPlHV / 4) * 128;
  }
  vrg_accum<kWvCols / 4, kWvCols>(w, pz, 32, acc);
#pragma unroll
  for (int s = 0; s < kVrgSpl; ++s) {
    if (!valid[s]) continue;
    f32x4* dst = reinterpret_cast<f32x4*>(S.rec + n[s] * kRecFloats);
    f32x4 v; v[0] = gx[s][0]; v[1] = gx[s][1]; v[2] = gx[s][2]; v[3] = acc[s][0];
    dst[0] = v;
#pragma unroll
    for (int q = 1; q < kRecFloats / 4; ++q) {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = 4 * q + k - kRecView < 27 ? acc[s][4 * q + k - kRecView] : 0.f;
      dst[q] = v;
    }
  }
}

}  // namespace

int64_t ray_grad_record_bytes(int64_t n_samples) { return n_samples * kRecFloats * 4; }

// the reduce launch both networks share: the levels' records, one wavefront per ray (4 or 8 samples a lane by the longer level)
static hipError_t launch_reduce(const RayGradLevel* lv, int nlevels, int64_t n_rays, int view_levels, int white_bkgd, const float* rays_d,
                                const float* viewdirs, float* g_rays_o, float* g_rays_d, float* g_viewdirs, hipStream_t stream) {
  RgReduceArgs R{};
  R.nlevels = nlevels; R.white_bkgd = white_bkgd; R.Lv = view_levels; R.n_rays = n_rays;
  R.rays_d = rays_d; R.viewdirs = viewdirs; R.g_o = g_rays_o; R.g_d = g_rays_d; R.g_v = g_viewdirs;
  int smax = 0;
  for (int l = 0; l < nlevels; ++l) {
    const RayGradLevel& L = lv[l];
    R.lvl[l] = RgReduceLevel{L.rec, L.t, L.raw, L.g_rgb, L.g_acc, L.g_depth, L.ap, L.S};
    smax = L.S > smax ? L.S : smax;
  }
  const dim3 grid((unsigned)((n_rays + 3) / 4));
  if (smax <= 256) ray_grad_reduce_kernel<4><<<grid, dim3(256), 0, stream>>>(R);
  else ray_grad_reduce_kernel<8><<<grid, dim3(256), 0, stream>>>(R);
  return hipGetLastError();
}

hipError_t launch_ray_grads(const RayGradLevel* lv, int nlevels, int64_t n_rays, int view_levels, int white_bkgd, const float* rays_d,
                            const float* viewdirs, float* g_rays_o, float* g_rays_d, float* g_viewdirs, hipStream_t stream) {
  if (nlevels < 1 || nlevels > 2 || n_rays <= 0 || view_levels < 0 || view_levels > 4) return hipErrorInvalidValue;
  if (!rays_d || !viewdirs || !g_rays_o || !g_rays_d || !g_viewdirs) return hipErrorInvalidValue;
  RgSampleArgs A{};
  A.nsegs = nlevels; A.V = enc_width(view_levels);
  int64_t blk = 0;
  for (int l = 0; l < nlevels; ++l) {
    const RayGradLevel& L = lv[l];
    if (!L.dplanes || !L.dxp || !L.params || !L.params[ap_deform_w(0)] || !L.params[ap_view_w(0)] || !L.rec || !L.t || !L.raw || !L.g_rgb) return hipErrorInvalidValue;
    const int64_t nvalid = n_rays * L.S;
    if (L.S < 1 || L.S > 512 || nvalid > L.Np) return hipErrorInvalidValue;
    A.seg[l] = RgSampleSeg{L.dplanes, L.dxp, L.params[ap_deform_w(0)], L.params[ap_view_w(0)], L.rec, nvalid, (int)blk};
    blk += (nvalid + 255) / 256;
    if (blk > 0x7fffffff) return hipErrorInvalidValue;
  }
  ray_grad_sample_kernel<<<dim3((unsigned)blk), dim3(256), 0, stream>>>(A);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  return launch_reduce(lv, nlevels, n_rays, view_levels, white_bkgd, rays_d, viewdirs, g_rays_o, g_rays_d, g_viewdirs, stream);
}

// One level of one block of rays from the stage calls' buffers: ray_grad_sample_kernel with ONE segment, then the
// reduce without the norm term.  The caller (aon_art_ray_grads) has checked every argument.
hipError_t launch_art_ray_grads(const float* dplanes, const float* dxp, const float* Wd0, const float* Wv0, const float* t_vals,
                                const float* viewdirs, int64_t n_rays, int S, int view_levels, float* rec, float* g_rays_o, float* g_rays_d,
                                float* g_viewdirs, hipStream_t stream) {
  if (n_rays <= 0 || S < 1 || view_levels < 0 || view_levels > 4) return hipErrorInvalidValue;
  const int64_t nvalid = n_rays * S, blk = (nvalid + 255) / 256;
  if (blk > 0x7fffffff) return hipErrorInvalidValue;
  RgSampleArgs A{};
  A.nsegs = 1; A.V = enc_width(view_levels);
  A.seg[0] = RgSampleSeg{dplanes, dxp, Wd0, Wv0, rec, nvalid, 0};
  ray_grad_sample_kernel<<<dim3((unsigned)blk), dim3(256), 0, stream>>>(A);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  const RgPlainArgs R{rec, t_vals, viewdirs, g_rays_o, g_rays_d, g_viewdirs, n_rays, S, view_levels};
  ray_grad_reduce_plain_kernel<<<dim3((unsigned)((n_rays + 3) / 4)), dim3(256), 0, stream>>>(R);
  return hipGetLastError();
}

hipError_t launch_vanilla_ray_grads(const RayGradLevel* lv, int nlevels, int64_t n_rays, int min_deg, int pos_levels, int view_levels,
                                    int white_bkgd, const float* rays_o, const float* rays_d, const float* viewdirs, float* g_rays_o,
                                    float* g_rays_d, float* g_viewdirs, hipStream_t stream) {
  if (nlevels < 1 || nlevels > 2 || n_rays <= 0 || view_levels < 0 || view_levels > 4 || pos_levels < 0 || pos_levels > 10 || min_deg < 0)
    return hipErrorInvalidValue;
  if (!rays_o || !rays_d || !viewdirs || !g_rays_o || !g_rays_d || !g_viewdirs) return hipErrorInvalidValue;
  VrgArgs A{};
  A.nsegs = nlevels; A.min_deg = min_deg; A.Lp = pos_levels; A.V = enc_width(view_levels);
  A.rays_o = rays_o; A.rays_d = rays_d;
  int64_t blk = 0;
  for (int l = 0; l < nlevels; ++l) {
    const RayGradLevel& L = lv[l];
    if (!L.dplanes || !L.params || !L.params[vp_trunk_w(0)] || !L.params[vp_trunk_w(5)] || !L.params[kVpView0W] || !L.rec || !L.t || !L.raw || !L.g_rgb) return hipErrorInvalidValue;
    const int64_t nvalid = n_rays * L.S;
    if (L.S < 1 || L.S > 512 || nvalid > L.Np) return hipErrorInvalidValue;
    A.seg[l] = VrgSeg{L.dplanes, L.params[vp_trunk_w(0)], L.params[vp_trunk_w(5)], L.params[kVpView0W], L.t, L.rec, nvalid, L.S, (int)blk};
    blk += (nvalid + kVrgBlock - 1) / kVrgBlock;
    if (blk > 0x7fffffff) return hipErrorInvalidValue;
  }
  vanilla_ray_grad_sample_kernel<<<dim3((unsigned)blk), dim3(256), 0, stream>>>(A);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  return launch_reduce(lv, nlevels, n_rays, view_levels, white_bkgd, rays_d, viewdirs, g_rays_o, g_rays_d, g_viewdirs, stream);
}

}  // namespace aon
