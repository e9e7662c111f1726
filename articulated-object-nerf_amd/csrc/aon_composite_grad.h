// The derivative of the volume-rendering composite (helper.volumetric_rendering, helper.py:157-195, with the activations of
// model.py:186-187 / model_autodecoder.py:321-323), as every backward kernel takes it: composite_bwd_kernel (aon_train.hip, d raw of one
// object's ray), ray_grad_reduce_kernel (aon_ray_grad.hip, d ||d||) and scene_composite_bwd_kernel (aon_scene_grad.hip, d raw of a ray's
// merged lists).  With w_i = alpha_i T_i, T_i = prod_{j < i} f_j and f_j = 1 - alpha_j + 1e-10:
//   dL/dw_i     = gC . c_i + g_acc - [white] sum(gC) + t_i g_depth                  (comp_rgb += 1 - acc, helper.py:187-188)
//   dL/dalpha_i = T_i dL/dw_i - Sfx_i / f_i,   Sfx_i = sum_{k > i} w_k dL/dw_k
// The two scans (T front to back, Sfx from the far end) are wave_exclusive_product_f64 / wave_exclusive_suffix_sum_f64 (aon_ray_core.h),
// and the fp32 norm is ray_norm_f32 there.  What differs between the callers stays in them: the noise add in front of the one-object
// kernels, the last interval (1e10 for one object, 0 for a scene list), the scene's g_obj_acc term and its exact-zero rule.
//
// Everything is evaluated in fp64 on the fp32 inputs and rounded to fp32 ONCE per output; the fp32 operations that are part of the function
// (the interval lengths, the norm, raw_sigma + sigma_bias) stay fp32.  dL/dalpha_i is a difference of nearly equal terms, and the
// density-head bias gradient is the plain sum of dL/d raw_sigma over every sample of a level -- on a field where that sum cancels to 1e-4 of
// its terms (constructor-fuzz seed 112: x6,368) the fp32 form's correlated rounding along each ray (both scans feed every sample in front of
// them) left the bias 3e-3 from the fp64 truth where torch's fp32 autograd happened to land at 9e-5 (tests/diag/diag_density_bias.py:
// per-sample errors 1.2x torch's, their per-ray sums 3-5x).  The kernels handle 20 B per sample and take 0.1 - 0.7 % of a step: fp64 costs
// nothing visible, and every output is the correctly rounded derivative of the reference's formula at the forward's fp32 inputs.
#pragma once
#include "aon_ray_core.h"

namespace aon {

__device__ __forceinline__ double sigmoid_f64(double x) { return 1.0 / (1.0 + exp(-x)); }

// One sample, recomputed from its record
struct CompositeSample {
  double sg, dsg;           // the density and its derivative by raw_sigma
  double ex;                // exp(-sigma dist)
  double alpha, f, kf;      // 1 - ex;  1 - alpha + 1e-10;  d alpha / d raw_sigma
  double c0, c1, c2;        // the colours
  double d0, d1, d2;        // d colour / d raw
};

// (templates on ACT for the scene kernel, which is one; composite_sample below is the run-time form for the kernels that are not)
template <int ACT>
__device__ __forceinline__ void density_activation(const ActParams& ap, float rw, CompositeSample& s) {
  if constexpr (ACT == 1) {
    s.sg = rw > 0.f ? (double)rw : 0.0; s.dsg = rw > 0.f ? 1.0 : 0.0;
  } else if constexpr (ACT == 2) {
    const float xs = __fadd_rn(rw, ap.sigma_bias);   // (an fp32 add in the forward: part of the function)
    s.sg = xs > 20.0f ? (double)xs : log1p(exp((double)xs)); s.dsg = xs > 20.0f ? 1.0 : sigmoid_f64(xs);   // torch Softplus, threshold 20
  } else {
    s.sg = rw; s.dsg = 1.0;
  }
}

// alpha and its derivative from the density over the fp32 interval length dist32 = delta ||d||
__device__ __forceinline__ void density_interval(float dist32, CompositeSample& s) {
  const double dist = dist32;
  s.ex = exp(-s.sg * dist);
  s.alpha = 1.0 - s.ex;
  s.f = (1.0 - s.alpha) + 1e-10;
  s.kf = dist * s.ex * s.dsg;   // d alpha / d sigma = dist exp(-sigma dist), times the density activation's derivative
}

template <int ACT>
__device__ __forceinline__ void density(const ActParams& ap, float rw, float dist32, CompositeSample& s) {
  density_activation<ACT>(ap, rw, s);
  density_interval(dist32, s);
}

template <int ACT>
__device__ __forceinline__ void colours(const ActParams& ap, const float4& r, CompositeSample& s) {
  if constexpr (ACT == 1) {
    s.c0 = sigmoid_f64(r.x); s.c1 = sigmoid_f64(r.y); s.c2 = sigmoid_f64(r.z);
    s.d0 = s.c0 * (1.0 - s.c0); s.d1 = s.c1 * (1.0 - s.c1); s.d2 = s.c2 * (1.0 - s.c2);
  } else if constexpr (ACT == 2) {
    const double s0 = sigmoid_f64(r.x), s1 = sigmoid_f64(r.y), s2 = sigmoid_f64(r.z);
    const double sc = ap.rgb_scale, sh = ap.rgb_shift;
    s.c0 = s0 * sc - sh; s.c1 = s1 * sc - sh; s.c2 = s2 * sc - sh;
    s.d0 = sc * s0 * (1.0 - s0); s.d1 = sc * s1 * (1.0 - s1); s.d2 = sc * s2 * (1.0 - s2);
  } else {
    s.c0 = r.x; s.c1 = r.y; s.c2 = r.z;
    // (stored in the order of the other branches: composite_sample joins the three, and `d0 = d1 = d2 = 1.0` stores d0 LAST, so the
    // compiler sank the branches' last stores below the join as one store to a choice of two addresses, which kept 24 B per lane of the
    // record in scratch)
    s.d0 = 1.0; s.d1 = 1.0; s.d2 = 1.0;
  }
}

// density<ap.act> and colours<ap.act>: the activations branch, the exp of the interval exists once
__device__ __forceinline__ void composite_sample(const ActParams& ap, const float4& r, float dist32, CompositeSample& s) {
  if (ap.act == 1) {
    density_activation<1>(ap, r.w, s); colours<1>(ap, r, s);
  } else if (ap.act == 2) {
    density_activation<2>(ap, r.w, s); colours<2>(ap, r, s);
  } else {
    density_activation<0>(ap, r.w, s); colours<0>(ap, r, s);
  }
  density_interval(dist32, s);
}

// The upstream gradients of one ray (null g_acc / g_depth = 0) and dL/dw of a sample at distance t
struct CompositeUpstream {
  double gC0, gC1, gC2, gw_const, gD;
  __device__ __forceinline__ CompositeUpstream(const float* g_rgb, const float* g_acc, const float* g_depth, int white_bkgd, int64_t ray) {
    gC0 = g_rgb[ray * 3]; gC1 = g_rgb[ray * 3 + 1]; gC2 = g_rgb[ray * 3 + 2];
    const double gA = g_acc ? (double)g_acc[ray] : 0.0;
    gD = g_depth ? (double)g_depth[ray] : 0.0;
    gw_const = gA - (white_bkgd ? (gC0 + gC1 + gC2) : 0.0);
  }
  __device__ __forceinline__ double gw(const CompositeSample& s, float t) const {
    return gC0 * s.c0 + gC1 * s.c1 + gC2 * s.c2 + gw_const + (double)t * gD;
  }
};

}  // namespace aon
