// Shared constants and small device helpers for the gfx950 (MI355X / CDNA4) NeRF render kernels.
// Wave size is 64 on CDNA; every wave-width constant below is hard-coded to 64.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "aon_params.h"

namespace aon {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// fp32(0.5*pi): the reference computes cos(x) as sin(x + 0.5*np.pi) with the add done in fp32
// (models/vanilla_nerf/helper.py:139).
#define AON_HALF_PI_F32 1.57079637050628662109375f

// Argument reduction by multiples of pi/2, shared by sin_f32 and cos_f32: ax = |x| -> the quadrant q (only q mod 4 matters) and the
// reduced argument r = ax - q pi/2, |r| <= pi/4 (+ a rounding).
//   ax < 2^19: three-term Cody-Waite reduction with FMA; k = rint(ax 2/pi) < 2^19, and the three terms of pi/2 carry 22 / 21 / 20
//     significant bits.  Beyond 2^19 the error of this r grows (on the device 2.9e-7 absolute on the sine in [2^20, 2^21)), and from
//     k >= 2^23 on the fp32 k is off by whole quadrants.
//   ax >= 2^19, every larger finite fp32: an exact quadrant reduction (Payne-Hanek).  ax = ia 2^(ex - 158) with the 32-bit integer
//     ia = mantissa << 8; ia * (2/pi) is formed modulo 4 from the 96 bits of 2/pi that can reach the two quadrant bits and the 62
//     fraction bits below them (higher bits of 2/pi give multiples of 4, lower ones less than 2^-62), rounded to the nearest
//     quadrant, and the signed fraction times pi/2 is rounded once, through fp64: r is the correctly rounded reduced argument up to
//     2^-31 relative, at any cancellation an fp32 argument can produce (the closest an fp32 comes to a multiple of pi/2 is ~2^-29
//     relative).  +-inf -> NaN (ex == 255 below); a NaN fails the comparison and stays NaN through the fast path.
// ACCURATE = false: the first form alone, for |x| < 2^19.  The fused MLP kernels (aon_mlp_core.h's in-register encodings, the
// articulated training chain's derivative) take it: they run at the register limit (256 VGPRs, one wave per SIMD), where the second
// form's branch changes the allocation of every instance, and what they encode stays inside the domain -- the default degrees' 2^9 |x| +
// pi/2, and the articulated network's 2^(max_deg_point - 1) |x'| with max_deg_point <= 16 (art_degrees_ok), i.e. |x'| < 16 at the
// limit.  pos_enc_kernel (the stage call, the layer-wise engine, the vanilla network at other degrees) and the ray-gradient kernels'
// derivative of the encoding (aon_ray_grad.hip) take the accurate form.
template <bool ACCURATE>
__device__ __forceinline__ float reduce_pio2_f32(float ax, int& q) {
  if (ACCURATE && ax >= 0x1p19f) {
    const uint32_t bits = __builtin_bit_cast(uint32_t, ax);
    const int ex = (int)(bits >> 23);                      // 146 .. 254 (255: inf)
    const uint32_t ia = (bits << 8) | 0x80000000u;
    // 2/pi = 0.A2F9836E 4E441529 FC2757D1 F534DDC0 DB629599 3C439041 ... (hex), with a zero word in front so that the window may
    // start above the binary point: it starts at bit ex - 128 of this string (18 .. 126) and is 96 bits long
    const int start = ex - 128, i = start >> 5, sh = start & 31;
    const uint32_t t0 = i == 0 ? 0u : i == 1 ? 0xA2F9836Eu : i == 2 ? 0x4E441529u : 0xFC2757D1u;
    const uint32_t t1 = i == 0 ? 0xA2F9836Eu : i == 1 ? 0x4E441529u : i == 2 ? 0xFC2757D1u : 0xF534DDC0u;
    const uint32_t t2 = i == 0 ? 0x4E441529u : i == 1 ? 0xFC2757D1u : i == 2 ? 0xF534DDC0u : 0xDB629599u;
    const uint32_t t3 = i == 0 ? 0xFC2757D1u : i == 1 ? 0xF534DDC0u : i == 2 ? 0xDB629599u : 0x3C439041u;
    const uint32_t hi = (uint32_t)((((uint64_t)t0 << 32) | t1) >> (32 - sh));
    const uint32_t mid = (uint32_t)((((uint64_t)t1 << 32) | t2) >> (32 - sh));
    const uint32_t lo = (uint32_t)((((uint64_t)t2 << 32) | t3) >> (32 - sh));
    // bits 32 .. 95 of the 128-bit product ia * (hi:mid:lo): two quadrant bits, then the fraction
    const uint64_t p = (((uint64_t)ia * lo) >> 32) + (uint64_t)ia * mid + (((uint64_t)ia * hi) << 32);
    q = (int)((p + 0x2000000000000000ull) >> 62);          // to the nearest quadrant
    const double f = (double)(int64_t)(p << 2);             // the signed fraction, in units of 2^-64
    const float r = (float)(f * 0x1.921fb54442d18p-64);    // * pi/2
    return ex == 255 ? __builtin_nanf("") : r;
  }
  const float k = __builtin_rintf(ax * 0.636619747f);
  q = (int)k;
  float r = __builtin_fmaf(k, -0x1.921fb4p+0f, ax);   // pi/2 = 0x3fc90fda + 0x33a22168 + 0x27c234c4
  r = __builtin_fmaf(k, -0x1.4442d0p-24f, r);
  r = __builtin_fmaf(k, -0x1.846988p-48f, r);
  return r;
}

// sin and cos of a reduced argument |r| <= pi/4: degree-7/8 minimax polynomials
__device__ __forceinline__ void sincos_poly_f32(float r, float& s, float& c) {
  const float z = r * r;
  float ps = __builtin_fmaf(z, -1.9515295891e-4f, 8.3321608736e-3f);
  ps = __builtin_fmaf(z, ps, -1.6666654611e-1f);
  s = __builtin_fmaf(r * z, ps, r);
  float pc = __builtin_fmaf(z, 2.443315711809948e-5f, -1.388731625493765e-3f);
  pc = __builtin_fmaf(z, pc, 4.166664568298827e-2f);
  c = __builtin_fmaf(z * z, pc, __builtin_fmaf(z, -0.5f, 1.0f));
}

// sin(x) for every fp32 x: reduce_pio2_f32, then the polynomials.  Against fp64 sin of the same fp32 argument the absolute error is
// at most 9.3e-8 for |x| < 2^19 -- the bits of this range are those of the branch-free form the function had while the default
// encodings were the only ones (their largest argument is 2^9 * 6 + pi/2) -- and below 4 * 2^-24, the bound OpenCL sets for sin, for
// every larger finite x (measured: 9.30e-8); +-inf and NaN give NaN, as torch.sin does.  tests/test_hip_device_math.py sweeps every
// binade on the device.  (The library sinf would serve the large arguments too; its small-argument path has other bits, and one
// function with one reduction is what cos_f32 can share.)  sin_f32<false>: |x| < 2^19 only, see reduce_pio2_f32.
template <bool ACCURATE = true>
__device__ __forceinline__ float sin_f32(float x) {
  int q;
  const float r = reduce_pio2_f32<ACCURATE>(__builtin_fabsf(x), q);
  float s, c;
  sincos_poly_f32(r, s, c);
  float res = (q & 1) ? c : s;
  res = (q & 2) ? -res : res;
  return x < 0.f ? -res : res;
}

// cos(x) with the same reduction / polynomials (the derivative of the encoding in the backward pass).
template <bool ACCURATE = true>
__device__ __forceinline__ float cos_f32(float x) {
  int q;
  const float r = reduce_pio2_f32<ACCURATE>(__builtin_fabsf(x), q);
  float s, c;
  sincos_poly_f32(r, s, c);
  // cos(|x|) = cos(r + q pi/2): q=0: c, 1: -s, 2: -c, 3: s
  float res = (q & 1) ? s : c;
  return ((q + 1) & 2) ? -res : res;
}

// torch Softplus(beta=1, threshold=20): x > 20 ? x : log1p(exp(x)), written as max(x, 0) + log1p(z), z = exp(-|x|) in (0, 1]
// (above 20 the second term is below half an ulp of x: the threshold needs no branch).  log1p(z) = z * P(z) with P the degree-10
// Chebyshev interpolant of log1p(z)/z on [0, 1] (1.1e-7 relative in fp32 Horner form; tests/test_hip_device_math.py checks the
// function on the device over [-100, 100]); z straight from the transcendental unit.  ~20 instructions against ~70 with the library expf and
// log1pf, which had the articulated compositing at twice the vanilla kernel's instruction count.  NaN stays NaN (through z),
// +inf -> +inf, -inf -> 0.
__device__ __forceinline__ float softplus_f32(float x) {
  const float z = __builtin_amdgcn_exp2f(__fmul_rn(__builtin_fabsf(x), -1.44269502162933349609375f));
  float p = 0.001986696617677808f;
  p = __builtin_fmaf(p, z, -0.013187826611101627f);
  p = __builtin_fmaf(p, z, 0.041006576269865036f);
  p = __builtin_fmaf(p, z, -0.08188041299581528f);
  p = __builtin_fmaf(p, z, 0.12377995997667313f);
  p = __builtin_fmaf(p, z, -0.16087622940540314f);
  p = __builtin_fmaf(p, z, 0.19885820150375366f);
  p = __builtin_fmaf(p, z, -0.24986496567726135f);
  p = __builtin_fmaf(p, z, 0.33332496881484985f);
  p = __builtin_fmaf(p, z, -0.4999997913837433f);
  p = __builtin_fmaf(p, z, 1.0f);
  return __fadd_rn(__builtin_fmaxf(x, 0.f), __fmul_rn(z, p));
}

// 1 / (1 + exp(-x)).  The compositing kernels are bound by VALU issue (SQ_INSTS_VALU: 437 wave instructions per 193-sample ray,
// three sigmoids per sample among them), so this is the short form: e = 2^(-x log2 e) straight on the transcendental unit --
// the rounding of the product costs |x| 4e-8 relative on e, which reaches the RESULT as at most 1e-8 absolute (e / (1 + e)^2
// is 0.25 at x = 0, where the product is exact, and 0.0066 at |x| = 5) -- then v_rcp_f32 (1 ulp) refined by one Newton step;
// 8 instructions against 18 with the library expf and its range fix-ups.  x < -87: e overflows, the true value is below
// 1.7e-38 -> 0 (a NaN input fails the comparison and stays NaN).  The density's alpha = 1 - exp(-sigma delta) keeps the
// library expf: its error goes into the transmittance product and the inverse CDF's weights.
__device__ __forceinline__ float sigmoid_f32(float x) {
  const float e = __builtin_amdgcn_exp2f(__fmul_rn(x, -1.44269502162933349609375f));
  const float d = __fadd_rn(1.0f, e);
  const float r = __builtin_amdgcn_rcpf(d);
  const float s = __builtin_fmaf(__builtin_fmaf(-d, r, 1.0f), r, r);
  return x < -87.0f ? 0.f : s;
}

// torch.max / torch.min of two values: NaN if either is NaN; equal operands (zeros of either sign) yield the first, as std::max / std::min
// do (the ray-box slab tests of aon_bounds.hip and aon_scene.hip)
__device__ __forceinline__ float torch_max(float a, float b) {
  if (a != a || b != b) return __builtin_nanf("");
  return a < b ? b : a;
}
__device__ __forceinline__ float torch_min(float a, float b) {
  if (a != a || b != b) return __builtin_nanf("");
  return b < a ? b : a;
}

// ------------------------------------------------------------------------------------------------
// Packed-weight stream of one vanilla NeRFMLP (models/vanilla_nerf/model.py:39-120).
//
// A *chunk* is the slice of one layer's weight matrix that multiplies one 32-feature input tile:
//   chunk[q][Tp][lane][c]  (q=0..3, Tp=0..NT_OUT-1, lane=0..63, c=0..3)  fp32, i.e. NT_OUT*4 KiB
//     = W[32*Tp + (lane&31)][ col(tile, 8q + 4*(lane>>5) + c) ]
// which is exactly the A operand of v_mfma_f32_32x32x2_f32 for output tile Tp when the B operand is
// accumulator register r = 4q+c of the producing layer's tile (rows (r&3)+8*(r>>2)+4*(lane>>5)).
// ------------------------------------------------------------------------------------------------
constexpr int kPosEnc = 63;    // 3 + 2*10*3
constexpr int kViewEnc = 27;   // 3 + 2*4*3

constexpr int kChL0 = 0;       // 2 chunks  (pos-enc tiles)            -> 256
constexpr int kChL1 = 2;       // 8 chunks each for L1..L4
constexpr int kChL5 = 34;      // 8 hidden + 2 pos-enc (skip concat)
constexpr int kChL6 = 44;
constexpr int kChL7 = 52;
constexpr int kChBott = 60;    // bottleneck 256 -> 256 (no activation)
constexpr int kChView = 68;    // 8 hidden + 1 view-enc               -> 128
constexpr int kNumChunks = 77;
constexpr int kNumBigChunks = 68;            // chunks with 8 output tiles (32 KiB)
constexpr int kBigChunkBytes = 8 * 4096;
constexpr int kSmallChunkBytes = 4 * 4096;   // view layer: 4 output tiles (16 KiB)

__host__ __device__ constexpr int chunk_bytes(int c) { return c < kNumBigChunks ? kBigChunkBytes : kSmallChunkBytes; }
__host__ __device__ constexpr int64_t chunk_offset(int c) {
  return c < kNumBigChunks ? (int64_t)c * kBigChunkBytes
                           : (int64_t)kNumBigChunks * kBigChunkBytes + (int64_t)(c - kNumBigChunks) * kSmallChunkBytes;
}
constexpr int64_t kStreamBytes = chunk_offset(kNumChunks);  // 2,375,680 B

// FOLDED form of the stream (round 5).  bottleneck_layer has NO activation and feeds views_linear[0] directly (model.py:109-114), so
//   W_v0[:, :256] (W_b h + b_b) + W_v0[:, 256:] ve + b_v0  =  (W_v0[:, :256] W_b) h + W_v0[:, 256:] ve + (W_v0[:, :256] b_b + b_v0):
// ONE 256 -> 128 layer W' = W_v0[:, :256] W_b where the literal form runs 256 -> 256 then 256 -> 128 -- 65,536 of the network's 593,408
// MACs per sample (11.0 %).  W' and b' are evaluated in fp64 from the fp32 parameters at pack time and rounded once
// (aon_fold.hip).  Chunks 0 .. 59 are the literal stream's; then the view-encoding chunk and 8 small chunks of W'.  The buffer keeps the
// literal size: the small block stays at kStreamBytes, and the 256 KiB between the end of the folded stream and the small block hold
// W' (128 x 256) and b' (128) for the pack kernel.  Which form a buffer holds is remembered per pointer (stream_form, aon_fold.hip).
// The view-encoding chunk comes FIRST in the view layer: b' + W_v0[:, 256:] ve, the head of every accumulation chain, is a constant of
// the RAY, and the whole-path calls hand it to the kernel as a per-ray bias (view_bias_kernel: the same fused multiply-adds in the same
// order, so both forms give the same bits) instead of 56 MFMAs, 12 sines and a 16 KiB chunk per 128-sample pass.
constexpr int kChFView = 60;        // 1 view-enc + 8 hidden (W'), 4 output tiles each
constexpr int kNumChunksF = 69;
__host__ __device__ constexpr int chunk_bytes_f(int c) { return c < kChFView ? kBigChunkBytes : kSmallChunkBytes; }
__host__ __device__ constexpr int64_t chunk_offset_f(int c) {
  return c < kChFView ? (int64_t)c * kBigChunkBytes : (int64_t)kChFView * kBigChunkBytes + (int64_t)(c - kChFView) * kSmallChunkBytes;
}
constexpr int64_t kStreamBytesF = chunk_offset_f(kNumChunksF);   // 2,113,536 B
constexpr int64_t kFoldTmpOff = kStreamBytesF;                   // W' (128 x 256 floats) then b' (128 floats), inside the literal-size buffer
static_assert(kStreamBytesF + (128 * 256 + 128) * 4 <= kStreamBytes, "fold temporaries fit between the folded stream and the small block");

// Small per-layer vectors, kept resident in LDS for the whole kernel (floats):
constexpr int kSmBias = 0;                    // 8 x 256  trunk biases
constexpr int kSmBiasBott = 8 * 256;          // 256
constexpr int kSmBiasView = kSmBiasBott + 256;  // 128
constexpr int kSmWSigma = kSmBiasView + 128;  // 256
constexpr int kSmWRgb = kSmWSigma + 256;      // 3 x 128
constexpr int kSmBSigma = kSmWRgb + 384;      // 1
constexpr int kSmBRgb = kSmBSigma + 1;        // 3
constexpr int kSmallFloats = 3076;            // padded to a multiple of 4
constexpr int64_t kSmallBytes = kSmallFloats * 4;

constexpr int64_t kPackedBytes = kStreamBytes + kSmallBytes;  // one packed MLP

// Training: ROW MAP of the activation planes of one vanilla NeRFMLP level (the memory layout of a row is step-major, see
// aon_mlp_core.h: [step of 32 samples][row / 4][sample][row % 4]; Np = samples padded to a multiple of 128).  Rows are TRUE
// feature indices (encodings: the reference's column order), so weight gradients come out in nn.Linear's (out,in) order
// without un-permuting.  The same row map is used for the pre-activation gradient planes written by the backward chain.
constexpr int kPlE = 0;                        // 64 rows: pos-enc (63 + zero pad)            input of L0 / L5 skip
__host__ __device__ constexpr int plane_h(int l) { return 64 + 256 * l; }  // 8 x 256 rows: trunk outputs (post-ReLU)
constexpr int kPlBot = 64 + 8 * 256;           // 256 rows: bottleneck output (no activation)
constexpr int kPlVE = kPlBot + 256;            // 32 rows: view-enc (27 + zero pad)
constexpr int kPlHV = kPlVE + 32;              // 128 rows: view-layer output (post-ReLU)
constexpr int kPlRows = kPlHV + 128;           // 2528 rows = 10,112 B per sample
constexpr int kMaskLayers = 9;                 // ReLU bit masks: trunk 0..7, view layer; [layer][Np*2] x 16 B

// Articulated network (model_autodecoder.py): plane rows and mask slots of one level
constexpr int kAPlPos = 0;                                   // 32 rows: 0..2 = sample position x, 3..5 = deformed position x'
__host__ __device__ constexpr int aplane_d(int l) { return 32 + 128 * l; }    // 4 x 128: deformation MLP outputs
constexpr int kAPlE = 32 + 4 * 128;                          // 64 rows: pos-enc of x'
__host__ __device__ constexpr int aplane_h(int l) { return kAPlE + 64 + 256 * l; }  // 8 x 256: trunk outputs
constexpr int kAPlBot = kAPlE + 64 + 8 * 256;                // 256
constexpr int kAPlVE = kAPlBot + 256;                        // 32
__host__ __device__ constexpr int aplane_v(int l) { return kAPlVE + 32 + 128 * l; }  // 4 x 128: view-branch outputs
constexpr int kAPlRows = kAPlVE + 32 + 4 * 128;              // 3456 rows = 13,824 B per sample
constexpr int kAMaskLayers = 16;                             // slots: D0..3 -> 0..3, H0..7 -> 4..11, V0..3 -> 12..15

// Output activations of a level (model.py:183-187, model_autodecoder.py:318-323) with the constructor's scalars as the reference's
// fp32 tensor arithmetic sees them, shared by the compositing kernel and its backward:
//   raw_sigma <- raw_sigma + noise * noise_std        when `noise` is given (the caller's torch.rand_like draw; model.py:183-184)
//   act 1: rgb = sigmoid(raw), sigma = relu(raw_sigma)
//   act 2: rgb = sigmoid(raw) * rgb_scale - rgb_shift  (rgb_scale = fp32(1 + 2 rgb_padding), rgb_shift = fp32(rgb_padding)),
//          sigma = softplus(raw_sigma + sigma_bias)     (sigma_bias = fp32(density_bias))
struct ActParams {
  int act;
  float rgb_scale, rgb_shift, sigma_bias;
  const float* noise;   // (n*S,) or null
  float noise_std;
};
inline ActParams default_act(int act) { return ActParams{act, 1.002f, 0.001f, -1.0f, nullptr, 0.f}; }

// One segment of a backward-chain launch (host side): a level's transposed stream, head weights and buffers.  The chains of the two
// levels of a training step are independent: launch_*_bwd_chain2 runs them as one persistent launch of two segments.
struct ChainSeg {
  const char* packed_bwd;
  const float* small;      // the level's small block (vanilla: packed_fwd + kStreamBytes)
  const float* d_raw;      // (Np,4)
  const void* masks;
  const float* planes;     // articulated: the level's forward planes (deformed position rows); vanilla: null
  float* dplanes;
  float* dxp;              // articulated: (Np,4); vanilla: null
  int64_t Np;
};

// One segment of a fused forward launch (host side), inference or training: a network's streams and one ray range's buffers at one level.
// launch_mlp_fwd / launch_art_mlp_fwd take one or two of these per launch: e.g. the fine level of ray range A together with the coarse
// level of ray range B, so the partial last round of workgroups of one is filled with passes of the other.  What a segment holds decides
// the kernel instance (see those launchers); everything a form does not use stays null / 0.
struct FwdSeg {
  const char* packed = nullptr;      // the level's packed forward stream
  const float* small = nullptr;      // articulated: the level's per-call small block; vanilla: null (it follows the stream)
  const float* rays_o = nullptr; const float* rays_d = nullptr; const float* viewdirs = nullptr;   // of the ray range
  const float* t_vals = nullptr;     // (n_rays, S)
  int64_t n_rays = 0; int S = 0;
  float* raw = nullptr;              // (n_rays * S, 4)
  float* planes = nullptr; void* masks = nullptr;   // [training] the range's offsets into the level's planes / decision bits
  int64_t np_total = 0;              // padded samples of the WHOLE level (slot stride of the decision bits); 0: this range alone
  const float* view_bias = nullptr;  // folded form: (n_rays, 128) per-ray bias of the view layer (launch_net_view_bias), or null
  // caller-made inputs instead of the in-kernel ray cast and encodings: [vanilla] samples_enc (n_rays*S, 63) and viewdirs_enc (n_rays, 27),
  // [articulated] pos (n_rays*S, 3) and viewdirs_enc
  const float* samples_enc = nullptr; const float* pos = nullptr; const float* viewdirs_enc = nullptr;
  // an occupancy list (aon_mlp_core.h): idx / count stay on the device; max_listed > 0: an upper bound of *count below n_rays * S (a round
  // of the early-termination loop lists a sub-range of every ray), which only sizes the grid
  const int* gather_idx = nullptr; const int64_t* gather_count = nullptr; int64_t max_listed = 0;
  // [vanilla] the trunk of the deferred view branch: the samples' marks and the live samples' layer-7 rows
  uint8_t* live_mark = nullptr; float* live_rows = nullptr;
};

// Sum of a double over the 64 lanes of a wave, the same value in every lane (the fp64 head / bias reductions of aon_wgrad.h and
// aon_train_latent.hip, the ray gradients' norm term).  A butterfly: not the prefix tree of wave_inclusive_sum_f64, which associates
// differently.
__device__ __forceinline__ double wsum64d(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// ------------------------------------------------------------------------------------------------
// Exclusive prefix over the threads of a 256-thread workgroup, and the total (integers: exact, so the order of the sums does not
// matter).  `red`: __shared__ T[4].  Marching cubes (aon_mesh.hip) and the occupancy compaction (aon_occ.hip) scan with it.
template <class T>
__device__ __forceinline__ T block_excl_scan(T v, T& total, T* red) {
  constexpr int kThreads = 256;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  if (lane == 63) red[wave] = x;
  __syncthreads();
  T base = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < kThreads / 64; ++w) {
    const T t = red[w];
    if (w < wave) base += t;
    total += t;
  }
  __syncthreads();   // `red` may be reused
  return base + x - v;
}

// ONE 256-thread workgroup turns n tile counts into their exclusive offsets, in tile order, and returns their total: 2,048 counts a round
// (8 per thread, block_excl_scan over the threads' sums, the total carried into the next round).  `red`: __shared__ int64_t[4].
template <class C, class O>
__device__ __forceinline__ int64_t block_scan_counts(const C* __restrict__ counts, int64_t n, O* __restrict__ offs, int64_t* red) {
  constexpr int kThreads = 256, kPer = 8;
  int64_t carry = 0;
  for (int64_t base = 0; base < n; base += (int64_t)kThreads * kPer) {
    const int64_t t0 = base + (int64_t)threadIdx.x * kPer;
    C cv[kPer];
    int64_t sv = 0;
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
      cv[r] = t0 + r < n ? counts[t0 + r] : 0;
      sv += cv[r];
    }
    int64_t tv;
    int64_t run = carry + block_excl_scan<int64_t>(sv, tv, red);
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
      if (t0 + r < n) offs[t0 + r] = (O)run;
      run += cv[r];
    }
    carry += tv;
  }
  return carry;
}

// An occupancy grid as the kernels see it (aon_occupancy, include/aon_hip.h; aon_occ.hip): hi = lo + cells * step, multiply then add
struct OccGrid {
  const uint32_t* bits;
  int64_t cells[3];
  float lo[3], step[3], hi[3];
};

// ------------------------------------------------------------------------------------------------
// Host side.  A kernel's dynamic-LDS limit (hipFuncAttributeMaxDynamicSharedMemorySize) is a per-DEVICE function
// attribute and the CU count is a per-device property: both are remembered per device ordinal, lock-free (a racing
// second thread merely repeats an idempotent call), so a process that drives cuda:0 and later cuda:1 launches correctly
// on both.
// ------------------------------------------------------------------------------------------------
constexpr int kMaxDevices = 64;

struct DeviceOnce {
  std::atomic<uint64_t> done{0};
};

template <class Kernel>
inline hipError_t set_max_lds(Kernel* kernel, int bytes, DeviceOnce& once) {
  int dev = 0;
  if (hipError_t e = hipGetDevice(&dev); e != hipSuccess) return e;
  if (dev < 0 || dev >= kMaxDevices) return hipErrorInvalidDevice;
  const uint64_t bit = 1ull << dev;
  if (once.done.load(std::memory_order_acquire) & bit) return hipSuccess;
  if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
      e != hipSuccess)
    return e;
  once.done.fetch_or(bit, std::memory_order_release);
  return hipSuccess;
}

}  // namespace aon
