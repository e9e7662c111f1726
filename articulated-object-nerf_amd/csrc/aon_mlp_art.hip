// Fused articulated NeRFMLP forward for gfx950: deformation MLP -> positional encoding of the deformed point ->
// latent-conditioned 8x256 trunk (+skip) -> sigma head, bottleneck -> 4x128 view branch -> rgb head.
//
// Replaces the reference's  models/vanilla_nerf/model_autodecoder.py:172-239 (NeRFMLP.forward with
// deformation_mlp=True, enc_after=True) preceded by helper.cast_rays (helper.py:25-26).
//
// Same register-resident transposed-MFMA scheme as aon_mlp.hip (see its header).  What is specific here:
//   * the three latents (shape 128, appearance 128, articulation 32) are broadcast to every sample by the
//     reference (einops.repeat, :186-194), i.e. every weight column that multiplies a latent contributes a
//     per-call constant.  aon_art_prepare folds those columns into effective bias vectors once per call
//     (the row strides of aon_params.h shrink to 3, 63, 319 and 283 effective columns), so the kernel never touches them.
//   * the 3->128 first deformation layer and the 128->3 deformation head are VALU work on register tiles;
//     the deformed point is encoded in registers exactly like the vanilla path.
#include "aon_art_common.h"
#include "aon_pass.h"

namespace aon {

struct ArtNet {
  static constexpr int kSlotBytes = kPairSlotBytes;  // a slot holds a pair of chunks
  static constexpr bool kPair = true;
  static constexpr int kNumChunks = kANumChunks;
  static constexpr int chunk_bytes(int c) { return (c < kAChT0 || c >= kAChV0) ? kSmallChunkBytes : kBigChunkBytes; }
  static constexpr int64_t chunk_offset(int c) {
    return c < kAChT0 ? (int64_t)c * kSmallChunkBytes
         : c < kAChV0 ? (int64_t)kAChT0 * kSmallChunkBytes + (int64_t)(c - kAChT0) * kBigChunkBytes
                      : (int64_t)kAChT0 * kSmallChunkBytes + (int64_t)(kAChV0 - kAChT0) * kBigChunkBytes +
                        (int64_t)(c - kAChV0) * kSmallChunkBytes;
  }
};
constexpr int64_t kAStreamBytes = ArtNet::chunk_offset(kANumChunks);  // 2,768,896 B

struct ArtFoldNet {   // folded form (aon_art_common.h)
  static constexpr int kSlotBytes = kPairSlotBytes;
  static constexpr bool kPair = true;
  static constexpr int kNumChunks = kANumChunksF;
  static constexpr int chunk_bytes(int c) { return (c < kAChT0 || c >= kAChFV0) ? kSmallChunkBytes : kBigChunkBytes; }
};
struct ArtFoldVbNet {   // folded form, view-encoding term as a per-ray bias: chunk c >= kAChFV0 here is chunk c + 1 of ArtFoldNet
  static constexpr int kSlotBytes = kPairSlotBytes;
  static constexpr bool kPair = true;
  static constexpr int kNumChunks = kANumChunksF - 1;
  static constexpr int chunk_bytes(int c) { return (c < kAChT0 || c >= kAChFV0) ? kSmallChunkBytes : kBigChunkBytes; }
  static constexpr int skip_before(int c) { return c == kAChFV0 ? kSmallChunkBytes : 0; }
};
constexpr int64_t kAStreamBytesF = (int64_t)kAChT0 * kSmallChunkBytes + (int64_t)(kAChFV0 - kAChT0) * kBigChunkBytes + (int64_t)(kANumChunksF - kAChFV0) * kSmallChunkBytes;
constexpr int64_t kAFoldTmpOff = kAStreamBytesF;   // W' (128 x 256 floats) for the pack kernel, inside the literal-size buffer
static_assert(kAStreamBytesF + 128 * 256 * 4 <= kAStreamBytes, "fold temporary fits behind the folded stream");

struct ArtPackArgs {
  const float* p[kNumArtParams];
};

// L / Lv: frequency levels of the network (defaults 10 / 4); the row strides of the concatenating layers follow (aon_params.h)
// FOLD: the folded form; W' was written to packed + kAFoldTmpOff by launch_fold_view on the same stream (b' belongs to the per-call block)
template <bool FOLD, class Args>   // Args: anything with the 40 parameter pointers as `p` (kernel arguments: read in place, never copied)
__device__ __forceinline__ void pack_art_element(const Args& a, float* __restrict__ packed, int L, int Lv, const int64_t idx) {
  const int P = enc_width(L), V = enc_width(Lv);
  auto pcol = [&](int c63) { return c63 < 0 ? -1 : pos_col_in(c63, L); };
  auto vcol = [&](int c27) { return c27 < 0 ? -1 : view_col_in(c27, Lv); };
  if (idx >= (FOLD ? kAStreamBytesF : kAStreamBytes) / 4) {   // [FOLD] W' (read below), then the unused tail of the literal-size buffer:
    if (FOLD && idx >= kAFoldTmpOff / 4 + 128 * 256 && idx < kAStreamBytes / 4) packed[idx] = 0.f;   // zeroed: every byte of the buffer is defined
    return;
  }
  // locate the chunk
  int c, r, nt;
  constexpr int first_small_tail = FOLD ? kAChFV0 : kAChV0;
  const int64_t s0 = (int64_t)kAChT0 * (kSmallChunkBytes / 4);
  const int64_t s1 = s0 + (int64_t)(first_small_tail - kAChT0) * (kBigChunkBytes / 4);
  if (idx < s0) { c = (int)(idx / (kSmallChunkBytes / 4)); r = (int)(idx % (kSmallChunkBytes / 4)); nt = 4; }
  else if (idx < s1) { c = kAChT0 + (int)((idx - s0) / (kBigChunkBytes / 4)); r = (int)((idx - s0) % (kBigChunkBytes / 4)); nt = 8; }
  else {
    c = first_small_tail + (int)((idx - s1) / (kSmallChunkBytes / 4)); r = (int)((idx - s1) % (kSmallChunkBytes / 4)); nt = 4;
    // the view branch's chunks take the literal branches below, W' for views_linear.0's hidden columns; views_linear.0's view-encoding chunk
    // is the FIRST of the folded layer (aon_art_common.h), the last of the literal one
    if constexpr (FOLD) c = c == kAChFV0 ? kAChV0 + 8 : (c <= kAChFV0 + 8 ? c - 1 : c) + (kAChV0 - kAChFV0);
  }
  const int cc = r & 3, lane = (r >> 2) & 63, rest = r >> 8;
  const int tp = rest % nt, q = rest / nt;
  const int h = lane >> 5, row = 32 * tp + (lane & 31);
  const int hid = 8 * q + 4 * h + cc;
  const float* W; int ld, col;
  if (c < kAChT0) { const int l = 1 + c / 4; W = a.p[ap_deform_w(l)]; ld = 128; col = 32 * (c % 4) + hid; }
  else if (c < kAChT1) { W = a.p[ap_trunk_w(0)]; ld = ap_trunk0_ld(P); col = pcol(posenc_col(c - kAChT0, q, cc, h)); }          // cols 0..P-1
  else if (c < kAChT5) { const int l = 1 + (c - kAChT1) / 8; W = a.p[ap_trunk_w(l)]; ld = 256; col = 32 * ((c - kAChT1) % 8) + hid; }
  else if (c < kAChT5 + 8) { W = a.p[ap_trunk_w(5)]; ld = ap_trunk5_ld(P); col = 32 * (c - kAChT5) + hid; }
  else if (c < kAChT6) { W = a.p[ap_trunk_w(5)]; ld = ap_trunk5_ld(P); col = pcol(posenc_col(c - kAChT5 - 8, q, cc, h)); if (col >= 0) col += kTrunk5EncCol; }
  else if (c < kAChT7) { W = a.p[ap_trunk_w(6)]; ld = 256; col = 32 * (c - kAChT6) + hid; }
  else if (c < kAChBott) { W = a.p[ap_trunk_w(7)]; ld = 256; col = 32 * (c - kAChT7) + hid; }
  else if (c < kAChV0) { W = a.p[kApBottW]; ld = 256; col = 32 * (c - kAChBott) + hid; }
  else if (c < kAChV0 + 8) {
    W = a.p[ap_view_w(0)]; ld = ap_view0_ld(V); col = 32 * (c - kAChV0) + hid;
    if constexpr (FOLD) { W = packed + kAFoldTmpOff / 4; ld = 256; }
  }
  else if (c < kAChV1) { W = a.p[ap_view_w(0)]; ld = ap_view0_ld(V); col = vcol(viewenc_col(q, cc, h)); if (col >= 0) col += kView0EncCol; }
  else { const int l = 1 + (c - kAChV1) / 4; W = a.p[ap_view_w(l)]; ld = 128; col = 32 * ((c - kAChV1) % 4) + hid; }
  packed[idx] = col >= 0 ? W[(int64_t)row * ld + col] : 0.f;  // every layer here has a multiple of 32 outputs
}
template <bool FOLD>
__global__ void pack_art_kernel(ArtPackArgs a, float* __restrict__ packed, int L, int Lv) {
  pack_art_element<FOLD>(a, packed, L, Lv, (int64_t)blockIdx.x * blockDim.x + threadIdx.x);
}

struct ArtPrepArgs {
  const float* p[kNumArtParams];
  const float* shape;  // (128) latents["density"]
  const float* app;    // (128) latents["color"]
  const float* art;    // (32)  latents["articulation"]
};

// small[] = plain copies of the small vectors + the latent-folded effective biases
// fold: the block of a FOLDED stream -- views_linear.0's effective bias additionally carries W_v0[:, :256] b_b: that sum is accumulated in fp64 and
// added to the fp32 value of b_v0 + (appearance term) -- which the literal form rounds as well -- so the effective bias is rounded TWICE (the
// fp32 chain of the latent term, then once more with the fp64 sum on top), not once like the vanilla b' (the earlier wording
// claimed one rounding; the un-folded gradients treat the bias as exact either way, and the second rounding is half an ulp of the bias)
__device__ __forceinline__ void prepare_art_element(const ArtPrepArgs& a, float* __restrict__ small, int min_deg, int L, int Lv, int fold, const int s) {
  const int P = enc_width(L), V = enc_width(Lv);
  if (s >= kASmallFloats) return;
  float v = 0.f;
  if (s >= kA_ESC) {   // encoding scales (exact powers of two), 0 for the levels this network lacks and for the pad
    const int l = s - kA_ESC;
    small[s] = l < L ? ldexpf(1.0f, min_deg + l) : 0.f;
    return;
  }
  if (s < kA_WD0) {  // b + W[:, shape cols].shape + W[:, articulation cols].art   (input = cat[pos, shape, articulation], :196-198)
    const float* w = a.p[ap_deform_w(0)] + (int64_t)s * kApDeform0Ld;
    float acc = a.p[ap_deform_b(0)][s];
    for (int k = 0; k < kShapeDim; ++k) acc = __builtin_fmaf(w[kApDeform0ShapeCol + k], a.shape[k], acc);
    for (int k = 0; k < kArtDim; ++k) acc = __builtin_fmaf(w[kApDeform0ArtCol + k], a.art[k], acc);
    v = acc;
  } else if (s < kA_BD) { const int i = s - kA_WD0; v = a.p[ap_deform_w(0)][(int64_t)(i & 127) * kApDeform0Ld + (i >> 7)]; }
  else if (s < kA_WDL) { const int i = s - kA_BD; v = a.p[ap_deform_b(1 + (i >> 7))][i & 127]; }
  else if (s < kA_BDL) { v = a.p[kApDeformOutW][s - kA_WDL]; }
  else if (s < kA_BT) { const int i = s - kA_BDL; v = i < 3 ? a.p[kApDeformOutB][i] : 0.f; }
  else if (s < kA_BBOT) {
    const int i = s - kA_BT, l = i >> 8, f = i & 255;
    float acc = a.p[ap_trunk_b(l)][f];
    if (l == 0) {        // cat[enc(63), shape(128)]  (:210)
      const float* w = a.p[ap_trunk_w(0)] + (int64_t)f * ap_trunk0_ld(P) + ap_trunk0_shape_col(P);
      for (int k = 0; k < kShapeDim; ++k) acc = __builtin_fmaf(w[k], a.shape[k], acc);
    } else if (l == 5) { // cat[h(256), enc(63), shape(128)]  (:216-217)
      const float* w = a.p[ap_trunk_w(5)] + (int64_t)f * ap_trunk5_ld(P) + ap_trunk5_shape_col(P);
      for (int k = 0; k < kShapeDim; ++k) acc = __builtin_fmaf(w[k], a.shape[k], acc);
    }
    v = acc;
  } else if (s < kA_BV) { v = a.p[kApBottB][s - kA_BBOT]; }
  else if (s < kA_WSIG) {
    const int i = s - kA_BV, l = i >> 7, f = i & 127;
    float acc = a.p[ap_view_b(l)][f];
    if (l == 0) {        // cat[bottleneck(256), viewenc(27), appearance(128)]  (:228-230)
      const float* w = a.p[ap_view_w(0)] + (int64_t)f * ap_view0_ld(V) + ap_view0_app_col(V);
      for (int k = 0; k < kAppDim; ++k) acc = __builtin_fmaf(w[k], a.app[k], acc);
      if (fold) {
        const float* wb = a.p[ap_view_w(0)] + (int64_t)f * ap_view0_ld(V);
        double t = 0.0;
        for (int k = 0; k < 256; ++k) t = __builtin_fma((double)wb[k], (double)a.p[kApBottB][k], t);
        acc = (float)((double)acc + t);
      }
    }
    v = acc;
  } else if (s < kA_WRGB) { v = a.p[kApSigmaW][s - kA_WSIG]; }
  else if (s < kA_BSIG) { v = a.p[kApRgbW][s - kA_WRGB]; }
  else if (s < kA_BRGB) { v = a.p[kApSigmaB][0]; }
  else if (s < kA_BRGB + 3) { v = a.p[kApRgbB][s - kA_BRGB]; }
  small[s] = v;
}
__global__ void prepare_art_kernel(ArtPrepArgs a, float* __restrict__ small, int min_deg, int L, int Lv, int fold) {
  prepare_art_element(a, small, min_deg, L, Lv, fold, blockIdx.x * blockDim.x + threadIdx.x);
}

// Round 6: the per-call blocks AND the forward streams of TWO networks (a training step's coarse and fine level) in one launch --
// blockIdx.y: network; blocks [0, kPrepBlocks): the per-call block, the rest: the stream.  Every element is computed by the code of the
// single-network kernels above (same bits); the folded form expects W' in each stream's fold area (aon_art_pack_step runs the products first).
constexpr int kPrepBlocks = (kASmallFloats + 255) / 256;
struct ArtPackPrep2Args {
  ArtPrepArgs net[2];
  float* small[2];
  float* packed[2];
};
template <bool FOLD>
__global__ void __launch_bounds__(256) pack_prepare_art2_kernel(ArtPackPrep2Args a, int min_deg, int L, int Lv) {
  const ArtPrepArgs& n = a.net[blockIdx.y];
  if ((int)blockIdx.x < kPrepBlocks) {
    prepare_art_element(n, a.small[blockIdx.y], min_deg, L, Lv, FOLD ? 1 : 0, (int)blockIdx.x * 256 + (int)threadIdx.x);
  } else {
    pack_art_element<FOLD>(n, a.packed[blockIdx.y], L, Lv, (int64_t)((int)blockIdx.x - kPrepBlocks) * 256 + threadIdx.x);
  }
}

// One SEGMENT of a launch: a run of 128-sample passes of one network over one ray range.  A launch carries one or two of them
// (round 4): the training forward merges the fine level of ray range A with the coarse level of ray range B -- different weight
// streams, small blocks, rays, planes -- into ONE persistent launch, so that the partial last round of the 65-sample level
// (8.125 rounds of 256 workgroups cost 9) is filled with passes of the other segment instead of idling 7/8 of the chip.
struct ArtSeg {
  const char* packed;     // kAStreamBytes
  const float* small;     // kASmallFloats (from prepare_art_kernel)
  const float* rays_o;    // [POS_IN_KERNEL]
  const float* rays_d;
  const float* viewdirs;
  const float* t_vals;
  const float* pos;          // (n*S,3)   [!POS_IN_KERNEL]
  const float* viewdirs_enc; // (n,27)
  float* raw;             // (n*S,4)
  int64_t total;
  int S;
  int npass;
  union {
    float* planes;          // [TRAIN] kAPlRows x Np
    const int* gather_idx;  // [GATHER] ascending sample indices of the segment (< total; aon_mlp_core.h)
  };
  union {
    u32x4* masks;           // [TRAIN] kAMaskLayers x (Np*2)
    const int64_t* gather_count;   // [GATHER] number of entries of gather_idx (device)
  };
  int64_t Np;
  const float* view_bias; // [VB] (n_rays,128): views_linear.0's effective bias + W_v0[:, 256:283] ve of the ray (launch_art_view_bias)
  static constexpr bool kPerCallBlock = true;
};
struct ArtMlpArgs {
  ArtSeg seg[2];
  int npass_total;        // seg[0].npass + seg[1].npass (seg[1].npass == 0: a one-segment launch)
};
__host__ __device__ __forceinline__ const char* seg_stream(const ArtSeg& s) { return s.packed; }
__device__ __forceinline__ const float* seg_small(const ArtSeg& s) { return s.small; }

struct ArtTrunk {   // trunk_fwd's view of the articulated stream, per-call block, planes and decision bits
  static constexpr int kL0 = kAChT0, kL1 = kAChT1, kL5 = kAChT5, kL6 = kAChT6, kL7 = kAChT7;
  static constexpr int kBias = kA_BT, kWSigma = kA_WSIG, kBSigma = kA_BSIG, kMask0 = 4;
  static constexpr int plane(int l) { return aplane_h(l); }
};

// Deformation MLP (model_autodecoder.py:196-205): the first layer's three xyz columns on the VALU (the latent columns are in its effective
// bias), three 128 x 128 layers, the deformation head on the VALU -> xd = x + deformation.  taps: FwdTaps of the pass, or NoTaps.
template <class Net, class Taps>
__device__ __forceinline__ void deform_fwd(Pipe& p, const float (&x)[3], const float* sm, int h, Taps& taps, float (&xd)[3]) {
  f32x16 H0[4], H1[4];
  init_bias(H0, sm + kA_BD0, h);  // effective bias, then the three xyz columns on the VALU
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(sm + kA_WD0 + a * 128 + 32 * t + 8 * gq + 4 * h);
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) H0[t][4 * gq + cc] = __builtin_fmaf(w[cc], x[a], H0[t][4 * gq + cc]);
      }
    }
  }
  relu_tiles(H0);
  init_bias(H1, sm + kA_BD + 0 * 128, h); dense_layer<Net, kAChD1 + 0, 4, 4>(p, H0, H1, taps.consume(H0, aplane_d(0), true)); taps.put_mask(0); relu_tiles(H1);
  init_bias(H0, sm + kA_BD + 1 * 128, h); dense_layer<Net, kAChD1 + 4, 4, 4>(p, H1, H0, taps.consume(H1, aplane_d(1), true)); taps.put_mask(1); relu_tiles(H0);
  init_bias(H1, sm + kA_BD + 2 * 128, h); dense_layer<Net, kAChD1 + 8, 4, 4>(p, H0, H1, taps.consume(H0, aplane_d(2), true)); taps.put_mask(2); relu_tiles(H1);
  taps.burst(H1, aplane_d(3), 3);
#pragma unroll
  for (int a = 0; a < 3; ++a) {  // x' = deformation_layer(h) + pos   (:205)
    float v = head_partial<4>(H1, sm + kA_WDL + a * 128, h);
    v = v + __shfl_xor(v, 32) + sm[kA_BDL + a];
    xd[a] = __fadd_rn(v, x[a]);
  }
}

// FOLD: stream and per-call block are the folded form's (aon_art_common.h): views_linear.0 reads the post-ReLU layer-7 output through W';
// no bottleneck layer and, [TRAIN], no bottleneck rows in the planes (rows kAPlBot .. kAPlBot + 255 stay unwritten).
// VB (folded form, in-kernel ray cast): views_linear.0's accumulators start from the ray's bias + view-encoding term (see mlp_fwd_kernel).
// GATHER (inference, in-kernel ray cast): the samples of a pass come from an occupancy list (aon_mlp_core.h).
template <bool POS_IN_KERNEL, bool TRAIN, bool FOLD, bool VB = false, bool GATHER = false>
__global__ void __launch_bounds__(256) art_mlp_fwd_kernel(ArtMlpArgs args) {
  static_assert((FOLD && POS_IN_KERNEL) || !VB, "the per-ray view bias belongs to the folded form of the whole-path kernels");
  static_assert(!GATHER || (POS_IN_KERNEL && !TRAIN), "the occupancy list serves the inference kernel with the in-kernel ray cast");
  using Net = std::conditional_t<VB, ArtFoldVbNet, std::conditional_t<FOLD, ArtFoldNet, ArtNet>>;
  constexpr int kV0 = FOLD ? kAChFV0 : kAChV0, kV1 = (FOLD ? kAChFV1 : kAChV1) - (VB ? 1 : 0);
  static_assert(!TRAIN || POS_IN_KERNEL, "the training path encodes the view direction from vd[], which only the in-kernel ray cast fills");
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int m = lane & 31, h = lane >> 5;
  const int wave_s = __builtin_amdgcn_readfirstlane(wave);   // the step base of the training planes is wave-uniform: keep it scalar

  run_passes<Net, kASmallFloats, GATHER>(args, [&](const ArtSeg& sg, int pass, Pipe& p, const float* sm, int64_t listed = 0) __attribute__((always_inline)) {
    int64_t g = (int64_t)pass * 128 + wave * 32 + m;
    bool valid;
    int64_t gc;
    if constexpr (GATHER) {   // the listed sample: everything below (ray, t, view bias, the record's address) follows it
      valid = g < listed;
      g = gc = sg.gather_idx[valid ? g : listed - 1];
    } else {
      valid = g < sg.total;
      gc = valid ? g : sg.total - 1;
    }
    const int64_t ray = gc / sg.S;
    float x[3], vd[3] = {0.f, 0.f, 0.f};
    f32x16 V;
    if constexpr (POS_IN_KERNEL) {
      const float t = sg.t_vals[gc];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        x[a] = __fadd_rn(sg.rays_o[ray * 3 + a], __fmul_rn(t, sg.rays_d[ray * 3 + a]));
        vd[a] = sg.viewdirs[ray * 3 + a];
      }
      if constexpr (!TRAIN && !VB) encode_view(vd, h, V);  // [TRAIN] encoded where the view branch needs it: 16 registers not held across the trunk
    } else {
#pragma unroll
      for (int a = 0; a < 3; ++a) x[a] = sg.pos[gc * 3 + a];
      load_view_enc(sg.viewdirs_enc + ray * kViewEnc, h, V);
    }

    PlaneIO io{};
    unsigned moff = 0;
    if constexpr (TRAIN) { io = make_plane_io(sg.planes, kAPlRows, (int64_t)pass * 4 + wave_s, m, h); moff = mask_lane_off(pass, tid); }
    // [TRAIN] planes and decision bits as side jobs of the consuming chunks; the VALU-computed first deformation layer's output and the
    // tiles consumed on the VALU (deformation head, rgb head) go out in bursts
    FwdTaps<TRAIN, ArtSeg> taps{sg, io, moff};
    auto save_row = [&](int row, float v) {  // one scalar per sample (lanes 0..31)
      if constexpr (TRAIN) { if (h == 0) *row_ptr(io, row) = v; }
    };
    if constexpr (TRAIN) {
#pragma unroll
      for (int a = 0; a < 3; ++a) save_row(kAPlPos + a, x[a]);
    }

    float xd[3];
    deform_fwd<Net>(p, x, sm, h, taps, xd);
    f32x16 E[2];
    encode_pos_scaled(xd, h, sm + kA_ESC, E);  // pos_enc after the deformation (enc_after=True, :207-208); scales: the network's degrees
    if constexpr (TRAIN) {
#pragma unroll
      for (int a = 0; a < 3; ++a) save_row(kAPlPos + 3 + a, xd[a]);
      store_pos_enc_plane(E, io, kAPlE, h);
    }

    // ---- trunk (:212-217), shape latent folded into the biases of layers 0 and 5; density_layer (:219) ----
    // (the encoding stays live across layers 1-4, 32 registers, as in the inference kernel.  Rounds 2-4 re-encoded it at layer 5 -- 30
    // sines -- to stay clear of spills; with the view encoding gone from the trunk (per-ray view bias) both forms build with 0 scratch and
    // this one is 0.04 ms per step faster: profiles/r05_view_bias_ab.txt)
    f32x16 X[8], Y[8], Z0[4], Z1[4];
    auto l7_side = [&](auto plain) {
      if constexpr (VB) {
        int ray32 = (int)ray;
        asm volatile("" : "+v"(ray32));
        return view_bias_side(plain, sg.view_bias + (int64_t)ray32 * kCondWidth + 4 * h, Z0);
      } else {
        return plain;
      }
    };
    const float sigma = trunk_fwd<Net, ArtTrunk>(p, E, X, Y, sm, h, taps, NoHook{}, l7_side);
    // ---- view branch (:227-234): cat[bottleneck, viewenc, appearance] -> 4 x (128, ReLU) ----
    auto view_enc_here = [&]() {   // [TRAIN] the view encoding where the branch needs it (and its plane rows)
      if constexpr (TRAIN) {
        encode_view(vd, h, V);
        store_view_enc_plane(V, io, kAPlVE, h);
      }
    };
    if constexpr (FOLD) {
      // bottleneck (:223, no activation) and views_linear.0's bottleneck columns as ONE layer W' on the layer-7 output (effective bias incl.
      // W_v0[:, :256] b_b); the view-encoding columns FIRST (chunk form) or already in Z0 with the bias (VB)
      view_enc_here();
      if constexpr (!VB) {
        init_bias(Z0, sm + kA_BV + 0 * 128, h);
        chunk_mma<Net, kV0, 4, 14>(p, V, Z0);
      }
      dense_layer<Net, kV0 + (VB ? 0 : 1), 8, 4>(p, Y, Z0, taps.consume(Y, aplane_h(7), true)); taps.put_mask(11);
    } else {
      init_bias(X, sm + kA_BBOT, h); dense_layer<Net, kAChBott, 8, 8>(p, Y, X, taps.consume(Y, aplane_h(7), true)); taps.put_mask(11);  // bottleneck (:223)
      init_bias(Z0, sm + kA_BV + 0 * 128, h);
      dense_layer<Net, kV0, 8, 4>(p, X, Z0, taps.consume(X, kAPlBot, false));
      view_enc_here();
      chunk_mma<Net, kV0 + 8, 4, 14>(p, V, Z0);
    }
    relu_tiles(Z0);
    init_bias(Z1, sm + kA_BV + 1 * 128, h); dense_layer<Net, kV1 + 0, 4, 4>(p, Z0, Z1, taps.consume(Z0, aplane_v(0), true)); taps.put_mask(12); relu_tiles(Z1);
    init_bias(Z0, sm + kA_BV + 2 * 128, h); dense_layer<Net, kV1 + 4, 4, 4>(p, Z1, Z0, taps.consume(Z1, aplane_v(1), true)); taps.put_mask(13); relu_tiles(Z0);
    init_bias(Z1, sm + kA_BV + 3 * 128, h); dense_layer<Net, kV1 + 8, 4, 4>(p, Z0, Z1, taps.consume(Z0, aplane_v(2), true)); taps.put_mask(14); relu_tiles(Z1);
    taps.burst(Z1, aplane_v(3), 15);
    float rgb[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {  // rgb_layer (:236)
      float v = head_partial<4>(Z1, sm + kA_WRGB + ch * kCondWidth, h);
      rgb[ch] = v + __shfl_xor(v, 32) + sm[kA_BRGB + ch];
    }
    if (valid && h == 0) {
      f32x4 o; o[0] = rgb[0]; o[1] = rgb[1]; o[2] = rgb[2]; o[3] = sigma;
      reinterpret_cast<f32x4*>(sg.raw)[g] = o;
    }
  });
}

// ---------------------------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------------------------
// The form packed is the process default at the time of the call (aon_set_bottleneck_fold), remembered for `packed` (stream_form).
// W' = W_v0[:, :256] W_b of one network into the fold area of its forward stream (the job launch_pack_art runs unless told it has been run)
FoldGemm art_fold_job_fwd(const float* const* params, float* packed, int view_levels) {
  // (b' is the per-call block's business: prepare_art_kernel; the 128 floats it would take here are not written)
  return FoldGemm{params[ap_view_w(0)], ap_view0_ld(enc_width(view_levels)), 1, params[kApBottW], 256, 1, packed + kAFoldTmpOff / 4, 256, 128, 256, 256, nullptr, nullptr};
}

hipError_t launch_pack_art(const float* const* params, float* packed, hipStream_t stream, int pos_levels, int view_levels, bool fold_done) {
  ArtPackArgs a;
  for (int i = 0; i < kNumArtParams; ++i) a.p[i] = params[i];
  const int form = fold_default();
  set_stream_form(packed, form);
  if (form == kFormFolded) {
    if (!fold_done) {   // (aon_art_pack_step runs the products of both networks and both directions as ONE launch in front)
      const FoldGemm job = art_fold_job_fwd(params, packed, view_levels);
      if (hipError_t e = launch_fold_gemms(&job, 1, stream); e != hipSuccess) return e;
    }
    const int64_t n = kAStreamBytes / 4;   // (the whole buffer: the kernel zeroes what lies behind W')
    pack_art_kernel<true><<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream>>>(a, packed, pos_levels, view_levels);
  } else {
    const int64_t n = kAStreamBytes / 4;
    pack_art_kernel<false><<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream>>>(a, packed, pos_levels, view_levels);
  }
  return hipGetLastError();
}

hipError_t launch_prepare_art(const float* const* params, const float* shape, const float* app, const float* art,
                              float* small, hipStream_t stream, int min_deg, int pos_levels, int view_levels) {
  ArtPrepArgs a;
  for (int i = 0; i < kNumArtParams; ++i) a.p[i] = params[i];
  a.shape = shape; a.app = app; a.art = art;
  // the block's form is the process default at the time of the call, remembered for `small`: a launch refuses a block and a stream of two forms
  const int form = fold_default();
  set_stream_form(small, form);
  prepare_art_kernel<<<dim3((kASmallFloats + 255) / 256), dim3(256), 0, stream>>>(a, small, min_deg, pos_levels, view_levels, form == kFormFolded ? 1 : 0);
  return hipGetLastError();
}

// both networks of a two-level model: per-call blocks + forward streams, one launch (the folded form's W' must be in place: fold_done)
hipError_t launch_pack_prepare_art2(const float* const* const params[2], const float* shape, const float* app, const float* art, float* const packed[2],
                                    float* const small[2], hipStream_t stream, int min_deg, int pos_levels, int view_levels, int form) {
  ArtPackPrep2Args a;   // (form: decided ONCE by the caller -- it has, or has not, run the fold products for it)
  for (int l = 0; l < 2; ++l) {
    for (int i = 0; i < kNumArtParams; ++i) a.net[l].p[i] = params[l][i];
    a.net[l].shape = shape; a.net[l].app = app; a.net[l].art = art;
    a.small[l] = small[l]; a.packed[l] = packed[l];
    set_stream_form(packed[l], form);
    set_stream_form(small[l], form);
  }
  const int64_t n = kAStreamBytes / 4;   // (either form: the whole buffer, see pack_art_element)
  const dim3 grid((unsigned)(kPrepBlocks + (n + 255) / 256), 2);
  if (form == kFormFolded) pack_prepare_art2_kernel<true><<<grid, dim3(256), 0, stream>>>(a, min_deg, pos_levels, view_levels);
  else pack_prepare_art2_kernel<false><<<grid, dim3(256), 0, stream>>>(a, min_deg, pos_levels, view_levels);
  return hipGetLastError();
}

template <bool POS, bool TRAIN, bool FOLD, bool VB = false, bool GATHER = false>
static hipError_t launch_art_tf(const ArtMlpArgs& args, hipStream_t stream) {
  static DeviceOnce lds_once;
  return launch_persistent(&art_mlp_fwd_kernel<POS, TRAIN, FOLD, VB, GATHER>, kALdsBytes, args.npass_total, lds_once, stream, args);
}

// the kernel of the form the launch's streams AND per-call blocks were made in (agreed_form); the per-ray view bias serves the in-kernel ray cast
template <bool POS, bool TRAIN, bool GATHER = false>
static hipError_t launch_art_t(const ArtMlpArgs& args, hipStream_t stream) {
  const int form = agreed_form(args);
  if (form == kFormUnknown) return hipErrorInvalidValue;
  if (args.seg[0].view_bias != nullptr) {
    if constexpr (POS) return launch_art_tf<POS, TRAIN, true, true, GATHER>(args, stream);
    else return hipErrorInvalidValue;
  }
  return form == kFormFolded ? launch_art_tf<POS, TRAIN, true, false, GATHER>(args, stream)
                             : launch_art_tf<POS, TRAIN, false, false, GATHER>(args, stream);
}

// views_linear.0's effective bias (per-call block: appearance latent and W_v0[:, :256] b_b folded in) + its view-encoding term, per ray
hipError_t launch_art_view_bias(const char* packed, const float* small, const float* viewdirs, int64_t n_rays, float* out, hipStream_t stream) {
  if (stream_form(packed) != kFormFolded || stream_form(small) != kFormFolded) return hipErrorInvalidValue;
  constexpr int64_t off = (int64_t)kAChT0 * kSmallChunkBytes + (int64_t)(kAChFV0 - kAChT0) * kBigChunkBytes;
  return launch_view_bias_raw(reinterpret_cast<const float*>(packed + off), small + kA_BV, viewdirs, n_rays, out, stream);
}

// The one forward launch of the articulated network: one or two segments in ONE persistent launch (see ArtSeg), the kernel instance read
// off what the segments hold (fwd_form) -- planes: the training forward; gather_idx: the samples of an occupancy list (aon_mlp_core.h);
// pos / viewdirs_enc: caller-made positions instead of the in-kernel ray cast.  A combination no instance serves (the training forward on
// caller-made positions, the vanilla network's deferred trunk) is hipErrorInvalidValue, as are an unknown form, mixed forms and a view bias
// on caller-made positions.
hipError_t launch_art_mlp_fwd(const FwdSeg* segs, int nsegs, hipStream_t stream) {
  const FwdForm f = fwd_form(segs, nsegs);
  if (!f.ok || f.defer || (f.train && f.own_inputs)) return hipErrorInvalidValue;
  ArtMlpArgs args{};
  for (int i = 0; i < nsegs; ++i) {
    if (segs[i].samples_enc) return hipErrorInvalidValue;   // the vanilla network's caller-made input
    fill_seg(args.seg[i], segs[i]);
  }
  finish_segs(args, nsegs);
  if (f.gather) return launch_art_t<true, false, true>(args, stream);
  if (f.train) return launch_art_t<true, true>(args, stream);
  return f.own_inputs ? launch_art_t<false, false>(args, stream) : launch_art_t<true, false>(args, stream);
}

// ---- density on a grid (aon_art_density_grid): deformation MLP -> encoding of x' -> trunk -> density head ----
// The stream truncated after layer 7: chunks 0 .. 71, which the literal and the folded forms share (aon_art_common.h); the prefetch of the
// next pass's first pair wraps at chunk 70.
struct ArtTrunkNet {
  static constexpr int kSlotBytes = kPairSlotBytes;
  static constexpr bool kPair = true;
  static constexpr int kNumChunks = kAChBott;
  static constexpr int chunk_bytes(int c) { return c < kAChT0 ? kSmallChunkBytes : kBigChunkBytes; }
};

// art_mlp_fwd_kernel up to its raw sigma -- the same deform_fwd and trunk_fwd, so the same operations in the same order and the same
// bits -- on points generated from the grid (grid_point)
__global__ void __launch_bounds__(256) art_density_grid_kernel(GridArgs args) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = lane & 31, h = lane >> 5;
  run_passes_one<ArtTrunkNet, kASmallFloats>(args.packed, args.small, args.npass, [&](int pass, Pipe& p, const float* sm) __attribute__((always_inline)) {
    const int64_t l0 = (int64_t)pass * 128 + wave * 32;
    const int64_t l = l0 + m;
    float x[3], xd[3];
    grid_point(args, l < args.total ? l : args.total - 1, x);
    NoTaps taps;
    deform_fwd<ArtTrunkNet>(p, x, sm, h, taps, xd);
    f32x16 E[2], X[8], Y[8];
    encode_pos_scaled(xd, h, sm + kA_ESC, E);
    const float sigma = trunk_fwd<ArtTrunkNet, ArtTrunk>(p, E, X, Y, sm, h, taps);
    grid_store(args.out, l0, args.total, lane, grid_activation(sigma, args.act));
  });
}

hipError_t launch_art_density_grid(const char* packed, const float* small, const int64_t* dims, const float* lo, const float* step,
                                   int64_t g_begin, int64_t g_end, int act, float* out, hipStream_t stream) {
  const int form = stream_form(packed);
  if (form == kFormUnknown || stream_form(small) != form) return hipErrorInvalidValue;   // as agreed_form
  static DeviceOnce lds_once;
  const GridArgs a = make_grid_args(packed, small, dims, lo, step, g_begin, g_end, act, out);
  return launch_persistent(&art_density_grid_kernel, kALdsBytes, a.npass, lds_once, stream, a);
}

int64_t art_stream_bytes() { return kAStreamBytes; }
int64_t art_small_bytes() { return (int64_t)kASmallFloats * 4; }

}  // namespace aon
