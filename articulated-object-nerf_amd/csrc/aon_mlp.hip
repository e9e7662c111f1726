// Fused vanilla NeRFMLP forward for gfx950 (MI355X / CDNA4): encode -> 8x256 trunk (+skip) -> sigma head,
// bottleneck -> view branch -> rgb head, one launch, activations never leave the register file.
//
// Replaces the eager-op sequence of the reference's  helper.cast_rays + helper.pos_enc + NeRFMLP.forward
// (models/vanilla_nerf/helper.py:25-26,136-140; models/vanilla_nerf/model.py:95-120).
//
// Mapping onto CDNA4 (not a GEMM-library call chain, not a CUDA tiling):
//   * one workgroup = 4 waves = one wave per SIMD; each wave owns 32 samples for the whole network.
//   * every layer is computed TRANSPOSED:  out^T[feature][sample] = W[feature][k] * act^T[k][sample]
//     with v_mfma_f32_32x32x2_f32 (exact fp32, bit-equal to an fmaf chain).  The weights are the A operand,
//     the activations the B operand.  In that orientation the accumulator layout of a 32x32 tile
//     (lane l, reg r  ->  feature (r&3)+8*(r>>2)+4*(l>>5), sample l&31) is *already* a valid B-operand
//     layout for the next layer: lanes 0-31 supply "k=0", lanes 32-63 "k=1" of a 2-deep MFMA step, and the
//     k order of a dot product is free as long as the weight operand is permuted the same way.  The
//     host-side pack kernel bakes that permutation into the weight stream once, so activations stay in
//     VGPR/AGPRs from the positional encoding to the rgb/sigma heads: no LDS or HBM round trip per layer.
//   * weights stream HBM/L2 -> LDS with LDS-DMA (global_load_lds_dwordx4, lane-linear image) in 32 KiB chunks
//     (one 32-feature input tile x all output tiles), double-buffered; the 4 waves share each chunk and
//     read their A operands with conflict-free ds_read_b128 (4 MFMA steps per read).
//   * per 128-sample pass a wave issues ~9.3k MFMAs (64 cycles each) against ~2.4k ds_read_b128 and a few
//     hundred VALU ops (bias init, ReLU, heads), so the kernel is bound by the fp32 matrix pipe.
#include "aon_pass.h"

namespace aon {

struct VanillaNet {
  static constexpr int kSlotBytes = kPairSlotBytes;  // a slot holds a pair of chunks
  static constexpr bool kPair = true;
  static constexpr int kNumChunks = aon::kNumChunks;
  static constexpr int chunk_bytes(int c) { return aon::chunk_bytes(c); }
};
// bottleneck_layer folded into views_linear[0] (aon_common.h): chunks 0 .. 59 of the literal stream, the view-encoding chunk, 8 small chunks of W'
struct VanillaFoldNet {
  static constexpr int kSlotBytes = kPairSlotBytes;
  static constexpr bool kPair = true;
  static constexpr int kNumChunks = aon::kNumChunksF;
  static constexpr int chunk_bytes(int c) { return aon::chunk_bytes_f(c); }
};
// ... with the view-encoding term as a per-ray bias: the same buffer without its chunk 60 (chunk c >= 60 here is chunk c + 1 there)
struct VanillaFoldVbNet {
  static constexpr int kSlotBytes = kPairSlotBytes;
  static constexpr bool kPair = true;
  static constexpr int kNumChunks = aon::kNumChunksF - 1;
  static constexpr int chunk_bytes(int c) { return aon::chunk_bytes_f(c < kChFView ? c : c + 1); }
  static constexpr int skip_before(int c) { return c == kChFView ? kSmallChunkBytes : 0; }
};

// (density grid, deferred-view trunk) The stream truncated after layer 7: chunks 0 .. 59, which the literal and the folded forms share (aon_common.h).  The prefetch of the
// next pass's first pair wraps at chunk 58 here (first_wrapping_chunk), not at the end of the view branch.
struct VanillaTrunkNet {
  static constexpr int kSlotBytes = kPairSlotBytes;
  static constexpr bool kPair = true;
  static constexpr int kNumChunks = kChBott;
  static constexpr int chunk_bytes(int) { return kBigChunkBytes; }
};

// ---------------------------------------------------------------------------------------------
// weight packing
// ---------------------------------------------------------------------------------------------
struct PackArgs {
  const float* p[kNumVanillaParams];
};

// (pos_col_in / view_col_in: aon_mlp_core.h)
// FOLD: the folded form (aon_common.h).  W' / b' were written to packed + kFoldTmpOff by launch_fold_view on the same stream; the pack
// kernel's own writes stay below kStreamBytesF, behind W' / b', or at / above kStreamBytes, so it never overwrites what it reads.
template <bool FOLD>
__global__ void pack_vanilla_kernel(PackArgs a, float* __restrict__ packed, int L, int Lv) {
  const int P = enc_width(L), V = enc_width(Lv);
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  constexpr int64_t stream_floats = kStreamBytes / 4;
  constexpr int64_t used_floats = FOLD ? kStreamBytesF / 4 : stream_floats;
  const float* Wf = packed + kFoldTmpOff / 4;      // [FOLD] (128, 256), then b' (128)
  if (idx >= stream_floats + kSmallFloats) return;
  if (idx >= used_floats && idx < stream_floats) {   // [FOLD] the fold temporaries, then the unused tail of the literal-size buffer:
    if (idx >= used_floats + 128 * 256 + 128) packed[idx] = 0.f;   // zeroed, so that every byte of the buffer the caller handed in is defined
    return;
  }
  if (idx >= stream_floats) {  // resident small vectors
    const int s = (int)(idx - stream_floats);
    float v = 0.f;
    if (s < kSmBiasBott) v = a.p[vp_trunk_b(s >> 8)][s & 255];
    else if (s < kSmBiasView) v = a.p[kVpBottB][s - kSmBiasBott];
    else if (s < kSmWSigma) v = FOLD ? Wf[128 * 256 + s - kSmBiasView] : a.p[kVpView0B][s - kSmBiasView];
    else if (s < kSmWRgb) v = a.p[kVpSigmaW][s - kSmWSigma];
    else if (s < kSmBSigma) v = a.p[kVpRgbW][s - kSmWRgb];
    else if (s < kSmBRgb) v = a.p[kVpSigmaB][0];
    else if (s < kSmBRgb + 3) v = a.p[kVpRgbB][s - kSmBRgb];
    packed[idx] = v;
    return;
  }
  int c, r, nt;
  constexpr int nbig = FOLD ? kChFView : kNumBigChunks;
  if (idx < (int64_t)nbig * (kBigChunkBytes / 4)) {
    c = (int)(idx / (kBigChunkBytes / 4)); r = (int)(idx % (kBigChunkBytes / 4)); nt = 8;
  } else {
    const int64_t i2 = idx - (int64_t)nbig * (kBigChunkBytes / 4);
    c = nbig + (int)(i2 / (kSmallChunkBytes / 4)); r = (int)(i2 % (kSmallChunkBytes / 4)); nt = 4;
    // the folded view chunks take the literal view layer's branches below, with W' for the hidden columns; the view-encoding chunk is the
    // FIRST of the folded view layer (aon_common.h), the last of the literal one
    if constexpr (FOLD) c = c == kChFView ? kChView + 8 : c - 1 + (kChView - kChFView);
  }
  const int cc = r & 3, lane = (r >> 2) & 63, rest = r >> 8;
  const int tp = rest % nt, q = rest / nt;
  const int h = lane >> 5, row = 32 * tp + (lane & 31);
  const float* W; int ld, n_out = 256, col;
  const int hid_col = 8 * q + 4 * h + cc;  // + 32*T
  auto pcol = [&](int c63) { return c63 < 0 ? -1 : pos_col_in(c63, L); };
  auto vcol = [&](int c27) { return c27 < 0 ? -1 : view_col_in(c27, Lv); };
  if (c < kChL1) { W = a.p[vp_trunk_w(0)]; ld = vp_trunk0_ld(P); col = pcol(posenc_col(c, q, cc, h)); }
  else if (c < kChL5) { const int l = 1 + (c - kChL1) / 8; W = a.p[vp_trunk_w(l)]; ld = 256; col = 32 * ((c - kChL1) % 8) + hid_col; }
  else if (c < kChL5 + 8) { W = a.p[vp_trunk_w(5)]; ld = vp_trunk5_ld(P); col = 32 * (c - kChL5) + hid_col; }
  else if (c < kChL6) { W = a.p[vp_trunk_w(5)]; ld = vp_trunk5_ld(P); col = pcol(posenc_col(c - kChL5 - 8, q, cc, h)); if (col >= 0) col += kTrunk5EncCol; }
  else if (c < kChL7) { W = a.p[vp_trunk_w(6)]; ld = 256; col = 32 * (c - kChL6) + hid_col; }
  else if (c < kChBott) { W = a.p[vp_trunk_w(7)]; ld = 256; col = 32 * (c - kChL7) + hid_col; }
  else if (c < kChView) { W = a.p[kVpBottW]; ld = 256; col = 32 * (c - kChBott) + hid_col; }
  else if (c < kChView + 8) {
    W = a.p[kVpView0W]; ld = vp_view0_ld(V); n_out = kCondWidth; col = 32 * (c - kChView) + hid_col;
    if constexpr (FOLD) { W = Wf; ld = 256; }
  }
  else { W = a.p[kVpView0W]; ld = vp_view0_ld(V); n_out = kCondWidth; col = vcol(viewenc_col(q, cc, h)); if (col >= 0) col += kView0EncCol; }
  packed[idx] = (col >= 0 && row < n_out) ? W[(int64_t)row * ld + col] : 0.f;
}

// ---------------------------------------------------------------------------------------------
// fused forward
// ---------------------------------------------------------------------------------------------
// One SEGMENT of a launch: a run of 128-sample passes of one network over one ray range (see ArtSeg, aon_mlp_art.hip: the training
// forward merges the fine level of one ray range with the coarse level of another into ONE persistent launch).
struct MlpSeg {
  const char* packed;        // kPackedBytes
  const float* rays_o;       // (n_rays,3)      [ENC_IN_KERNEL]
  const float* rays_d;       // (n_rays,3)
  const float* viewdirs;     // (n_rays,3)
  const float* t_vals;       // (n_rays,S)
  const float* samples_enc;  // (n_rays*S,63)   [!ENC_IN_KERNEL]
  const float* viewdirs_enc; // (n_rays,27)
  float* raw;                // (n_rays*S,4) = raw rgb, raw sigma
  int64_t total;             // n_rays*S
  int S;
  int npass;                 // ceil(total/128)
  union {
    float* planes;             // [TRAIN] kPlRows x Np activation planes, step-major (aon_mlp_core.h)
    const int* gather_idx;     // [GATHER] ascending sample indices of the segment (< total)
    float* live_rows;          // [DEFER] (total, 256): the post-ReLU layer-7 output of every live sample, one 1 KiB row at the sample's index
  };
  union {
    u32x4* masks;              // [TRAIN] kMaskLayers x (Np*2) ReLU bit masks
    const int64_t* gather_count;   // [GATHER] number of entries of gather_idx (device)
    uint8_t* live_mark;        // [DEFER] (total,): 1 where raw sigma > 0, else 0 (the compaction's ray_live bytes, one "row" per sample)
  };
  int64_t Np;                // npass * 128
  const float* view_bias;    // [VB] (n_rays,128): b' + W_v0[:, 256:] ve of the ray (view_bias_kernel)
  static constexpr bool kPerCallBlock = false;   // the small block follows the stream
};
struct MlpArgs {
  MlpSeg seg[2];
  int npass_total;           // seg[0].npass + seg[1].npass (seg[1].npass == 0: a one-segment launch)
};
__host__ __device__ __forceinline__ const char* seg_stream(const MlpSeg& s) { return s.packed; }
__device__ __forceinline__ const float* seg_small(const MlpSeg& s) { return reinterpret_cast<const float*>(s.packed + kStreamBytes); }

constexpr int kLdsBytes = kRingBytes + (int)kSmallBytes;

struct VanillaTrunk {   // trunk_fwd's view of the vanilla stream, small block, planes and decision bits
  static constexpr int kL0 = kChL0, kL1 = kChL1, kL5 = kChL5, kL6 = kChL6, kL7 = kChL7;
  static constexpr int kBias = kSmBias, kWSigma = kSmWSigma, kBSigma = kSmBSigma, kMask0 = 0;
  static constexpr int plane(int l) { return plane_h(l); }
};

// TRAIN additionally stores every layer's input/output activations as step-major planes (aon_mlp_core.h) for the backward pass.
// FOLD: the stream is the folded form -- the view layer reads the post-ReLU layer-7 output through W' (aon_common.h), there is no
// bottleneck layer (and, [TRAIN], no bottleneck rows in the planes: rows kPlBot .. kPlBot + 255 stay unwritten).
// VB (folded form only): the view layer's accumulators start from the ray's b' + W_v0[:, 256:] ve, fetched from `view_bias` while the last
// chunk of layer 7 runs, instead of from b' followed by the view-encoding chunk -- same bits (aon_common.h), 56 MFMAs, 12 sines and a
// 16 KiB chunk fewer per pass; the inference kernel no longer carries the 16 registers of the view encoding through the trunk.
// GATHER (inference on the in-kernel encodings only): the samples of a pass come from an occupancy list (aon_mlp_core.h).
// DEFER (the VB inference form only): the TRUNK of that form.  The kernel ends behind layer 7 and the density head
// -- the stream is the buffer's chunks 0 .. 59 (VanillaTrunkNet), no view-bias loads, no view layer, no rgb head -- and writes the record
// (+0, +0, +0, raw sigma), the sample's mark (raw sigma > 0; NaN is not) and, for a marked sample only, its 256 post-ReLU layer-7 values
// as a 1 KiB row in feature order: a quad of accumulator registers is four consecutive features, so the row goes out in 32 16-byte
// stores straight from the registers.  view_kernel below finishes the marked samples from their rows.
template <bool ENC_IN_KERNEL, bool TRAIN, bool FOLD, bool VB = false, bool GATHER = false, bool DEFER = false>
__global__ void __launch_bounds__(256) mlp_fwd_kernel(MlpArgs args) {
  static_assert(FOLD || !VB, "the per-ray view bias belongs to the folded form");
  static_assert(!GATHER || (ENC_IN_KERNEL && !TRAIN), "the occupancy list serves the inference kernel on in-kernel encodings");
  static_assert(!DEFER || (ENC_IN_KERNEL && !TRAIN && VB && !GATHER), "the deferred view branch serves the dense per-ray-bias inference form");
  using Net = std::conditional_t<DEFER, VanillaTrunkNet, std::conditional_t<VB, VanillaFoldVbNet, std::conditional_t<FOLD, VanillaFoldNet, VanillaNet>>>;
  // <false, true>: training on caller-encoded inputs (other encoding degrees in the padded 63 / 27-slot layout): where the
  // in-kernel form re-encodes from x[] / vd[], this one re-reads the encodings.
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int m = lane & 31, h = lane >> 5;
  const int wave_s = __builtin_amdgcn_readfirstlane(wave);   // the step base of the training planes is wave-uniform: keep it scalar

  run_passes<Net, kSmallFloats, GATHER>(args, [&](const MlpSeg& sg, int pass, Pipe& p, const float* sm, int64_t listed = 0) __attribute__((always_inline)) {
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

    // ---- encode: E[0..1] = 63-wide positional encoding, V = 27-wide view encoding, accumulator layout ----
    f32x16 E[2], V;
    float x[3] = {0.f, 0.f, 0.f}, vd[3] = {0.f, 0.f, 0.f};
    if constexpr (ENC_IN_KERNEL) {
      const float t = sg.t_vals[gc];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        // helper.cast_rays (helper.py:25-26): origins + t * directions, multiply then add
        x[a] = __fadd_rn(sg.rays_o[ray * 3 + a], __fmul_rn(t, sg.rays_d[ray * 3 + a]));
        vd[a] = sg.viewdirs[ray * 3 + a];
      }
      encode_pos(x, h, E);
      if constexpr (!VB || TRAIN) encode_view(vd, h, V);   // [VB] only the training planes still want the view encoding
    } else {
      load_pos_enc(sg.samples_enc + gc * kPosEnc, h, E);
      if constexpr (!VB || TRAIN) load_view_enc(sg.viewdirs_enc + ray * kViewEnc, h, V);
    }
    int ray32 = (int)ray;   // [VB] the one value of the prologue that is still needed at the view layer
    (void)ray32;

    PlaneIO io{};
    unsigned moff = 0;
    if constexpr (TRAIN) { io = make_plane_io(sg.planes, kPlRows, (int64_t)pass * 4 + wave_s, m, h); moff = mask_lane_off(pass, tid); }
    if constexpr (TRAIN) {
      store_pos_enc_plane(E, io, kPlE, h);
      store_view_enc_plane(V, io, kPlVE, h);
    }
    FwdTaps<TRAIN, MlpSeg> taps{sg, io, moff};   // [TRAIN] planes and decision bits, as side jobs of the consuming chunks
    f32x16 X[8], Y[8], Z[4];
    // (the in-kernel encoding stays live across layers 1-4, 32 registers, as in the inference kernel: with the view encoding gone from the
    // trunk every form builds with 0 scratch, and re-encoding at layer 5 -- 30 sines -- was the slower way: see art_mlp_fwd_kernel)
    auto reread_enc = [&]() {
      if constexpr (TRAIN && !ENC_IN_KERNEL) {
        int64_t gq = gc;
        asm volatile("" : "+v"(gq));   // opaque: a second read, not the first one kept live
        load_pos_enc(sg.samples_enc + gq * kPosEnc, h, E);
      }
    };
    auto l7_side = [&](auto plain) {
      if constexpr (VB && !DEFER) {
        asm volatile("" : "+v"(ray32));
        return view_bias_side(plain, sg.view_bias + (int64_t)ray32 * kCondWidth + 4 * h, Z);
      } else {
        return plain;
      }
    };
    const float sigma = trunk_fwd<Net, VanillaTrunk>(p, E, X, Y, sm, h, taps, reread_enc, l7_side);
    if constexpr (DEFER) {
      const bool live = sigma > 0.f;   // both half-waves hold the same sum (a + b == b + a)
      if (valid) {
        if (h == 0) {
          f32x4 o; o[0] = 0.f; o[1] = 0.f; o[2] = 0.f; o[3] = sigma;
          reinterpret_cast<f32x4*>(sg.raw)[g] = o;
          sg.live_mark[g] = live ? 1 : 0;
        }
        if (live) {
          char* row = reinterpret_cast<char*>(sg.live_rows) + g * 1024 + h * 16;   // features 32 t + 8 q + 4 h + {0..3}
#pragma unroll
          for (int t = 0; t < 8; ++t) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              f32x4 v; v[0] = Y[t][4 * q]; v[1] = Y[t][4 * q + 1]; v[2] = Y[t][4 * q + 2]; v[3] = Y[t][4 * q + 3];
              // streaming (`nt`) stores, as the training planes' (store_quad): the rows are read back once, by view_kernel, and written with
              // the default policy they push the weight stream out of the L2 (measured: 564.7 against 568.0 ms per 640x480 frame)
              __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(row + (32 * t + 8 * q) * 4));
            }
          }
        }
      }
    } else {
      constexpr int kChV = FOLD ? kChFView : kChView;
      auto reencode_view = [&]() {   // [TRAIN] the view encoding again (same function, same bits): 16 registers not held across the trunk
        if constexpr (TRAIN && ENC_IN_KERNEL) {
          asm volatile("" : "+v"(vd[0]), "+v"(vd[1]), "+v"(vd[2]));
          encode_view(vd, h, V);
        }
        if constexpr (TRAIN && !ENC_IN_KERNEL) {
          int64_t rq = ray;
          asm volatile("" : "+v"(rq));
          load_view_enc(sg.viewdirs_enc + rq * kViewEnc, h, V);
        }
      };
      if constexpr (FOLD) {
        // bottleneck (no activation, model.py:109) and the view layer's hidden columns (model.py:110-116) as ONE layer W' = W_v0[:, :256] W_b,
        // b' = W_v0[:, :256] b_b + b_v0 on the post-ReLU layer-7 output; the view-encoding columns FIRST (chunk form) or already in Z (VB)
        if constexpr (!VB) {
          init_bias(Z, sm + kSmBiasView, h);
          reencode_view();
          chunk_mma<Net, kChV, 4, 14>(p, V, Z);
        }
        dense_layer<Net, kChV + (VB ? 0 : 1), 8, 4>(p, Y, Z, taps.consume(Y, plane_h(7), true)); taps.put_mask(7);
      } else {
        // bottleneck, no activation (model.py:109)
        init_bias(X, sm + kSmBiasBott, h); dense_layer<Net, kChBott, 8, 8>(p, Y, X, taps.consume(Y, plane_h(7), true)); taps.put_mask(7);
        // view branch: cat[bottleneck(256), viewenc(27)] -> 128, ReLU (model.py:110-116)
        init_bias(Z, sm + kSmBiasView, h);
        dense_layer<Net, kChV, 8, 4>(p, X, Z, taps.consume(X, kPlBot, false));
        reencode_view();
        chunk_mma<Net, kChV + 8, 4, 14>(p, V, Z);
      }
      relu_tiles(Z);
      taps.burst(Z, kPlHV, 8);   // the view layer's output feeds the rgb head on the VALU
      // rgb head (model.py:118)
      float rgb[3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        float v = head_partial<4>(Z, sm + kSmWRgb + ch * kCondWidth, h);
        rgb[ch] = v + __shfl_xor(v, 32) + sm[kSmBRgb + ch];
      }
      if (valid && h == 0) {
        f32x4 o; o[0] = rgb[0]; o[1] = rgb[1]; o[2] = rgb[2]; o[3] = sigma;
        reinterpret_cast<f32x4*>(sg.raw)[g] = o;
      }
    }
  });
}

// ---------------------------------------------------------------------------------------------
// host launchers (called from the C ABI)
// ---------------------------------------------------------------------------------------------
// The form packed is the process default at the time of the call (aon_set_bottleneck_fold), remembered for `packed` (stream_form).
// W' and b' of one network into the fold area of its forward stream (the jobs launch_pack_vanilla runs unless told they have been run)
void vanilla_fold_jobs_fwd(const float* const* params, float* packed, int view_levels, FoldGemm jobs[2]) {
  float* Wf = packed + kFoldTmpOff / 4;
  fold_view_jobs(params[kVpView0W], vp_view0_ld(enc_width(view_levels)), params[kVpView0B], params[kVpBottW], params[kVpBottB], Wf, Wf + 128 * 256, jobs);
}

hipError_t launch_pack_vanilla(const float* const* params, float* packed, hipStream_t stream, int pos_levels, int view_levels, bool fold_done) {
  PackArgs a;
  for (int i = 0; i < kNumVanillaParams; ++i) a.p[i] = params[i];
  const int64_t n = kStreamBytes / 4 + kSmallFloats;
  const int form = fold_default();
  set_stream_form(packed, form);
  if (form == kFormFolded) {
    if (!fold_done) {   // (aon_vanilla_pack_step runs the products of both networks and both directions as ONE launch in front)
      FoldGemm jobs[2];
      vanilla_fold_jobs_fwd(params, packed, view_levels, jobs);
      if (hipError_t e = launch_fold_gemms(jobs, 2, stream); e != hipSuccess) return e;
    }
    pack_vanilla_kernel<true><<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream>>>(a, packed, pos_levels, view_levels);
  } else {
    pack_vanilla_kernel<false><<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream>>>(a, packed, pos_levels, view_levels);
  }
  return hipGetLastError();
}

int num_cus() {  // CUs of the CURRENT device, cached per device ordinal (ops.py may drive any tensor.device)
  static std::atomic<int> cache[kMaxDevices];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return -1;
  if (dev < 0 || dev >= kMaxDevices) return -1;
  int cus = cache[dev].load(std::memory_order_relaxed);
  if (cus == 0) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return -1;
    cus = prop.multiProcessorCount;
    cache[dev].store(cus, std::memory_order_relaxed);
  }
  return cus;
}

template <bool ENC, bool TRAIN, bool FOLD, bool VB = false, bool GATHER = false, bool DEFER = false>
static hipError_t launch_mlp_tf(const MlpArgs& args, hipStream_t stream) {
  static DeviceOnce lds_once;  // one per template instance
  return launch_persistent(&mlp_fwd_kernel<ENC, TRAIN, FOLD, VB, GATHER, DEFER>, kLdsBytes, args.npass_total, lds_once, stream, args);   // [GATHER] npass_total: the passes of a full list
}

// the kernel of the form the launch's streams were packed in (agreed_form); the per-ray view bias serves the whole-path calls on the
// in-kernel encodings
template <bool ENC, bool TRAIN, bool GATHER = false>
static hipError_t launch_mlp_t(const MlpArgs& args, hipStream_t stream) {
  const int form = agreed_form(args);
  if (form == kFormUnknown) return hipErrorInvalidValue;
  if (args.seg[0].view_bias != nullptr) {
    if constexpr (ENC) return launch_mlp_tf<ENC, TRAIN, true, true, GATHER>(args, stream);
    else return hipErrorInvalidValue;
  }
  return form == kFormFolded ? launch_mlp_tf<ENC, TRAIN, true, false, GATHER>(args, stream)
                             : launch_mlp_tf<ENC, TRAIN, false, false, GATHER>(args, stream);
}

// b' + W_v0[:, 256:] ve per ray, the head of the view layer's accumulation chains (aon_common.h): the fused multiply-adds the view-encoding
// chunk performs, in its order -- register r = 0 .. 13 of the encoding tile, half-wave 0 then 1 (one v_mfma_f32_32x32x2_f32 step adds the
// k = 0 product, then the k = 1 product) -- with the weights read from the packed chunk itself.  One workgroup serves eight rays.
__global__ __launch_bounds__(256) void view_bias_kernel(const float* chunk, const float* bias_vec, const float* viewdirs, int64_t n_rays, float* out) {
  __shared__ float enc[8][2][16];
  const int tid = threadIdx.x;
  const int64_t ray0 = (int64_t)blockIdx.x * 8;
  if (tid < 16) {
    const int64_t ray = ray0 + (tid >> 1);
    if (ray < n_rays) {
      float vd[3] = {viewdirs[ray * 3], viewdirs[ray * 3 + 1], viewdirs[ray * 3 + 2]};
      f32x16 V;
      encode_view(vd, tid & 1, V);
#pragma unroll
      for (int r = 0; r < 16; ++r) enc[tid >> 1][tid & 1][r] = V[r];
    }
  }
  const int row = tid & 127, tp = row >> 5;
  const float bias = bias_vec[row];
  float w[14][2];
#pragma unroll
  for (int r = 0; r < 14; ++r)
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) w[r][hh] = chunk[((((r >> 2) * 4 + tp) * 64 + hh * 32 + (row & 31)) << 2) + (r & 3)];
  __syncthreads();
  for (int k = tid >> 7; k < 8; k += 2) {
    const int64_t ray = ray0 + k;
    if (ray >= n_rays) break;
    float acc = bias;
#pragma unroll
    for (int r = 0; r < 14; ++r) {
      acc = __builtin_fmaf(w[r][0], enc[k][0][r], acc);
      acc = __builtin_fmaf(w[r][1], enc[k][1][r], acc);
    }
    out[ray * kCondWidth + row] = acc;
  }
}

// chunk: the view-encoding chunk of a folded stream (4 output tiles); bias_vec: the 128 biases the chunk form starts the view layer from
hipError_t launch_view_bias_raw(const float* chunk, const float* bias_vec, const float* viewdirs, int64_t n_rays, float* out, hipStream_t stream) {
  if (n_rays <= 0) return hipSuccess;
  view_bias_kernel<<<dim3((unsigned)((n_rays + 7) / 8)), dim3(256), 0, stream>>>(chunk, bias_vec, viewdirs, n_rays, out);
  return hipGetLastError();
}

hipError_t launch_view_bias(const char* packed, const float* viewdirs, int64_t n_rays, float* out, hipStream_t stream) {
  if (stream_form(packed) != kFormFolded) return hipErrorInvalidValue;
  return launch_view_bias_raw(reinterpret_cast<const float*>(packed + chunk_offset_f(kChFView)), reinterpret_cast<const float*>(packed + kStreamBytes) + kSmBiasView,
                              viewdirs, n_rays, out, stream);
}

// ---------------------------------------------------------------------------------------------
// deferred view branch: the view layer and the rgb head of the LISTED samples of a trunk launch
// ---------------------------------------------------------------------------------------------
// The vanilla density is relu(raw sigma): a sample with raw sigma <= 0 composites with weight exactly 0 and its colour is never seen.  The
// DEFER instance of mlp_fwd_kernel stops behind the density head; the live samples are compacted (aon_occ.hip) and this kernel runs the
// folded view layer W' (256 -> 128), its ReLU and the rgb head on them alone -- the operations of mlp_fwd_kernel's VB form in its order, so
// the same bits: accumulators from the ray's view bias, then input tile j = 0 .. 7, register quad q, output tile tp, four two-deep MFMA
// steps each (chunk_mma with NT_OUT = 4).  One wave = 32 listed samples, one wave per SIMD; W' (the stream's chunks 61 .. 68, 128 KiB) and
// the small block sit in LDS for the whole launch: no ring, no barrier after the first.  The rows of a wave's NEXT tile are fetched into a
// second register set while the current tile's MFMAs run.
struct ViewArgs {
  const char* packed;        // the level's folded stream
  const float* rows;         // (total, 256) post-ReLU layer-7 rows, written for the listed samples
  const int* idx;            // ascending live sample indices
  const int64_t* count;      // their number (device)
  const float* view_bias;    // (n_rays, 128)
  float* raw;                // (total, 4): rgb of the listed samples is written, sigma stays
  int S;
};
constexpr int kViewWBytes = 8 * kSmallChunkBytes;
constexpr int kViewLdsBytes = kViewWBytes + (int)kSmallBytes;

__device__ __forceinline__ int view_listed(const ViewArgs& a, int64_t listed, int64_t tile, int m) {
  const int64_t e = tile * 32 + m;
  return a.idx[e < listed ? e : listed - 1];   // a partial last tile repeats the last entry; its lanes do not store
}
// rows of input tile t of sample g: features 32 t + 8 q + 4 h + {0..3}, the accumulator layout the trunk stored them from
__device__ __forceinline__ void view_gather_tile(const ViewArgs& a, int g, int h, int t, f32x16& Y) {
  const char* row = reinterpret_cast<const char*>(a.rows) + (int64_t)g * 1024 + h * 16;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(row + (32 * t + 8 * q) * 4);
    Y[4 * q] = v[0]; Y[4 * q + 1] = v[1]; Y[4 * q + 2] = v[2]; Y[4 * q + 3] = v[3];
  }
}
__device__ __forceinline__ void view_bias_init(const ViewArgs& a, int g, int h, f32x16 (&Z)[4]) {
  const float* vb = a.view_bias + (int64_t)(g / a.S) * kCondWidth + 4 * h;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(vb + 32 * (i >> 2) + 8 * (i & 3));
    Z[i >> 2][4 * (i & 3)] = v[0]; Z[i >> 2][4 * (i & 3) + 1] = v[1]; Z[i >> 2][4 * (i & 3) + 2] = v[2]; Z[i >> 2][4 * (i & 3) + 3] = v[3];
  }
}
// Z[tp] += W'[tp][input tile j] Y: chunk_mma's steps for NT_OUT = 4, NREG = 16 (q = i / 4, tp = i % 4, four two-deep MFMA steps each)
// Z0: the tile's view bias; chunk 0's first step into each output tile takes it as the C operand (the fused multiply-add a zero-cost copy
// would feed), so the bias of the NEXT samples can land in its own registers while this tile's accumulators are busy
__device__ __forceinline__ void view_chunk(const char* w, int j, int lane, const f32x16& Y, f32x16 (&Z)[4], const f32x16 (&Z0)[4]) {
  const char* buf = w + j * kSmallChunkBytes + lane * 16;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int q = i / 4, tp = i % 4;
    const f32x4 av = *reinterpret_cast<const f32x4*>(buf + i * 1024);
#pragma unroll
    for (int cc = 0; cc < 4; ++cc)
      Z[tp] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cc], Y[4 * q + cc], (j == 0 && q == 0 && cc == 0) ? Z0[tp] : Z[tp], 0, 0, 0);
  }
}

__global__ void __launch_bounds__(256) view_kernel(ViewArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int64_t listed = *a.count;
  const int64_t ntiles = (listed + 31) / 32;
  if ((int64_t)blockIdx.x * 4 >= ntiles) return;   // (workgroup-uniform; an empty list: every workgroup leaves here)
  float* sm = reinterpret_cast<float*>(smem + kViewWBytes);
  {
    const f32x4* src = reinterpret_cast<const f32x4*>(a.packed + chunk_offset_f(kChFView + 1));
    f32x4* dst = reinterpret_cast<f32x4*>(smem);
    for (int i = threadIdx.x; i < kViewWBytes / 16; i += 256) dst[i] = src[i];
  }
  load_small_block<kSmallFloats>(sm, reinterpret_cast<const float*>(a.packed + kStreamBytes));
  __syncthreads();
  const int lane = threadIdx.x & 63, m = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t stride = (int64_t)gridDim.x * 4;
  int64_t tile = (int64_t)blockIdx.x * 4 + wave;
  if (tile >= ntiles) return;
  // ONE set of 8 input tiles: tile j of the wave's NEXT 32 samples is fetched into the registers of tile j as soon as the current samples'
  // chunk j has consumed them, so every row load has 7/8 of a tile's MFMAs (12 us) to arrive.  The next samples' view bias is fetched in
  // the middle of the tile into a set of its own (Zb): vmcnt retires in order, and the bias is the first thing the next tile waits for.
  f32x16 Y[8], Z[4], Zb[4];
  int g = view_listed(a, listed, tile, m);
  int gn = view_listed(a, listed, tile + stride, m);
  __builtin_amdgcn_sched_barrier(0);   // the loop's order here too -- list entries, bias, rows: its waits are sized for the later of its two entries
  view_bias_init(a, g, h, Zb);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int t = 0; t < 8; ++t) view_gather_tile(a, g, h, t, Y[t]);
  __builtin_amdgcn_sched_barrier(0);
  while (true) {
    // (no branch around the fetches: the wave's last tiles re-read the list's last entry -- valid memory -- because a load that may or
    // may not have been issued makes every later vmcnt wait for everything.  The list entry is fetched TWO tiles ahead: the row
    // addresses of the next tile are formed early in this one, and a wait for an entry fetched here would be a wait for every row.)
    const int64_t nxt = tile + stride;
    const int gnn = view_listed(a, listed, nxt + stride, m);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      view_chunk(smem, j, lane, Y[j], Z, Zb);
      __builtin_amdgcn_sched_barrier(0);
      view_gather_tile(a, gn, h, j, Y[j]);
      if (j == 3) view_bias_init(a, gn, h, Zb);
      __builtin_amdgcn_sched_barrier(0);
    }
    relu_tiles(Z);
    float rgb[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float v = head_partial<4>(Z, sm + kSmWRgb + ch * kCondWidth, h);
      rgb[ch] = v + __shfl_xor(v, 32) + sm[kSmBRgb + ch];
    }
    if (tile * 32 + m < listed && h == 0) {
      float* rec = a.raw + (int64_t)g * 4;
      rec[0] = rgb[0]; rec[1] = rgb[1]; rec[2] = rgb[2];
    }
    if (nxt >= ntiles) break;
    tile = nxt; g = gn; gn = gnn;
  }
}

// ... and the view branch of the listed samples (view_kernel); max_listed: an upper bound of *count, which only sizes the grid
hipError_t launch_view_deferred(const char* packed, const float* live_rows, const int* idx, const int64_t* count, int64_t max_listed,
                                const float* view_bias, int S, float* raw, hipStream_t stream) {
  if (stream_form(packed) != kFormFolded) return hipErrorInvalidValue;
  if (max_listed <= 0) return hipSuccess;
  static DeviceOnce lds_once;
  if (hipError_t e = set_max_lds(&view_kernel, kViewLdsBytes, lds_once); e != hipSuccess) return e;
  const int cus = num_cus();
  if (cus <= 0) return hipErrorInvalidDevice;
  const int64_t groups = (max_listed + 127) / 128;
  const ViewArgs a{packed, live_rows, idx, count, view_bias, raw, S};
  view_kernel<<<dim3((unsigned)(groups < cus ? groups : cus)), dim3(256), kViewLdsBytes, stream>>>(a);
  return hipGetLastError();
}

// The one forward launch of the vanilla network: one or two segments in ONE persistent launch (see MlpSeg), the kernel instance read off
// what the segments hold (fwd_form) --
//   planes: the training forward, which also stores the activation planes (kPlRows x Np floats, Np = 128*ceil(n*S/128)) and decision bits;
//           np_total: the padded sample count of the WHOLE batch when the segment covers a ray range of it starting on a pass boundary
//           (planes / masks / raw / t_vals already point at the range): the decision bits' slot stride is the whole batch's;
//   gather_idx: the samples of an occupancy list (aon_mlp_core.h);
//   samples_enc / viewdirs_enc: caller-encoded inputs (padded 63 / 27-column layout) instead of the in-kernel encodings;
//   live_rows: the trunk of the per-ray-bias form (mlp_fwd_kernel, DEFER): records (0, 0, 0, raw sigma), marks and the live samples' rows
//           -- folded streams only, and the segment carries the view bias launch_view_deferred will finish the samples with.
// A combination no instance serves is hipErrorInvalidValue, as are an unknown form, mixed forms and a view bias on caller-made encodings.
hipError_t launch_mlp_fwd(const FwdSeg* segs, int nsegs, hipStream_t stream) {
  const FwdForm f = fwd_form(segs, nsegs);
  if (!f.ok) return hipErrorInvalidValue;
  MlpArgs args{};
  for (int i = 0; i < nsegs; ++i) {
    if (segs[i].pos) return hipErrorInvalidValue;   // the articulated network's caller-made input
    fill_seg(args.seg[i], segs[i]);
  }
  finish_segs(args, nsegs);
  if (f.defer) {
    if (!segs[0].view_bias || agreed_form(args) != kFormFolded) return hipErrorInvalidValue;
    return launch_mlp_tf<true, false, true, true, false, true>(args, stream);
  }
  if (f.gather) return launch_mlp_t<true, false, true>(args, stream);
  if (f.train) return f.own_inputs ? launch_mlp_t<false, true>(args, stream) : launch_mlp_t<true, true>(args, stream);
  return f.own_inputs ? launch_mlp_t<false, false>(args, stream) : launch_mlp_t<true, false>(args, stream);
}

// ---------------------------------------------------------------------------------------------
// density on a grid (aon_density_grid, mesh extraction)
// ---------------------------------------------------------------------------------------------
// (GridArgs, grid_point, grid_activation, grid_store: aon_mlp_core.h)

// encode -> trunk -> density head of mlp_fwd_kernel -- the same trunk_fwd, so the same operations in the same order and the same bits as
// its raw sigma -- on points generated from the grid; no view encoding, view branch or rgb head.  One wave = 32 grid points, as there.
__global__ void __launch_bounds__(256) density_grid_kernel(GridArgs args) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = lane & 31, h = lane >> 5;
  run_passes_one<VanillaTrunkNet, kSmallFloats>(args.packed, reinterpret_cast<const float*>(args.packed + kStreamBytes), args.npass,
                                                [&](int pass, Pipe& p, const float* sm) __attribute__((always_inline)) {
    const int64_t l0 = (int64_t)pass * 128 + wave * 32;
    const int64_t l = l0 + m;
    float x[3];
    grid_point(args, l < args.total ? l : args.total - 1, x);
    f32x16 E[2], X[8], Y[8];
    encode_pos(x, h, E);
    NoTaps taps;
    const float sigma = trunk_fwd<VanillaTrunkNet, VanillaTrunk>(p, E, X, Y, sm, h, taps);
    grid_store(args.out, l0, args.total, lane, grid_activation(sigma, args.act));
  });
}

hipError_t launch_density_grid(const char* packed, const int64_t* dims, const float* lo, const float* step, int64_t g_begin, int64_t g_end,
                               int act, float* out, hipStream_t stream) {
  if (stream_form(packed) == kFormUnknown) return hipErrorInvalidValue;   // never packed / declared (mlp_fwd refuses it too)
  static DeviceOnce lds_once;
  const GridArgs a = make_grid_args(packed, nullptr, dims, lo, step, g_begin, g_end, act, out);
  return launch_persistent(&density_grid_kernel, kLdsBytes, a.npass, lds_once, stream, a);
}

}  // namespace aon
