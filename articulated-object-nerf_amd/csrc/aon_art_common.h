// Constants shared by the articulated forward (aon_mlp_art.hip) and backward (aon_train_art.hip).
#pragma once
#include "aon_mlp_core.h"

namespace aon {

// ---- per-call small block (floats), rebuilt by aon_art_prepare because it depends on the latents ----
constexpr int kA_BD0 = 0;       // 128   effective bias of deformations_linear.0 (shape + articulation folded in)
constexpr int kA_WD0 = 128;     // 3x128 deformations_linear.0 weight, [xyz][feature]
constexpr int kA_BD = 512;      // 3x128 biases of deformations_linear.1..3
constexpr int kA_WDL = 896;     // 3x128 deformation_layer weight rows
constexpr int kA_BDL = 1280;    // 3 (+1 pad)
constexpr int kA_BT = 1284;     // 8x256 trunk biases (layers 0 and 5 effective: shape latent folded in)
constexpr int kA_BBOT = 3332;   // 256
constexpr int kA_BV = 3588;     // 4x128 view-branch biases (layer 0 effective: appearance latent folded in)
constexpr int kA_WSIG = 4100;   // 256
constexpr int kA_WRGB = 4356;   // 3x128
constexpr int kA_BSIG = 4740;   // 1
constexpr int kA_BRGB = 4741;   // 3
constexpr int kA_ESC = 4744;    // 10 (+2 pad): encoding scales 2^(min_deg_point + l), 0 for levels the network lacks (round 4: other degrees)
constexpr int kASmallFloats = 4756;
constexpr int kALdsBytes = kRingBytes + kASmallFloats * 4;

// ---- chunk stream of one articulated MLP (execution order) ----
constexpr int kAChD1 = 0;     // deformations_linear.1..3 : 4 chunks each, 4 output tiles (16 KiB)
constexpr int kAChT0 = 12;    // pts_linears.0 : 2 pos-enc chunks (32 KiB)
constexpr int kAChT1 = 14;    // pts_linears.1..4 : 8 chunks each
constexpr int kAChT5 = 46;    // pts_linears.5 : 8 hidden + 2 pos-enc
constexpr int kAChT6 = 56;
constexpr int kAChT7 = 64;
constexpr int kAChBott = 72;
constexpr int kAChV0 = 80;    // views_linear.0 : 8 hidden + 1 view-enc, 4 output tiles (16 KiB)
constexpr int kAChV1 = 89;    // views_linear.1..3 : 4 chunks each
constexpr int kANumChunks = 101;

// ---- transposed chunk stream (execution order of the backward chain) ----
constexpr int kABwV3 = 0;      // views_linear.3^T, .2^T, .1^T : 4 chunks each, 4 output tiles (16 KiB)
constexpr int kABwV0 = 12;     // views_linear.0[:, :256]^T : 4 chunks, 8 output tiles (32 KiB)
constexpr int kABwBott = 16;   // bottleneck^T : 8
constexpr int kABwL7 = 24;     // pts_linears.7^T, .6^T : 8 each
constexpr int kABwL5E = 40;    // pts_linears.5[:, 256:319]^T : 8 chunks, 2 output tiles (8 KiB)  -> d pos-enc
constexpr int kABwL5 = 48;     // pts_linears.5[:, :256]^T, then .4 .3 .2 .1 : 8 each
constexpr int kABwL0E = 88;    // pts_linears.0[:, :63]^T : 8 chunks, 2 output tiles              -> d pos-enc
constexpr int kABwD3 = 96;     // deformations_linear.3^T, .2^T, .1^T : 4 chunks each, 4 output tiles
constexpr int kABwNumChunks = 108;

// ---- FOLDED forms (round 5; aon_common.h kChFView for the algebra): bottleneck_layer (no activation, model_autodecoder.py:223) folded into
// views_linear.0's 256 bottleneck columns, W' = W_v0[:, :256] W_b -- 65,536 of the 692,480 MACs per sample the un-folded kernels execute.
// Forward stream: the eight bottleneck chunks are gone, every later chunk moves up by 8; views_linear.0's hidden chunks hold W' and
// read the post-ReLU layer-7 output.  The per-call block's effective bias of views_linear.0 additionally carries W_v0[:, :256] b_b.
// views_linear.0's view-encoding chunk comes FIRST (as in the vanilla network, aon_common.h): its term and the effective bias are a constant
// of the ray, handed to the whole-path kernels as a per-ray bias (ArtFoldVbNet: the same buffer without that chunk).
constexpr int kAChFV0 = 72;    // W' : 1 view-enc + 8 hidden
constexpr int kAChFV1 = 81;
constexpr int kANumChunksF = 93;
// Transposed stream: views_linear.0's four chunks hold W'^T (d H7 directly), the eight bottleneck chunks are gone.
constexpr int kABwFL7 = 16;
constexpr int kABwFL5E = 32;
constexpr int kABwFL5 = 40;
constexpr int kABwFL0E = 80;
constexpr int kABwFD3 = 88;
constexpr int kABwFNumChunks = 100;

// ---- latent gradients (the table: art_latent_entry, aon_params.h) ----
// d latent[k] = sum over the latent's (W, db) pairs, sum_f W[f][col_off + k] * db[f], db the bias gradient of the layer.  One record for the
// full backward's finishing kernels (aon_train_art.hip: db points at the bias gradients the weight-gradient launches wrote) and the
// latent-only backward (aon_train_latent.hip: db is null, the kernel forms bias gradient `src` in LDS at lat_db_off(src)).
struct LatentJob {
  const float* W[kMaxLatentPairs]; const float* db[kMaxLatentPairs];
  int ld[kMaxLatentPairs], col_off[kMaxLatentPairs], M[kMaxLatentPairs], src[kMaxLatentPairs];
  int npairs; int L;
  float* out;
  const float* add;   // null, or the other level's result: out = add + this level's (both MLPs see the same latents; may alias out)
};
// the three jobs of one level (zero-initialised by the caller), pair by pair in table order; grads: the level's parameter gradients, or null
inline void art_latent_jobs(const float* const* params, float* const* grads, int P, int V, LatentJob lat[kNumLatents]) {
  for (int i = 0; i < kNumLatentEntries; ++i) {
    const LatentEntry e = art_latent_entry(i, P, V);
    LatentJob& j = lat[e.latent];
    const int pi = j.npairs++;
    j.W[pi] = params[e.w]; j.db[pi] = grads ? grads[e.b] : nullptr;
    j.ld[pi] = e.ld; j.col_off[pi] = e.col; j.M[pi] = e.M; j.src[pi] = e.src;
    j.L = e.L;
  }
}

// W^T db of NL levels' jobs for one latent in lockstep (the levels' jobs have the same shape: L, pairs, M) -- NL independent chains of
// multiply-adds, each in its own order, their loads in flight together: the finishing kernels are load latency from end to end.  A
// 1,024-thread block: 8 row groups x 128 columns, group g takes rows f = g, g + 8, ... (independent loads, coalesced over k), the eight
// group sums are added in group order through LDS (deterministic).  db_of(l, pi): the bias gradient of pair pi at level l.
// store(k, t): called in the threads of row group 0 with k < L, t[l] level l's d latent[k].
template <int NL, class DbOf, class Store>
__device__ __forceinline__ void latent_wt_db(const LatentJob* const (&j)[NL], DbOf db_of, float (*red)[8][128], Store store) {
  const int k = threadIdx.x & 127, g = threadIdx.x >> 7;
  const int L = j[0]->L;
  float s[NL];
#pragma unroll
  for (int l = 0; l < NL; ++l) s[l] = 0.f;
  if (k < L) {
    for (int pi = 0; pi < j[0]->npairs; ++pi) {
      const float* W[NL]; const float* db[NL]; int ld[NL];
#pragma unroll
      for (int l = 0; l < NL; ++l) { W[l] = j[l]->W[pi] + j[l]->col_off[pi] + k; db[l] = db_of(l, pi); ld[l] = j[l]->ld[pi]; }
#pragma unroll 4
      for (int f = g; f < j[0]->M[pi]; f += 8) {
#pragma unroll
        for (int l = 0; l < NL; ++l) s[l] = __builtin_fmaf(W[l][(int64_t)f * ld[l]], db[l][f], s[l]);
      }
    }
  }
#pragma unroll
  for (int l = 0; l < NL; ++l) red[l][g][k] = s[l];
  __syncthreads();
  if (g == 0 && k < L) {
    float t[NL];
#pragma unroll
    for (int l = 0; l < NL; ++l) t[l] = red[l][0][k];
#pragma unroll
    for (int q = 1; q < 8; ++q) {
#pragma unroll
      for (int l = 0; l < NL; ++l) t[l] += red[l][q][k];
    }
    store(k, t);
  }
}

}  // namespace aon
