// Latent-only second stage of the articulated backward: the gradients of the three latent codes of a FROZEN network,
// without a single weight gradient.
//
// Every latent is broadcast to all samples (model_autodecoder.py:186-194), so  d latent = sum over (W, db) pairs of W[:, cols]^T db  where db is
// the bias gradient of a layer the latent enters (the latent table of aon_params.h; LatentJob, aon_art_common.h) -- five pairs over FOUR bias gradients:
//   deformations_linear.0 (shape, articulation), pts_linears.0 and .5 (shape), views_linear.0 (appearance).
// The full backward gets those four as by-products of its weight-gradient launches.  Here they are taken from the chain's gradient planes
// directly, and to the BIT as the full backward forms them, which fixes the order of every sum:
//   * pts_linears.0 / .5, views_linear.0: wgrad_grouped_kernel (aon_wgrad.h) keeps fp32 row sums of dZ beside its MFMAs -- per workgroup
//     SEGMENT of the level's work line, per wave split, per half-wave: lane (unit row, kh) adds the samples 2 p + kh of its pairs p, step after
//     step; the two half-waves are added; wgrad_reduce_block sums those partials in fp64 (16 interleaved groups, added in group order) and rounds
//     once.  A CHAIN below is one such lane: the same samples in the same order, the segments from the same plan (wg_make_plan over the level's
//     whole layer list -- the work line depends on every job's cost, not only on the three that are summed here);
//   * deformations_linear.0: head_wgrad_kernel's channel 4 (fp64 from the first add: 256 interleaved thread sums per segment of
//     head_segments(), a 64-lane butterfly, four wave sums), then the segments in order.
// No atomics, no spin-waits: two ordinary launches on the caller's stream.  Nothing here writes a parameter gradient.
#include "aon_art_common.h"
#include "aon_launch.h"
#include "aon_wgrad.h"

namespace aon {

namespace {

// ---- launch 1: the partial sums of both levels ----
struct LatBiasJob {       // one bias-carrying weight-gradient job of one level, as the grouped kernel would run it
  const float* a;         // first unit row of dZ in the level's gradient planes
  float* part;            // partial[nspan * nsplit][M]
  int64_t step_floats;    // rows * 32
  int64_t p_begin, w_total;
  int nsteps, cost, nwgs, first_wg;
  int nsplit, M;
  int blk_begin, blocks_per_wg;   // 64 chains per block: (M / 4) unit rows x 2 half-waves x nsplit chains per workgroup segment
};
struct LatHeadJob {       // row sums of dZ of deformations_linear.0 (128 rows): 16 blocks of 8 rows per segment
  const float* a;
  double* part;           // partial[nseg][128]
  int64_t step_floats, Np, seg_len;
  int blk_begin;
};
struct LatentDbArgs {
  LatBiasJob bias[6];
  LatHeadJob head[2];
  int nbias, nhead, head_blk_begin;
};

// one chain: steps [c_begin, c_end), PW samples (stride two) of each.  The adds are one dependent fp32 sequence per row; the loads of 32 samples
// (32 / PW steps) are issued together in front of their adds -- the kernel is as fast as it keeps bytes in flight.
template <int PW>
__device__ __forceinline__ f32x4 lat_chain(const float* __restrict__ base, const int64_t step_floats, const int c_begin, const int c_end) {
  constexpr int U = 32 / PW;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  int c = c_begin;
  for (; c + U <= c_end; c += U) {
    f32x4 v[U * PW];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int q = 0; q < PW; ++q) v[u * PW + q] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(base + (int64_t)(c + u) * step_floats + q * 8));
#pragma unroll
    for (int i = 0; i < U * PW; ++i) s += v[i];
  }
  for (; c < c_end; ++c) {
    f32x4 v[PW];
#pragma unroll
    for (int q = 0; q < PW; ++q) v[q] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(base + (int64_t)c * step_floats + q * 8));
#pragma unroll
    for (int q = 0; q < PW; ++q) s += v[q];
  }
  return s;
}

__global__ void __launch_bounds__(64) latent_db_kernel(LatentDbArgs a) {
  const int bx = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (bx >= a.head_blk_begin) {
    int j = 0;
    if (a.nhead > 1 && bx >= a.head[1].blk_begin) j = 1;
    const LatHeadJob& H = a.head[j];
    const int b = bx - H.blk_begin;
    const int rb = b & 15, seg = b >> 4;
    const int64_t n0 = (int64_t)seg * H.seg_len;
    const int64_t n1 = n0 + H.seg_len < H.Np ? n0 + H.seg_len : H.Np;
    const float* u0 = H.a + (int64_t)rb * 256;   // two unit rows = eight plane rows
    // this lane stands for the threads lane, lane + 64, lane + 128, lane + 192 of head_wgrad_kernel's 256: four sums per row, each over n = first + 256 k
    double s[4][8];
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
      for (int r = 0; r < 8; ++r) s[w][r] = 0.0;
    for (int64_t nb = n0; nb < n1; nb += 256) {
      f32x4 x0[4], x1[4];
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const int64_t n = nb + w * 64 + lane;
        x0[w] = f32x4{0.f, 0.f, 0.f, 0.f}; x1[w] = x0[w];
        if (n < n1) {
          const float* p = u0 + (n >> 5) * H.step_floats + (int)(n & 31) * 4;
          x0[w] = *reinterpret_cast<const f32x4*>(p);
          x1[w] = *reinterpret_cast<const f32x4*>(p + 128);
        }
      }
#pragma unroll
      for (int w = 0; w < 4; ++w)
        if (nb + w * 64 + lane < n1) {
#pragma unroll
          for (int r = 0; r < 4; ++r) { s[w][r] += (double)x0[w][r]; s[w][4 + r] += (double)x1[w][r]; }
        }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      double v[4];
#pragma unroll
      for (int w = 0; w < 4; ++w) v[w] = wsum64d(s[w][r]);
      if (lane == 0) H.part[(int64_t)seg * 128 + rb * 8 + r] = (v[0] + v[1]) + (v[2] + v[3]);
    }
    return;
  }
  int j = 0;
#pragma unroll 1
  for (int t = 1; t < a.nbias; ++t)
    if (bx >= a.bias[t].blk_begin) j = t;
  const LatBiasJob& J = a.bias[j];
  const int b = bx - J.blk_begin;
  const int wl = b / J.blocks_per_wg, wg = J.first_wg + wl;
  const int id = (b % J.blocks_per_wg) * 64 + lane;
  const int kh = id & 1, split = (id >> 1) % J.nsplit, g = id / (2 * J.nsplit);
  const int64_t lo = J.w_total * wg / J.nwgs, hi = J.w_total * (wg + 1) / J.nwgs;
  const int c_begin = wg_first_step(lo, J.p_begin, J.cost, J.nsteps), c_end = wg_first_step(hi, J.p_begin, J.cost, J.nsteps);
  const int pw = 16 / J.nsplit;
  const float* base = J.a + (int64_t)g * 128 + (2 * split * pw + kh) * 4;
  const f32x4 s = J.nsplit == 1 ? lat_chain<16>(base, J.step_floats, c_begin, c_end) : lat_chain<8>(base, J.step_floats, c_begin, c_end);
  f32x4 v;
#pragma unroll
  for (int ca = 0; ca < 4; ++ca) v[ca] = s[ca] + __shfl_xor(s[ca], 1);   // the two half-waves of the grouped kernel: chains kh = 0, 1
  if (kh == 0) *reinterpret_cast<f32x4*>(J.part + (int64_t)(wl * J.nsplit + split) * J.M + 4 * g) = v;
}

// ---- launch 2: partials -> the four bias gradients (in LDS) -> W^T db, level 0 then level 1 added onto it ----
struct LatDbSrc {
  const void* part;   // fp32 partial[nparts][M] of a weight-gradient job, or fp64 partial[nparts][M] of the head job
  int nparts, M, is_head;
};
struct LatFinLevel {
  LatDbSrc src[kNumLatentBiases];   // deformations_linear.0, pts_linears.0, pts_linears.5, views_linear.0
  LatentJob lat[kNumLatents];       // shape, appearance, articulation: the bias gradients by index (src), out in level 0's
};
struct LatentFinishArgs {
  LatFinLevel lvl[2];
  int nlevels;
};

__global__ void __launch_bounds__(1024) latent_finish_kernel(LatentFinishArgs a) {
  __shared__ float db[2][kLatDbFloats];
  __shared__ double redd[16][64];
  __shared__ float red[2][8][128];
  const int tid = (int)threadIdx.x;
  const int lat = (int)blockIdx.x;
  // the bias gradients this latent needs, as wgrad_reduce_block forms them (same sums, same order)
  for (int l = 0; l < a.nlevels; ++l) {
    const LatentJob& j = a.lvl[l].lat[lat];
    for (int pi = 0; pi < j.npairs; ++pi) {
      const LatDbSrc& S = a.lvl[l].src[j.src[pi]];
      float* out = db[l] + lat_db_off(j.src[pi]);
      if (S.is_head) {
        if (tid < S.M) {
          const double* P = static_cast<const double*>(S.part) + tid;
          double s = 0.0;
          for (int p = 0; p < S.nparts; ++p) s += P[(int64_t)p * S.M];
          out[tid] = (float)s;
        }
        __syncthreads();
        continue;
      }
      const int r = tid & 63, g = tid >> 6;   // 64 rows a pass; thread (r, g) sums partials g, g + 16, ..., the 16 group sums are added in group order
      for (int row0 = 0; row0 < S.M; row0 += 64) {
        const float* B = static_cast<const float*>(S.part) + row0 + r;
        double s = 0.0;
        for (int pp = g; pp < S.nparts; pp += 16) s += (double)B[(int64_t)pp * S.M];
        redd[g][r] = s;
        __syncthreads();
        if (g == 0) {
          double t = 0.0;
#pragma unroll
          for (int q = 0; q < 16; ++q) t += redd[q][r];
          out[row0 + r] = (float)t;
        }
        __syncthreads();
      }
    }
  }
  // blocks 0..2 of art_finish2_kernel (one level: of art_finish_kernel), the bias gradients read from LDS
  const LatentJob* const j[2] = {&a.lvl[0].lat[lat], &a.lvl[a.nlevels - 1].lat[lat]};
  auto db_of = [&](int l, int pi) { return db[l] + lat_db_off(j[l]->src[pi]); };
  if (a.nlevels == 2) {
    latent_wt_db<2>(j, db_of, red, [&](int k, const float (&t)[2]) { j[0]->out[k] = t[0] + t[1]; });
  } else {
    const LatentJob* const j0[1] = {j[0]};
    latent_wt_db<1>(j0, db_of, red, [&](int k, const float (&t)[1]) { j[0]->out[k] = t[0]; });
  }
}

}  // namespace

// workspace of ONE level: the fp32 partials of the three jobs (a job spans at most 304 workgroups: 304 x 256 + 608 x 256 + 608 x 128 floats = 1.2 MB)
// and the head job's 256 x 128 doubles at most
int64_t art_latent_ws_bytes() { return (int64_t)2 << 20; }

hipError_t launch_art_latent_grads(const ArtLatentLevel* lv, int nlevels, int Lp, int Lv, float* g_shape, float* g_app, float* g_art, hipStream_t stream) {
  if (nlevels < 1 || nlevels > 2 || !g_shape || !g_app || !g_art) return hipErrorInvalidValue;
  const int cus = num_cus();
  if (cus <= 0) return hipErrorInvalidDevice;
  const int P = enc_width(Lp), V = enc_width(Lv);
  LatentDbArgs D{};
  LatentFinishArgs F{};
  F.nlevels = nlevels;
  float* const g_latents[kNumLatents] = {g_shape, g_app, g_art};   // (kLatShape, kLatApp, kLatArt)
  int blk = 0;
  for (int l = 0; l < nlevels; ++l) {
    const ArtLatentLevel& A = lv[l];
    if (!A.dplanes || !A.params || !A.ws || !A.packed_bwd || A.Np <= 0 || (A.Np & 31)) return hipErrorInvalidValue;
    const int form = stream_form(A.packed_bwd);
    if (form == kFormUnknown) return hipErrorInvalidValue;
    // the level's layer list exactly as launch_art_wgrad builds it; the output pointers only NAME the jobs here (never dereferenced)
    float* names[kNumArtParams];
    for (int i = 0; i < kNumArtParams; ++i) names[i] = A.ws + i;
    WgLayerDesc L[kWgMaxJobs];
    const int n = art_wgrad_layers(names, L, Lp, Lv, A.ws, form == kFormFolded ? A.ws : nullptr);
    WgPlan plan;
    if (!wg_make_plan(L, n, nullptr, A.dplanes, kAPlRows, A.Np, cus < 304 ? cus : 304, A.ws, 0, plan)) return hipErrorInvalidValue;
    int64_t off = 0;   // floats into this level's workspace
    LatFinLevel& FL = F.lvl[l];
    for (int i = 0; i < kNumLatentEntries; ++i) {
      const LatentEntry e = art_latent_entry(i, P, V);
      if (!A.params[e.w]) return hipErrorInvalidValue;
      if (e.src == 0) continue;   // (deformations_linear.0's bias gradient is the head job's, below)
      int jf = -1;
      for (int j = 0; j < n; ++j)
        if (L[j].bias_out == names[e.b]) jf = j;
      if (jf < 0 || D.nbias >= 6) return hipErrorInvalidValue;
      const WgJob& J = plan.args.job[jf];
      const int nsplit = wg_nsplit(J.kind), M = wg_M(J.kind), span = J.last_wg - J.first_wg + 1;
      if (nsplit > 2 || L[jf].a_row % 4) return hipErrorInvalidValue;   // (the three jobs are of the 256x64, 256x256 and 128x256 kinds)
      LatBiasJob& B = D.bias[D.nbias++];
      B.a = A.dplanes + (int64_t)J.a_unit * 128;
      B.part = A.ws + off;
      B.step_floats = (int64_t)kAPlRows * 32;
      B.p_begin = J.p_begin; B.w_total = plan.args.w_total;
      B.nsteps = plan.args.nsteps; B.cost = J.cost; B.nwgs = plan.args.nwgs; B.first_wg = J.first_wg;
      B.nsplit = nsplit; B.M = M;
      B.blocks_per_wg = (M / 4) * 2 * nsplit / 64;
      B.blk_begin = blk; blk += span * B.blocks_per_wg;
      FL.src[e.src] = LatDbSrc{B.part, span * nsplit, M, 0};
      off += (int64_t)span * nsplit * M;
    }
    off += off & 1;
    int nseg; int64_t seg_len;
    head_segments(A.Np, nseg, seg_len);
    LatHeadJob& H = D.head[D.nhead++];
    H.a = A.dplanes + (int64_t)(aplane_d(0) / 4) * 128;
    H.part = reinterpret_cast<double*>(A.ws + off);
    H.step_floats = (int64_t)kAPlRows * 32; H.Np = A.Np; H.seg_len = seg_len;
    H.blk_begin = nseg;   // (segments for now: the head blocks follow every level's chain blocks)
    FL.src[0] = LatDbSrc{H.part, nseg, 128, 1};
    off += (int64_t)nseg * 128 * 2;
    if (off * 4 > art_latent_ws_bytes()) return hipErrorInvalidValue;
    // the (W, db) pairs of launch_art_wgrad's LatentJobs
    art_latent_jobs(A.params, nullptr, P, V, FL.lat);
    for (int k = 0; k < kNumLatents; ++k) FL.lat[k].out = g_latents[k];
  }
  D.head_blk_begin = blk;
  for (int h = 0; h < D.nhead; ++h) {
    const int nseg = D.head[h].blk_begin;
    D.head[h].blk_begin = blk;
    blk += 16 * nseg;
  }
  latent_db_kernel<<<dim3(blk), dim3(64), 0, stream>>>(D);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  latent_finish_kernel<<<dim3(kNumLatents), dim3(1024), 0, stream>>>(F);
  return hipGetLastError();
}

}  // namespace aon
