// The persistent pass loop of the fused MLP kernels (device) and the one launch path of those kernels (host).
//
// A launch carries one or two SEGMENTS: a run of 128-sample passes of one network over one range (MlpSeg, ArtSeg, BwdSeg, ArtBwdSeg).
// The forward segments are filled from the host-side record FwdSeg (aon_common.h) by fill_seg, and fwd_form reads off the record which
// kernel instance the launch names.
// A segment record shows the driver two things through overloads next to its definition:
//   seg_stream(sg)  the weight stream its passes run on,
//   seg_small(sg)   the small block (biases, head weights) resident in LDS behind the ring while they run.
// The launch record holds `seg[2]` and `npass_total` (finish_segs below).
#pragma once
#include "aon_launch.h"
#include "aon_mlp_core.h"

namespace aon {

// resident small vectors -> LDS (visible after the next workgroup barrier)
template <int SMALL_FLOATS>
__device__ __forceinline__ void load_small_block(float* sm, const float* small) {
  const f32x4* src = reinterpret_cast<const f32x4*>(small);
  f32x4* dst = reinterpret_cast<f32x4*>(sm);
  for (int i = threadIdx.x; i < SMALL_FLOATS / 4; i += 256) dst[i] = src[i];
}

// Everything of a persistent kernel around its per-pass body: workgroup w runs global passes w, w + gridDim.x, ... of the launch;
// `body(sg, pass, p, sm)` computes pass `pass` of segment `sg` with the weight pipe `p` and the small block `sm`.
// GATHER (inference kernels, one segment): the pass count is the occupancy list's, read from device memory (aon_mlp_core.h), and the body
// takes the list's length as a fifth argument.
// The driver keeps nothing per lane across passes, and a body must not rely on it to: the backward chains re-derive their lane
// coordinates inside the body every pass, because loop-invariant per-lane values hoisted out of this loop are what they spill.
template <class Net, int SMALL_FLOATS, bool GATHER = false, class Args, class Body>
__device__ __forceinline__ void run_passes(const Args& args, Body body) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* sm = reinterpret_cast<float*>(smem + kRingBytes);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // [GATHER] one segment; its pass count is the occupancy list's
  int64_t listed = 0;
  if constexpr (GATHER) listed = *args.seg[0].gather_count;
  const int npass0 = GATHER ? (int)((listed + 127) / 128) : args.seg[0].npass;
  int cur = (int)blockIdx.x >= npass0 ? 1 : 0;               // segment of this workgroup's first pass
  load_small_block<SMALL_FLOATS>(sm, seg_small(args.seg[cur]));
  Pipe p;
  pipe_init<Net>(p, seg_stream(args.seg[cur]), smem, wave, lane);  // also publishes the small block just written to LDS

  for (int gpass = blockIdx.x; gpass < (GATHER ? npass0 : args.npass_total); gpass += gridDim.x) {
    const int si = gpass >= npass0 ? 1 : 0;
    if (si != cur) {   // (workgroup-uniform, at most once per launch) the other network's biases / head weights replace the resident block
      __syncthreads();
      load_small_block<SMALL_FLOATS>(sm, seg_small(args.seg[si]));
      __syncthreads();
      cur = si;
    }
    const auto& sg = args.seg[si];
    const int pass = gpass - (si ? npass0 : 0);
    {   // weight stream of this pass, and of this workgroup's next one (its first chunk pair is fetched during this pass's last chunks)
      const int nxt = gpass + (int)gridDim.x;
      p.stream = seg_stream(sg);
      p.next_stream = seg_stream(args.seg[(nxt >= npass0 && nxt < (GATHER ? npass0 : args.npass_total)) ? 1 : si]);
    }
    if constexpr (GATHER) body(sg, pass, p, sm, listed);
    else body(sg, pass, p, sm);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the last prefetched chunk must land before the LDS is released
}

// the one-segment form (density-grid kernels): one stream, one small block, `body(pass, p, sm)`
template <class Net, int SMALL_FLOATS, class Body>
__device__ __forceinline__ void run_passes_one(const char* stream, const float* small, int npass, Body body) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* sm = reinterpret_cast<float*>(smem + kRingBytes);
  load_small_block<SMALL_FLOATS>(sm, small);
  Pipe p;
  pipe_init<Net>(p, stream, smem, threadIdx.x >> 6, threadIdx.x & 63);  // also publishes the small block
  for (int pass = blockIdx.x; pass < npass; pass += gridDim.x) body(pass, p, sm);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the last prefetched chunk must land before the LDS is released
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// seg[0 .. nsegs-1] are filled: the pass total, and the two forms the kernels never see -- a one-segment launch has an empty copy of its
// segment as seg[1]; an empty first segment leaves the second one alone.
template <class Args>
inline void finish_segs(Args& a, int nsegs) {
  a.npass_total = 0;
  for (int i = 0; i < nsegs; ++i) a.npass_total += a.seg[i].npass;
  if (nsegs == 1) { a.seg[1] = a.seg[0]; a.seg[1].npass = 0; }
  else if (a.seg[0].npass == 0) { a.seg[0] = a.seg[1]; a.seg[1].npass = 0; }
}

// One workgroup per CU at most, each looping over the passes; `once`: the kernel's dynamic-LDS limit, set once per device (one
// DeviceOnce per kernel instance, at the call site).  A launch without passes is a success.
template <class Kernel, class Args>
inline hipError_t launch_persistent(Kernel* kernel, int lds_bytes, int npasses, DeviceOnce& once, hipStream_t stream, const Args& args) {
  if (hipError_t e = set_max_lds(kernel, lds_bytes, once); e != hipSuccess) return e;
  const int cus = num_cus();
  if (cus <= 0) return hipErrorInvalidDevice;
  const int grid = npasses < cus ? npasses : cus;
  if (grid <= 0) return hipSuccess;
  kernel<<<dim3(grid), dim3(256), lds_bytes, stream>>>(args);
  return hipGetLastError();
}

// The form the streams of a forward launch were packed in, or kFormUnknown where the launch must be refused: a stream never packed or
// declared (a copy: refuse instead of guessing), segments of two forms, a per-call block of another form than its stream, the per-ray view
// bias on some segments only (every segment of the launch or none), or on a form other than the folded one.
template <class Args>
inline int agreed_form(const Args& a) {
  using Seg = std::remove_reference_t<decltype(a.seg[0])>;
  const int form = stream_form(a.seg[0].packed);
  const bool vb = a.seg[0].view_bias != nullptr;
  for (int i = 0; i < 2; ++i) {
    const Seg& s = a.seg[i];
    if (i > 0 && s.npass <= 0) break;
    if (stream_form(s.packed) != form || (s.view_bias != nullptr) != vb) return kFormUnknown;
    if constexpr (Seg::kPerCallBlock) {
      if (stream_form(s.small) != form) return kFormUnknown;
    }
  }
  return vb && form != kFormFolded ? kFormUnknown : form;
}

// A forward segment from the host-side record, all of it: the ray range or the caller-made inputs, the buffers, and whichever of the
// training planes, the occupancy list (with the pass count of max_listed) or the deferred trunk's marks and rows the record holds.
template <class Seg>
inline void fill_seg(Seg& a, const FwdSeg& t) {
  a.packed = t.packed;
  if constexpr (Seg::kPerCallBlock) { a.small = t.small; a.pos = t.pos; }
  else a.samples_enc = t.samples_enc;
  a.viewdirs_enc = t.viewdirs_enc;
  a.rays_o = t.rays_o; a.rays_d = t.rays_d; a.viewdirs = t.viewdirs; a.t_vals = t.t_vals; a.view_bias = t.view_bias;
  a.raw = t.raw; a.total = t.n_rays * t.S; a.S = t.S; a.npass = (int)(((t.max_listed > 0 ? t.max_listed : a.total) + 127) / 128);
  if (t.planes) {   // training: Np is the padded sample count of the WHOLE level where the segment is a ray range of it
    a.planes = t.planes; a.masks = static_cast<u32x4*>(t.masks); a.Np = t.np_total > 0 ? t.np_total : (int64_t)a.npass * 128;
  } else if (t.gather_idx) {
    a.gather_idx = t.gather_idx; a.gather_count = t.gather_count;
  } else if constexpr (!Seg::kPerCallBlock) {
    if (t.live_rows) { a.live_rows = t.live_rows; a.live_mark = t.live_mark; }
  }
}

// What the segments of a forward launch hold, which names the kernel instance (launch_mlp_fwd, launch_art_mlp_fwd).  `ok` is false where
// no instance serves the launch whatever the network: nsegs outside 1..2, two segments that hold different things, more than one of
// planes / list / deferred rows (the kernels' static_asserts), or an occupancy list on two segments (run_passes reads seg[0]'s count).
struct FwdForm { bool ok, train, gather, own_inputs, defer; };
inline FwdForm fwd_form(const FwdSeg* segs, int nsegs) {
  auto of = [](const FwdSeg& s) { return FwdForm{true, s.planes != nullptr, s.gather_idx != nullptr, s.samples_enc || s.pos, s.live_rows != nullptr}; };
  FwdForm f{};
  if (nsegs < 1 || nsegs > 2) return f;
  f = of(segs[0]);
  if (nsegs == 2) {
    const FwdForm g = of(segs[1]);
    if (g.train != f.train || g.gather != f.gather || g.own_inputs != f.own_inputs || g.defer != f.defer || f.gather) f.ok = false;
  }
  if ((int)f.train + (int)f.gather + (int)f.defer > 1 || ((f.gather || f.defer) && f.own_inputs)) f.ok = false;
  return f;
}

}  // namespace aon
