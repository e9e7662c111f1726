// extern "C" surface, the training step in two calls: workspace carvers, the library's side streams, train_fwd_impl / train_bwd_impl for both
// networks and the schedule switches.
#include "aon_capi_util.h"
#include "../../include/aon_hip_inputs.h"

using namespace aon::capi;

extern "C" {   // (opened in front of the file's internals, as ever: its two small kernels keep their plain names in kernel traces)

// ---- training step in two calls (aon_render_fwd_train + aon_render_bwd) ----
// The whole forward of NeRF.forward / NeRF_AE_Art.forward under grad mode, then the whole backward of the reference's
// training loss, each as ONE C call on the exact-fp32 engine: the per-level staging that autograd.py used to drive from
// Python (sample -> fused MLP + planes -> composite -> inverse CDF | composite backward -> chain -> weight gradients)
// happens here.  Everything the backward needs stays in the caller's workspace between the two calls.
namespace {

struct TrainLevel {
  float* t;        // n*S
  float* raw;      // Np*4 (first n*S records valid)
  float* planes;   // rows*Np
  char* masks;     // mask_layers*Np*32
  float* coords; float* enc; float* venc;   // other encoding degrees only: n*S*3, n*S*63, n*27 (forward-only temporaries)
  float* vbias;    // n*128, the level's per-ray view bias (forward-only temporary; not for the vanilla network at other degrees)
  int S; int64_t Np;
};
// What the forward leaves for the backward (caller-owned, pinned by the autograd graph): per level t, raw, planes, ReLU bits.
struct TrainWs {
  TrainLevel lvl[2];
  float* w_c;      // n*Sc coarse weights
  int64_t bytes;
};
// Backward-only temporaries (round 3: a separate `scratch` of aon_render_bwd, allocated when the backward runs -- round 2 carved
// them into the forward's workspace, so every live graph pinned 26 GB instead of 15 GB at 4096 articulated rays), one set per
// level: the two levels' backward passes are independent and run on two streams.
struct TrainScratch {
  float* d_raw[2];    // Np*4
  float* dplanes[2];  // rows*Np
  float* dxp[2];      // Np*4 (articulated)
  float* wgrad_ws[2];
  float* lat_tmp;     // 288 floats: second level's latent gradients before they are added (articulated)
  float* grad_tmp[2]; // other encoding degrees: the three encoding-fed weight gradients in the kernels' 63 / 27-column layout
  int64_t bytes;
};
constexpr int64_t kGradTmpFloats = 256 * aon::vp_trunk0_ld(aon::kPosEnc) + 256 * aon::vp_trunk5_ld(aon::kPosEnc) + 128 * aon::vp_view0_ld(aon::kViewEnc);

int64_t level_np(int64_t n, int l, const Geo& g) { return align_up(n * g.S(l), 128); }

// both carves cover only the levels in use: num_levels = 1 (BASELINE config 1) takes a quarter of the two-level size
TrainWs carve_train(char* base, int64_t n, bool art, int num_levels, const Geo& g) {
  TrainWs w{};
  const int64_t rows = art ? aon::kAPlRows : aon::kPlRows;
  const int64_t mlayers = art ? aon::kAMaskLayers : aon::kMaskLayers;
  int64_t off = 0;
  auto take = [&](int64_t bytes) { char* p = base + off; off += align_up(bytes, 256); return p; };
  for (int l = 0; l < num_levels; ++l) {
    const int S = g.S(l);
    const int64_t Np = level_np(n, l, g);
    w.lvl[l].S = S; w.lvl[l].Np = Np;
    w.lvl[l].t = reinterpret_cast<float*>(take(n * S * 4));
    w.lvl[l].raw = reinterpret_cast<float*>(take(Np * 16));
    w.lvl[l].planes = reinterpret_cast<float*>(take(rows * Np * 4));
    w.lvl[l].masks = take(mlayers * Np * 32);
    if (g.other_degrees && !art) {
      w.lvl[l].coords = reinterpret_cast<float*>(take(n * S * 12));
      w.lvl[l].enc = reinterpret_cast<float*>(take(n * S * (int64_t)aon::kPosEnc * 4));
      w.lvl[l].venc = reinterpret_cast<float*>(take(n * (int64_t)aon::kViewEnc * 4));
    }
    if (!g.other_degrees || art) w.lvl[l].vbias = reinterpret_cast<float*>(take(n * (int64_t)aon::kCondWidth * 4));
  }
  w.w_c = reinterpret_cast<float*>(take(n * g.Sc * 4));
  w.bytes = off;
  return w;
}

TrainScratch carve_scratch(char* base, int64_t n, bool art, int num_levels, const Geo& g) {
  TrainScratch sc{};
  const int64_t rows = art ? aon::kAPlRows : aon::kPlRows;
  int64_t off = 0;
  auto take = [&](int64_t bytes) { char* p = base + off; off += align_up(bytes, 256); return p; };
  for (int l = 0; l < num_levels; ++l) {
    const int64_t Np = level_np(n, l, g);
    sc.d_raw[l] = reinterpret_cast<float*>(take(Np * 16));
    sc.dplanes[l] = reinterpret_cast<float*>(take(rows * Np * 4));
    sc.dxp[l] = reinterpret_cast<float*>(take(Np * 16));
    sc.wgrad_ws[l] = reinterpret_cast<float*>(take(aon::wgrad_workspace_bytes()));
    if (g.other_degrees && !art) sc.grad_tmp[l] = reinterpret_cast<float*>(take(kGradTmpFloats * 4));
  }
  sc.lat_tmp = reinterpret_cast<float*>(take(288 * 4));
  sc.bytes = off;
  return sc;
}

// dst (rows, hidden + 3 + 6 L) <- src (rows, hidden + 3 + 6 Lfull): the columns of an encoding with L levels picked out of the
// kernels' Lfull-level slot layout [x ; first block of 3 Lfull ; shifted block of 3 Lfull]
__global__ void remap_enc_cols_kernel(const float* __restrict__ src, float* __restrict__ dst, int rows, int hidden, int L, int Lfull) {
  const int cols = hidden + 3 + 6 * L, lds = hidden + 3 + 6 * Lfull;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)rows * cols) return;
  const int r = (int)(i / cols), c = (int)(i % cols);
  int sc = c;
  if (c >= hidden + 3 + 3 * L) sc = c + 3 * (Lfull - L);
  dst[i] = src[(int64_t)r * lds + sc];
}

__global__ void add_into_kernel(float* __restrict__ dst, const float* __restrict__ src, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] += src[i];
}

// Two library-owned streams per device for the backward of the two levels (independent until the latent gradients are
// added): kernels of one level fill the CUs the other level's tail rounds leave idle.  Ordered against the caller's stream by
// events on both sides, so from the caller's view the whole backward is enqueued on its stream.
struct LevelStreams {
  hipStream_t s[2] = {nullptr, nullptr};
  hipEvent_t fork = nullptr, join[2] = {nullptr, nullptr};
  aon::WgAux aux[2] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};   // per level: side stream of the head reductions
  std::mutex enqueue;   // held from the fork record to the join waits: the one event set is re-recorded by every call
};
LevelStreams* level_streams() {
  static LevelStreams per_dev[aon::kMaxDevices];
  static std::mutex mu;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= aon::kMaxDevices) return nullptr;
  std::lock_guard<std::mutex> lk(mu);
  LevelStreams& ls = per_dev[dev];
  if (!ls.fork) {
    auto make = [](hipStream_t* st) { return hipStreamCreateWithFlags(st, hipStreamNonBlocking); };
    for (int i = 0; i < 2; ++i) {
      if (make(&ls.s[i]) != hipSuccess) return nullptr;
      if (hipEventCreateWithFlags(&ls.join[i], hipEventDisableTiming) != hipSuccess) return nullptr;
      if (make(&ls.aux[i].stream) != hipSuccess) return nullptr;
      if (hipEventCreateWithFlags(&ls.aux[i].fork, hipEventDisableTiming) != hipSuccess) return nullptr;
      if (hipEventCreateWithFlags(&ls.aux[i].join, hipEventDisableTiming) != hipSuccess) return nullptr;
    }
    if (hipEventCreateWithFlags(&ls.fork, hipEventDisableTiming) != hipSuccess) return nullptr;
  }
  return &ls;
}

// One backward's use of the two streams.  The constructor takes the device's enqueue lock and forks (fork event on the
// caller's stream, both side streams wait for it); join() -- also run by the destructor, so on EVERY return path, error
// returns included -- records a join event behind whatever was enqueued on each side stream and makes the caller's stream
// wait for both.  Two host threads driving the same device from different caller streams therefore cannot interleave their
// event records, and no side-stream work is ever left un-joined while the caller frees the workspace on its stream.
class LevelFork {
 public:
  // aux_only: no level streams -- the caller's stream carries both levels -- but the side streams of the head reductions (aux()) are
  // handed out (each use forks from / joins to the stream it is given inside run_wgrad_plan); the device's enqueue lock is held alike
  LevelFork(bool overlap, hipStream_t caller, const char* who, bool aux_only = false) : caller_(caller), who_(who), aux_only_(aux_only) {
    if (!overlap) return;
    ls_ = level_streams();
    if (!ls_) return;   // no streams: run serially on the caller's stream
    lk_ = std::unique_lock<std::mutex>(ls_->enqueue);
    if (!aux_only_) {
      rc_ = check(hipEventRecord(ls_->fork, caller_), who_);
      for (int l = 0; l < 2 && !rc_; ++l) rc_ = check(hipStreamWaitEvent(ls_->s[l], ls_->fork, 0), who_);
    }
    forked_ = true;     // even on a partial failure: join() is harmless and keeps the caller ordered behind the side streams
  }
  ~LevelFork() { (void)join(); }
  int rc() const { return rc_; }
  hipStream_t stream(int level) const { return forked_ && !aux_only_ ? ls_->s[level] : caller_; }
  // side stream of a level's head reductions (only while this object holds the device's enqueue lock: the events are shared)
  const aon::WgAux* aux(int level) const { return forked_ ? &ls_->aux[level] : nullptr; }
  int join() {
    if (!forked_) return AON_OK;
    forked_ = false;
    int rc = AON_OK;
    for (int l = 0; l < 2 && !aux_only_; ++l) {
      hipError_t e = hipEventRecord(ls_->join[l], ls_->s[l]);
      if (e == hipSuccess) e = hipStreamWaitEvent(caller_, ls_->join[l], 0);
      if (e != hipSuccess && !rc) rc = check(e, who_);
    }
    lk_.unlock();
    return rc;
  }
 private:
  LevelStreams* ls_ = nullptr;
  hipStream_t caller_;
  const char* who_;
  std::unique_lock<std::mutex> lk_;
  int rc_ = AON_OK;
  bool forked_ = false;
  bool aux_only_ = false;
};
std::atomic<int> g_bwd_overlap{1};
std::atomic<int> g_fwd_overlap{2};
std::atomic<int> g_fwd_merge{1};
std::atomic<int> g_bwd_merge{1};   // the backward chains of the two levels as ONE persistent launch of two segments (round 4)
// Round 5: the head / bias reductions that need nothing from the chain (density head on H7, rgb head, sums of d_raw: 60 % of the head
// kernel's bytes) run on a library side stream BESIDE the merged chain launch, whose last round of workgroups is a quarter full
// (8,256 passes on 256 CUs): they fill compute units that would idle for one pass.  Phases kWgEarly / kWgRest of the levels' weight-gradient calls.
std::atomic<int> g_bwd_early_heads{1};

// The merged training forward (round 4) runs the two levels of two ray ranges A = [0, kA), B = [kA, n) as THREE persistent launches
//   coarse(A)  |  fine(A) + coarse(B)  |  fine(B)
// (the levels of a range depend on each other through its own inverse CDF only).  kA, a multiple of 128 rays, is chosen so that the
// three launches together take the fewest rounds of `cus` workgroups: 4096 rays x (65 + 193) samples on 256 CUs are 32.25 rounds of
// work; one launch per level costs 9 + 25 = 34 rounds, the split at 1,920 rays 4 + 16 + 13 = 33.  Ties: the more balanced split.
int64_t merged_split(int64_t n, int Sc, int Sf, int cus, bool always) {
  auto rounds = [&](int64_t passes) { return (passes + cus - 1) / cus; };
  auto passes = [&](int64_t rays, int S) { return (rays * S + 127) / 128; };
  int64_t best = 0, best_cost = -1, best_bal = 0;
  for (int64_t k = 128; k < n; k += 128) {
    const int64_t cost = rounds(passes(k, Sc)) + rounds(passes(k, Sf) + passes(n - k, Sc)) + rounds(passes(n - k, Sf));
    const int64_t bal = k < n - k ? n - 2 * k : 2 * k - n;
    if (best_cost < 0 || cost < best_cost || (cost == best_cost && bal < best_bal)) { best = k; best_cost = cost; best_bal = bal; }
  }
  // not worth it when one launch per level is as good (small batches: everything fits one round)
  if (best_cost < 0 || (!always && best_cost >= rounds(passes(n, Sc)) + rounds(passes(n, Sf)))) return 0;
  return best;
}

struct TrainNet {   // one level's network handles
  const void* packed_fwd; const float* small; const void* packed_bwd;
};

int train_fwd_impl(const char* who, bool art, const TrainNet* nets, const PathCall& c) {
  auto bad = [&](const char* what) { return fail(AON_E_INVALID, (std::string(who) + ": " + what).c_str()); };
  // [per-ray bounds, DESIGN.md section 4.11] level 0's t from near_ray / far_ray; the backward reads t from the workspace and does not change
  if (c.bounds && c.bounds->live) return bad("ray_live is inference only (bounds->live must be NULL)");
  Geo g;
  if (const char* msg = make_geo(c.opts, g)) return fail(AON_E_INVALID, msg);
  if (g.Sf > 512) return bad("more than 512 samples per ray at the fine level");
  if (art) g.other_degrees = false;   // (as in render_impl: no stage-kernel encodings for the articulated network)
  if (int rc = path_call_check(who, c, g, false)) return rc;
  // (the record's fields under the names the schedules below use)
  const float* near_ray = c.bounds ? c.bounds->near_ray : nullptr;
  const float* far_ray = c.bounds ? c.bounds->far_ray : nullptr;
  const float* rays_o = c.rays_o; const float* rays_d = c.rays_d; const float* viewdirs = c.viewdirs;
  const float* t_rand = c.t_rand; const float* u = c.u;
  const int64_t n = c.n_rays, u_stride = c.u_stride;
  const int num_levels = c.num_levels, white_bkgd = c.white_bkgd;
  const float near_ = c.near_, far_ = c.far_;
  float* const* rgb = c.rgb; float* const* acc = c.acc; float* const* depth = c.depth;
  const hipStream_t stream = c.stream;
  const TrainWs w = carve_train(static_cast<char*>(c.workspace), n, art, num_levels, g);
  if (w.bytes > c.workspace_bytes) return fail(AON_E_WORKSPACE, (std::string(who) + ": workspace smaller than aon_train_workspace_bytes()").c_str());
  const bool fuse = num_levels == 2 && g.default_sizes && g_fuse_coarse.load(std::memory_order_relaxed) != 0;
  for (int l = 0; l < num_levels; ++l)
    if (!nets[l].packed_fwd || (art && !nets[l].small)) return bad("null level pointer");
  for (int l = 0; l < num_levels; ++l)
    if ((art && forms_differ(nets[l].packed_fwd, nets[l].small)) || forms_differ(nets[l].packed_fwd, nets[0].packed_fwd))
      return bad("the levels' streams / per-call blocks were made in different forms (aon_set_bottleneck_fold changed in between)");
  const int64_t rows = art ? aon::kAPlRows : aon::kPlRows;
  // the view-encoding term of the first view layer as a per-ray bias (aon_set_view_bias): both levels' biases of the whole batch up front
  const bool use_vb = !g.other_degrees && g_view_bias.load(std::memory_order_relaxed) != 0 && aon::stream_form(nets[0].packed_fwd) == aon::kFormFolded;
  if (use_vb)
    for (int l = 0; l < num_levels; ++l)
      if (int rc = check(aon::launch_net_view_bias(art, static_cast<const char*>(nets[l].packed_fwd), nets[l].small, viewdirs, n, w.lvl[l].vbias, stream), who))
        return rc;

  // The forward segment of level l of the ray range [r0, r0 + nk), and what follows its launch (LevelTail).  r0 is a multiple of 128, so
  // the range's samples start on a pass boundary at both levels: its planes / decision bits / raw records are the whole batch's buffers
  // at an offset, the slot stride of the decision bits stays the whole batch's Np.
  auto seg_of = [&](int64_t r0, int64_t nk, int l) {
    const TrainLevel& L = w.lvl[l];
    const int64_t s0 = r0 * L.S;
    return aon::FwdSeg{.packed = static_cast<const char*>(nets[l].packed_fwd), .small = nets[l].small, .rays_o = rays_o + r0 * 3, .rays_d = rays_d + r0 * 3,
                       .viewdirs = viewdirs + r0 * 3, .t_vals = L.t + s0, .n_rays = nk, .S = L.S, .raw = L.raw + s0 * 4, .planes = L.planes + s0 * rows,
                       .masks = L.masks + s0 * 32, .np_total = L.Np, .view_bias = use_vb ? L.vbias + r0 * aon::kCondWidth : nullptr};
  };
  auto tail_of = [&](int64_t r0, int64_t nk, int l, hipStream_t st) {
    const TrainLevel& L = w.lvl[l];
    const bool next = l == 0 && num_levels == 2;
    return LevelTail{L.raw + r0 * L.S * 4, L.t + r0 * L.S, rays_d + r0 * 3, nk, L.S, r0, white_bkgd, art, g, fuse && l == 0, u, u_stride,
                     rgb[l] + r0 * 3, acc[l] + r0, depth[l] + r0, next ? w.w_c + r0 * g.Sc : nullptr, next ? w.lvl[1].t + r0 * w.lvl[1].S : nullptr, st, who};
  };
  auto mlp = [&](const aon::FwdSeg* segs, int ns, hipStream_t st) {
    int64_t samples = 0;
    for (int i = 0; i < ns; ++i) samples += segs[i].n_rays * segs[i].S;
    MlpTimer timer(st, samples);
    return check(aon::launch_net_fwd(art, segs, ns, st), who);
  };

  // Both levels of the ray range [r0, r0 + nk) on stream `st`.
  auto run_range = [&](int64_t r0, int64_t nk, hipStream_t st) -> int {
    {
      KTimer timer(kSampleT, st, nk);
      if (int rc = check(aon::launch_sample_along_rays(rays_o + r0 * 3, rays_d + r0 * 3, nk, g.Sc, near_, far_, t_rand ? t_rand + r0 * g.Sc : nullptr,
                                                       w.lvl[0].t + r0 * g.Sc, nullptr, st, g.lindisp, g.inv_near, g.inv_far, near_ray ? near_ray + r0 : nullptr,
                                                       far_ray ? far_ray + r0 : nullptr), who)) return rc;
    }
    for (int l = 0; l < num_levels; ++l) {
      aon::FwdSeg seg = seg_of(r0, nk, l);
      if (g.other_degrees) {
        // other encoding degrees: encodings by the stage kernels in the padded 63 / 27-slot layout, then the training forward on
        // caller-encoded inputs (same planes, same decision bits)
        const TrainLevel& L = w.lvl[l];
        const int64_t s0 = r0 * L.S;
        float* coords = L.coords + s0 * 3; float* enc = L.enc + s0 * aon::kPosEnc; float* venc = L.venc + r0 * aon::kViewEnc;
        if (int rc = check(aon::launch_cast_rays(seg.t_vals, seg.rays_o, seg.rays_d, nk, L.S, coords, st), who)) return rc;
        if (int rc = check(aon::launch_pos_enc(coords, nk * L.S, g.min_deg, g.max_deg, enc, st, aon::kPosEnc, 10), who)) return rc;
        if (int rc = check(aon::launch_pos_enc(seg.viewdirs, nk, 0, g.deg_view, venc, st, aon::kViewEnc, 4), who)) return rc;
        seg.rays_o = seg.rays_d = seg.viewdirs = seg.t_vals = nullptr;
        seg.samples_enc = enc; seg.viewdirs_enc = venc;
      }
      if (int rc = mlp(&seg, 1, st)) return rc;
      if (int rc = l == 0 ? coarse_tail(tail_of(r0, nk, 0, st)) : fine_tail(tail_of(r0, nk, 1, st))) return rc;
    }
    return AON_OK;
  };

  // Merged form (round 4, default): coarse(A) | fine(A) + coarse(B) | fine(B) as three persistent launches on the caller's stream.
  if (const int merge = g_fwd_merge.load(std::memory_order_relaxed); num_levels == 2 && !g.other_degrees && merge) {
    const int cus = aon::num_cus();
    const int64_t kA = cus > 0 ? merged_split(n, g.Sc, g.Sf, cus, merge == 2) : 0;
    if (kA > 0) {
      struct Rng { int64_t r0, nk; };
      const Rng R[2] = {{0, kA}, {kA, n - kA}};
      auto coarse = [&](const Rng& r) { return coarse_tail(tail_of(r.r0, r.nk, 0, stream)); };   // compositing + inverse CDF -> the range's fine t
      auto fine = [&](const Rng& r) { return fine_tail(tail_of(r.r0, r.nk, 1, stream)); };
      {   // stratified t of the whole batch
        KTimer timer(kSampleT, stream, n);
        if (int rc = check(aon::launch_sample_along_rays(rays_o, rays_d, n, g.Sc, near_, far_, t_rand, w.lvl[0].t, nullptr, stream, g.lindisp, g.inv_near,
                                                         g.inv_far, near_ray, far_ray), who)) return rc;
      }
      const aon::FwdSeg cA = seg_of(R[0].r0, R[0].nk, 0), fB = seg_of(R[1].r0, R[1].nk, 1);
      const aon::FwdSeg mid[2] = {seg_of(R[0].r0, R[0].nk, 1), seg_of(R[1].r0, R[1].nk, 0)};
      if (int rc = mlp(&cA, 1, stream)) return rc;
      if (int rc = coarse(R[0])) return rc;
      if (int rc = mlp(mid, 2, stream)) return rc;
      if (int rc = coarse(R[1])) return rc;
      if (int rc = fine(R[0])) return rc;
      if (int rc = mlp(&fB, 1, stream)) return rc;
      return fine(R[1]);
    }
  }

  // Two ray halves on the two library streams (round 3): the levels of a half depend on each other through its own inverse CDF
  // only, so one half's fine level fills the CUs the other half's coarse level leaves idle in its last, partial round of
  // workgroups (8.125 rounds of 256 cost 9 at 4096 x 65 samples), as the backward does with its two levels.
  const int parts = g_fwd_overlap.load(std::memory_order_relaxed);   // 0 / 1: one stream; k >= 2: k ray ranges alternating on the two streams
  const int64_t piece = parts >= 2 ? (n / parts) / 128 * 128 : 0;
  if (num_levels == 2 && piece > 0) {
    LevelFork fork(true, stream, who);
    if (fork.rc()) return fork.rc();
    for (int k = 0; k < parts; ++k) {
      const int64_t r0 = k * piece, nk = k == parts - 1 ? n - r0 : piece;
      if (int rc = run_range(r0, nk, fork.stream(k & 1))) return rc;
    }
    return fork.join();
  }
  return run_range(0, n, stream);
}

// What a backward entry point brings beside its call record (BwdCall, aon_capi_util.h) and its TrainNet[2]; pointers it does not have are null.
struct BwdIo {
  const float* const* params[2];   // [articulated] the forward's parameters, 40 device pointers per level
  const float* latents[3];         // [articulated, full backward] shape, appearance, articulation
  float* const* grads[2];          // [full backward] the parameter gradients per level
  float* g_latents[3];             // [articulated]
  const aon_ray_grads* rg;         // [aon_art_render_bwd_inputs]
};

// One level's compositing backward on `st`, the first stage of every backward here: d_raw (Np, 4) with its padded tail zeroed.
// (static, as train_bwd_impl: under this file's extern "C" a function of the unnamed namespace would still be exported by name)
static int composite_bwd_stage(const char* who, bool art, int l, const TrainLevel& L, float* d_raw, const Geo& g, const BwdCall& c, hipStream_t st) {
  const int64_t valid = c.n_rays * L.S;
  if (int rc = check(hipMemsetAsync(d_raw + valid * 4, 0, (size_t)(L.Np - valid) * 16, st), who)) return rc;
  KTimer timer(kCompositeBwd, st, c.n_rays);
  return check(aon::launch_composite_bwd(L.raw, L.t, c.rays_d, c.g_rgb[l], c.acc(l), c.depth(l), c.n_rays, L.S, c.white_bkgd, g.act(art, l, 0), d_raw, st), who);
}
// [articulated] one level's segment of the backward chain: the per-call block, planes and dxp
static aon::ChainSeg art_chain_seg(const TrainNet& net, const TrainLevel& L, float* d_raw, float* dplanes, float* dxp) {
  return aon::ChainSeg{static_cast<const char*>(net.packed_bwd), net.small, d_raw, L.masks, L.planes, dplanes, dxp, L.Np};
}

// The whole backward of a training step, shared by the vanilla and the articulated network (as train_fwd_impl is for the forward): composite
// backward -> backward chain -> weight gradients per level, in the schedule the switches select.  What differs between the networks is
// marked [vanilla] / [articulated] where it happens:
//   the chain segment, the null / form checks, the overlap mode, who waits for the early head reductions, the conditions of the merged second
//   stage, the remap of the encoding-fed gradients at other degrees [vanilla], the latent gradients [articulated].
static int train_bwd_impl(const char* who, bool art, const TrainNet* nets, const BwdCall& c, const BwdIo& io) {
  auto bad = [&](int code, const char* what) { return fail(code, (std::string(who) + ": " + what).c_str()); };
  Geo g;
  if (const char* b = make_geo(c.opts, g)) return fail(AON_E_INVALID, b);
  if (art) g.other_degrees = false;   // (as in train_fwd_impl: the articulated kernels carry their degrees themselves)
  const bool lat_null = !io.params[0] || !io.latents[0] || !io.latents[1] || !io.latents[2] || !io.g_latents[0] || !io.g_latents[1] || !io.g_latents[2];
  if (int rc = bwd_call_check(who, c, !io.grads[0] || (art && lat_null))) return rc;
  // (the record's fields under the names the schedule below uses)
  const int64_t n_rays = c.n_rays;
  const int num_levels = c.num_levels;
  const hipStream_t caller = c.stream;
  const float* const* const* params = io.params; const float* const* latents = io.latents;
  float* const* const* grads = io.grads; float* const* g_latents = io.g_latents;
  const TrainWs w = carve_train(static_cast<char*>(c.workspace), n_rays, art, num_levels, g);
  if (w.bytes > c.workspace_bytes) return bad(AON_E_WORKSPACE, "workspace smaller than aon_train_workspace_bytes()");
  const TrainScratch sc = carve_scratch(static_cast<char*>(c.scratch), n_rays, art, num_levels, g);
  if (sc.bytes > c.scratch_bytes) return bad(AON_E_WORKSPACE, "scratch smaller than aon_train_scratch_bytes()");
  const int nparams = art ? aon::kNumArtParams : aon::kNumVanillaParams;
  for (int l = 0; l < num_levels; ++l) {
    // the transposed stream's form is checked against its mate's: [vanilla] the forward stream, [articulated] the per-call block
    const void* pb = nets[l].packed_bwd;
    const void* mate = art ? static_cast<const void*>(nets[l].small) : nets[l].packed_fwd;
    if (!pb || !mate || !grads[l] || (art && !params[l]) || !c.g_rgb[l]) return bad(AON_E_INVALID, "null level pointer");
    if (aon::stream_form(pb) != aon::stream_form(mate) || aon::stream_form(pb) != aon::stream_form(nets[0].packed_bwd))
      return bad(AON_E_INVALID, art ? "transposed stream and per-call block were made in different forms (aon_set_bottleneck_fold changed in between)"
                                    : "forward and transposed streams were packed in different forms (aon_set_bottleneck_fold changed in between)");
    for (int i = 0; i < nparams; ++i)
      if (!grads[l][i] || (art && !params[l][i])) return bad(AON_E_INVALID, art ? "null parameter / gradient pointer" : "null gradient pointer");
  }
  auto composite_bwd = [&](int l, hipStream_t st) { return composite_bwd_stage(who, art, l, w.lvl[l], sc.d_raw[l], g, c, st); };
  // [vanilla] the small block sits behind the forward stream, no planes / dxp
  auto chain_seg = [&](int l) -> aon::ChainSeg {
    const TrainLevel& L = w.lvl[l];
    if (art) return art_chain_seg(nets[l], L, sc.d_raw[l], sc.dplanes[l], sc.dxp[l]);
    return aon::ChainSeg{static_cast<const char*>(nets[l].packed_bwd),
                         reinterpret_cast<const float*>(static_cast<const char*>(nets[l].packed_fwd) + aon::kStreamBytes), sc.d_raw[l], L.masks, nullptr,
                         sc.dplanes[l], nullptr, L.Np};
  };
  auto chain = [&](const aon::ChainSeg* segs, int ns, hipStream_t st) {
    return check(art ? aon::launch_art_bwd_chain2(segs, ns, st) : aon::launch_mlp_bwd_chain2(segs, ns, st), who);
  };
  // Round 4: the two levels' chains are independent -> ONE persistent launch of two segments on the caller's stream (33 rounds of
  // workgroups instead of 9 + 25 at 4096 x (65 + 193) samples), then the weight gradients of the two levels on the two streams.
  const bool merged = num_levels == 2 && g_bwd_merge.load(std::memory_order_relaxed) != 0;
  // 0: none; 1: round-3 level streams when not merged; 2: + head reductions on side streams when merged.  [articulated] mode 1 means
  // mode 2 -- each level's remaining head reductions (six jobs, 70 + 185 us, HBM-bound ordinary blocks) go onto the level's aux stream
  // just BEFORE its grouped kernel and run beside it instead of in front of it (30.418 -> 30.309 ms per 4096-ray step, same bits); the
  // vanilla network's three head jobs gain nothing (24.446 vs 24.423 ms) and keep mode 1.
  const int overlap_raw = g_bwd_overlap.load(std::memory_order_relaxed);
  const int overlap_mode = (art && overlap_raw == 1) ? 2 : overlap_raw;
  // Round 5: the head / bias reductions that need nothing from the chain run on a side stream beside the merged chain launch (g_bwd_early_heads)
  const bool early_heads = merged && g_bwd_early_heads.load(std::memory_order_relaxed) != 0;
  // fork: with two levels each runs on its own library stream, ordered after everything already enqueued on the caller's
  // (merged: no LEVEL streams -- chain and weight gradients follow each other on the caller's stream; with equal-cost workgroups filling the
  // chip in every launch the dispatcher's sharing of compute units between streams costs more than the tails it used to fill:
  // profiles/r04_backward_schedules.txt.  The one tail that is left, the chain's last quarter-full round, takes the early head reductions.)
  LevelFork fork(num_levels == 2 && (merged ? (overlap_mode == 2 || early_heads) : overlap_mode != 0), caller, who, merged);
  if (fork.rc()) return fork.rc();
  const aon::WgAux* side = early_heads ? fork.aux(0) : nullptr;
  // Round 6: ONE second stage for both levels.  Level 0's (reduce 20 us -> un-folding products 18 us -> finishing kernel 15 us, plus an
  // event gap either side) used to sit between the two grouped kernels with the chip all but idle; deferred, the grouped kernels follow
  // each other and the levels' reduce blocks, un-folding products and [articulated] finishing kernels go out as 1 + 1 (+ 2) launches behind
  // level 1's (launch_*_wgrad_post2; every block does what it did: same bits, tools/grad_hash.py).  Default degrees only (other degrees put
  // remap launches between the stages).
  const bool post_merged = merged &&
                           (art ? g.max_deg - g.min_deg == 10 && g.deg_view == 4 && aon::art_wgrad_deferred_bytes() <= aon::kArtWgDeferredBytes
                                : !g.other_degrees && aon::vanilla_wgrad_deferred_bytes() <= aon::kVanillaWgDeferredBytes);
  constexpr int kDeferBytes = aon::kArtWgDeferredBytes > aon::kVanillaWgDeferredBytes ? aon::kArtWgDeferredBytes : aon::kVanillaWgDeferredBytes;
  alignas(16) unsigned char defer_store[2][kDeferBytes];
  auto vanilla_deferred = [&](int l) { return reinterpret_cast<aon::VanillaWgDeferred*>(defer_store[l]); };
  auto art_deferred = [&](int l) { return reinterpret_cast<aon::ArtWgDeferred*>(defer_store[l]); };
  // one level's weight-gradient call.  gl: where its parameter gradients go; wait_first: [vanilla] see below
  auto level_wgrad = [&](int l, hipStream_t st, const aon::WgAux* aux, int phase, float* const* gl, hipEvent_t wait_first) {
    const TrainLevel& L = w.lvl[l];
    const bool defer = post_merged && phase != aon::kWgEarly;
    if (!art)
      return check(aon::launch_vanilla_wgrad(L.planes, sc.dplanes[l], sc.d_raw[l], L.Np, gl, sc.wgrad_ws[l], st, aux, nets[l].packed_bwd, phase, wait_first,
                                             defer ? vanilla_deferred(l) : nullptr), who);
    // [articulated] level 0 writes the latent gradients, level 1 adds its own (both MLPs see the same latents).  Merged schedule (round 6): both
    // levels' finishing kernels run on the caller's stream in level order, so level 1's adds onto level 0's result in place (g = coarse + fine, the
    // bits of the three add launches this replaces); level streams: into a temporary, added after the join
    const bool acc = merged && l == 1;
    float* gs = (l == 0 || acc) ? g_latents[0] : sc.lat_tmp, *ga = (l == 0 || acc) ? g_latents[1] : sc.lat_tmp + 128, *gt = (l == 0 || acc) ? g_latents[2] : sc.lat_tmp + 256;
    return check(aon::launch_art_wgrad(L.planes, sc.dplanes[l], sc.d_raw[l], sc.dxp[l], L.Np, params[l], latents[0], latents[1], latents[2], gl, gs, ga, gt,
                                       sc.wgrad_ws[l], st, aux, g.max_deg - g.min_deg, g.deg_view, nets[l].packed_bwd, phase, acc, defer ? art_deferred(l) : nullptr), who);
  };
  bool early_unjoined = false;   // (the early reductions are on the side stream and the caller's stream has not been told to wait for them)
  if (merged) {
    for (int l = 0; l < 2; ++l)
      if (int rc = composite_bwd(l, caller)) return rc;
    if (side)
      if (int rc = check(hipEventRecord(side->fork, caller), who)) return rc;
    {
      const aon::ChainSeg segs[2] = {chain_seg(1), chain_seg(0)};
      KTimer timer(kBwdChain, caller, w.lvl[0].Np + w.lvl[1].Np);
      if (int rc = chain(segs, 2, caller)) return rc;
    }
    if (side) {   // enqueued BEHIND the chain in host order, eligible from the fork event on: the chain's workgroups take the chip first
      int rc = check(hipStreamWaitEvent(side->stream, side->fork, 0), who);
      for (int l = 0; l < 2 && !rc; ++l) rc = level_wgrad(l, side->stream, nullptr, aon::kWgEarly, grads[l], nullptr);
      const int rj = check(hipEventRecord(side->join, side->stream), who);
      // Who waits for the early reductions (round 6): nobody needs their partial sums before level 0's SECOND stage (wgrad_reduce), so the
      // caller's stream does not wait here -- level 0's grouped kernel follows the chain directly instead of sitting out the reductions' tail
      // (90-160 us past the chain's end at 4096 rays, plus the event round trip).
      //   [vanilla] in every overlap mode: level 0's second stage is handed the event (wait_first), or the merged second stage waits for it.
      //   [articulated] in overlap mode 2 only: level 0's remaining reductions are queued on this very stream (aux(0) == side), behind the
      //   early ones, and run_wgrad_plan joins it in front of the second stage.  Mode 1 (remaining reductions on the caller's stream, no later
      //   join): the caller's stream waits here.
      early_unjoined = (!art || overlap_mode == 2) && !rc && !rj;
      const int rw = early_unjoined ? AON_OK : check(hipStreamWaitEvent(caller, side->join, 0), who);
      if (rc || rj || rw) return rc ? rc : (rj ? rj : rw);
    }
  }
  for (int l = 0; l < num_levels; ++l) {
    const TrainLevel& L = w.lvl[l];
    const hipStream_t stream = merged ? caller : fork.stream(l);
    if (!merged) {
      if (int rc = composite_bwd(l, stream)) return rc;
      const aon::ChainSeg seg = chain_seg(l);
      KTimer timer(kBwdChain, stream, L.Np);
      if (int rc = chain(&seg, 1, stream)) return rc;
    }
    KTimer timer(kWgrad, stream, L.Np);
    float* gl[aon::kMaxNetParams];
    for (int i = 0; i < nparams; ++i) gl[i] = grads[l][i];
    if (g.other_degrees) {   // [vanilla] the three encoding-fed weights come out in the kernels' 63 / 27-column layout, then lose the empty slots
      gl[aon::vp_trunk_w(0)] = sc.grad_tmp[l];
      gl[aon::vp_trunk_w(5)] = gl[aon::vp_trunk_w(0)] + 256 * aon::vp_trunk0_ld(aon::kPosEnc);
      gl[aon::kVpView0W] = gl[aon::vp_trunk_w(5)] + 256 * aon::vp_trunk5_ld(aon::kPosEnc);
    }
    const hipEvent_t wait_first = (!art && early_unjoined && l == 0 && !post_merged) ? side->join : nullptr;
    if (int rc = level_wgrad(l, stream, (merged && overlap_mode != 2) ? nullptr : fork.aux(l), side ? aon::kWgRest : aon::kWgAll, gl, wait_first)) {
      // the call failed before anything waited for the early reductions: the caller's stream waits here -- never leave side-stream work behind
      // the caller's view of this call (the workspace is the caller's to free)
      if (early_unjoined) (void)hipStreamWaitEvent(caller, side->join, 0);
      return rc;
    }
    // [articulated] run_wgrad_plan joined aux(0) == the early reductions' stream in front of level 0's second stage; [vanilla] level 0's second
    // stage has been told to wait for them -- or, merged second stage: still un-joined, joined in front of it below
    if (art || !post_merged) early_unjoined = false;
    if (g.other_degrees) {
      const int Lp = g.max_deg - g.min_deg, P = aon::enc_width(Lp), V = aon::enc_width(g.deg_view);
      auto remap = [&](const float* src, float* dst, int rows, int hidden, int Lx, int Lfull, int cols) {
        const int64_t tot = (int64_t)rows * cols;
        remap_enc_cols_kernel<<<dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, stream>>>(src, dst, rows, hidden, Lx, Lfull);
      };
      remap(gl[aon::vp_trunk_w(0)], grads[l][aon::vp_trunk_w(0)], 256, 0, Lp, 10, aon::vp_trunk0_ld(P));
      remap(gl[aon::vp_trunk_w(5)], grads[l][aon::vp_trunk_w(5)], 256, aon::kTrunk5EncCol, Lp, 10, aon::vp_trunk5_ld(P));
      remap(gl[aon::kVpView0W], grads[l][aon::kVpView0W], 128, aon::kView0EncCol, g.deg_view, 4, aon::vp_view0_ld(V));
      if (int rc = check(hipGetLastError(), who)) return rc;
    }
  }
  if (post_merged) {
    if (early_unjoined)
      if (int rc = check(hipStreamWaitEvent(caller, side->join, 0), who)) return rc;
    KTimer timer(kWgrad, caller, 0);
    if (int rc = check(art ? aon::launch_art_wgrad_post2(art_deferred(0), art_deferred(1), caller)
                           : aon::launch_vanilla_wgrad_post2(vanilla_deferred(0), vanilla_deferred(1), caller), who)) return rc;
  }
  if (int rc = fork.join()) return rc;   // the caller's stream continues after both levels
  if (art && num_levels == 2 && !merged) {   // [articulated] level 1's latent gradients, from the temporary
    add_into_kernel<<<dim3(1), dim3(128), 0, caller>>>(g_latents[0], sc.lat_tmp, 128);
    add_into_kernel<<<dim3(1), dim3(128), 0, caller>>>(g_latents[1], sc.lat_tmp + 128, 128);
    add_into_kernel<<<dim3(1), dim3(32), 0, caller>>>(g_latents[2], sc.lat_tmp + 256, 32);
    return check(hipGetLastError(), who);
  }
  return AON_OK;
}

// ---- the backwards of a frozen network: latent gradients [articulated] and ray gradients (DESIGN.md sections 4.13 - 4.15) ----
// TrainScratch without its weight-gradient workspaces (96 MiB a level) and temporaries: what the compositing backward and the chain write,
// [articulated] the partial sums of the four bias gradients a latent enters through, and behind all of that the ray gradients' per-sample records.
struct FrozenScratch {
  float* d_raw[2]; float* dplanes[2];
  float* dxp[2]; float* ws[2];   // [articulated]
  float* rec[2];                 // with ray_records
  int64_t bytes;
};
static FrozenScratch carve_scratch_frozen(char* base, int64_t n, bool art, int num_levels, const Geo& g, bool ray_records) {
  FrozenScratch sc{};
  int64_t off = 0;
  auto take = [&](int64_t bytes) { char* p = base + off; off += align_up(bytes, 256); return reinterpret_cast<float*>(p); };
  for (int l = 0; l < num_levels; ++l) {
    const int64_t Np = level_np(n, l, g);
    sc.d_raw[l] = take(Np * 16);
    sc.dplanes[l] = take((int64_t)(art ? aon::kAPlRows : aon::kPlRows) * Np * 4);
    if (!art) continue;
    sc.dxp[l] = take(Np * 16);
    sc.ws[l] = take(aon::art_latent_ws_bytes());
  }
  if (ray_records)
    for (int l = 0; l < num_levels; ++l) sc.rec[l] = take(aon::ray_grad_record_bytes(level_np(n, l, g)));
  sc.bytes = off;
  return sc;
}

// Shared by the two networks as train_bwd_impl is: composite backward -> backward chain by the functions train_bwd_impl launches them with
// (same gradient planes), then [articulated] the two launches of aon_train_latent.hip and, with io.rg, the two of the ray gradients.
// Everything on the caller's stream; no weight-gradient stage, no head reductions, no un-folding.
//   io.rg: [articulated] optional -- without it the call IS the latent-only call; [vanilla] required
static int frozen_bwd_impl(const char* who, bool art, const TrainNet* nets, const BwdCall& c, const BwdIo& io) {
  auto bad = [&](int code, const char* what) { return fail(code, (std::string(who) + ": " + what).c_str()); };
  Geo g;
  if (const char* b = make_geo(c.opts, g)) return fail(AON_E_INVALID, b);
  if (art) g.other_degrees = false;   // (the articulated kernels carry their degrees themselves)
  const aon_ray_grads* rg = io.rg;
  float* const* g_latents = io.g_latents;
  // [articulated; ray gradients, DESIGN.md section 4.14] with rg the three latent outputs may all be null (a pose fitted under fixed codes)
  const bool want_latents = art && (g_latents[0] || g_latents[1] || g_latents[2] || !rg);
  const char* rg_bad = (!rg && !art) ? "null aon_ray_grads"
                       : (rg && (!rg->rays_o || !rg->viewdirs || !rg->g_rays_o || !rg->g_rays_d || !rg->g_viewdirs)) ? "null member of aon_ray_grads" : nullptr;
  if (int rc = bwd_call_check(who, c, want_latents && (!g_latents[0] || !g_latents[1] || !g_latents[2]), rg_bad)) return rc;
  const int64_t n_rays = c.n_rays;
  const int num_levels = c.num_levels;
  const hipStream_t caller = c.stream;
  const float* const* const* params = io.params;
  const TrainWs w = carve_train(static_cast<char*>(c.workspace), n_rays, art, num_levels, g);
  if (w.bytes > c.workspace_bytes) return bad(AON_E_WORKSPACE, "workspace smaller than aon_train_workspace_bytes()");
  const FrozenScratch sc = carve_scratch_frozen(static_cast<char*>(c.scratch), n_rays, art, num_levels, g, rg != nullptr);
  if (sc.bytes > c.scratch_bytes)
    return bad(AON_E_WORKSPACE, !art ? "scratch smaller than aon_train_scratch_bytes_inputs_vanilla()"
                                : rg ? "scratch smaller than aon_train_scratch_bytes_inputs()" : "scratch smaller than aon_train_scratch_bytes_latents()");
  for (int l = 0; l < num_levels; ++l) {
    // the transposed stream's form is checked against its mate's: [vanilla] the forward stream, [articulated] the per-call block
    const void* pb = nets[l].packed_bwd;
    const void* mate = art ? static_cast<const void*>(nets[l].small) : nets[l].packed_fwd;
    if (!pb || !mate || !params[l] || !c.g_rgb[l]) return bad(AON_E_INVALID, "null level pointer");
    if (aon::stream_form(pb) != aon::stream_form(mate) || aon::stream_form(pb) != aon::stream_form(nets[0].packed_bwd))
      return bad(AON_E_INVALID, art ? "transposed stream and per-call block were made in different forms (aon_set_bottleneck_fold changed in between)"
                                    : "forward and transposed streams were packed in different forms (aon_set_bottleneck_fold changed in between)");
    // [articulated] the weights a latent enters: all the W^T db products read (the ray gradients read 0 and 26); [vanilla] the weights the
    // encodings enter through
    const int read[4] = {0, 10, art ? 20 : 16, 26};
    for (int k = 0; k < (art ? 4 : 3); ++k)
      if (!params[l][read[k]]) return bad(AON_E_INVALID, "null parameter pointer");
  }
  for (int l = 0; l < num_levels; ++l)
    if (int rc = composite_bwd_stage(who, art, l, w.lvl[l], sc.d_raw[l], g, c, caller)) return rc;
  // [vanilla] the small block sits behind the forward stream, no planes / dxp
  auto chain_seg = [&](int l) {
    const TrainLevel& L = w.lvl[l];
    if (art) return art_chain_seg(nets[l], L, sc.d_raw[l], sc.dplanes[l], sc.dxp[l]);
    return aon::ChainSeg{static_cast<const char*>(nets[l].packed_bwd),
                         reinterpret_cast<const float*>(static_cast<const char*>(nets[l].packed_fwd) + aon::kStreamBytes), sc.d_raw[l], L.masks, nullptr,
                         sc.dplanes[l], nullptr, L.Np};
  };
  auto chain = [&](const aon::ChainSeg* segs, int ns, int64_t units) {
    KTimer timer(kBwdChain, caller, units);
    return check(art ? aon::launch_art_bwd_chain2(segs, ns, caller) : aon::launch_mlp_bwd_chain2(segs, ns, caller), who);
  };
  // two levels merged into one chain launch of two segments (aon_set_bwd_merge, as train_bwd_impl), else one launch per level
  if (num_levels == 2 && g_bwd_merge.load(std::memory_order_relaxed) != 0) {
    const aon::ChainSeg segs[2] = {chain_seg(1), chain_seg(0)};
    if (int rc = chain(segs, 2, w.lvl[0].Np + w.lvl[1].Np)) return rc;
  } else {
    for (int l = 0; l < num_levels; ++l) {
      const aon::ChainSeg seg = chain_seg(l);
      if (int rc = chain(&seg, 1, w.lvl[l].Np)) return rc;
    }
  }
  KTimer timer(kWgrad, caller, w.lvl[0].Np + (num_levels == 2 ? w.lvl[1].Np : 0));   // (the class of the stage these launches replace)
  if (want_latents) {
    aon::ArtLatentLevel lv[2];
    for (int l = 0; l < num_levels; ++l) lv[l] = aon::ArtLatentLevel{sc.dplanes[l], w.lvl[l].Np, nets[l].packed_bwd, params[l], sc.ws[l]};
    if (int rc = check(aon::launch_art_latent_grads(lv, num_levels, g.max_deg - g.min_deg, g.deg_view, g_latents[0], g_latents[1], g_latents[2], caller), who))
      return rc;
  }
  if (!rg) return AON_OK;
  // the ray gradients read what the chain left (gradient planes, [articulated] dxp) and the forward's t / raw: two launches, both levels in each
  aon::RayGradLevel rl[2];
  for (int l = 0; l < num_levels; ++l) {
    const TrainLevel& L = w.lvl[l];
    rl[l] = aon::RayGradLevel{sc.dplanes[l], sc.dxp[l], L.Np, params[l], sc.rec[l], L.t, L.raw, c.g_rgb[l], c.acc(l), c.depth(l), g.act(art, l, 0), L.S};
  }
  return check(art ? aon::launch_ray_grads(rl, num_levels, n_rays, g.deg_view, c.white_bkgd, c.rays_d, rg->viewdirs, rg->g_rays_o, rg->g_rays_d, rg->g_viewdirs, caller)
                   : aon::launch_vanilla_ray_grads(rl, num_levels, n_rays, g.min_deg, g.max_deg - g.min_deg, g.deg_view, c.white_bkgd, rg->rays_o, c.rays_d,
                                                   rg->viewdirs, rg->g_rays_o, rg->g_rays_d, rg->g_viewdirs, caller), who);
}

}  // namespace

int aon_set_bwd_overlap(int on) {
  g_bwd_overlap.store(on == 2 ? 2 : (on ? 1 : 0), std::memory_order_relaxed);
  return AON_OK;
}

int aon_set_bwd_early_heads(int on) {
  g_bwd_early_heads.store(on ? 1 : 0, std::memory_order_relaxed);
  return AON_OK;
}

int aon_set_bwd_merge(int on) {
  g_bwd_merge.store(on ? 1 : 0, std::memory_order_relaxed);
  return AON_OK;
}

int aon_set_fwd_merge(int on) {
  g_fwd_merge.store(on == 2 ? 2 : (on ? 1 : 0), std::memory_order_relaxed);   // 2 (tests): merge whenever there are two ranges, gain or not
  return AON_OK;
}

int aon_set_fwd_overlap(int on) {
  g_fwd_overlap.store(on < 0 ? 0 : (on == 1 ? 2 : (on > 16 ? 16 : on)), std::memory_order_relaxed);   // 1 = the default two halves; k >= 2: k ranges (measurements)
  return AON_OK;
}

// the size queries: the forward's workspace or one of the backwards' scratch for n_rays (at least one) of the levels in use
enum TrainBytes { kWorkspaceBytes, kScratchBytes, kLatentScratchBytes, kInputScratchBytes };
static int64_t train_bytes_query(TrainBytes what, int64_t n_rays, int articulated, int num_levels, const aon_render_opts* opts) {
  Geo g;
  if (const char* bad = make_geo(opts, g)) return fail(AON_E_INVALID, bad);
  if (n_rays < 1) n_rays = 1;
  const int levels = num_levels == 1 ? 1 : 2;
  switch (what) {
    case kWorkspaceBytes: return carve_train(nullptr, n_rays, articulated != 0, levels, g).bytes;
    case kScratchBytes: return carve_scratch(nullptr, n_rays, articulated != 0, levels, g).bytes;
    default: return carve_scratch_frozen(nullptr, n_rays, articulated != 0, levels, g, what == kInputScratchBytes).bytes;
  }
}
int64_t aon_train_workspace_bytes_ex(int64_t n_rays, int articulated, int num_levels, const aon_render_opts* opts) {
  return train_bytes_query(kWorkspaceBytes, n_rays, articulated, num_levels, opts);
}
int64_t aon_train_workspace_bytes(int64_t n_rays, int articulated, int num_levels) {
  return aon_train_workspace_bytes_ex(n_rays, articulated, num_levels, nullptr);
}
int64_t aon_train_scratch_bytes_ex(int64_t n_rays, int articulated, int num_levels, const aon_render_opts* opts) {
  return train_bytes_query(kScratchBytes, n_rays, articulated, num_levels, opts);
}
int64_t aon_train_scratch_bytes(int64_t n_rays, int articulated, int num_levels) {
  return aon_train_scratch_bytes_ex(n_rays, articulated, num_levels, nullptr);
}
int64_t aon_train_scratch_bytes_latents(int64_t n_rays, int num_levels, const aon_render_opts* opts) {
  return train_bytes_query(kLatentScratchBytes, n_rays, 1, num_levels, opts);
}
int64_t aon_train_scratch_bytes_inputs(int64_t n_rays, int num_levels, const aon_render_opts* opts) {
  return train_bytes_query(kInputScratchBytes, n_rays, 1, num_levels, opts);
}

// ---- the exported training forwards: each lists its parameters once (the ABI) and builds the call record; _ex is _bounds without bounds ----
// per-ray near / far under grad mode: DESIGN.md section 4.11; model.py:147-160, model_autodecoder.py:278-291 with (N, 1) tensors
int aon_render_fwd_train_bounds(const void* packed_coarse, const void* packed_fine, const float* rays_o, const float* rays_d, const float* viewdirs,
                                int64_t n_rays, float near_, float far_, int white_bkgd, int num_levels, const float* t_rand, const float* u,
                                int64_t u_stride, float* rgb_c, float* acc_c, float* depth_c, float* rgb_f, float* acc_f, float* depth_f,
                                void* workspace, int64_t workspace_bytes, void* stream, const aon_render_opts* opts, const aon_ray_bounds* bounds) {
  const TrainNet nets[2] = {{packed_coarse, nullptr, nullptr}, {packed_fine, nullptr, nullptr}};
  return train_fwd_impl(bounds ? "aon_render_fwd_train_bounds" : "aon_render_fwd_train", false, nets,
                        path_call(rays_o, rays_d, viewdirs, n_rays, near_, far_, white_bkgd, num_levels, t_rand, u, u_stride, rgb_c, acc_c, depth_c, rgb_f,
                                  acc_f, depth_f, workspace, workspace_bytes, stream, opts, bounds));
}
int aon_render_fwd_train_ex(const void* packed_coarse, const void* packed_fine, const float* rays_o, const float* rays_d, const float* viewdirs,
                            int64_t n_rays, float near_, float far_, int white_bkgd, int num_levels, const float* t_rand, const float* u,
                            int64_t u_stride, float* rgb_c, float* acc_c, float* depth_c, float* rgb_f, float* acc_f, float* depth_f,
                            void* workspace, int64_t workspace_bytes, void* stream, const aon_render_opts* opts) {
  return aon_render_fwd_train_bounds(packed_coarse, packed_fine, rays_o, rays_d, viewdirs, n_rays, near_, far_, white_bkgd, num_levels, t_rand, u,
                                     u_stride, rgb_c, acc_c, depth_c, rgb_f, acc_f, depth_f, workspace, workspace_bytes, stream, opts, nullptr);
}
int aon_render_fwd_train(const void* packed_coarse, const void* packed_fine, const float* rays_o, const float* rays_d, const float* viewdirs,
                         int64_t n_rays, float near_, float far_, int white_bkgd, int num_levels, const float* t_rand, const float* u,
                         int64_t u_stride, float* rgb_c, float* acc_c, float* depth_c, float* rgb_f, float* acc_f, float* depth_f,
                         void* workspace, int64_t workspace_bytes, void* stream) {
  return aon_render_fwd_train_ex(packed_coarse, packed_fine, rays_o, rays_d, viewdirs, n_rays, near_, far_, white_bkgd, num_levels, t_rand, u,
                                 u_stride, rgb_c, acc_c, depth_c, rgb_f, acc_f, depth_f, workspace, workspace_bytes, stream, nullptr);
}

int aon_art_render_fwd_train_bounds(const void* packed_coarse, const void* small_coarse, const void* packed_fine, const void* small_fine,
                                    const float* rays_o, const float* rays_d, const float* viewdirs, int64_t n_rays, float near_, float far_,
                                    int white_bkgd, int num_levels, const float* t_rand, const float* u, int64_t u_stride, float* rgb_c,
                                    float* acc_c, float* depth_c, float* rgb_f, float* acc_f, float* depth_f, void* workspace,
                                    int64_t workspace_bytes, void* stream, const aon_render_opts* opts, const aon_ray_bounds* bounds) {
  const TrainNet nets[2] = {{packed_coarse, static_cast<const float*>(small_coarse), nullptr}, {packed_fine, static_cast<const float*>(small_fine), nullptr}};
  return train_fwd_impl(bounds ? "aon_art_render_fwd_train_bounds" : "aon_art_render_fwd_train", true, nets,
                        path_call(rays_o, rays_d, viewdirs, n_rays, near_, far_, white_bkgd, num_levels, t_rand, u, u_stride, rgb_c, acc_c, depth_c, rgb_f,
                                  acc_f, depth_f, workspace, workspace_bytes, stream, opts, bounds));
}
int aon_art_render_fwd_train_ex(const void* packed_coarse, const void* small_coarse, const void* packed_fine, const void* small_fine,
                                const float* rays_o, const float* rays_d, const float* viewdirs, int64_t n_rays, float near_, float far_,
                                int white_bkgd, int num_levels, const float* t_rand, const float* u, int64_t u_stride, float* rgb_c,
                                float* acc_c, float* depth_c, float* rgb_f, float* acc_f, float* depth_f, void* workspace,
                                int64_t workspace_bytes, void* stream, const aon_render_opts* opts) {
  return aon_art_render_fwd_train_bounds(packed_coarse, small_coarse, packed_fine, small_fine, rays_o, rays_d, viewdirs, n_rays, near_, far_, white_bkgd,
                                         num_levels, t_rand, u, u_stride, rgb_c, acc_c, depth_c, rgb_f, acc_f, depth_f, workspace, workspace_bytes,
                                         stream, opts, nullptr);
}
int aon_art_render_fwd_train(const void* packed_coarse, const void* small_coarse, const void* packed_fine, const void* small_fine,
                             const float* rays_o, const float* rays_d, const float* viewdirs, int64_t n_rays, float near_, float far_,
                             int white_bkgd, int num_levels, const float* t_rand, const float* u, int64_t u_stride, float* rgb_c,
                             float* acc_c, float* depth_c, float* rgb_f, float* acc_f, float* depth_f, void* workspace,
                             int64_t workspace_bytes, void* stream) {
  return aon_art_render_fwd_train_ex(packed_coarse, small_coarse, packed_fine, small_fine, rays_o, rays_d, viewdirs, n_rays, near_, far_, white_bkgd,
                                     num_levels, t_rand, u, u_stride, rgb_c, acc_c, depth_c, rgb_f, acc_f, depth_f, workspace, workspace_bytes,
                                     stream, nullptr);
}

// ---- the exported backwards: each lists its parameters once (the ABI), builds the call record and says what its network brings ----
int aon_render_bwd(const void* packed_bwd_coarse, const void* packed_fwd_coarse, const void* packed_bwd_fine, const void* packed_fwd_fine,
                   const float* rays_d, int64_t n_rays, int white_bkgd, int num_levels, const float* const* g_rgb_host,
                   const float* const* g_acc_host, const float* const* g_depth_host, float* const* grads_coarse_host,
                   float* const* grads_fine_host, void* workspace, int64_t workspace_bytes, void* scratch, int64_t scratch_bytes,
                   void* stream_) {
  return aon_render_bwd_ex(packed_bwd_coarse, packed_fwd_coarse, packed_bwd_fine, packed_fwd_fine, rays_d, n_rays, white_bkgd, num_levels, g_rgb_host,
                           g_acc_host, g_depth_host, grads_coarse_host, grads_fine_host, workspace, workspace_bytes, scratch, scratch_bytes, stream_,
                           nullptr);
}
int aon_render_bwd_ex(const void* packed_bwd_coarse, const void* packed_fwd_coarse, const void* packed_bwd_fine, const void* packed_fwd_fine,
                      const float* rays_d, int64_t n_rays, int white_bkgd, int num_levels, const float* const* g_rgb_host,
                      const float* const* g_acc_host, const float* const* g_depth_host, float* const* grads_coarse_host,
                      float* const* grads_fine_host, void* workspace, int64_t workspace_bytes, void* scratch, int64_t scratch_bytes,
                      void* stream_, const aon_render_opts* opts) {
  const TrainNet nets[2] = {{packed_fwd_coarse, nullptr, packed_bwd_coarse}, {packed_fwd_fine, nullptr, packed_bwd_fine}};
  BwdIo io{};
  io.grads[0] = grads_coarse_host; io.grads[1] = grads_fine_host;
  return train_bwd_impl("aon_render_bwd", false, nets,
                        bwd_call(rays_d, n_rays, white_bkgd, num_levels, g_rgb_host, g_acc_host, g_depth_host, workspace, workspace_bytes, scratch,
                                 scratch_bytes, stream_, opts), io);
}

// [articulated] what the three backwards of the articulated network share: the levels' handles, the parameter arrays, the latent gradients
struct ArtBwd { TrainNet nets[2]; BwdIo io; };
static ArtBwd art_bwd(const void* packed_bwd_coarse, const void* small_coarse, const void* packed_bwd_fine, const void* small_fine,
               const float* const* params_coarse_host, const float* const* params_fine_host, float* g_shape, float* g_appearance, float* g_articulation) {
  ArtBwd a{{{nullptr, static_cast<const float*>(small_coarse), packed_bwd_coarse}, {nullptr, static_cast<const float*>(small_fine), packed_bwd_fine}}, {}};
  a.io.params[0] = params_coarse_host; a.io.params[1] = params_fine_host;
  a.io.g_latents[0] = g_shape; a.io.g_latents[1] = g_appearance; a.io.g_latents[2] = g_articulation;
  return a;
}

int aon_art_render_bwd(const void* packed_bwd_coarse, const void* small_coarse, const void* packed_bwd_fine, const void* small_fine,
                       const float* rays_d, int64_t n_rays, int white_bkgd, int num_levels, const float* const* g_rgb_host,
                       const float* const* g_acc_host, const float* const* g_depth_host, const float* const* params_coarse_host,
                       const float* const* params_fine_host, const float* shape, const float* appearance, const float* articulation,
                       float* const* grads_coarse_host, float* const* grads_fine_host, float* g_shape, float* g_appearance,
                       float* g_articulation, void* workspace, int64_t workspace_bytes, void* scratch, int64_t scratch_bytes, void* stream_) {
  return aon_art_render_bwd_ex(packed_bwd_coarse, small_coarse, packed_bwd_fine, small_fine, rays_d, n_rays, white_bkgd, num_levels, g_rgb_host, g_acc_host,
                               g_depth_host, params_coarse_host, params_fine_host, shape, appearance, articulation, grads_coarse_host, grads_fine_host,
                               g_shape, g_appearance, g_articulation, workspace, workspace_bytes, scratch, scratch_bytes, stream_, nullptr);
}
int aon_art_render_bwd_ex(const void* packed_bwd_coarse, const void* small_coarse, const void* packed_bwd_fine, const void* small_fine,
                          const float* rays_d, int64_t n_rays, int white_bkgd, int num_levels, const float* const* g_rgb_host,
                          const float* const* g_acc_host, const float* const* g_depth_host, const float* const* params_coarse_host,
                          const float* const* params_fine_host, const float* shape, const float* appearance, const float* articulation,
                          float* const* grads_coarse_host, float* const* grads_fine_host, float* g_shape, float* g_appearance,
                          float* g_articulation, void* workspace, int64_t workspace_bytes, void* scratch, int64_t scratch_bytes, void* stream_,
                          const aon_render_opts* opts) {
  ArtBwd a = art_bwd(packed_bwd_coarse, small_coarse, packed_bwd_fine, small_fine, params_coarse_host, params_fine_host, g_shape, g_appearance, g_articulation);
  a.io.latents[0] = shape; a.io.latents[1] = appearance; a.io.latents[2] = articulation;
  a.io.grads[0] = grads_coarse_host; a.io.grads[1] = grads_fine_host;
  return train_bwd_impl("aon_art_render_bwd", true, a.nets,
                        bwd_call(rays_d, n_rays, white_bkgd, num_levels, g_rgb_host, g_acc_host, g_depth_host, workspace, workspace_bytes, scratch,
                                 scratch_bytes, stream_, opts), a.io);
}

// the latent-only backward and, with `rg`, the ray gradients (section 4.14); rg == NULL IS the latent-only call, name included
int aon_art_render_bwd_inputs(const void* packed_bwd_coarse, const void* small_coarse, const void* packed_bwd_fine, const void* small_fine,
                              const float* rays_d, int64_t n_rays, int white_bkgd, int num_levels, const float* const* g_rgb_host,
                              const float* const* g_acc_host, const float* const* g_depth_host, const float* const* params_coarse_host,
                              const float* const* params_fine_host, float* g_shape, float* g_appearance, float* g_articulation,
                              void* workspace, int64_t workspace_bytes, void* scratch, int64_t scratch_bytes, void* stream_,
                              const aon_render_opts* opts, const aon_ray_grads* rg) {
  ArtBwd a = art_bwd(packed_bwd_coarse, small_coarse, packed_bwd_fine, small_fine, params_coarse_host, params_fine_host, g_shape, g_appearance, g_articulation);
  a.io.rg = rg;
  return frozen_bwd_impl(rg ? "aon_art_render_bwd_inputs" : "aon_art_render_bwd_latents", true, a.nets,
                         bwd_call(rays_d, n_rays, white_bkgd, num_levels, g_rgb_host, g_acc_host, g_depth_host, workspace, workspace_bytes, scratch,
                                  scratch_bytes, stream_, opts), a.io);
}
int aon_art_render_bwd_latents(const void* packed_bwd_coarse, const void* small_coarse, const void* packed_bwd_fine, const void* small_fine,
                               const float* rays_d, int64_t n_rays, int white_bkgd, int num_levels, const float* const* g_rgb_host,
                               const float* const* g_acc_host, const float* const* g_depth_host, const float* const* params_coarse_host,
                               const float* const* params_fine_host, float* g_shape, float* g_appearance, float* g_articulation,
                               void* workspace, int64_t workspace_bytes, void* scratch, int64_t scratch_bytes, void* stream_,
                               const aon_render_opts* opts) {
  return aon_art_render_bwd_inputs(packed_bwd_coarse, small_coarse, packed_bwd_fine, small_fine, rays_d, n_rays, white_bkgd, num_levels, g_rgb_host,
                                   g_acc_host, g_depth_host, params_coarse_host, params_fine_host, g_shape, g_appearance, g_articulation, workspace,
                                   workspace_bytes, scratch, scratch_bytes, stream_, opts, nullptr);
}

// the ray gradients of a frozen vanilla network (declared in include/aon_hip_inputs.h)
int64_t aon_train_scratch_bytes_inputs_vanilla(int64_t n_rays, int num_levels, const aon_render_opts* opts) {
  return train_bytes_query(kInputScratchBytes, n_rays, 0, num_levels, opts);
}
int aon_render_bwd_inputs(const void* packed_bwd_coarse, const void* packed_fwd_coarse, const void* packed_bwd_fine, const void* packed_fwd_fine,
                          const float* rays_d, int64_t n_rays, int white_bkgd, int num_levels, const float* const* g_rgb_host,
                          const float* const* g_acc_host, const float* const* g_depth_host, const float* const* params_coarse_host,
                          const float* const* params_fine_host, void* workspace, int64_t workspace_bytes, void* scratch, int64_t scratch_bytes,
                          void* stream_, const aon_render_opts* opts, const aon_ray_grads* rg) {
  const TrainNet nets[2] = {{packed_fwd_coarse, nullptr, packed_bwd_coarse}, {packed_fwd_fine, nullptr, packed_bwd_fine}};
  BwdIo io{};
  io.params[0] = params_coarse_host; io.params[1] = params_fine_host;
  io.rg = rg;
  return frozen_bwd_impl("aon_render_bwd_inputs", false, nets,
                         bwd_call(rays_d, n_rays, white_bkgd, num_levels, g_rgb_host, g_acc_host, g_depth_host, workspace, workspace_bytes, scratch,
                                          scratch_bytes, stream_, opts), io);
}

}  // extern "C"
