// What the translation units of the extern "C" surface (aon_capi*.hip) share: the error record, the argument checks, the sampler /
// activation geometry of a call and the live profiler.  The state is defined once, in aon_capi.hip.  Hidden visibility: none of this is
// part of the library's interface.
#pragma once
#include "../../include/aon_hip.h"
#include "aon_launch.h"

#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

namespace aon {
namespace capi __attribute__((visibility("hidden"))) {

extern thread_local char g_err[256];

int fail(int code, const char* msg);
int check(hipError_t e, const char* where);

constexpr int kSc = 65, kSf = 193;

// round 5: the articulated calls take a packed stream AND a per-call block; both carry a form (bottleneck folded / literal, aon_fold.h)
extern const char* const kFormsMsg;
extern const char* const kNullBwdMsg;
// (an unknown pointer -- a copy nobody declared -- differs from everything, itself included)
inline bool forms_differ(const void* a, const void* b) {
  return a && b && (aon::stream_form(a) != aon::stream_form(b) || aon::stream_form(a) == aon::kFormUnknown);
}

// process-wide switches read by more than one file; every call reads them ONCE
extern std::atomic<int> g_fuse_coarse;   // aon_set_coarse_fusion
extern std::atomic<int> g_view_bias;     // aon_set_view_bias
extern std::atomic<int> g_deferred_view;   // aon_set_deferred_view

// Optional live timing of the path's kernels with HIP events on the LAUNCH stream (torch.cuda.Event would only see torch's
// current stream), by kernel class; bench.py turns the totals into roofline figures.  Off unless aon_profile_begin() was
// called: one mutex-guarded branch per launch otherwise.
enum KClass { kMlpFwd = AON_PROF_MLP_FWD, kBwdChain = AON_PROF_BWD_CHAIN, kWgrad = AON_PROF_WGRAD, kComposite = AON_PROF_COMPOSITE,
              kSamplePdf = AON_PROF_SAMPLE_PDF, kCompositeBwd = AON_PROF_COMPOSITE_BWD, kCompositePdf = AON_PROF_COMPOSITE_PDF, kSampleT = AON_PROF_SAMPLE_T,
              kNumClasses = AON_PROF_NUM_CLASSES };

struct Profiler {
  std::mutex mu;
  bool on = false;
  struct Rec { int cls; hipEvent_t start, stop; };
  std::vector<hipEvent_t> pool;
  size_t used = 0;
  std::vector<Rec> recs;
  int64_t units[kNumClasses] = {};
  // totals of the last completed aon_profile_end()
  double last_ms[kNumClasses] = {};
  int64_t last_launches[kNumClasses] = {};
  int64_t last_units[kNumClasses] = {};
};
extern Profiler g_prof;

struct KTimer {
  hipEvent_t stop = nullptr;
  hipStream_t stream;
  KTimer(int cls, hipStream_t s, int64_t units) : stream(s) {
    std::lock_guard<std::mutex> lk(g_prof.mu);
    if (!g_prof.on) return;
    while (g_prof.used + 2 > g_prof.pool.size()) {
      hipEvent_t e;
      if (hipEventCreate(&e) != hipSuccess) return;
      g_prof.pool.push_back(e);
    }
    hipEvent_t start = g_prof.pool[g_prof.used];
    stop = g_prof.pool[g_prof.used + 1];
    g_prof.used += 2;
    g_prof.recs.push_back({cls, start, stop});
    g_prof.units[cls] += units;
    (void)hipEventRecord(start, stream);
  }
  ~KTimer() { if (stop) (void)hipEventRecord(stop, stream); }
};
struct MlpTimer : KTimer {
  MlpTimer(hipStream_t s, int64_t samples) : KTimer(kMlpFwd, s, samples) {}
};

inline int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

// The sampler / activation geometry of one call: aon_render_opts resolved against the reference's defaults.
struct Geo {
  int Sc, Sf, nf;          // t values of level 0 / level 1, draws of the inverse CDF
  bool default_sizes;      // 65 / 193: the specialised per-ray kernels apply
  int lindisp; float inv_near, inv_far;
  const float* noise[2]; float noise_std;
  float rgb_scale, rgb_shift, sigma_bias;
  int min_deg, max_deg, deg_view;   // encoding degrees of a vanilla network on the fused kernels
  bool other_degrees;               // != (0, 10, 4): encodings computed outside the MLP kernel, in its padded 63 / 27 layout
  int S(int l) const { return l == 0 ? Sc : Sf; }
  aon::ActParams act(bool art, int level, int64_t ray0) const {
    aon::ActParams ap{art ? AON_ACT_ARTICULATED : AON_ACT_VANILLA, rgb_scale, rgb_shift, sigma_bias, nullptr, noise_std};
    if (noise[level] && noise_std > 0.f) ap.noise = noise[level] + ray0 * S(level);
    return ap;
  }
};

// returns nullptr when fine, else what is wrong
// `general_engine`: the aon_grender_* entry points take the network's degrees from aon_mlp_geometry and ignore the degree fields of
// aon_render_opts, so those fields are neither validated against the fused kernels' limits nor turned into `other_degrees` there (a C
// caller who fills them to match a (1, 12, 5) geometry used to get AON_E_INVALID from the general engine: ADVICE r3).
const char* make_geo(const aon_render_opts* o, Geo& g, bool general_engine = false);

// An aon_occupancy as handed to an entry point (DESIGN.md sections 4.9, 4.17): nullptr when fine, else what is wrong; occ_grid_bad also fills
// the kernels' view of the grid (hi = lo + cells * step: multiply, then add -- the last grid point of ops.grid_points)
inline const char* occ_cells_bad(const int64_t* cells3) {
  if (!cells3) return "null cell counts";
  for (int a = 0; a < 3; ++a)
    if (cells3[a] < 1 || cells3[a] > (int64_t)1 << 24) return "every cell count must be in [1, 2^24]";
  if (cells3[0] > ((int64_t)1 << 40) / cells3[1] / cells3[2]) return "grid too large (more than 2^40 cells)";
  return nullptr;
}
inline const char* occ_grid_bad(const aon_occupancy* occ, aon::OccGrid& G) {
  if (!occ || !occ->bits) return "null occupancy grid";
  if (const char* msg = occ_cells_bad(occ->cells)) return msg;
  G.bits = occ->bits;
  for (int a = 0; a < 3; ++a) {
    if (!std::isfinite(occ->lo[a]) || !std::isfinite(occ->step[a]) || !(occ->step[a] > 0.f)) return "occupancy lo must be finite and step finite and > 0";
    G.cells[a] = occ->cells[a]; G.lo[a] = occ->lo[a]; G.step[a] = occ->step[a];
    const float span = (float)occ->cells[a] * occ->step[a];   // the last grid point: multiply, then add (ops.grid_points)
    G.hi[a] = occ->lo[a] + span;
    if (!std::isfinite(G.hi[a])) return "occupancy box not finite";
  }
  return nullptr;
}

// The call record of the whole-path forward entry points: what aon_render_fwd* / aon_art_render_fwd* /
// aon_*render_fwd_train* / aon_grender_fwd* have in common.  An exported function lists its parameters once -- that list is the ABI --
// builds the record with path_call() and passes the record on; nothing behind it takes those parameters by position again.
struct PathCall {
  const float* rays_o; const float* rays_d; const float* viewdirs; int64_t n_rays;
  float near_, far_; int white_bkgd, num_levels;
  const float* t_rand; const float* u; int64_t u_stride;
  float* rgb[2]; float* acc[2]; float* depth[2];   // per level
  void* workspace; int64_t workspace_bytes; hipStream_t stream;
  const aon_render_opts* opts;
  const aon_ray_bounds* bounds;   // per-ray near / far / live or null
};
// (the one function that takes the ABI's list: in the exported functions' order, so a call site reads as its own parameter list)
inline PathCall path_call(const float* rays_o, const float* rays_d, const float* viewdirs, int64_t n_rays, float near_, float far_, int white_bkgd,
                          int num_levels, const float* t_rand, const float* u, int64_t u_stride, float* rgb_c, float* acc_c, float* depth_c,
                          float* rgb_f, float* acc_f, float* depth_f, void* workspace, int64_t workspace_bytes, void* stream,
                          const aon_render_opts* opts, const aon_ray_bounds* bounds = nullptr) {
  return PathCall{rays_o, rays_d, viewdirs, n_rays, near_, far_, white_bkgd, num_levels, t_rand, u, u_stride, {rgb_c, rgb_f}, {acc_c, acc_f},
                  {depth_c, depth_f}, workspace, workspace_bytes, static_cast<hipStream_t>(stream), opts, bounds};
}

// The pointer / size checks every whole-path forward makes, before any launch: AON_OK, a failure code (the text carries `who`), or
// kPathEmpty for a call without rays where the entry point takes that as a successful no-op (`empty_ok`; the training forwards refuse it).
// The network handles are the caller's to check.
constexpr int kPathEmpty = 1;
inline int path_call_check(const char* who, const PathCall& c, const Geo& g, bool empty_ok) {
  auto bad = [&](const char* what) { return fail(AON_E_INVALID, (std::string(who) + ": " + what).c_str()); };
  if (c.n_rays < 0 || (c.n_rays == 0 && !empty_ok) || (c.num_levels != 1 && c.num_levels != 2)) return bad("bad size / num_levels");
  if (c.n_rays == 0) return kPathEmpty;
  if (!c.rays_o || !c.rays_d || !c.viewdirs || !c.rgb[0] || !c.acc[0] || !c.depth[0] || !c.workspace) return bad("null pointer");
  if (c.num_levels == 2 && (!c.rgb[1] || !c.acc[1] || !c.depth[1] || !c.u)) return bad("null fine-level pointer");
  if (c.num_levels == 2 && c.u_stride != 0 && c.u_stride < g.nf) return bad("bad u_stride");
  if (reinterpret_cast<uintptr_t>(c.workspace) & 255) return bad("workspace must be 256-byte aligned");
  if (c.bounds && (!c.bounds->near_ray || !c.bounds->far_ray)) return bad("null near_ray / far_ray in bounds");
  return AON_OK;
}

// What follows a level's MLP launch, for inference (render_impl) and training (train_fwd_impl) alike: the level of the n rays from r0 on,
// every pointer already at r0 (u: the call's, offset here by its stride).
struct LevelTail {
  const float* raw; const float* t; const float* d; int64_t n; int S; int64_t r0;
  int white_bkgd; bool art; const Geo& g; bool fuse;
  const float* u; int64_t u_stride;
  float* rgb; float* acc; float* depth;   // the level's outputs
  float* w_c; float* t_next;              // [coarse] its weights and the fine level's t, both null when there is no fine level
  hipStream_t stream; const char* who;
};
// level 0 (model.py:162-197): compositing, then the fine level's t by the inverse CDF -- in one kernel where `fuse` says so (the coarse
// weights stay in registers)
inline int coarse_tail(const LevelTail& a) {
  const float* uu = (a.u && a.u_stride) ? a.u + a.r0 * a.u_stride : a.u;
  if (a.fuse) {
    KTimer timer(kCompositePdf, a.stream, a.n);
    return check(aon::launch_composite_pdf(a.raw, a.t, a.d, a.n, a.white_bkgd, a.g.act(a.art, 0, a.r0), uu, a.u_stride, a.rgb, a.acc, a.depth, nullptr,
                                           a.t_next, a.stream), a.who);
  }
  {
    KTimer timer(kComposite, a.stream, a.n);
    if (int rc = check(aon::launch_composite(a.raw, 4, a.raw + 3, 4, a.t, a.d, a.n, a.S, a.white_bkgd, a.g.act(a.art, 0, a.r0), a.rgb, a.acc, a.depth,
                                             a.w_c, a.stream), a.who)) return rc;
  }
  if (!a.t_next) return AON_OK;
  KTimer timer(kSamplePdf, a.stream, a.n);
  return check(a.g.default_sizes ? aon::launch_sample_pdf(nullptr, a.w_c + 1, kSc, a.t, uu, a.u_stride, a.n, nullptr, a.t_next, a.stream)
                                 : aon::launch_sample_pdf_n(nullptr, a.w_c + 1, a.g.Sc, a.t, uu, a.u_stride, a.n, a.g.Sc - 1, a.g.nf, a.g.Sc, nullptr,
                                                            a.t_next, a.stream), a.who);
}
// level 1 (model.py:175-197): compositing
inline int fine_tail(const LevelTail& a) {
  KTimer timer(kComposite, a.stream, a.n);
  return check(aon::launch_composite(a.raw, 4, a.raw + 3, 4, a.t, a.d, a.n, a.S, a.white_bkgd, a.g.act(a.art, 1, a.r0), a.rgb, a.acc, a.depth, nullptr,
                                     a.stream), a.who);
}

// The call record of the whole-path backward entry points (aon_render_bwd* / aon_art_render_bwd* / aon_grender_bwd), as PathCall is the
// forwards': what the ABI's lists have in common around the network's own pointers.  g_rgb / g_acc / g_depth: the host arrays of per-level
// device pointers as passed (g_acc / g_depth may be null, and so may their entries).
struct BwdCall {
  const float* rays_d; int64_t n_rays; int white_bkgd, num_levels;
  const float* const* g_rgb; const float* const* g_acc; const float* const* g_depth;
  void* workspace; int64_t workspace_bytes; void* scratch; int64_t scratch_bytes; hipStream_t stream;
  const aon_render_opts* opts;
  const float* acc(int l) const { return g_acc ? g_acc[l] : nullptr; }
  const float* depth(int l) const { return g_depth ? g_depth[l] : nullptr; }
};
// (in the exported functions' order, without the network's pointers between g_depth_host and workspace)
inline BwdCall bwd_call(const float* rays_d, int64_t n_rays, int white_bkgd, int num_levels, const float* const* g_rgb_host, const float* const* g_acc_host,
                        const float* const* g_depth_host, void* workspace, int64_t workspace_bytes, void* scratch, int64_t scratch_bytes, void* stream,
                        const aon_render_opts* opts) {
  return BwdCall{rays_d, n_rays, white_bkgd, num_levels, g_rgb_host, g_acc_host, g_depth_host, workspace, workspace_bytes, scratch, scratch_bytes,
                 static_cast<hipStream_t>(stream), opts};
}

// The checks every whole-path backward makes before any launch, in their order: size / num_levels, null pointers, alignment.  Two of
// an entry point's own refusals rank among these and are handed in already judged: `site_first` (its message, or null) is reported right
// behind the size check, `site_null` (a pointer of the network's that the call needs is null) with the common null pointers.  Everything else the
// network brings (level pointers, forms, parameter and gradient arrays) and the two size refusals, which follow a carve, stay at the site.
inline int bwd_call_check(const char* who, const BwdCall& c, bool site_null = false, const char* site_first = nullptr) {
  auto bad = [&](const char* what) { return fail(AON_E_INVALID, (std::string(who) + ": " + what).c_str()); };
  if (c.n_rays <= 0 || (c.num_levels != 1 && c.num_levels != 2)) return bad("bad size / num_levels");
  if (site_first) return bad(site_first);
  if (!c.rays_d || !c.g_rgb || !c.workspace || !c.scratch || site_null) return bad("null pointer");
  if ((reinterpret_cast<uintptr_t>(c.workspace) | reinterpret_cast<uintptr_t>(c.scratch)) & 255) return bad("workspace / scratch must be 256-byte aligned");
  return AON_OK;
}

}  // namespace capi
}  // namespace aon
