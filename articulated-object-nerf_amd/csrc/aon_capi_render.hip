// extern "C" surface, whole-path inference: render_impl for both networks, occupancy-grid acceleration and early ray termination.
#include "aon_capi_util.h"

using namespace aon::capi;

namespace {

// workspace layout for a chunk of n rays
struct Ws {
  float* t_c;   // n*Sc
  float* w_c;   // n*Sc
  float* t_f;   // n*Sf
  float* raw;   // n*Sf*4 (coarse raw uses the first n*Sc*4)
  float* coords; float* enc; float* venc;   // other_degrees only: n*Sf*3, n*Sf*63, n*27
  float* vbias;   // n*128: the level's per-ray view bias (vanilla, folded form; launch_view_bias) -- both levels in turn
  char* occ;      // [occupancy] the level's sample list, tile counts and list length (aon::occ_list_bytes of n*Sf) -- both levels in turn
  char* stop;     // [early termination] the level's per-ray tau and stop index (aon::occ_stop_state_bytes of n) -- both levels in turn
  // [deferred view branch, DESIGN.md section 4.19] of a slab of `slab` rays, both levels in turn: the samples' marks, their live list
  // (aon::occ_list_bytes of slab*Sf) and the live samples' layer-7 rows (1 KiB per sample)
  int64_t slab; uint8_t* live_mark; char* live_list; float* live_rows;
  int64_t bytes;
};

// deferred view branch: what a slab of s rays adds to the workspace, and the largest slab (the rows stay at or under 8 GiB with every sample live)
int64_t defer_bytes(int64_t s, const Geo& g) {
  return s <= 0 ? 0 : align_up(s * g.Sf, 256) + aon::occ_list_bytes(s * g.Sf) + align_up(s * g.Sf * 1024, 256);
}
std::atomic<int> g_defer_slab_test{0};   // aon_test_set_deferred_slab
constexpr int64_t kDeferSlabRays = 32768, kDeferMinSlabRays = 4096;
int64_t defer_slab_cap(const Geo& g) {
  if (const int t = g_defer_slab_test.load(std::memory_order_relaxed); t > 0) return t;
  const int64_t by_rows = ((int64_t)8 << 30) / ((int64_t)g.Sf * 1024);
  return by_rows < kDeferSlabRays ? (by_rows < 1 ? 1 : by_rows) : kDeferSlabRays;
}

Ws carve(char* base, int64_t n, const Geo& g, bool occ = false, bool stop = false, int64_t slab = 0) {
  Ws w{};
  int64_t off = 0;
  w.t_c = reinterpret_cast<float*>(base + off); off += align_up(n * g.Sc * 4, 256);
  w.w_c = reinterpret_cast<float*>(base + off); off += align_up(n * g.Sc * 4, 256);
  w.t_f = reinterpret_cast<float*>(base + off); off += align_up(n * g.Sf * 4, 256);
  w.raw = reinterpret_cast<float*>(base + off); off += align_up(n * g.Sf * 16, 256);
  if (g.other_degrees) {
    w.coords = reinterpret_cast<float*>(base + off); off += align_up(n * g.Sf * 12, 256);
    w.enc = reinterpret_cast<float*>(base + off); off += align_up(n * g.Sf * (int64_t)aon::kPosEnc * 4, 256);
    w.venc = reinterpret_cast<float*>(base + off); off += align_up(n * (int64_t)aon::kViewEnc * 4, 256);
  } else {
    w.vbias = reinterpret_cast<float*>(base + off); off += align_up(n * (int64_t)aon::kCondWidth * 4, 256);
  }
  if (occ) { w.occ = base + off; off += aon::occ_list_bytes(n * g.Sf); }
  if (stop) { w.stop = base + off; off += aon::occ_stop_state_bytes(n); }
  if (slab > 0) {   // behind everything else: the plain layout does not move
    w.slab = slab;
    w.live_mark = reinterpret_cast<uint8_t*>(base + off); off += align_up(slab * g.Sf, 256);
    w.live_list = base + off; off += aon::occ_list_bytes(slab * g.Sf);
    w.live_rows = reinterpret_cast<float*>(base + off); off += align_up(slab * g.Sf * 1024, 256);
  }
  w.bytes = off;
  return w;
}

// the largest k in [lo, hi] with bytes_of(k) <= budget for a size function that does not decrease in k, or lo - 1 when not even lo fits
template <class F>
int64_t largest_fit(int64_t lo, int64_t hi, int64_t budget, F bytes_of) {
  if (hi >= lo && bytes_of(hi) <= budget) return hi;
  int64_t fit = lo - 1;   // invariant: fit fits (or is lo - 1), hi does not
  while (hi - fit > 1) {
    const int64_t mid = fit + (hi - fit) / 2;
    if (bytes_of(mid) <= budget) fit = mid; else hi = mid;
  }
  return fit;
}

}  // namespace

extern "C" {

// the workspace-size queries: one chunk of n_rays (at least one; [occupancy] at most what the int32 sample list indexes)
static int64_t workspace_query(int64_t n_rays, const aon_render_opts* opts, bool occ, bool stop) {
  Geo g;
  if (const char* bad = make_geo(opts, g)) return fail(AON_E_INVALID, bad);
  if (n_rays < 1) n_rays = 1;
  if (occ && n_rays > INT32_MAX / g.Sf) n_rays = INT32_MAX / g.Sf;
  return carve(nullptr, n_rays, g, occ, stop).bytes;
}
int64_t aon_render_workspace_bytes_ex(int64_t n_rays, const aon_render_opts* opts) { return workspace_query(n_rays, opts, false, false); }
int64_t aon_render_workspace_bytes(int64_t n_rays) { return aon_render_workspace_bytes_ex(n_rays, nullptr); }
// ... plus what the deferred view branch of the vanilla network takes (a slab's marks, list and rows): with less, aon_render_fwd* runs the
// single-kernel form
int64_t aon_render_deferred_workspace_bytes(int64_t n_rays, const aon_render_opts* opts) {
  const int64_t plain = workspace_query(n_rays, opts, false, false);
  if (plain < 0) return plain;
  Geo g;
  (void)make_geo(opts, g);
  if (g.other_degrees) return plain;
  if (n_rays < 1) n_rays = 1;
  const int64_t cap = defer_slab_cap(g);
  return plain + defer_bytes(n_rays < cap ? n_rays : cap, g);
}
int aon_test_set_deferred_slab(int rays) {
  g_defer_slab_test.store(rays > 0 ? rays : 0, std::memory_order_relaxed);
  return AON_OK;
}

// Whole-path orchestration shared by the vanilla and the articulated network (NeRF.forward, model.py:147-199;
// NeRF_AE_Art.forward, model_autodecoder.py:278-337): only the MLP launch and the output activation differ.

struct NetRef {
  bool articulated;
  const void* packed;
  const float* small;  // articulated only
};
struct Nets { NetRef c, f; };   // coarse, fine
static Nets vanilla_nets(const void* packed_coarse, const void* packed_fine) {
  return {{false, packed_coarse, nullptr}, {false, packed_fine, nullptr}};
}
static Nets art_nets(const void* packed_coarse, const void* small_coarse, const void* packed_fine, const void* small_fine) {
  return {{true, packed_coarse, static_cast<const float*>(small_coarse)}, {true, packed_fine, static_cast<const float*>(small_fine)}};
}

// An occupancy grid handed to aon_render_fwd_occ / aon_art_render_fwd_occ: the kernels' view of it, and the
// caller's per-level tally of samples run through the MLP (or null)
// [early termination, DESIGN.md section 4.10] rounds: the level runs front to back in rounds of R samples and a ray stops once its optical
// depth reaches tau_stop; grid.bits may then be null (no grid: every live sample is listed).  stop_dev: the caller's (n_rays, 2) map or null
struct OccCtx {
  aon::OccGrid grid;
  int64_t* tally;
  bool rounds;
  float tau_stop;
  int R;
  int32_t* stop_dev;
};

// One level of a chunk of rays through the MLP: the network, the chunk's rays and the level's t, where the records go, and what the call
// brings along (geometry, workspace, occupancy).
struct LevelRun {
  const NetRef& net;
  const float* o; const float* d; const float* v; const float* t;
  int64_t n; int S; float* raw; int level; const uint8_t* live; hipStream_t stream;
  const Geo& g; const Ws& w; const OccCtx* occ;
};
// the whole level as one forward segment on the in-kernel encodings; the forms below add what is theirs
static aon::FwdSeg level_seg(const LevelRun& r, const float* vbias) {
  return aon::FwdSeg{.packed = static_cast<const char*>(r.net.packed), .small = r.net.small, .rays_o = r.o, .rays_d = r.d, .viewdirs = r.v, .t_vals = r.t,
                     .n_rays = r.n, .S = r.S, .raw = r.raw, .view_bias = vbias};
}

// NeRF(min_deg_point, max_deg_point, deg_view) with at most 10 / 4 levels: the encodings are computed by the stage kernels in the fused
// kernel's 63 / 27-slot layout (zeros in the missing levels' slots, matched by zero weights in the packed stream, aon_pack_vanilla_mlp_deg)
// and the MLP runs as NeRFMLP.forward(x, condition) on them: 252 B/sample of extra HBM traffic against 1.19 MFLOP/sample
static hipError_t run_other_degrees(const LevelRun& r) {
  if (hipError_t e = aon::launch_cast_rays(r.t, r.o, r.d, r.n, r.S, r.w.coords, r.stream); e != hipSuccess) return e;
  if (hipError_t e = aon::launch_pos_enc(r.w.coords, r.n * r.S, r.g.min_deg, r.g.max_deg, r.w.enc, r.stream, aon::kPosEnc, 10); e != hipSuccess) return e;
  if (hipError_t e = aon::launch_pos_enc(r.v, r.n, 0, r.g.deg_view, r.w.venc, r.stream, aon::kViewEnc, 4); e != hipSuccess) return e;
  MlpTimer timer(r.stream, r.n * r.S);
  const aon::FwdSeg seg{.packed = static_cast<const char*>(r.net.packed), .n_rays = r.n, .S = r.S, .raw = r.raw, .samples_enc = r.w.enc, .viewdirs_enc = r.w.venc};
  return aon::launch_net_fwd(false, &seg, 1, r.stream);
}

// occ: mark the level's samples, compact the occupied ones into a list (aon_occ.hip) and run the MLP on that list alone (the GATHER
// instances); the empty samples' records hold the zero-density sentinel.  Same view bias, same kernel arithmetic per sample.
// The compaction of the level's samples [s0, s1) of every ray: one segment, the buffers laid out for the whole level -> the list in `seg`
static hipError_t compact_level(const LevelRun& r, int s0, int s1, const int* stop, aon::FwdSeg& seg) {
  const int64_t starts[2] = {0, r.n};
  const aon::OccCompact c{&r.occ->grid, starts, 1, r.S, s0, s1, r.o, r.d, r.t, r.live, stop};
  return aon::launch_occ_compact(c, r.raw, r.w.occ, (r.n * r.S + 1023) / 1024, r.occ->tally ? r.occ->tally + r.level : nullptr, &seg.gather_idx,
                                 &seg.gather_count, r.stream);
}
// [early termination] per round: mark -> scan -> emit -> the GATHER launch on the round's list -> the live rays' optical depth; all stream-ordered
static hipError_t run_rounds(const LevelRun& r, const float* vbias) {
  if (hipError_t e = aon::launch_occ_stop_init(r.w.stop, r.n, r.S, r.stream); e != hipSuccess) return e;
  const int R = r.occ->R < r.S ? r.occ->R : r.S;
  const aon::ActParams ap = r.g.act(r.net.articulated, r.level, 0);   // (no noise on this path)
  aon::FwdSeg seg = level_seg(r, vbias);
  for (int s0 = 0; s0 < r.S; s0 += R) {
    const int s1 = s0 + R < r.S ? s0 + R : r.S;
    if (hipError_t e = compact_level(r, s0, s1, aon::occ_stop_state(r.w.stop, r.n).stop, seg); e != hipSuccess) return e;
    {
      MlpTimer timer(r.stream, r.n * (s1 - s0));
      seg.max_listed = r.n * (s1 - s0);
      if (hipError_t e = aon::launch_net_fwd(r.net.articulated, &seg, 1, r.stream); e != hipSuccess) return e;
    }
    if (s1 < r.S)   // the last round (sample S-1 and its 1e10 interval) decides nothing
      if (hipError_t e = aon::launch_occ_depth(r.raw, r.t, r.d, r.n, r.S, s0, s1, ap, r.occ->tau_stop, r.w.stop, r.stream); e != hipSuccess) return e;
  }
  return hipSuccess;
}
static hipError_t run_listed(const LevelRun& r, const float* vbias) {
  aon::FwdSeg seg = level_seg(r, vbias);
  if (hipError_t e = compact_level(r, 0, r.S, nullptr, seg); e != hipSuccess) return e;
  MlpTimer timer(r.stream, r.n * r.S);
  return aon::launch_net_fwd(r.net.articulated, &seg, 1, r.stream);
}
// [deferred view branch] per slab of rays: the trunk, the compaction of its marks (one "row" per sample, the mark as its ray_live byte,
// no grid: the list holds the slab's live sample indices) and the view branch of the listed samples; all stream-ordered.
static hipError_t run_deferred(const LevelRun& r, const float* vbias) {
  MlpTimer timer(r.stream, r.n * r.S);
  const char* packed = static_cast<const char*>(r.net.packed);
  const int S = r.S;
  for (int64_t r0 = 0; r0 < r.n; r0 += r.w.slab) {
    const int64_t ns = r.n - r0 < r.w.slab ? r.n - r0 : r.w.slab;
    float* raw_s = r.raw + r0 * S * 4;
    const float* vb_s = vbias + r0 * aon::kCondWidth;
    const aon::FwdSeg trunk{.packed = packed, .rays_o = r.o + r0 * 3, .rays_d = r.d + r0 * 3, .viewdirs = r.v + r0 * 3, .t_vals = r.t + r0 * S, .n_rays = ns,
                            .S = S, .raw = raw_s, .view_bias = vb_s, .live_mark = r.w.live_mark, .live_rows = r.w.live_rows};
    if (hipError_t e = aon::launch_net_fwd(false, &trunk, 1, r.stream); e != hipSuccess) return e;
    const int64_t starts[2] = {0, ns * S};
    const aon::OccGrid no_grid{};
    const aon::OccCompact c{&no_grid, starts, 1, 1, 0, 1, nullptr, nullptr, nullptr, r.w.live_mark, nullptr};
    const int* live_idx = nullptr;
    const int64_t* live_count = nullptr;
    if (hipError_t e = aon::launch_occ_compact(c, nullptr, r.w.live_list, (ns * S + 1023) / 1024, nullptr, &live_idx, &live_count, r.stream); e != hipSuccess) return e;
    if (hipError_t e = aon::launch_view_deferred(packed, r.w.live_rows, live_idx, live_count, ns * S, vb_s, S, raw_s, r.stream); e != hipSuccess) return e;
  }
  return hipSuccess;
}
static hipError_t run_dense(const LevelRun& r, const float* vbias) {
  MlpTimer timer(r.stream, r.n * r.S);
  const aon::FwdSeg seg = level_seg(r, vbias);
  return aon::launch_net_fwd(r.net.articulated, &seg, 1, r.stream);
}

// The form of a level, in order of precedence: other degrees, rounds, listed, deferred, dense.  The per-ray view bias of the folded form is
// computed once, here.  Density noise can lift a sample with raw sigma <= 0 above zero: such a level keeps the single kernel.
static hipError_t launch_net(const LevelRun& r) {
  if (r.g.other_degrees) return run_other_degrees(r);
  const float* vbias = nullptr;
  if (r.w.vbias && g_view_bias.load(std::memory_order_relaxed) != 0 && aon::stream_form(r.net.packed) == aon::kFormFolded) {
    if (hipError_t e = aon::launch_net_view_bias(r.net.articulated, static_cast<const char*>(r.net.packed), r.net.small, r.v, r.n, r.w.vbias, r.stream);
        e != hipSuccess) return e;
    vbias = r.w.vbias;
  }
  if (r.occ) return r.occ->rounds ? run_rounds(r, vbias) : run_listed(r, vbias);
  const bool noisy = r.g.noise[r.level] && r.g.noise_std > 0.f;
  if (!r.net.articulated && r.w.slab > 0 && vbias && !noisy) return run_deferred(r, vbias);
  return run_dense(r, vbias);
}

static int render_impl(const char* who, const NetRef& coarse, const NetRef& fine, const PathCall& c, const OccCtx* occ = nullptr) {
  Geo g;
  if (const char* bad = make_geo(c.opts, g)) return fail(AON_E_INVALID, bad);
  if (int rc = path_call_check(who, c, g, true)) return rc == kPathEmpty ? AON_OK : rc;
  const int64_t n_rays = c.n_rays;
  const int num_levels = c.num_levels;
  const hipStream_t stream = c.stream;
  auto bad = [&](const char* what) { return fail(AON_E_INVALID, (std::string(who) + ": " + what).c_str()); };
  if (!coarse.packed || (num_levels == 2 && !fine.packed)) return bad("null pointer");
  if (coarse.articulated && (!coarse.small || (num_levels == 2 && !fine.small))) return bad("null latent block");
  if (coarse.articulated && (forms_differ(coarse.packed, coarse.small) || (num_levels == 2 && forms_differ(fine.packed, fine.small)))) return fail(AON_E_INVALID, kFormsMsg);
  const bool art = coarse.articulated;
  if (art) g.other_degrees = false;   // the articulated kernels carry their degrees in the packed stream and the small block (aon_*_deg)
  const bool fuse_coarse = num_levels == 2 && g.default_sizes && g_fuse_coarse.load(std::memory_order_relaxed) != 0;
  const bool with_occ = occ != nullptr;
  const bool with_stop = with_occ && occ->rounds;

  // largest chunk the workspace admits ([occupancy] and whose sample indices fit the int32 list)
  const int64_t chunk = largest_fit(1, with_occ && n_rays > INT32_MAX / g.Sf ? INT32_MAX / g.Sf : n_rays, c.workspace_bytes,
                                    [&](int64_t k) { return carve(nullptr, k, g, with_occ, with_stop).bytes; });
  if (chunk < 1) return fail(AON_E_WORKSPACE, with_stop ? "render: workspace smaller than aon_render_stop_workspace_bytes(1)"
                                              : with_occ ? "render: workspace smaller than aon_render_occ_workspace_bytes(1)"
                                                       : "render: workspace smaller than aon_render_workspace_bytes(1)");
  // [deferred view branch] the dense renders of the vanilla network on the fused encodings, when the switch is on and the workspace holds a
  // slab's marks, list and rows behind the plain layout (aon_render_deferred_workspace_bytes): the largest slab that fits, up to the cap
  int64_t slab = 0;
  if (!art && !with_occ && !g.other_degrees && g_deferred_view.load(std::memory_order_relaxed) != 0) {
    const int64_t s = largest_fit(1, defer_slab_cap(g) < chunk ? defer_slab_cap(g) : chunk, c.workspace_bytes - carve(nullptr, chunk, g).bytes,
                                  [&](int64_t k) { return defer_bytes(k, g); });
    const bool hook = g_defer_slab_test.load(std::memory_order_relaxed) > 0;
    if (s > 0 && (hook || s >= kDeferMinSlabRays || s >= chunk)) slab = s;
  }
  const Ws w = carve(static_cast<char*>(c.workspace), chunk, g, with_occ, with_stop, slab);
  if (with_occ && occ->tally) {
    if (int rc = check(hipMemsetAsync(occ->tally, 0, 2 * sizeof(int64_t), stream), who); rc != AON_OK) return rc;
  }

  for (int64_t r0 = 0; r0 < n_rays; r0 += chunk) {
    const int64_t n = n_rays - r0 < chunk ? n_rays - r0 : chunk;
    const float* o = c.rays_o + r0 * 3;
    const float* d = c.rays_d + r0 * 3;
    const float* v = c.viewdirs + r0 * 3;
    // [per-ray bounds, DESIGN.md section 4.11] the chunk's near / far / live
    const float* near_ray = c.bounds ? c.bounds->near_ray + r0 : nullptr;
    const float* far_ray = c.bounds ? c.bounds->far_ray + r0 : nullptr;
    const uint8_t* live = c.bounds && c.bounds->live ? c.bounds->live + r0 : nullptr;
    int rc;
    // level 0 (model.py:150-160, :175-197)
    {
      KTimer timer(kSampleT, stream, n);
      rc = check(aon::launch_sample_along_rays(o, d, n, g.Sc, c.near_, c.far_, c.t_rand ? c.t_rand + r0 * g.Sc : nullptr, w.t_c, nullptr, stream,
                                               g.lindisp, g.inv_near, g.inv_far, near_ray, far_ray), who);
    }
    if (rc) return rc;
    rc = check(launch_net(LevelRun{coarse, o, d, v, w.t_c, n, g.Sc, w.raw, 0, live, stream, g, w, occ}), who);
    if (rc) return rc;
    if (with_stop && occ->stop_dev) {
      rc = check(aon::launch_occ_stop_store(w.stop, 0, occ->stop_dev + r0 * 2, n, 2, stream), who);
      if (rc) return rc;
    }
    const bool two = num_levels == 2;
    rc = coarse_tail(LevelTail{w.raw, w.t_c, d, n, g.Sc, r0, c.white_bkgd, art, g, fuse_coarse, c.u, c.u_stride, c.rgb[0] + r0 * 3, c.acc[0] + r0,
                               c.depth[0] + r0, two ? w.w_c : nullptr, two ? w.t_f : nullptr, stream, who});
    if (rc) return rc;
    if (!two) continue;
    // level 1 (model.py:162-173, :175-197)
    rc = check(launch_net(LevelRun{fine, o, d, v, w.t_f, n, g.Sf, w.raw, 1, live, stream, g, w, occ}), who);
    if (rc) return rc;
    if (with_stop && occ->stop_dev) {
      rc = check(aon::launch_occ_stop_store(w.stop, 0, occ->stop_dev + r0 * 2 + 1, n, 2, stream), who);
      if (rc) return rc;
    }
    rc = fine_tail(LevelTail{w.raw, w.t_f, d, n, g.Sf, r0, c.white_bkgd, art, g, false, nullptr, 0, c.rgb[1] + r0 * 3, c.acc[1] + r0, c.depth[1] + r0,
                             nullptr, nullptr, stream, who});
    if (rc) return rc;
  }
  return AON_OK;
}

// ---- occupancy-grid accelerated inference (aon_occ.hip) ----
int64_t aon_occupancy_bytes(const int64_t* cells3_host) {
  if (const char* msg = occ_cells_bad(cells3_host)) return fail(AON_E_INVALID, (std::string("aon_occupancy_bytes: ") + msg).c_str());
  return (cells3_host[0] * cells3_host[1] * cells3_host[2] + 31) / 32 * 4;
}
int aon_occupancy_build(const float* density, const int64_t* dims3_host, float threshold, int dilate, uint32_t* bits, void* stream) {
  if (!dims3_host) return fail(AON_E_INVALID, "aon_occupancy_build: null dims");
  const int64_t cells[3] = {dims3_host[0] - 1, dims3_host[1] - 1, dims3_host[2] - 1};
  if (const char* msg = occ_cells_bad(cells)) return fail(AON_E_INVALID, (std::string("aon_occupancy_build: every dimension must be >= 2; ") + msg).c_str());
  if (dilate < 0 || dilate > 8) return fail(AON_E_INVALID, "aon_occupancy_build: dilate must be in [0, 8]");
  if (threshold != threshold) return fail(AON_E_INVALID, "aon_occupancy_build: threshold is NaN");
  if (!density || !bits) return fail(AON_E_INVALID, "aon_occupancy_build: null pointer");
  return check(aon::launch_occ_build(density, dims3_host, threshold, dilate, bits, (hipStream_t)stream), "aon_occupancy_build");
}
// the inference-only limits of the occupancy path, checked before any launch
static const char* occ_opts_bad(const aon_render_opts* opts, bool art, const float* t_rand) {
  Geo g;
  if (const char* bad = make_geo(opts, g)) return bad;
  if (t_rand) return "occupancy rendering is inference only: t_rand (randomized sampling) is refused";
  if (g.noise_std > 0.f && (g.noise[0] || g.noise[1])) return "occupancy rendering is inference only: density noise is refused";
  if (!art && g.other_degrees) return "occupancy rendering needs the default encoding degrees (0, 10, 4) of the vanilla network";
  return nullptr;
}
int64_t aon_render_occ_workspace_bytes(int64_t n_rays, const aon_render_opts* opts) { return workspace_query(n_rays, opts, true, false); }

// ---- early ray termination on the occupancy renders ----
int64_t aon_render_stop_workspace_bytes(int64_t n_rays, const aon_render_opts* opts) { return workspace_query(n_rays, opts, true, true); }

// The checks and the eps == 0 route shared by the _occ, _stop and _bounds forms of both networks.  need_grid: the _occ forms, which have no
// eps / round_samples arguments (they pass 0 / 1) and refuse a null grid.
static int render_stop(const char* who, const Nets& nets, const PathCall& c, const aon_occupancy* occ, int64_t* occupied_dev, float eps,
                       int round_samples, int32_t* stop_dev, bool need_grid = false) {
  auto bad = [&](const char* what) { return fail(AON_E_INVALID, (std::string(who) + ": " + what).c_str()); };
  const aon_ray_bounds* bounds = c.bounds;
  OccCtx ctx{};
  if (bounds && bounds->live && c.t_rand) return bad("ray_live is inference only: t_rand (randomized sampling) is refused");
  if (occ || need_grid)
    if (const char* msg = occ_grid_bad(occ, ctx.grid)) return bad(msg);
  // the compaction path (mark / scan / emit and the GATHER launches): a grid, early termination or a ray mask
  const bool compact = occ || (bounds && bounds->live) || eps != 0.f;
  // (bounds alone: aon_render_fwd_ex with per-ray planes, and that call's rules -- t_rand, noise and other degrees are its to take)
  if (!bounds || compact)
    if (const char* msg = occ_opts_bad(c.opts, nets.c.articulated, c.t_rand)) return bad(msg);
  if (!(eps >= 0.f && eps < 1.f)) return bad("eps must be in [0, 1)");
  if (round_samples < 1) return bad("round_samples must be >= 1");
  ctx.tally = occupied_dev;
  if (eps == 0.f) {   // off: today's single-launch paths, and the bookkeeping of a render in which no ray stopped
    const int rc = render_impl(who, nets.c, nets.f, c, compact ? &ctx : nullptr);
    if (rc != AON_OK || c.n_rays == 0) return rc;
    Geo g;
    (void)make_geo(c.opts, g);
    if (!compact && occupied_dev)
      if (int r2 = check(aon::launch_occ_tally_set(occupied_dev, c.n_rays * g.Sc, c.num_levels == 2 ? c.n_rays * g.Sf : 0, c.stream), who); r2 != AON_OK) return r2;
    if (stop_dev)
      for (int l = 0; l < c.num_levels; ++l)
        if (int r2 = check(aon::launch_occ_stop_store(nullptr, g.S(l), stop_dev + l, c.n_rays, 2, c.stream), who); r2 != AON_OK) return r2;
    return AON_OK;
  }
  ctx.rounds = true;
  ctx.tau_stop = (float)(-std::log((double)eps));   // fp64, rounded once
  ctx.R = round_samples;
  ctx.stop_dev = stop_dev;
  return render_impl(who, nets.c, nets.f, c, &ctx);
}

// ---- the exported whole-path forwards: each lists its parameters once (the ABI) and builds the call record ----
int aon_render_fwd_ex(const void* packed_coarse, const void* packed_fine, const float* rays_o, const float* rays_d,
                      const float* viewdirs, int64_t n_rays, float near_, float far_, int white_bkgd, int num_levels,
                      const float* t_rand, const float* u, int64_t u_stride, float* rgb_c, float* acc_c, float* depth_c,
                      float* rgb_f, float* acc_f, float* depth_f, void* workspace, int64_t workspace_bytes, void* stream,
                      const aon_render_opts* opts) {
  const Nets nets = vanilla_nets(packed_coarse, packed_fine);
  return render_impl("aon_render_fwd", nets.c, nets.f,
                     path_call(rays_o, rays_d, viewdirs, n_rays, near_, far_, white_bkgd, num_levels, t_rand, u, u_stride, rgb_c, acc_c, depth_c, rgb_f,
                               acc_f, depth_f, workspace, workspace_bytes, stream, opts));
}
int aon_render_fwd(const void* packed_coarse, const void* packed_fine, const float* rays_o, const float* rays_d,
                   const float* viewdirs, int64_t n_rays, float near_, float far_, int white_bkgd, int num_levels,
                   const float* t_rand, const float* u, int64_t u_stride, float* rgb_c, float* acc_c, float* depth_c,
                   float* rgb_f, float* acc_f, float* depth_f, void* workspace, int64_t workspace_bytes, void* stream) {
  return aon_render_fwd_ex(packed_coarse, packed_fine, rays_o, rays_d, viewdirs, n_rays, near_, far_, white_bkgd, num_levels, t_rand, u,
                           u_stride, rgb_c, acc_c, depth_c, rgb_f, acc_f, depth_f, workspace, workspace_bytes, stream, nullptr);
}
int aon_render_fwd_occ(const void* packed_coarse, const void* packed_fine, const float* rays_o, const float* rays_d,
                       const float* viewdirs, int64_t n_rays, float near_, float far_, int white_bkgd, int num_levels,
                       const float* t_rand, const float* u, int64_t u_stride, float* rgb_c, float* acc_c, float* depth_c,
                       float* rgb_f, float* acc_f, float* depth_f, void* workspace, int64_t workspace_bytes, void* stream,
                       const aon_render_opts* opts, const aon_occupancy* occ, int64_t* occupied_dev) {
  return render_stop("aon_render_fwd_occ", vanilla_nets(packed_coarse, packed_fine),
                     path_call(rays_o, rays_d, viewdirs, n_rays, near_, far_, white_bkgd, num_levels, t_rand, u, u_stride, rgb_c, acc_c, depth_c, rgb_f,
                               acc_f, depth_f, workspace, workspace_bytes, stream, opts),
                     occ, occupied_dev, 0.f, 1, nullptr, true);
}
int aon_render_fwd_stop(const void* packed_coarse, const void* packed_fine, const float* rays_o, const float* rays_d,
                        const float* viewdirs, int64_t n_rays, float near_, float far_, int white_bkgd, int num_levels,
                        const float* t_rand, const float* u, int64_t u_stride, float* rgb_c, float* acc_c, float* depth_c,
                        float* rgb_f, float* acc_f, float* depth_f, void* workspace, int64_t workspace_bytes, void* stream,
                        const aon_render_opts* opts, const aon_occupancy* occ, int64_t* occupied_dev, float eps, int round_samples,
                        int32_t* stop_dev) {
  return render_stop("aon_render_fwd_stop", vanilla_nets(packed_coarse, packed_fine),
                     path_call(rays_o, rays_d, viewdirs, n_rays, near_, far_, white_bkgd, num_levels, t_rand, u, u_stride, rgb_c, acc_c, depth_c, rgb_f,
                               acc_f, depth_f, workspace, workspace_bytes, stream, opts),
                     occ, occupied_dev, eps, round_samples, stop_dev);
}
// per-ray near / far (NeRF.forward / NeRF_AE_Art.forward called with the (N, 1) tensors of helper.get_ray_limits,
// model.py:147-160, model_autodecoder.py:278-291); bounds == NULL is the _stop call
int aon_render_fwd_bounds(const void* packed_coarse, const void* packed_fine, const float* rays_o, const float* rays_d,
                          const float* viewdirs, int64_t n_rays, float near_, float far_, int white_bkgd, int num_levels,
                          const float* t_rand, const float* u, int64_t u_stride, float* rgb_c, float* acc_c, float* depth_c,
                          float* rgb_f, float* acc_f, float* depth_f, void* workspace, int64_t workspace_bytes, void* stream,
                          const aon_render_opts* opts, const aon_occupancy* occ, int64_t* occupied_dev, float eps, int round_samples,
                          int32_t* stop_dev, const aon_ray_bounds* bounds) {
  return render_stop(bounds ? "aon_render_fwd_bounds" : "aon_render_fwd_stop", vanilla_nets(packed_coarse, packed_fine),
                     path_call(rays_o, rays_d, viewdirs, n_rays, near_, far_, white_bkgd, num_levels, t_rand, u, u_stride, rgb_c, acc_c, depth_c, rgb_f,
                               acc_f, depth_f, workspace, workspace_bytes, stream, opts, bounds),
                     occ, occupied_dev, eps, round_samples, stop_dev);
}

int aon_art_render_fwd_ex(const void* packed_coarse, const void* small_coarse, const void* packed_fine, const void* small_fine,
                          const float* rays_o, const float* rays_d, const float* viewdirs, int64_t n_rays, float near_, float far_,
                          int white_bkgd, int num_levels, const float* t_rand, const float* u, int64_t u_stride, float* rgb_c,
                          float* acc_c, float* depth_c, float* rgb_f, float* acc_f, float* depth_f, void* workspace,
                          int64_t workspace_bytes, void* stream, const aon_render_opts* opts) {
  const Nets nets = art_nets(packed_coarse, small_coarse, packed_fine, small_fine);
  return render_impl("aon_art_render_fwd", nets.c, nets.f,
                     path_call(rays_o, rays_d, viewdirs, n_rays, near_, far_, white_bkgd, num_levels, t_rand, u, u_stride, rgb_c, acc_c, depth_c, rgb_f,
                               acc_f, depth_f, workspace, workspace_bytes, stream, opts));
}
int aon_art_render_fwd(const void* packed_coarse, const void* small_coarse, const void* packed_fine, const void* small_fine,
                       const float* rays_o, const float* rays_d, const float* viewdirs, int64_t n_rays, float near_, float far_,
                       int white_bkgd, int num_levels, const float* t_rand, const float* u, int64_t u_stride, float* rgb_c,
                       float* acc_c, float* depth_c, float* rgb_f, float* acc_f, float* depth_f, void* workspace,
                       int64_t workspace_bytes, void* stream) {
  return aon_art_render_fwd_ex(packed_coarse, small_coarse, packed_fine, small_fine, rays_o, rays_d, viewdirs, n_rays, near_, far_, white_bkgd,
                               num_levels, t_rand, u, u_stride, rgb_c, acc_c, depth_c, rgb_f, acc_f, depth_f, workspace, workspace_bytes, stream,
                               nullptr);
}
int aon_art_render_fwd_occ(const void* packed_coarse, const void* small_coarse, const void* packed_fine, const void* small_fine,
                           const float* rays_o, const float* rays_d, const float* viewdirs, int64_t n_rays, float near_, float far_,
                           int white_bkgd, int num_levels, const float* t_rand, const float* u, int64_t u_stride, float* rgb_c,
                           float* acc_c, float* depth_c, float* rgb_f, float* acc_f, float* depth_f, void* workspace,
                           int64_t workspace_bytes, void* stream, const aon_render_opts* opts, const aon_occupancy* occ,
                           int64_t* occupied_dev) {
  return render_stop("aon_art_render_fwd_occ", art_nets(packed_coarse, small_coarse, packed_fine, small_fine),
                     path_call(rays_o, rays_d, viewdirs, n_rays, near_, far_, white_bkgd, num_levels, t_rand, u, u_stride, rgb_c, acc_c, depth_c, rgb_f,
                               acc_f, depth_f, workspace, workspace_bytes, stream, opts),
                     occ, occupied_dev, 0.f, 1, nullptr, true);
}
int aon_art_render_fwd_stop(const void* packed_coarse, const void* small_coarse, const void* packed_fine, const void* small_fine,
                            const float* rays_o, const float* rays_d, const float* viewdirs, int64_t n_rays, float near_, float far_,
                            int white_bkgd, int num_levels, const float* t_rand, const float* u, int64_t u_stride, float* rgb_c,
                            float* acc_c, float* depth_c, float* rgb_f, float* acc_f, float* depth_f, void* workspace,
                            int64_t workspace_bytes, void* stream, const aon_render_opts* opts, const aon_occupancy* occ,
                            int64_t* occupied_dev, float eps, int round_samples, int32_t* stop_dev) {
  return render_stop("aon_art_render_fwd_stop", art_nets(packed_coarse, small_coarse, packed_fine, small_fine),
                     path_call(rays_o, rays_d, viewdirs, n_rays, near_, far_, white_bkgd, num_levels, t_rand, u, u_stride, rgb_c, acc_c, depth_c, rgb_f,
                               acc_f, depth_f, workspace, workspace_bytes, stream, opts),
                     occ, occupied_dev, eps, round_samples, stop_dev);
}
int aon_art_render_fwd_bounds(const void* packed_coarse, const void* small_coarse, const void* packed_fine, const void* small_fine,
                              const float* rays_o, const float* rays_d, const float* viewdirs, int64_t n_rays, float near_, float far_,
                              int white_bkgd, int num_levels, const float* t_rand, const float* u, int64_t u_stride, float* rgb_c,
                              float* acc_c, float* depth_c, float* rgb_f, float* acc_f, float* depth_f, void* workspace,
                              int64_t workspace_bytes, void* stream, const aon_render_opts* opts, const aon_occupancy* occ,
                              int64_t* occupied_dev, float eps, int round_samples, int32_t* stop_dev, const aon_ray_bounds* bounds) {
  return render_stop(bounds ? "aon_art_render_fwd_bounds" : "aon_art_render_fwd_stop", art_nets(packed_coarse, small_coarse, packed_fine, small_fine),
                     path_call(rays_o, rays_d, viewdirs, n_rays, near_, far_, white_bkgd, num_levels, t_rand, u, u_stride, rgb_c, acc_c, depth_c, rgb_f,
                               acc_f, depth_f, workspace, workspace_bytes, stream, opts, bounds),
                     occ, occupied_dev, eps, round_samples, stop_dev);
}

}  // extern "C"
