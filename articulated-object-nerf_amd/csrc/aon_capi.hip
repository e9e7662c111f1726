// extern "C" surface of libaon_hip.so (declared in include/aon_hip.h): errors, version, profiler, the stage entry points, the packs and the
// optimiser / metrics / mesh wrappers.  The whole-path renders are in aon_capi_render.hip, the training step in aon_capi_train.hip, the
// layer-wise engine's entry points in aon_capi_gmlp.hip; aon_capi_util.h is what the four share, and its state is defined here.
#include "aon_capi_util.h"

namespace aon {
namespace capi __attribute__((visibility("hidden"))) {

thread_local char g_err[256] = "";

int fail(int code, const char* msg) {
  std::snprintf(g_err, sizeof(g_err), "%s", msg);
  return code;
}

int check(hipError_t e, const char* where) {
  if (e == hipSuccess) return AON_OK;
  std::snprintf(g_err, sizeof(g_err), "%s: %s", where, hipGetErrorString(e));
  return AON_E_HIP_BASE - (int)e;
}

const char* const kFormsMsg = "two of the packed buffers of this call were made in different forms (aon_set_bottleneck_fold changed between the pack / prepare calls), "
                              "or one of them was never packed or declared by this process (a copy: aon_declare_stream_form)";
const char* const kNullBwdMsg = "packed_bwd is NULL (= literal planes) while the process default is the folded form: pass the transposed stream the chain ran with";

Profiler g_prof;

// The coarse level's compositing and the fine level's sampling as ONE kernel (model.py:160-173): the whole-path entry points
// use it; aon_set_coarse_fusion(0) puts them back on the two stage kernels (A/B measurements, equality tests).
std::atomic<int> g_fuse_coarse{1};
// Round 5: whole-path calls of the vanilla network in its folded form hand the view layer b' + W_v0[:, 256:] ve as a per-ray bias
// (launch_view_bias) instead of running the view-encoding chunk per sample -- same bits (aon_common.h).  0: the chunk form.
std::atomic<int> g_view_bias{1};
// Whole-path dense renders of the vanilla network (folded form, per-ray view bias): the view branch runs only on the samples with raw
// sigma > 0, behind a compaction -- same bits: the others' colours are multiplied by a weight of exactly 0.
// 0: the single kernel.
std::atomic<int> g_deferred_view{1};

const char* make_geo(const aon_render_opts* o, Geo& g, bool general_engine) {
  aon_render_opts d;
  aon_render_opts_init(&d);
  if (o) d = *o;
  if (d.num_coarse_samples < 2 || d.num_coarse_samples > 1023) return "num_coarse_samples must be in [2, 1023]";
  if (d.num_fine_samples < 1) return "num_fine_samples must be >= 1";
  g.Sc = d.num_coarse_samples + 1; g.nf = d.num_fine_samples; g.Sf = g.Sc + g.nf;
  g.default_sizes = g.Sc == kSc && g.Sf == kSf;
  if (!g.default_sizes && aon::sample_pdf_n_lds_bytes(g.Sc - 1, g.nf, g.Sc, nullptr) > 64 * 1024) return "num_coarse_samples / num_fine_samples too large for the per-ray LDS image";
  g.lindisp = d.lindisp != 0; g.inv_near = d.inv_near; g.inv_far = d.inv_far;
  g.noise[0] = d.noise_c; g.noise[1] = d.noise_f; g.noise_std = d.noise_std;
  g.rgb_scale = d.rgb_scale; g.rgb_shift = d.rgb_shift; g.sigma_bias = d.sigma_bias;
  g.min_deg = d.min_deg_point; g.max_deg = d.max_deg_point; g.deg_view = d.deg_view;
  if (general_engine) { g.min_deg = 0; g.max_deg = 10; g.deg_view = 4; g.other_degrees = false; return nullptr; }   // (its rule: make_gg)
  if (g.min_deg < -32 || g.max_deg > 32) return "min_deg_point / max_deg_point must lie in [-32, 32]";
  if (g.max_deg < g.min_deg || g.max_deg - g.min_deg > 10 || g.deg_view < 0 || g.deg_view > 4)
    return "the fused kernels hold up to 10 position and 4 view frequency levels (other degrees: aon_grender_*)";
  g.other_degrees = !(g.min_deg == 0 && g.max_deg == 10 && g.deg_view == 4);
  return nullptr;
}

}  // namespace capi
}  // namespace aon

using namespace aon::capi;

extern "C" {

int aon_abi_version(void) { return AON_ABI_VERSION; }

const char* aon_last_error(void) { return g_err; }

int aon_raygen(const float* c2w_host, int H, int W, float focal, int64_t pix_begin, int64_t pix_end, float* rays_o,
               float* viewdirs, float* rays_d, void* stream) {
  if (!c2w_host || !rays_o || !viewdirs) return fail(AON_E_INVALID, "aon_raygen: null pointer");
  if (H <= 0 || W <= 0 || !(focal > 0.f) || pix_begin < 0 || pix_end < pix_begin || pix_end > (int64_t)H * W)
    return fail(AON_E_INVALID, "aon_raygen: bad geometry");
  return check(aon::launch_raygen(c2w_host, H, W, focal, nullptr, pix_begin, pix_end, rays_o, viewdirs, rays_d,
                                  (hipStream_t)stream), "aon_raygen");
}

int aon_train_loss_fwd(const float* rgb_coarse, const float* rgb_fine, const float* target, int64_t n, const float* const* latents_host, const int* latent_len_host,
                       float reg_scale, float* stats, float* loss, void* stream) {
  if (!rgb_fine || !target || !stats || !loss) return fail(AON_E_INVALID, "aon_train_loss_fwd: null pointer");
  if (n <= 0) return fail(AON_E_INVALID, "aon_train_loss_fwd: bad size");
  for (int k = 0; k < 3 && latents_host; ++k)
    if (latents_host[k] && (!latent_len_host || latent_len_host[k] <= 0)) return fail(AON_E_INVALID, "aon_train_loss_fwd: bad latent length");
  return check(aon::launch_train_loss(false, rgb_coarse, rgb_fine, target, n, latents_host, latent_len_host, reg_scale, stats, loss, nullptr, nullptr, nullptr, nullptr,
                                      (hipStream_t)stream), "aon_train_loss_fwd");
}

int aon_train_loss_bwd(const float* rgb_coarse, const float* rgb_fine, const float* target, int64_t n, const float* const* latents_host, const int* latent_len_host,
                       float reg_scale, const float* grad_loss, float* d_rgb_coarse, float* d_rgb_fine, float* const* d_latents_host, void* stream) {
  if (!rgb_fine || !target || !grad_loss || !d_rgb_fine) return fail(AON_E_INVALID, "aon_train_loss_bwd: null pointer");
  if (n <= 0) return fail(AON_E_INVALID, "aon_train_loss_bwd: bad size");
  if ((rgb_coarse == nullptr) != (d_rgb_coarse == nullptr)) return fail(AON_E_INVALID, "aon_train_loss_bwd: coarse level input / gradient mismatch");
  for (int k = 0; k < 3 && latents_host; ++k)
    if (latents_host[k] && (!latent_len_host || latent_len_host[k] <= 0)) return fail(AON_E_INVALID, "aon_train_loss_bwd: bad latent length");
  return check(aon::launch_train_loss(true, rgb_coarse, rgb_fine, target, n, latents_host, latent_len_host, reg_scale, nullptr, nullptr, grad_loss, d_rgb_coarse, d_rgb_fine,
                                      d_latents_host, (hipStream_t)stream), "aon_train_loss_bwd");
}

int aon_view_bias(const void* packed, const float* viewdirs, int64_t n_rays, float* view_bias, void* stream) {
  if (n_rays < 0) return fail(AON_E_INVALID, "aon_view_bias: bad size");
  if (n_rays == 0) return AON_OK;
  if (!packed || !viewdirs || !view_bias) return fail(AON_E_INVALID, "aon_view_bias: null pointer");
  if (aon::stream_form(packed) != aon::kFormFolded) return fail(AON_E_INVALID, "aon_view_bias: the stream was packed in the literal form (aon_set_bottleneck_fold)");
  return check(aon::launch_view_bias(static_cast<const char*>(packed), viewdirs, n_rays, view_bias, (hipStream_t)stream), "aon_view_bias");
}

int aon_ray_directions(int H, int W, float focal, float* directions, void* stream) {
  if (H <= 0 || W <= 0 || !(focal > 0.f) || !directions) return fail(AON_E_INVALID, "aon_ray_directions: bad argument");
  return check(aon::launch_ray_directions(H, W, focal, directions, (hipStream_t)stream), "aon_ray_directions");
}

int aon_get_rays(const float* directions, const float* c2w_host, int64_t n, float* rays_o, float* viewdirs, float* rays_d,
                 void* stream) {
  if (n < 0) return fail(AON_E_INVALID, "aon_get_rays: bad size");
  if (n == 0) return AON_OK;
  if (!directions || !c2w_host || !rays_o || !viewdirs) return fail(AON_E_INVALID, "aon_get_rays: null pointer");
  // geometry arguments are unused when directions are supplied; W = n keeps the pixel index math in range
  return check(aon::launch_raygen(c2w_host, 1, (int)(n > INT32_MAX ? INT32_MAX : n), 1.0f, directions, 0, n, rays_o, viewdirs,
                                  rays_d, (hipStream_t)stream), "aon_get_rays");
}

int aon_ray_radii(const float* directions, const float* c2w_host, int H, int W, float* radii, void* stream) {
  if (!directions || !c2w_host || !radii) return fail(AON_E_INVALID, "aon_ray_radii: null pointer");
  if (H < 3 || W < 1) return fail(AON_E_INVALID, "aon_ray_radii: needs H >= 3 image rows (ray_utils.py:141 indexes dx[-2])");
  return check(aon::launch_ray_radii(directions, c2w_host, H, W, radii, (hipStream_t)stream), "aon_ray_radii");
}

int aon_cast_rays(const float* t_vals, const float* origins, const float* directions, int64_t n_rays, int S, float* coords,
                  void* stream) {
  if (n_rays < 0 || S < 1) return fail(AON_E_INVALID, "aon_cast_rays: bad size");
  if (n_rays == 0) return AON_OK;
  if (!t_vals || !origins || !directions || !coords) return fail(AON_E_INVALID, "aon_cast_rays: null pointer");
  return check(aon::launch_cast_rays(t_vals, origins, directions, n_rays, S, coords, (hipStream_t)stream), "aon_cast_rays");
}

int aon_sample_along_rays(const float* rays_o, const float* rays_d, int64_t n_rays, int S, float near_, float far_,
                          const float* t_rand, float* t_vals, float* coords, void* stream) {
  if (n_rays < 0 || S < 2) return fail(AON_E_INVALID, "aon_sample_along_rays: bad size");
  if (n_rays == 0) return AON_OK;
  if (!t_vals || (coords && (!rays_o || !rays_d))) return fail(AON_E_INVALID, "aon_sample_along_rays: null pointer");
  return check(aon::launch_sample_along_rays(rays_o, rays_d, n_rays, S, near_, far_, t_rand, t_vals, coords, (hipStream_t)stream),
               "aon_sample_along_rays");
}

int aon_pos_enc(const float* x, int64_t n, int min_deg, int max_deg, float* out, void* stream) {
  if (n < 0 || max_deg < min_deg) return fail(AON_E_INVALID, "aon_pos_enc: bad size");
  if (n == 0) return AON_OK;
  if (!x || !out) return fail(AON_E_INVALID, "aon_pos_enc: null pointer");
  return check(aon::launch_pos_enc(x, n, min_deg, max_deg, out, (hipStream_t)stream), "aon_pos_enc");
}

int64_t aon_mlp_packed_bytes(void) { return aon::kPackedBytes; }

int aon_pack_vanilla_mlp(const float* const* params_host, void* packed, void* stream) {
  if (!params_host || !packed) return fail(AON_E_INVALID, "aon_pack_vanilla_mlp: null pointer");
  for (int i = 0; i < aon::kNumVanillaParams; ++i)
    if (!params_host[i]) return fail(AON_E_INVALID, "aon_pack_vanilla_mlp: null parameter pointer");
  if (reinterpret_cast<uintptr_t>(packed) & 15) return fail(AON_E_INVALID, "aon_pack_vanilla_mlp: packed must be 16-byte aligned");
  return check(aon::launch_pack_vanilla(params_host, static_cast<float*>(packed), (hipStream_t)stream), "aon_pack_vanilla_mlp");
}

int aon_pack_vanilla_mlp_deg(const float* const* params_host, int min_deg_point, int max_deg_point, int deg_view, void* packed, void* stream) {
  if (!params_host || !packed) return fail(AON_E_INVALID, "aon_pack_vanilla_mlp_deg: null pointer");
  for (int i = 0; i < aon::kNumVanillaParams; ++i)
    if (!params_host[i]) return fail(AON_E_INVALID, "aon_pack_vanilla_mlp_deg: null parameter pointer");
  if (reinterpret_cast<uintptr_t>(packed) & 15) return fail(AON_E_INVALID, "aon_pack_vanilla_mlp_deg: packed must be 16-byte aligned");
  const int L = max_deg_point - min_deg_point;
  if (L < 0 || L > 10 || deg_view < 0 || deg_view > 4)
    return fail(AON_E_INVALID, "aon_pack_vanilla_mlp_deg: the stream holds up to 10 position and 4 view frequency levels");
  return check(aon::launch_pack_vanilla(params_host, static_cast<float*>(packed), (hipStream_t)stream, L, deg_view), "aon_pack_vanilla_mlp_deg");
}

int aon_mlp_fwd(const void* packed, const float* rays_o, const float* rays_d, const float* viewdirs, const float* t_vals,
                int64_t n_rays, int S, float* raw, void* stream) {
  if (n_rays < 0 || S < 1) return fail(AON_E_INVALID, "aon_mlp_fwd: bad size");
  if (n_rays == 0) return AON_OK;
  if (!packed || !rays_o || !rays_d || !viewdirs || !t_vals || !raw) return fail(AON_E_INVALID, "aon_mlp_fwd: null pointer");
  if (n_rays * (int64_t)S > (int64_t)INT32_MAX * 64) return fail(AON_E_INVALID, "aon_mlp_fwd: too many samples for one call");
  MlpTimer timer((hipStream_t)stream, n_rays * S);
  const aon::FwdSeg seg{.packed = static_cast<const char*>(packed), .rays_o = rays_o, .rays_d = rays_d, .viewdirs = viewdirs, .t_vals = t_vals,
                        .n_rays = n_rays, .S = S, .raw = raw};
  return check(aon::launch_net_fwd(false, &seg, 1, (hipStream_t)stream), "aon_mlp_fwd");
}

int aon_mlp_fwd_enc(const void* packed, const float* samples_enc, const float* viewdirs_enc, int64_t n_rays, int S,
                    float* raw, void* stream) {
  if (n_rays < 0 || S < 1) return fail(AON_E_INVALID, "aon_mlp_fwd_enc: bad size");
  if (n_rays == 0) return AON_OK;
  if (!packed || !samples_enc || !viewdirs_enc || !raw) return fail(AON_E_INVALID, "aon_mlp_fwd_enc: null pointer");
  const aon::FwdSeg seg{.packed = static_cast<const char*>(packed), .n_rays = n_rays, .S = S, .raw = raw, .samples_enc = samples_enc,
                        .viewdirs_enc = viewdirs_enc};
  return check(aon::launch_net_fwd(false, &seg, 1, (hipStream_t)stream), "aon_mlp_fwd_enc");
}

int aon_composite(const float* rgb, int rgb_stride, const float* sigma, int sigma_stride, const float* t_vals,
                  const float* dirs, int64_t n_rays, int S, int white_bkgd, int act, float* comp_rgb, float* acc,
                  float* depth, float* weights, void* stream) {
  if (n_rays < 0 || S < 1 || rgb_stride < 3 || sigma_stride < 1 || act < 0 || act > 2)
    return fail(AON_E_INVALID, "aon_composite: bad size / stride / act");
  if (n_rays == 0) return AON_OK;
  if (!rgb || !sigma || !t_vals || !dirs || !comp_rgb || !acc || !depth) return fail(AON_E_INVALID, "aon_composite: null pointer");
  KTimer timer(kComposite, (hipStream_t)stream, n_rays);
  return check(aon::launch_composite(rgb, rgb_stride, sigma, sigma_stride, t_vals, dirs, n_rays, S, white_bkgd, aon::default_act(act), comp_rgb,
                                     acc, depth, weights, (hipStream_t)stream), "aon_composite");
}

void aon_render_opts_init(aon_render_opts* o) {
  if (!o) return;
  o->num_coarse_samples = 64; o->num_fine_samples = 128; o->lindisp = 0; o->inv_near = 0.f; o->inv_far = 0.f;
  o->noise_std = 0.f; o->noise_c = nullptr; o->noise_f = nullptr;
  o->rgb_scale = 1.002f; o->rgb_shift = 0.001f; o->sigma_bias = -1.0f;
  o->min_deg_point = 0; o->max_deg_point = 10; o->deg_view = 4;
}

int aon_sample_along_rays_ex(const float* rays_o, const float* rays_d, int64_t n_rays, int S, float near_, float far_, int lindisp,
                             float inv_near, float inv_far, const float* t_rand, float* t_vals, float* coords, void* stream) {
  if (n_rays < 0 || S < 2) return fail(AON_E_INVALID, "aon_sample_along_rays_ex: bad size");
  if (n_rays == 0) return AON_OK;
  if (!t_vals || (coords && (!rays_o || !rays_d))) return fail(AON_E_INVALID, "aon_sample_along_rays_ex: null pointer");
  return check(aon::launch_sample_along_rays(rays_o, rays_d, n_rays, S, near_, far_, t_rand, t_vals, coords, (hipStream_t)stream,
                                             lindisp != 0, inv_near, inv_far), "aon_sample_along_rays_ex");
}

// ---- per-ray near / far (aon_bounds.hip) ----
static const char* box_bad(const float* lo3, const float* hi3) {
  if (!lo3 || !hi3) return "null box";
  for (int a = 0; a < 3; ++a)
    if (lo3[a] != lo3[a] || hi3[a] != hi3[a]) return "box bound is NaN";
  return nullptr;
}
int aon_ray_limits_box(const float* rays_o, const float* rays_d, int64_t n_rays, const float* lo3_host, const float* hi3_host, float* near_ray,
                       float* far_ray, void* stream) {
  if (n_rays < 0) return fail(AON_E_INVALID, "aon_ray_limits_box: bad size");
  if (const char* bad = box_bad(lo3_host, hi3_host)) return fail(AON_E_INVALID, (std::string("aon_ray_limits_box: ") + bad).c_str());
  if (n_rays == 0) return AON_OK;
  if (!rays_o || !rays_d || !near_ray || !far_ray) return fail(AON_E_INVALID, "aon_ray_limits_box: null pointer");
  return check(aon::launch_ray_limits(rays_o, rays_d, n_rays, lo3_host, hi3_host, near_ray, far_ray, nullptr, nullptr, (hipStream_t)stream),
               "aon_ray_limits_box");
}
int64_t aon_ray_limits_workspace_bytes(int64_t n_rays) { return aon::ray_limits_workspace_bytes(n_rays < 1 ? 1 : n_rays); }
int aon_ray_limits(const float* rays_o, const float* rays_d, int64_t n_rays, const float* lo3_host, const float* hi3_host, float* near_ray,
                   float* far_ray, uint8_t* live, void* workspace, int64_t workspace_bytes, void* stream) {
  if (n_rays < 0) return fail(AON_E_INVALID, "aon_ray_limits: bad size");
  if (const char* bad = box_bad(lo3_host, hi3_host)) return fail(AON_E_INVALID, (std::string("aon_ray_limits: ") + bad).c_str());
  if (n_rays == 0) return AON_OK;
  if (!rays_o || !rays_d || !near_ray || !far_ray || !workspace) return fail(AON_E_INVALID, "aon_ray_limits: null pointer");
  if (reinterpret_cast<uintptr_t>(workspace) & 3) return fail(AON_E_INVALID, "aon_ray_limits: workspace must be 4-byte aligned");
  if (workspace_bytes < aon::ray_limits_workspace_bytes(n_rays)) return fail(AON_E_WORKSPACE, "aon_ray_limits: workspace smaller than aon_ray_limits_workspace_bytes()");
  return check(aon::launch_ray_limits(rays_o, rays_d, n_rays, lo3_host, hi3_host, near_ray, far_ray, live, static_cast<char*>(workspace),
                                      (hipStream_t)stream), "aon_ray_limits");
}
int aon_sample_along_rays_bounds(const float* rays_o, const float* rays_d, int64_t n_rays, int S, const float* near_ray, const float* far_ray,
                                 int lindisp, const float* t_rand, float* t_vals, float* coords, void* stream) {
  if (n_rays < 0 || S < 2) return fail(AON_E_INVALID, "aon_sample_along_rays_bounds: bad size");
  if (n_rays == 0) return AON_OK;
  if (!t_vals || !near_ray || !far_ray || (coords && (!rays_o || !rays_d))) return fail(AON_E_INVALID, "aon_sample_along_rays_bounds: null pointer");
  return check(aon::launch_sample_along_rays(rays_o, rays_d, n_rays, S, 0.f, 0.f, t_rand, t_vals, coords, (hipStream_t)stream, lindisp != 0, 0.f, 0.f,
                                             near_ray, far_ray), "aon_sample_along_rays_bounds");
}

int aon_composite_ex(const float* rgb, int rgb_stride, const float* sigma, int sigma_stride, const float* t_vals, const float* dirs,
                     int64_t n_rays, int S, int white_bkgd, int act, const aon_render_opts* opts, float* comp_rgb, float* acc,
                     float* depth, float* weights, void* stream) {
  if (n_rays < 0 || S < 1 || rgb_stride < 3 || sigma_stride < 1 || act < 0 || act > 2)
    return fail(AON_E_INVALID, "aon_composite_ex: bad size / stride / act");
  if (n_rays == 0) return AON_OK;
  if (!rgb || !sigma || !t_vals || !dirs || !comp_rgb || !acc || !depth) return fail(AON_E_INVALID, "aon_composite_ex: null pointer");
  aon::ActParams ap = aon::default_act(act);
  if (opts) {
    ap.rgb_scale = opts->rgb_scale; ap.rgb_shift = opts->rgb_shift; ap.sigma_bias = opts->sigma_bias;
    if (opts->noise_c && opts->noise_std > 0.f) { ap.noise = opts->noise_c; ap.noise_std = opts->noise_std; }
  }
  KTimer timer(kComposite, (hipStream_t)stream, n_rays);
  return check(aon::launch_composite(rgb, rgb_stride, sigma, sigma_stride, t_vals, dirs, n_rays, S, white_bkgd, ap, comp_rgb, acc, depth,
                                     weights, (hipStream_t)stream), "aon_composite_ex");
}

int aon_sample_pdf_n(const float* bins, const float* weights, int64_t w_stride, const float* t_coarse, const float* u,
                     int64_t u_stride, int64_t n_rays, int num_bins, int num_samples, int num_t, float* samples, float* t_fine,
                     void* stream) {
  if (n_rays < 0 || num_bins < 2 || num_samples < 1 || num_t < 0 || w_stride < num_bins - 1 || (u_stride != 0 && u_stride < num_samples))
    return fail(AON_E_INVALID, "aon_sample_pdf_n: bad size / stride");
  if (!bins && num_t != num_bins + 1) return fail(AON_E_INVALID, "aon_sample_pdf_n: bins == NULL needs num_t == num_bins + 1 (mid-points of t_coarse)");
  if (aon::sample_pdf_n_lds_bytes(num_bins, num_samples, num_t, nullptr) > 64 * 1024) return fail(AON_E_INVALID, "aon_sample_pdf_n: sizes exceed the per-ray LDS image");
  if (n_rays == 0) return AON_OK;
  if (!weights || !u || (!bins && !t_coarse) || (t_fine && !t_coarse) || (!samples && !t_fine))
    return fail(AON_E_INVALID, "aon_sample_pdf_n: null pointer");
  KTimer timer(kSamplePdf, (hipStream_t)stream, n_rays);
  return check(aon::launch_sample_pdf_n(bins, weights, w_stride, t_coarse, u, u_stride, n_rays, num_bins, num_samples, t_coarse ? num_t : 0,
                                        samples, t_fine, (hipStream_t)stream), "aon_sample_pdf_n");
}

int aon_sample_pdf(const float* bins, const float* weights, int64_t w_stride, const float* t_coarse, const float* u,
                   int64_t u_stride, int64_t n_rays, float* samples, float* t_fine, void* stream) {
  if (n_rays < 0 || w_stride < 63 || (u_stride != 0 && u_stride < 128)) return fail(AON_E_INVALID, "aon_sample_pdf: bad size / stride");
  if (n_rays == 0) return AON_OK;
  if (!weights || !u || (!bins && !t_coarse) || (t_fine && !t_coarse) || (!samples && !t_fine))
    return fail(AON_E_INVALID, "aon_sample_pdf: null pointer");
  KTimer timer(kSamplePdf, (hipStream_t)stream, n_rays);
  return check(aon::launch_sample_pdf(bins, weights, w_stride, t_coarse, u, u_stride, n_rays, samples, t_fine,
                                      (hipStream_t)stream), "aon_sample_pdf");
}

int aon_set_coarse_fusion(int on) {
  g_fuse_coarse.store(on ? 1 : 0, std::memory_order_relaxed);
  return AON_OK;
}

int aon_composite_pdf(const float* raw, const float* t_coarse, const float* dirs, int64_t n_rays, int white_bkgd, int act,
                      const float* u, int64_t u_stride, float* comp_rgb, float* acc, float* depth, float* weights, float* t_fine,
                      void* stream) {
  if (n_rays < 0 || act < 0 || act > 2 || (u_stride != 0 && u_stride < 128)) return fail(AON_E_INVALID, "aon_composite_pdf: bad size / stride / act");
  if (n_rays == 0) return AON_OK;
  if (!raw || !t_coarse || !dirs || !u || !comp_rgb || !acc || !depth || !t_fine) return fail(AON_E_INVALID, "aon_composite_pdf: null pointer");
  if (reinterpret_cast<uintptr_t>(raw) & 15) return fail(AON_E_INVALID, "aon_composite_pdf: raw must be 16-byte aligned");
  KTimer timer(kCompositePdf, (hipStream_t)stream, n_rays);
  return check(aon::launch_composite_pdf(raw, t_coarse, dirs, n_rays, white_bkgd, aon::default_act(act), u, u_stride, comp_rgb, acc, depth, weights,
                                         t_fine, (hipStream_t)stream), "aon_composite_pdf");
}

// ---- training (R14) ----
int64_t aon_train_plane_rows(void) { return aon::kPlRows; }
int64_t aon_bwd_packed_bytes(void) { return aon::bwd_stream_bytes(); }
int64_t aon_wgrad_workspace_bytes(void) { return aon::wgrad_workspace_bytes(); }

int aon_wgrad_plan(int articulated, int64_t Np, int cus, int32_t* jobs6, int max_jobs, int64_t* ws_bytes) {
  if (!jobs6 || max_jobs < 1) return fail(AON_E_INVALID, "aon_wgrad_plan: null / empty output");
  const int n = aon::wgrad_plan_describe(articulated != 0, Np, cus, jobs6, max_jobs, ws_bytes);
  if (n < 0) return fail(AON_E_INVALID, n == -1 ? "aon_wgrad_plan: Np must be a positive multiple of 32, cus >= 1"
                                       : n == -2 ? "aon_wgrad_plan: no plan" : "aon_wgrad_plan: max_jobs too small");
  return n;
}

int aon_wgrad_plan_segment(int articulated, int64_t Np, int cus, int job, int workgroup, int32_t* begin_end) {
  if (!begin_end) return fail(AON_E_INVALID, "aon_wgrad_plan_segment: null output");
  const int r = aon::wgrad_plan_segment(articulated != 0, Np, cus, job, workgroup, begin_end);
  if (r < 0) return fail(AON_E_INVALID, "aon_wgrad_plan_segment: bad argument");
  return r;
}

int aon_set_wgrad_probe(void* device_buffer) {
  aon::set_wgrad_probe(static_cast<long long*>(device_buffer));
  return AON_OK;
}

int aon_wgrad_kind_bench(int kind, int nlayers, const float* planes, const float* dplanes, int rows, int64_t Np, void* workspace,
                         int64_t workspace_bytes, void* stream) {
  if (!planes || !dplanes || !workspace || rows < 512 || (rows & 31) || Np <= 0 || (Np & 127))
    return fail(AON_E_INVALID, "aon_wgrad_kind_bench: bad argument");
  if (workspace_bytes < aon::wgrad_workspace_bytes()) return fail(AON_E_WORKSPACE, "aon_wgrad_kind_bench: workspace too small");
  KTimer timer(kWgrad, (hipStream_t)stream, Np);
  return check(aon::launch_wgrad_kind_bench(kind, nlayers, planes, dplanes, rows, Np, static_cast<float*>(workspace), nullptr,
                                            (hipStream_t)stream), "aon_wgrad_kind_bench");
}

int aon_pack_vanilla_mlp_bwd(const float* const* params_host, void* packed_bwd, void* stream) {
  if (!params_host || !packed_bwd) return fail(AON_E_INVALID, "aon_pack_vanilla_mlp_bwd: null pointer");
  for (int i = 0; i < aon::kNumVanillaParams; ++i)
    if (!params_host[i]) return fail(AON_E_INVALID, "aon_pack_vanilla_mlp_bwd: null parameter pointer");
  if (reinterpret_cast<uintptr_t>(packed_bwd) & 15) return fail(AON_E_INVALID, "aon_pack_vanilla_mlp_bwd: buffer must be 16-byte aligned");
  return check(aon::launch_pack_vanilla_bwd(params_host, static_cast<float*>(packed_bwd), (hipStream_t)stream), "aon_pack_vanilla_mlp_bwd");
}

int aon_pack_vanilla_mlp_bwd_deg(const float* const* params_host, int min_deg_point, int max_deg_point, int deg_view, void* packed_bwd, void* stream) {
  if (!params_host || !packed_bwd) return fail(AON_E_INVALID, "aon_pack_vanilla_mlp_bwd_deg: null pointer");
  for (int i = 0; i < aon::kNumVanillaParams; ++i)
    if (!params_host[i]) return fail(AON_E_INVALID, "aon_pack_vanilla_mlp_bwd_deg: null parameter pointer");
  const int L = max_deg_point - min_deg_point;
  if (L < 0 || L > 10 || deg_view < 0 || deg_view > 4)
    return fail(AON_E_INVALID, "aon_pack_vanilla_mlp_bwd_deg: up to 10 position and 4 view frequency levels");
  return check(aon::launch_pack_vanilla_bwd(params_host, static_cast<float*>(packed_bwd), (hipStream_t)stream, aon::enc_width(L), aon::enc_width(deg_view)),
               "aon_pack_vanilla_mlp_bwd_deg");
}

// Round 6: everything a training step of a TWO-level vanilla model packs, in one call -- both networks' forward and transposed streams --
// with the eight fp64 fold products (W' and b' of each network, once for its forward and once for its transposed stream) as ONE launch in
// front instead of four launches of 13-16 us in a row with their pack kernels.  The same kernels on the same operands as the four separate
// calls: same bytes in every buffer.  packed_bwd_* may be NULL (no backward wanted).
int aon_vanilla_pack_step(const float* const* params_coarse_host, const float* const* params_fine_host, int min_deg_point, int max_deg_point, int deg_view,
                          void* packed_coarse, void* packed_bwd_coarse, void* packed_fine, void* packed_bwd_fine, void* stream_) {
  if (!params_coarse_host || !params_fine_host || !packed_coarse || !packed_fine) return fail(AON_E_INVALID, "aon_vanilla_pack_step: null pointer");
  for (int i = 0; i < aon::kNumVanillaParams; ++i)
    if (!params_coarse_host[i] || !params_fine_host[i]) return fail(AON_E_INVALID, "aon_vanilla_pack_step: null parameter pointer");
  for (const void* p : {(const void*)packed_coarse, (const void*)packed_fine, (const void*)packed_bwd_coarse, (const void*)packed_bwd_fine})
    if (reinterpret_cast<uintptr_t>(p) & 15) return fail(AON_E_INVALID, "aon_vanilla_pack_step: buffers must be 16-byte aligned");
  const int L = max_deg_point - min_deg_point;
  if (L < 0 || L > 10 || deg_view < 0 || deg_view > 4)
    return fail(AON_E_INVALID, "aon_vanilla_pack_step: the streams hold up to 10 position and 4 view frequency levels");
  hipStream_t stream = (hipStream_t)stream_;
  const float* const* P[2] = {params_coarse_host, params_fine_host};
  float* fwd[2] = {static_cast<float*>(packed_coarse), static_cast<float*>(packed_fine)};
  float* bwd[2] = {static_cast<float*>(packed_bwd_coarse), static_cast<float*>(packed_bwd_fine)};
  const bool folded = aon::fold_default() == aon::kFormFolded;
  if (folded) {
    aon::FoldGemm jobs[8];
    int n = 0;
    for (int l = 0; l < 2; ++l) { aon::vanilla_fold_jobs_fwd(P[l], fwd[l], deg_view, jobs + n); n += 2; }
    for (int l = 0; l < 2; ++l)
      if (bwd[l]) { aon::vanilla_fold_jobs_bwd(P[l], bwd[l], aon::enc_width(deg_view), jobs + n); n += 2; }
    if (int rc = check(aon::launch_fold_gemms(jobs, n, stream), "aon_vanilla_pack_step")) return rc;
  }
  for (int l = 0; l < 2; ++l)
    if (int rc = check(aon::launch_pack_vanilla(P[l], fwd[l], stream, L, deg_view, folded), "aon_vanilla_pack_step")) return rc;
  for (int l = 0; l < 2; ++l)
    if (bwd[l])
      if (int rc = check(aon::launch_pack_vanilla_bwd(P[l], bwd[l], stream, aon::enc_width(L), aon::enc_width(deg_view), folded), "aon_vanilla_pack_step")) return rc;
  return AON_OK;
}

int64_t aon_train_mask_bytes(int64_t Np) { return (int64_t)aon::kMaskLayers * Np * 2 * 16; }

int aon_mlp_fwd_train(const void* packed, const float* rays_o, const float* rays_d, const float* viewdirs, const float* t_vals,
                      int64_t n_rays, int S, float* raw, float* planes, void* masks, void* stream) {
  if (n_rays < 0 || S < 1) return fail(AON_E_INVALID, "aon_mlp_fwd_train: bad size");
  if (n_rays == 0) return AON_OK;
  if (!packed || !rays_o || !rays_d || !viewdirs || !t_vals || !raw || !planes || !masks)
    return fail(AON_E_INVALID, "aon_mlp_fwd_train: null pointer");
  if (reinterpret_cast<uintptr_t>(masks) & 15) return fail(AON_E_INVALID, "aon_mlp_fwd_train: masks must be 16-byte aligned");
  MlpTimer timer((hipStream_t)stream, n_rays * S);
  const aon::FwdSeg seg{.packed = static_cast<const char*>(packed), .rays_o = rays_o, .rays_d = rays_d, .viewdirs = viewdirs, .t_vals = t_vals,
                        .n_rays = n_rays, .S = S, .raw = raw, .planes = planes, .masks = masks};
  return check(aon::launch_net_fwd(false, &seg, 1, (hipStream_t)stream), "aon_mlp_fwd_train");
}

int aon_composite_bwd(const float* raw, const float* t_vals, const float* dirs, const float* g_rgb, const float* g_acc,
                      const float* g_depth, int64_t n_rays, int S, int white_bkgd, int act, float* d_raw, void* stream) {
  if (n_rays < 0 || S < 1 || S > 512 || act < 0 || act > 2) return fail(AON_E_INVALID, "aon_composite_bwd: bad size / act (S <= 512)");
  if (n_rays == 0) return AON_OK;
  if (!raw || !t_vals || !dirs || !g_rgb || !d_raw) return fail(AON_E_INVALID, "aon_composite_bwd: null pointer");
  KTimer timer(kCompositeBwd, (hipStream_t)stream, n_rays);
  return check(aon::launch_composite_bwd(raw, t_vals, dirs, g_rgb, g_acc, g_depth, n_rays, S, white_bkgd, aon::default_act(act), d_raw,
                                         (hipStream_t)stream), "aon_composite_bwd");
}

int aon_mlp_bwd_chain(const void* packed_bwd, const void* packed_fwd, const float* d_raw, const void* masks, float* dplanes,
                      int64_t Np, void* stream) {
  if (Np < 0 || (Np & 127)) return fail(AON_E_INVALID, "aon_mlp_bwd_chain: Np must be a multiple of 128");
  if (Np == 0) return AON_OK;
  if (!packed_bwd || !packed_fwd || !d_raw || !masks || !dplanes) return fail(AON_E_INVALID, "aon_mlp_bwd_chain: null pointer");
  if (forms_differ(packed_bwd, packed_fwd)) return fail(AON_E_INVALID, kFormsMsg);   // (the masks / planes came from packed_fwd's kernel: ADVICE r5)
  KTimer timer(kBwdChain, (hipStream_t)stream, Np);
  return check(aon::launch_mlp_bwd_chain(static_cast<const char*>(packed_bwd), static_cast<const char*>(packed_fwd), d_raw, masks,
                                         dplanes, Np, (hipStream_t)stream), "aon_mlp_bwd_chain");
}

int aon_vanilla_wgrad(const float* planes, const float* dplanes, const float* d_raw, int64_t Np, float* const* grads_host,
                      void* workspace, int64_t workspace_bytes, void* stream, const void* packed_bwd) {
  if (Np <= 0 || (Np & 127)) return fail(AON_E_INVALID, "aon_vanilla_wgrad: Np must be a positive multiple of 128");
  if (!planes || !dplanes || !d_raw || !grads_host || !workspace) return fail(AON_E_INVALID, "aon_vanilla_wgrad: null pointer");
  for (int i = 0; i < aon::kNumVanillaParams; ++i)
    if (!grads_host[i]) return fail(AON_E_INVALID, "aon_vanilla_wgrad: null gradient pointer");
  if (workspace_bytes < aon::wgrad_workspace_bytes()) return fail(AON_E_WORKSPACE, "aon_vanilla_wgrad: workspace too small");
  if (!packed_bwd && aon::fold_default() == aon::kFormFolded) return fail(AON_E_INVALID, kNullBwdMsg);
  KTimer timer(kWgrad, (hipStream_t)stream, Np);
  return check(aon::launch_vanilla_wgrad(planes, dplanes, d_raw, Np, grads_host, static_cast<float*>(workspace), (hipStream_t)stream, nullptr, packed_bwd),
               "aon_vanilla_wgrad");
}

// ---- training, articulated network ----
int64_t aon_art_train_plane_rows(void) { return aon::kAPlRows; }
int64_t aon_art_train_mask_bytes(int64_t Np) { return (int64_t)aon::kAMaskLayers * Np * 2 * 16; }
int64_t aon_art_bwd_packed_bytes(void) { return aon::art_bwd_stream_bytes(); }

static const char* art_degrees_ok(int min_deg_point, int max_deg_point, int deg_view) {
  const int L = max_deg_point - min_deg_point;
  if (L < 0 || L > 10 || deg_view < 0 || deg_view > 4) return "up to 10 position and 4 view frequency levels";
  if (min_deg_point < -32 || max_deg_point > 32) return "min_deg_point / max_deg_point must lie in [-32, 32]";
  // the fused kernels encode the deformed point with the short sine (sin_f32<false>, aon_common.h): 2^(max_deg_point - 1) |x'| < 2^19
  if (max_deg_point > 16) return "the articulated kernels' in-register encoding holds for max_deg_point <= 16";
  return nullptr;
}

int aon_pack_art_mlp_bwd(const float* const* params_host, void* packed_bwd, void* stream) {
  return aon_pack_art_mlp_bwd_deg(params_host, 0, 10, 4, packed_bwd, stream);
}
int aon_pack_art_mlp_bwd_deg(const float* const* params_host, int min_deg_point, int max_deg_point, int deg_view, void* packed_bwd, void* stream) {
  if (!params_host || !packed_bwd) return fail(AON_E_INVALID, "aon_pack_art_mlp_bwd: null pointer");
  for (int i = 0; i < aon::kNumArtParams; ++i)
    if (!params_host[i]) return fail(AON_E_INVALID, "aon_pack_art_mlp_bwd: null parameter pointer");
  if (reinterpret_cast<uintptr_t>(packed_bwd) & 15) return fail(AON_E_INVALID, "aon_pack_art_mlp_bwd: buffer must be 16-byte aligned");
  if (const char* bad = art_degrees_ok(min_deg_point, max_deg_point, deg_view)) return fail(AON_E_INVALID, bad);
  return check(aon::launch_pack_art_bwd(params_host, static_cast<float*>(packed_bwd), (hipStream_t)stream, max_deg_point - min_deg_point, deg_view),
               "aon_pack_art_mlp_bwd");
}

int aon_art_mlp_fwd_train(const void* packed, const void* small, const float* rays_o, const float* rays_d, const float* viewdirs,
                          const float* t_vals, int64_t n_rays, int S, float* raw, float* planes, void* masks, void* stream) {
  if (n_rays < 0 || S < 1) return fail(AON_E_INVALID, "aon_art_mlp_fwd_train: bad size");
  if (n_rays == 0) return AON_OK;
  if (!packed || !small || !rays_o || !rays_d || !viewdirs || !t_vals || !raw || !planes || !masks)
    return fail(AON_E_INVALID, "aon_art_mlp_fwd_train: null pointer");
  if (forms_differ(packed, small)) return fail(AON_E_INVALID, kFormsMsg);
  if (reinterpret_cast<uintptr_t>(masks) & 15) return fail(AON_E_INVALID, "aon_art_mlp_fwd_train: masks must be 16-byte aligned");
  MlpTimer timer((hipStream_t)stream, n_rays * S);
  const aon::FwdSeg seg{.packed = static_cast<const char*>(packed), .small = static_cast<const float*>(small), .rays_o = rays_o, .rays_d = rays_d,
                        .viewdirs = viewdirs, .t_vals = t_vals, .n_rays = n_rays, .S = S, .raw = raw, .planes = planes, .masks = masks};
  return check(aon::launch_net_fwd(true, &seg, 1, (hipStream_t)stream), "aon_art_mlp_fwd_train");
}

int aon_art_bwd_chain(const void* packed_bwd, const void* small, const float* d_raw, const void* masks, const float* planes,
                      float* dplanes, float* dxp, int64_t Np, void* stream) {
  if (Np < 0 || (Np & 127)) return fail(AON_E_INVALID, "aon_art_bwd_chain: Np must be a multiple of 128");
  if (Np == 0) return AON_OK;
  if (!packed_bwd || !small || !d_raw || !masks || !planes || !dplanes || !dxp) return fail(AON_E_INVALID, "aon_art_bwd_chain: null pointer");
  if (forms_differ(packed_bwd, small)) return fail(AON_E_INVALID, kFormsMsg);
  KTimer timer(kBwdChain, (hipStream_t)stream, Np);
  return check(aon::launch_art_bwd_chain(static_cast<const char*>(packed_bwd), static_cast<const float*>(small), d_raw, masks, planes,
                                         dplanes, dxp, Np, (hipStream_t)stream), "aon_art_bwd_chain");
}

int aon_art_wgrad(const float* planes, const float* dplanes, const float* d_raw, const float* dxp, int64_t Np,
                  const float* const* params_host, const float* shape, const float* appearance, const float* articulation,
                  float* const* grads_host, float* g_shape, float* g_appearance, float* g_articulation, void* workspace,
                  int64_t workspace_bytes, void* stream, const void* packed_bwd) {
  return aon_art_wgrad_deg(planes, dplanes, d_raw, dxp, Np, params_host, shape, appearance, articulation, grads_host, g_shape, g_appearance,
                           g_articulation, workspace, workspace_bytes, stream, 0, 10, 4, packed_bwd);
}
int aon_art_wgrad_deg(const float* planes, const float* dplanes, const float* d_raw, const float* dxp, int64_t Np,
                      const float* const* params_host, const float* shape, const float* appearance, const float* articulation,
                      float* const* grads_host, float* g_shape, float* g_appearance, float* g_articulation, void* workspace,
                      int64_t workspace_bytes, void* stream, int min_deg_point, int max_deg_point, int deg_view, const void* packed_bwd) {
  if (const char* bad = art_degrees_ok(min_deg_point, max_deg_point, deg_view)) return fail(AON_E_INVALID, bad);
  if (Np <= 0 || (Np & 127)) return fail(AON_E_INVALID, "aon_art_wgrad: Np must be a positive multiple of 128");
  if (!planes || !dplanes || !d_raw || !dxp || !params_host || !shape || !appearance || !articulation || !grads_host || !g_shape ||
      !g_appearance || !g_articulation || !workspace)
    return fail(AON_E_INVALID, "aon_art_wgrad: null pointer");
  for (int i = 0; i < aon::kNumArtParams; ++i)
    if (!params_host[i] || !grads_host[i]) return fail(AON_E_INVALID, "aon_art_wgrad: null parameter / gradient pointer");
  if (workspace_bytes < aon::wgrad_workspace_bytes()) return fail(AON_E_WORKSPACE, "aon_art_wgrad: workspace too small");
  if (!packed_bwd && aon::fold_default() == aon::kFormFolded) return fail(AON_E_INVALID, kNullBwdMsg);
  KTimer timer(kWgrad, (hipStream_t)stream, Np);
  return check(aon::launch_art_wgrad(planes, dplanes, d_raw, dxp, Np, params_host, shape, appearance, articulation, grads_host, g_shape,
                                     g_appearance, g_articulation, static_cast<float*>(workspace), (hipStream_t)stream, nullptr,
                                     max_deg_point - min_deg_point, deg_view, packed_bwd), "aon_art_wgrad");
}

// ---- round 6: the end of a training step on one parameter arena (csrc/aon_optim.hip) ----
int aon_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, double lr, double beta1, double beta2, double eps,
                  int64_t step, void* stream) {
  if (n < 0 || step < 1) return fail(AON_E_INVALID, "aon_adam_step: n must be >= 0 and step >= 1 (the count AFTER this update, as torch.optim.Adam's state['step'])");
  if (n == 0) return AON_OK;
  if (!params || !grads || !exp_avg || !exp_avg_sq) return fail(AON_E_INVALID, "aon_adam_step: null pointer");
  if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0)) return fail(AON_E_INVALID, "aon_adam_step: bad hyper-parameter");
  return check(aon::launch_adam(params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, step, (hipStream_t)stream), "aon_adam_step");
}

static int code_library_call(bool backward, const float* const* src, const int64_t* const* ids, const int* rows, const int* dims, float* const* dst, void* stream,
                             const char* who) {
  if (!src || !ids || !rows || !dims || !dst) return fail(AON_E_INVALID, "aon_code_library: null array");
  for (int t = 0; t < 3; ++t)
    if (!src[t] || !ids[t] || !dst[t] || rows[t] < 1 || dims[t] < 1 || (int64_t)rows[t] * dims[t] > (1 << 28)) return fail(AON_E_INVALID, "aon_code_library: null pointer or bad table size");
  return check(aon::launch_code_library(backward, src, ids, rows, dims, dst, (hipStream_t)stream), who);
}
int aon_code_library_fwd(const float* const* tables_host, const int64_t* const* ids_host, const int* rows_host, const int* dims_host, float* const* out_host,
                         void* stream) {
  return code_library_call(false, tables_host, ids_host, rows_host, dims_host, out_host, stream, "aon_code_library_fwd");
}
int aon_code_library_bwd(const float* const* g_rows_host, const int64_t* const* ids_host, const int* rows_host, const int* dims_host, float* const* g_tables_host,
                         void* stream) {
  return code_library_call(true, g_rows_host, ids_host, rows_host, dims_host, g_tables_host, stream, "aon_code_library_bwd");
}

// ---- test-epoch SSIM (csrc/aon_metrics.hip) ----
static const char* ssim_sizes_ok(int n_images, const int* h_host, const int* w_host) {
  if (!h_host || !w_host) return "null size array";
  for (int i = 0; i < n_images; ++i)
    if (h_host[i] < 11 || w_host[i] < 11 || h_host[i] > 32768 || w_host[i] > 32768)
      return "every image needs 11 <= h, w <= 32768 (the 11 x 11 window is applied without padding)";
  return nullptr;
}
int64_t aon_ssim_workspace_bytes(int n_images, const int* h_host, const int* w_host) {
  if (n_images < 0) return fail(AON_E_INVALID, "aon_ssim_workspace_bytes: n_images < 0");
  if (n_images == 0) return 0;
  if (const char* msg = ssim_sizes_ok(n_images, h_host, w_host)) return fail(AON_E_INVALID, msg);
  return aon::ssim_workspace_bytes(n_images, h_host, w_host);
}
int aon_ssim(int n_images, const float* const* preds_host, const float* const* gts_host, const int* h_host, const int* w_host, void* workspace,
             int64_t workspace_bytes, float* out, void* stream) {
  if (n_images < 0) return fail(AON_E_INVALID, "aon_ssim: n_images < 0");
  if (n_images == 0) return AON_OK;
  if (!preds_host || !gts_host || !out || !workspace) return fail(AON_E_INVALID, "aon_ssim: null pointer");
  if (reinterpret_cast<uintptr_t>(workspace) & 7) return fail(AON_E_INVALID, "aon_ssim: workspace is not 8-byte aligned");
  for (int i = 0; i < n_images; ++i)
    if (!preds_host[i] || !gts_host[i]) return fail(AON_E_INVALID, "aon_ssim: null image pointer");
  if (const char* msg = ssim_sizes_ok(n_images, h_host, w_host)) return fail(AON_E_INVALID, msg);
  if (workspace_bytes < aon::ssim_workspace_bytes(n_images, h_host, w_host)) return fail(AON_E_WORKSPACE, "aon_ssim: workspace too small");
  return check(aon::launch_ssim(n_images, preds_host, gts_host, h_host, w_host, static_cast<double*>(workspace), out, (hipStream_t)stream), "aon_ssim");
}

// ---- mesh extraction: density on a grid (aon_mlp.hip, aon_mlp_art.hip) and marching cubes (aon_mesh.hip) ----
static const char* grid_args_bad(const int64_t* dims3_host, const float* lo3_host, const float* step3_host, int64_t g_begin, int64_t g_end, int act) {
  if (!dims3_host || !lo3_host || !step3_host) return "null grid argument";
  for (int a = 0; a < 3; ++a)
    if (dims3_host[a] < 1 || dims3_host[a] > (int64_t)1 << 24) return "every grid dimension must be in [1, 2^24] (its indices are exact in fp32)";
  if (dims3_host[0] > INT64_MAX / dims3_host[1] / dims3_host[2]) return "grid too large";
  const int64_t P = dims3_host[0] * dims3_host[1] * dims3_host[2];
  if (g_begin < 0 || g_end < g_begin || g_end > P) return "need 0 <= g_begin <= g_end <= nx * ny * nz";
  if (g_end - g_begin > (int64_t)INT32_MAX * 64) return "too many points for one call";
  if (act < 0 || act > 2) return "act must be 0 (raw), 1 (relu) or 2 (softplus(raw - 1))";
  return nullptr;
}
int aon_density_grid(const void* packed, const int64_t* dims3_host, const float* lo3_host, const float* step3_host, int64_t g_begin, int64_t g_end,
                     int act, float* out, void* stream) {
  if (const char* msg = grid_args_bad(dims3_host, lo3_host, step3_host, g_begin, g_end, act)) return fail(AON_E_INVALID, (std::string("aon_density_grid: ") + msg).c_str());
  if (g_end == g_begin) return AON_OK;
  if (!packed || !out) return fail(AON_E_INVALID, "aon_density_grid: null pointer");
  return check(aon::launch_density_grid(static_cast<const char*>(packed), dims3_host, lo3_host, step3_host, g_begin, g_end, act, out, (hipStream_t)stream),
               "aon_density_grid");
}
int aon_art_density_grid(const void* packed, const void* small, const int64_t* dims3_host, const float* lo3_host, const float* step3_host, int64_t g_begin,
                         int64_t g_end, int act, float* out, void* stream) {
  if (const char* msg = grid_args_bad(dims3_host, lo3_host, step3_host, g_begin, g_end, act)) return fail(AON_E_INVALID, (std::string("aon_art_density_grid: ") + msg).c_str());
  if (g_end == g_begin) return AON_OK;
  if (!packed || !small || !out) return fail(AON_E_INVALID, "aon_art_density_grid: null pointer");
  if (forms_differ(packed, small)) return fail(AON_E_INVALID, kFormsMsg);
  return check(aon::launch_art_density_grid(static_cast<const char*>(packed), static_cast<const float*>(small), dims3_host, lo3_host, step3_host, g_begin,
                                            g_end, act, out, (hipStream_t)stream), "aon_art_density_grid");
}
static const char* mc_dims_bad(const int64_t* dims3_host) {
  if (!dims3_host) return "null dims";
  for (int a = 0; a < 3; ++a)
    if (dims3_host[a] < 2 || dims3_host[a] > (int64_t)1 << 24) return "every grid dimension must be in [2, 2^24]";
  if (dims3_host[0] > ((int64_t)1 << 40) / dims3_host[1] / dims3_host[2]) return "grid too large (more than 2^40 points)";
  return nullptr;
}
int64_t aon_marching_cubes_workspace_bytes(const int64_t* dims3_host) {
  if (const char* msg = mc_dims_bad(dims3_host)) return fail(AON_E_INVALID, (std::string("aon_marching_cubes_workspace_bytes: ") + msg).c_str());
  return aon::mc_workspace_bytes(dims3_host);
}
int aon_marching_cubes_count(const float* grid, const int64_t* dims3_host, float level, void* workspace, int64_t workspace_bytes, int64_t* counts2_host,
                             void* stream) {
  if (const char* msg = mc_dims_bad(dims3_host)) return fail(AON_E_INVALID, (std::string("aon_marching_cubes_count: ") + msg).c_str());
  if (!grid || !workspace || !counts2_host) return fail(AON_E_INVALID, "aon_marching_cubes_count: null pointer");
  if (reinterpret_cast<uintptr_t>(workspace) & 15) return fail(AON_E_INVALID, "aon_marching_cubes_count: workspace is not 16-byte aligned");
  if (workspace_bytes < aon::mc_workspace_bytes(dims3_host)) return fail(AON_E_WORKSPACE, "aon_marching_cubes_count: workspace too small");
  if (int rc = check(aon::launch_mc_count(grid, dims3_host, level, workspace, (hipStream_t)stream, counts2_host), "aon_marching_cubes_count"); rc != AON_OK)
    return rc;
  if (counts2_host[0] > INT32_MAX)
    return fail(AON_E_INVALID, "aon_marching_cubes_count: more than 2^31 - 1 vertices (faces hold int32 vertex ids): use a coarser grid");
  return AON_OK;
}
int aon_marching_cubes(const float* grid, const int64_t* dims3_host, float level, const float* lo3_host, const float* step3_host, void* workspace,
                       int64_t workspace_bytes, float* verts, int64_t n_verts, int32_t* faces, int64_t n_faces, void* stream) {
  if (const char* msg = mc_dims_bad(dims3_host)) return fail(AON_E_INVALID, (std::string("aon_marching_cubes: ") + msg).c_str());
  if (!grid || !workspace || !lo3_host || !step3_host) return fail(AON_E_INVALID, "aon_marching_cubes: null pointer");
  if (n_verts < 0 || n_faces < 0 || n_verts > INT32_MAX) return fail(AON_E_INVALID, "aon_marching_cubes: bad output size");
  if ((n_verts > 0 && !verts) || (n_faces > 0 && !faces)) return fail(AON_E_INVALID, "aon_marching_cubes: null output");
  if (reinterpret_cast<uintptr_t>(workspace) & 15) return fail(AON_E_INVALID, "aon_marching_cubes: workspace is not 16-byte aligned");
  if (workspace_bytes < aon::mc_workspace_bytes(dims3_host)) return fail(AON_E_WORKSPACE, "aon_marching_cubes: workspace too small");
  return check(aon::launch_mc(grid, dims3_host, level, lo3_host, step3_host, workspace, verts, n_verts, faces, n_faces, (hipStream_t)stream),
               "aon_marching_cubes");
}

int aon_profile_begin(void) {
  std::lock_guard<std::mutex> lk(g_prof.mu);
  g_prof.on = true; g_prof.used = 0; g_prof.recs.clear();
  for (int c = 0; c < kNumClasses; ++c) g_prof.units[c] = 0;
  return AON_OK;
}

int aon_profile_end(double* mlp_ms, int64_t* mlp_launches, int64_t* mlp_samples) {
  std::lock_guard<std::mutex> lk(g_prof.mu);
  g_prof.on = false;
  for (int c = 0; c < kNumClasses; ++c) { g_prof.last_ms[c] = 0.0; g_prof.last_launches[c] = 0; g_prof.last_units[c] = g_prof.units[c]; }
  for (const auto& r : g_prof.recs) {
    hipError_t e = hipEventSynchronize(r.stop);
    if (e != hipSuccess) return check(e, "aon_profile_end");
    float ms = 0.f;
    e = hipEventElapsedTime(&ms, r.start, r.stop);
    if (e != hipSuccess) return check(e, "aon_profile_end");
    g_prof.last_ms[r.cls] += ms;
    g_prof.last_launches[r.cls] += 1;
  }
  if (mlp_ms) *mlp_ms = g_prof.last_ms[kMlpFwd];
  if (mlp_launches) *mlp_launches = g_prof.last_launches[kMlpFwd];
  if (mlp_samples) *mlp_samples = g_prof.last_units[kMlpFwd];
  g_prof.used = 0; g_prof.recs.clear();
  return AON_OK;
}

int aon_profile_class(int cls, double* ms, int64_t* launches, int64_t* units) {
  if (cls < 0 || cls >= kNumClasses) return fail(AON_E_INVALID, "aon_profile_class: unknown kernel class");
  std::lock_guard<std::mutex> lk(g_prof.mu);
  if (ms) *ms = g_prof.last_ms[cls];
  if (launches) *launches = g_prof.last_launches[cls];
  if (units) *units = g_prof.last_units[cls];
  return AON_OK;
}

int aon_set_bottleneck_fold(int on) {
  aon::set_fold_default(on);
  return AON_OK;
}
int aon_get_bottleneck_fold(void) { return aon::fold_default(); }
int aon_stream_is_folded(const void* packed) { return aon::stream_form(packed) == aon::kFormFolded ? 1 : 0; }
int aon_stream_form(const void* packed) { return aon::stream_form(packed); }
int aon_declare_stream_form(const void* packed, int form) {
  if (!packed || (form != aon::kFormLiteral && form != aon::kFormFolded)) return fail(AON_E_INVALID, "aon_declare_stream_form: null pointer or form not 0 / 1");
  aon::set_stream_form(packed, form);
  return AON_OK;
}

int aon_set_view_bias(int on) {
  g_view_bias.store(on ? 1 : 0, std::memory_order_relaxed);
  return AON_OK;
}

int aon_get_view_bias(void) { return g_view_bias.load(std::memory_order_relaxed); }

int aon_set_deferred_view(int on) {
  g_deferred_view.store(on ? 1 : 0, std::memory_order_relaxed);
  return AON_OK;
}

int aon_get_deferred_view(void) { return g_deferred_view.load(std::memory_order_relaxed); }

// ---- articulated network (model_autodecoder.py) ----
int64_t aon_art_packed_bytes(void) { return aon::art_stream_bytes(); }
int64_t aon_art_small_bytes(void) { return aon::art_small_bytes(); }

int aon_pack_art_mlp(const float* const* params_host, void* packed, void* stream) {
  return aon_pack_art_mlp_deg(params_host, 0, 10, 4, packed, stream);
}
int aon_pack_art_mlp_deg(const float* const* params_host, int min_deg_point, int max_deg_point, int deg_view, void* packed, void* stream) {
  if (const char* bad = art_degrees_ok(min_deg_point, max_deg_point, deg_view)) return fail(AON_E_INVALID, bad);
  if (!params_host || !packed) return fail(AON_E_INVALID, "aon_pack_art_mlp: null pointer");
  for (int i = 0; i < aon::kNumArtParams; ++i)
    if (!params_host[i]) return fail(AON_E_INVALID, "aon_pack_art_mlp: null parameter pointer");
  if (reinterpret_cast<uintptr_t>(packed) & 15) return fail(AON_E_INVALID, "aon_pack_art_mlp: packed must be 16-byte aligned");
  return check(aon::launch_pack_art(params_host, static_cast<float*>(packed), (hipStream_t)stream, max_deg_point - min_deg_point, deg_view),
               "aon_pack_art_mlp");
}

int aon_art_prepare(const float* const* params_host, const float* shape, const float* appearance, const float* articulation,
                    void* small, void* stream) {
  return aon_art_prepare_deg(params_host, shape, appearance, articulation, 0, 10, 4, small, stream);
}
int aon_art_prepare_deg(const float* const* params_host, const float* shape, const float* appearance, const float* articulation,
                        int min_deg_point, int max_deg_point, int deg_view, void* small, void* stream) {
  if (const char* bad = art_degrees_ok(min_deg_point, max_deg_point, deg_view)) return fail(AON_E_INVALID, bad);
  if (!params_host || !shape || !appearance || !articulation || !small) return fail(AON_E_INVALID, "aon_art_prepare: null pointer");
  for (int i = 0; i < aon::kNumArtParams; ++i)
    if (!params_host[i]) return fail(AON_E_INVALID, "aon_art_prepare: null parameter pointer");
  if (reinterpret_cast<uintptr_t>(small) & 15) return fail(AON_E_INVALID, "aon_art_prepare: small must be 16-byte aligned");
  return check(aon::launch_prepare_art(params_host, shape, appearance, articulation, static_cast<float*>(small), (hipStream_t)stream, min_deg_point,
                                       max_deg_point - min_deg_point, deg_view), "aon_art_prepare");
}

// Round 6: everything a training step of a TWO-level articulated model packs, in one call -- both networks' forward streams, per-call blocks
// and transposed streams -- with the four 128 x 256 x 256 fp64 products (W' of each network, once for its forward and once for its transposed
// stream) as ONE launch in front instead of four launches of 17 us each in a row with their pack kernels, then both networks' per-call blocks +
// forward streams as one launch and both transposed streams as another (the step's prologue: 174 -> 68 us, profiles/r06_step_timeline.txt).
// The same kernels on the same operands as the six separate calls: same bytes in every buffer.  packed_bwd_* may be NULL (no backward wanted).
int aon_art_pack_step(const float* const* params_coarse_host, const float* const* params_fine_host, const float* shape, const float* appearance,
                      const float* articulation, int min_deg_point, int max_deg_point, int deg_view, void* packed_coarse, void* small_coarse,
                      void* packed_bwd_coarse, void* packed_fine, void* small_fine, void* packed_bwd_fine, void* stream_) {
  if (const char* bad = art_degrees_ok(min_deg_point, max_deg_point, deg_view)) return fail(AON_E_INVALID, bad);
  if (!params_coarse_host || !params_fine_host || !shape || !appearance || !articulation || !packed_coarse || !small_coarse || !packed_fine || !small_fine)
    return fail(AON_E_INVALID, "aon_art_pack_step: null pointer");
  for (int i = 0; i < aon::kNumArtParams; ++i)
    if (!params_coarse_host[i] || !params_fine_host[i]) return fail(AON_E_INVALID, "aon_art_pack_step: null parameter pointer");
  for (const void* p : {(const void*)packed_coarse, (const void*)small_coarse, (const void*)packed_fine, (const void*)small_fine, (const void*)packed_bwd_coarse, (const void*)packed_bwd_fine})
    if (reinterpret_cast<uintptr_t>(p) & 15) return fail(AON_E_INVALID, "aon_art_pack_step: buffers must be 16-byte aligned");
  hipStream_t stream = (hipStream_t)stream_;
  const int Lp = max_deg_point - min_deg_point, Lv = deg_view;
  const float* const* P[2] = {params_coarse_host, params_fine_host};
  float* fwd[2] = {static_cast<float*>(packed_coarse), static_cast<float*>(packed_fine)};
  float* sm[2] = {static_cast<float*>(small_coarse), static_cast<float*>(small_fine)};
  float* bwd[2] = {static_cast<float*>(packed_bwd_coarse), static_cast<float*>(packed_bwd_fine)};
  const int form = aon::fold_default();   // read ONCE: the merged launches below are told, the single-buffer ones cope with either answer
  const bool folded = form == aon::kFormFolded;
  if (folded) {
    aon::FoldGemm jobs[4];
    int n = 0;
    for (int l = 0; l < 2; ++l) jobs[n++] = aon::art_fold_job_fwd(P[l], fwd[l], Lv);
    for (int l = 0; l < 2; ++l)
      if (bwd[l]) jobs[n++] = aon::art_fold_job_bwd(P[l], bwd[l], Lv);
    if (int rc = check(aon::launch_fold_gemms(jobs, n, stream), "aon_art_pack_step")) return rc;
  }
  if (int rc = check(aon::launch_pack_prepare_art2(P, shape, appearance, articulation, fwd, sm, stream, min_deg_point, Lp, Lv, form), "aon_art_pack_step")) return rc;
  if (bwd[0] && bwd[1]) return check(aon::launch_pack_art_bwd2(P, bwd, stream, Lp, Lv, form), "aon_art_pack_step");
  for (int l = 0; l < 2; ++l)   // only one transposed buffer given: its own pack launch
    if (bwd[l])
      if (int rc = check(aon::launch_pack_art_bwd(P[l], bwd[l], stream, Lp, Lv, folded), "aon_art_pack_step")) return rc;
  return AON_OK;
}

int aon_art_mlp_fwd(const void* packed, const void* small, const float* rays_o, const float* rays_d, const float* viewdirs,
                    const float* t_vals, int64_t n_rays, int S, float* raw, void* stream) {
  if (n_rays < 0 || S < 1) return fail(AON_E_INVALID, "aon_art_mlp_fwd: bad size");
  if (n_rays == 0) return AON_OK;
  if (!packed || !small || !rays_o || !rays_d || !viewdirs || !t_vals || !raw) return fail(AON_E_INVALID, "aon_art_mlp_fwd: null pointer");
  if (forms_differ(packed, small)) return fail(AON_E_INVALID, kFormsMsg);
  MlpTimer timer((hipStream_t)stream, n_rays * S);
  const aon::FwdSeg seg{.packed = static_cast<const char*>(packed), .small = static_cast<const float*>(small), .rays_o = rays_o, .rays_d = rays_d,
                        .viewdirs = viewdirs, .t_vals = t_vals, .n_rays = n_rays, .S = S, .raw = raw};
  return check(aon::launch_net_fwd(true, &seg, 1, (hipStream_t)stream), "aon_art_mlp_fwd");
}

int aon_art_mlp_fwd_pos(const void* packed, const void* small, const float* pos, const float* viewdirs_enc, int64_t n_rays, int S,
                        float* raw, void* stream) {
  if (n_rays < 0 || S < 1) return fail(AON_E_INVALID, "aon_art_mlp_fwd_pos: bad size");
  if (n_rays == 0) return AON_OK;
  if (!packed || !small || !pos || !viewdirs_enc || !raw) return fail(AON_E_INVALID, "aon_art_mlp_fwd_pos: null pointer");
  if (forms_differ(packed, small)) return fail(AON_E_INVALID, kFormsMsg);
  const aon::FwdSeg seg{.packed = static_cast<const char*>(packed), .small = static_cast<const float*>(small), .n_rays = n_rays, .S = S, .raw = raw,
                        .pos = pos, .viewdirs_enc = viewdirs_enc};
  return check(aon::launch_net_fwd(true, &seg, 1, (hipStream_t)stream), "aon_art_mlp_fwd_pos");
}

}  // extern "C"
