// The library's internal launch interface: the ONE declaration, with its default arguments, of every aon:: host function that is called from
// another translation unit, and the small structs and constants that cross translation units.  Declarations (and the two one-line network
// dispatchers) only -- no kernels.  Every file
// that defines one of these functions includes this header, so a definition that disagrees with its declaration does not compile.
// (The fold products and the layer-wise engine keep their own headers: aon_fold.h, aon_gmlp.h.)
#pragma once
#include "aon_common.h"
#include "aon_fold.h"

struct aon_scene_list;   // include/aon_hip_scene_lists.h

namespace aon {

// ---- aon_mlp.hip: the vanilla network's packs, forward kernels and density grid ----
int num_cus();   // CUs of the CURRENT device, cached per device ordinal
hipError_t launch_pack_vanilla(const float* const* params, float* packed, hipStream_t stream, int pos_levels = 10, int view_levels = 4, bool fold_done = false);
void vanilla_fold_jobs_fwd(const float* const* params, float* packed, int view_levels, FoldGemm jobs[2]);
// the one fused forward launch, inference and training: one or two segments, the kernel instance read off what they hold (FwdSeg, aon_common.h)
hipError_t launch_mlp_fwd(const FwdSeg* segs, int nsegs, hipStream_t stream);
// the view layer + rgb head of the samples a deferred trunk (a segment with live_rows) listed
hipError_t launch_view_deferred(const char* packed, const float* live_rows, const int* idx, const int64_t* count, int64_t max_listed,
                                const float* view_bias, int S, float* raw, hipStream_t stream);
hipError_t launch_view_bias(const char* packed, const float* viewdirs, int64_t n_rays, float* out, hipStream_t stream);
hipError_t launch_view_bias_raw(const float* chunk, const float* bias_vec, const float* viewdirs, int64_t n_rays, float* out, hipStream_t stream);
hipError_t launch_density_grid(const char* packed, const int64_t* dims, const float* lo, const float* step, int64_t g_begin, int64_t g_end,
                               int act, float* out, hipStream_t stream);

// ---- aon_mlp_art.hip: the articulated network's packs, per-call block, forward kernels and density grid ----
int64_t art_stream_bytes();
int64_t art_small_bytes();
hipError_t launch_pack_art(const float* const* params, float* packed, hipStream_t stream, int pos_levels = 10, int view_levels = 4, bool fold_done = false);
FoldGemm art_fold_job_fwd(const float* const* params, float* packed, int view_levels);
hipError_t launch_prepare_art(const float* const* params, const float* shape, const float* app, const float* art,
                              float* small, hipStream_t stream, int min_deg = 0, int pos_levels = 10, int view_levels = 4);
hipError_t launch_pack_prepare_art2(const float* const* const params[2], const float* shape, const float* app, const float* art, float* const packed[2],
                                    float* const small[2], hipStream_t stream, int min_deg, int pos_levels, int view_levels, int form);
hipError_t launch_art_mlp_fwd(const FwdSeg* segs, int nsegs, hipStream_t stream);
hipError_t launch_art_view_bias(const char* packed, const float* small, const float* viewdirs, int64_t n_rays, float* out, hipStream_t stream);
hipError_t launch_art_density_grid(const char* packed, const float* small, const int64_t* dims, const float* lo, const float* step,
                                   int64_t g_begin, int64_t g_end, int act, float* out, hipStream_t stream);

// ---- the single place where the network of a forward launch is chosen (small: the articulated per-call block, null for the vanilla network) ----
inline hipError_t launch_net_fwd(bool art, const FwdSeg* segs, int nsegs, hipStream_t stream) {
  return art ? launch_art_mlp_fwd(segs, nsegs, stream) : launch_mlp_fwd(segs, nsegs, stream);
}
inline hipError_t launch_net_view_bias(bool art, const char* packed, const float* small, const float* viewdirs, int64_t n_rays, float* out, hipStream_t stream) {
  return art ? launch_art_view_bias(packed, small, viewdirs, n_rays, out, stream) : launch_view_bias(packed, viewdirs, n_rays, out, stream);
}

// ---- the weight-gradient stage shared by aon_train.hip and aon_train_art.hip (kernels and plan types: aon_wgrad.h) ----
struct WgLayerDesc;
struct HeadDesc;
struct HeadOut;
struct ReduceArgs;

// An optional side stream for the head reductions of a level (with its fork / join events): they are HBM-bound plane-row sums
// with a small register / LDS footprint, so their workgroups fit next to the weight-gradient workgroups (384 of the 512 registers
// per SIMD, 144 of the 160 KB of LDS) and run in their shadow instead of behind them.  Null: everything on one stream.
struct WgAux {
  hipStream_t stream;
  hipEvent_t fork, join;
};

enum : int { kWgAll = 0, kWgEarly = 1, kWgRest = 2 };   // phases of a level's weight-gradient call (run_wgrad_plan)

// A level's second stage handed back instead of launched (launch_*_wgrad_post2 serves both levels): opaque to the C ABI layer, which keeps
// two of each in storage of these sizes on its stack.  The static_asserts sit at the structs (aon_train.hip, aon_train_art.hip).
struct VanillaWgDeferred;
struct ArtWgDeferred;
constexpr int kVanillaWgDeferredBytes = 4096;
constexpr int kArtWgDeferredBytes = 4096;

// ---- aon_train.hip: composite backward, the vanilla network's transposed pack, backward chain and weight gradients ----
hipError_t launch_composite_bwd(const float* raw, const float* t_vals, const float* dirs, const float* g_rgb, const float* g_acc,
                                const float* g_depth, int64_t n_rays, int S, int white_bkgd, const ActParams& ap, float* d_raw,
                                hipStream_t stream);
void vanilla_fold_jobs_bwd(const float* const* params, float* packed, int view_size, FoldGemm jobs[2]);
hipError_t launch_pack_vanilla_bwd(const float* const* params, float* packed, hipStream_t stream, int pos_size = 63, int view_size = 27, bool fold_done = false);
int64_t bwd_stream_bytes();
hipError_t launch_mlp_bwd_chain(const char* packed_bwd, const char* packed_fwd, const float* d_raw, const void* masks,
                                float* dplanes, int64_t Np, hipStream_t stream);
hipError_t launch_mlp_bwd_chain2(const ChainSeg* segs, int nsegs, hipStream_t stream);
int64_t wgrad_workspace_bytes();
float* wgrad_fold_tmp(float* ws);
void set_wgrad_probe(long long* buf);
// wait_first: an event the level's second stage waits for before it starts (the early head reductions a side stream ran beside the chain)
hipError_t run_wgrad_plan(const WgLayerDesc* layers, int nlayers, const HeadDesc* heads, int nheads, const HeadOut* outs, const int* out_head, int nouts,
                          const float* planes, const float* dplanes, int rows_total, int64_t Np, float* ws, hipStream_t stream, const WgAux* aux,
                          int phase, int n_early, hipEvent_t wait_first, ReduceArgs* defer_reduce, int* defer_blocks);
hipError_t launch_wgrad_reduce2(const ReduceArgs& a0, int n0, const ReduceArgs& a1, int n1, hipStream_t stream);
hipError_t launch_wgrad_kind_bench(int kind, int nlayers, const float* planes, const float* dplanes, int rows_total, int64_t Np, float* ws,
                                   float* out_scratch, hipStream_t stream);
hipError_t launch_vanilla_wgrad(const float* planes, const float* dplanes, const float* d_raw, int64_t Np, float* const* grads,
                                float* ws, hipStream_t stream, const WgAux* aux, const void* packed_bwd, int phase = kWgAll, hipEvent_t wait_first = nullptr,
                                VanillaWgDeferred* defer = nullptr);
hipError_t launch_vanilla_wgrad_post2(const VanillaWgDeferred* d0, const VanillaWgDeferred* d1, hipStream_t stream);
int vanilla_wgrad_deferred_bytes();
int wgrad_plan_describe(bool art, int64_t Np, int cus, int32_t* out6, int max_jobs, int64_t* ws_bytes);
int wgrad_plan_segment(bool art, int64_t Np, int cus, int j, int wg, int32_t* begin_end);

// ---- aon_train_art.hip: the articulated network's transposed pack, backward chain and weight gradients ----
FoldGemm art_fold_job_bwd(const float* const* params, float* packed, int view_levels);
hipError_t launch_pack_art_bwd(const float* const* params, float* packed, hipStream_t stream, int pos_levels = 10, int view_levels = 4, bool fold_done = false);
hipError_t launch_pack_art_bwd2(const float* const* const params[2], float* const packed[2], hipStream_t stream, int pos_levels, int view_levels, int form);
int64_t art_bwd_stream_bytes();
hipError_t launch_art_bwd_chain(const char* packed_bwd, const float* small, const float* d_raw, const void* masks, const float* planes,
                                float* dplanes, float* dxp, int64_t Np, hipStream_t stream);
hipError_t launch_art_bwd_chain2(const ChainSeg* segs, int nsegs, hipStream_t stream);
int art_wgrad_layers(float* const* grads, WgLayerDesc* L, int Lp, int Lv, float* enc_tmp, float* fold_tmp);
hipError_t launch_art_wgrad(const float* planes, const float* dplanes, const float* d_raw, const float* dxp, int64_t Np,
                            const float* const* params, const float* shape, const float* app, const float* art,
                            float* const* grads, float* g_shape, float* g_app, float* g_art, float* ws, hipStream_t stream, const WgAux* aux, int pos_levels, int view_levels,
                            const void* packed_bwd, int phase = kWgAll, bool accumulate_latents = false, ArtWgDeferred* defer = nullptr);
hipError_t launch_art_wgrad_post2(const ArtWgDeferred* d0, const ArtWgDeferred* d1, hipStream_t stream);
int art_wgrad_deferred_bytes();

// ---- aon_train_latent.hip: the latent gradients of a frozen articulated network from the chain's gradient planes (no weight gradient) ----
struct ArtLatentLevel {
  const float* dplanes;          // the level's gradient planes, written by the backward chain
  int64_t Np;
  const void* packed_bwd;        // the transposed stream that chain ran with (its form decides the level's layer list)
  const float* const* params;    // the level's kNumArtParams parameters; read: the weights a latent enters (art_latent_entry, aon_params.h)
  float* ws;                     // art_latent_ws_bytes() of partial sums
};
int64_t art_latent_ws_bytes();
hipError_t launch_art_latent_grads(const ArtLatentLevel* levels, int nlevels, int pos_levels, int view_levels, float* g_shape, float* g_app, float* g_art,
                                   hipStream_t stream);

// ---- aon_ray_grad.hip: dL/d rays_o, rays_d, viewdirs of a frozen network from the chain's outputs (DESIGN.md sections 4.14, 4.15) ----
struct RayGradLevel {
  const float* dplanes;          // the level's gradient planes, written by the backward chain
  const float* dxp;              // [articulated] (Np,4): d x' per sample, written by the same launch; [vanilla] null: x is rebuilt from rays_o, rays_d and t
  int64_t Np;
  // the level's parameters (aon_params.h); read: [articulated] deformations_linear.0.weight, views_linear.0.weight;
  // [vanilla] pts_linears.0.weight, pts_linears.5.weight, views_linear.0.weight
  const float* const* params;
  float* rec;                    // ray_grad_record_bytes(n_rays * S) of per-sample records
  const float* t;                // (n_rays, S)
  const float* raw;              // (n_rays * S, 4), as the forward wrote it
  const float* g_rgb; const float* g_acc; const float* g_depth;   // upstream gradients of the level (g_acc / g_depth: or null)
  ActParams ap;
  int S;
};
int64_t ray_grad_record_bytes(int64_t n_samples);
hipError_t launch_ray_grads(const RayGradLevel* levels, int nlevels, int64_t n_rays, int view_levels, int white_bkgd, const float* rays_d,
                            const float* viewdirs, float* g_rays_o, float* g_rays_d, float* g_viewdirs, hipStream_t stream);
hipError_t launch_vanilla_ray_grads(const RayGradLevel* levels, int nlevels, int64_t n_rays, int min_deg, int pos_levels, int view_levels,
                                    int white_bkgd, const float* rays_o, const float* rays_d, const float* viewdirs, float* g_rays_o,
                                    float* g_rays_d, float* g_viewdirs, hipStream_t stream);
// one level of one block of rays, g_rays_d without the norm term: Wd0 / Wv0 the storages of
// deformations_linear.0.weight / views_linear.0.weight, rec ray_grad_record_bytes(n_rays * S)
hipError_t launch_art_ray_grads(const float* dplanes, const float* dxp, const float* Wd0, const float* Wv0, const float* t_vals,
                                const float* viewdirs, int64_t n_rays, int S, int view_levels, float* rec, float* g_rays_o, float* g_rays_d,
                                float* g_viewdirs, hipStream_t stream);

// ---- aon_render.hip: rays, sampling, encodings, compositing, the training loss ----
hipError_t launch_raygen(const float* c2w, int H, int W, float focal, const float* directions, int64_t pix_begin,
                         int64_t pix_end, float* rays_o, float* viewdirs, float* rays_d, hipStream_t stream);
hipError_t launch_ray_directions(int H, int W, float focal, float* out, hipStream_t stream);
hipError_t launch_ray_radii(const float* directions, const float* c2w, int H, int W, float* radii, hipStream_t stream);
hipError_t launch_cast_rays(const float* t_vals, const float* o, const float* d, int64_t n_rays, int S, float* coords,
                            hipStream_t stream);
hipError_t launch_sample_along_rays(const float* rays_o, const float* rays_d, int64_t n_rays, int S, float near, float far,
                                    const float* t_rand, float* t_vals, float* coords, hipStream_t stream, int lindisp = 0,
                                    float inv_near = 0.f, float inv_far = 0.f, const float* near_ray = nullptr, const float* far_ray = nullptr);
hipError_t launch_pos_enc(const float* x, int64_t n, int min_deg, int max_deg, float* out, hipStream_t stream, int ld = 0, int levels_out = 0);
hipError_t launch_composite(const float* rgb, int rgb_stride, const float* sigma, int sigma_stride, const float* t_vals,
                            const float* dirs, int64_t n_rays, int S, int white_bkgd, const ActParams& ap, float* comp_rgb,
                            float* acc, float* depth, float* weights, hipStream_t stream);
hipError_t launch_sample_pdf(const float* bins, const float* weights, int64_t w_stride, const float* t_coarse,
                             const float* u, int64_t u_stride, int64_t n_rays, float* samples, float* t_fine,
                             hipStream_t stream);
hipError_t launch_composite_pdf(const float* raw, const float* t_coarse, const float* dirs, int64_t n_rays, int white_bkgd, const ActParams& ap,
                                const float* u, int64_t u_stride, float* comp_rgb, float* acc, float* depth, float* weights,
                                float* t_fine, hipStream_t stream);
hipError_t launch_sample_pdf_n(const float* bins, const float* weights, int64_t w_stride, const float* t_coarse, const float* u,
                               int64_t u_stride, int64_t n_rays, int nb, int nf, int nt, float* samples, float* t_fine, hipStream_t stream);
int64_t sample_pdf_n_lds_bytes(int nb, int nf, int nt, int* P_out);
hipError_t launch_train_loss(bool backward, const float* rgb_c, const float* rgb_f, const float* target, int64_t n, const float* const* lat, const int* lat_len,
                             float reg_scale, float* stats, float* loss, const float* go, float* d_rgb_c, float* d_rgb_f, float* const* d_lat, hipStream_t stream);

// ---- aon_optim.hip ----
hipError_t launch_adam(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2, double eps, int64_t step, hipStream_t stream);
hipError_t launch_code_library(bool backward, const float* const* src, const int64_t* const* idx, const int* rows, const int* dim, float* const* dst, hipStream_t stream);

// ---- aon_metrics.hip ----
int64_t ssim_workspace_bytes(int n, const int* h, const int* w);
hipError_t launch_ssim(int n, const float* const* x, const float* const* y, const int* h, const int* w, double* part, float* out, hipStream_t stream);

// ---- aon_mesh.hip ----
int64_t mc_workspace_bytes(const int64_t* dims);
hipError_t launch_mc_count(const float* grid, const int64_t* dims, float level, void* ws, hipStream_t stream, int64_t* counts2_host);
hipError_t launch_mc(const float* grid, const int64_t* dims, float level, const float* lo, const float* step, void* ws, float* verts, int64_t vcap,
                     int* faces, int64_t fcap, hipStream_t stream);

// ---- aon_occ.hip ----
hipError_t launch_occ_build(const float* dens, const int64_t* dims, float thr, int dilate, uint32_t* bits, hipStream_t stream);
// One compaction (mark / scan / emit) of K segments of rows, each against its own grid, over the sample window [s0, s1) of every row.
struct OccCompact {
  const OccGrid* grids;      // K records; bits == nullptr: no grid (every cell occupied)
  const int64_t* starts;     // K + 1 segment starts in rows; starts[K] * S <= INT32_MAX
  int K, S, s0, s1;          // [0, S): a whole level
  const float* rays_o; const float* rays_d; const float* t_vals;   // (rows,3), (rows,3), (rows,S)
  const uint8_t* ray_live;   // (rows,) or null: a dead ray's samples get the sentinel record and are not listed
  const int* stop;           // (rows,) or null: so do the samples i >= stop[row] (occ_stop_state().stop)
};
// A segment without a grid, with ray_live and stop null, is DENSE: not touched, its count all of its samples.  ws: 256-byte aligned, as
// occ_list_bytes / scene_occ_list_bytes size it, tile_cap the tile capacity that function used (ceil(total / 1024) / scene_occ_tile_cap)
// -> idx (segment k's ascending list of segment-local sample indices row_local * S + i at idx + starts[k] * S) and counts (K int64: the
// lists' lengths, the device counters of the gather launches), which are also added to tally[k] when tally is given
int64_t occ_list_bytes(int64_t total);
int64_t scene_occ_tile_cap(int64_t pairs, int K, int S);
int64_t scene_occ_list_bytes(int64_t pairs, int K, int S);
hipError_t launch_occ_compact(const OccCompact& c, float* raw, char* ws, int64_t tile_cap, int64_t* tally, const int** idx_out,
                              const int64_t** counts_out, hipStream_t stream);
// early termination: the per-ray state of a level, tau (fp32) then stop (int32), each padded to 256 bytes (state == nullptr: both null)
struct OccStopState { float* tau; int* stop; };
int64_t occ_stop_state_bytes(int64_t n);
OccStopState occ_stop_state(char* state, int64_t n);
hipError_t launch_occ_stop_init(char* state, int64_t n, int S, hipStream_t stream);
hipError_t launch_occ_stop_store(char* state, int value, int* dst, int64_t n, int stride, hipStream_t stream);
hipError_t launch_occ_tally_set(int64_t* tally, int64_t v0, int64_t v1, hipStream_t stream);
hipError_t launch_occ_depth(const float* raw, const float* t_vals, const float* dirs, int64_t n, int S, int s0, int s1, const ActParams& ap,
                            float tau_stop, char* state, hipStream_t stream);

// ---- aon_bounds.hip: per-ray near / far from a ray-box intersection ----
int64_t ray_limits_workspace_bytes(int64_t n);
hipError_t launch_ray_limits(const float* rays_o, const float* rays_d, int64_t n, const float* lo3, const float* hi3, float* near, float* far,
                             uint8_t* live, char* ws, hipStream_t stream);

// ---- aon_scene_grad.hip: the backward of the merged scene composite ----
int64_t scene_composite_bwd_wave_bytes(int K, int S);   // LDS of one wavefront (= one ray)
hipError_t launch_scene_composite_bwd(const float* raw, const float* t_vals, const int32_t* slot, const float* dirs, const float* g_rgb,
                                      const float* g_acc, const float* g_depth, const float* g_obj_acc, int64_t n, int K, int64_t pairs, int S,
                                      int white_bkgd, const ActParams& ap, float* d_raw, hipStream_t stream);

// ---- aon_scene_lists_grad.hip: the backward of the per-list merged composite ----
int64_t scene_composite_lists_bwd_wave_bytes(int K, int S);   // LDS of one wavefront (= one ray)
hipError_t launch_scene_composite_lists_bwd(const float* raw, const float* t_vals, const int32_t* slot, const float* dirs, const float* g_rgb,
                                            const float* g_acc, const float* g_depth, const float* g_obj_acc, int64_t n, int K, int64_t pairs,
                                            int S, int white_bkgd, const aon_scene_list* lists_host, float* d_raw, hipStream_t stream);

}  // namespace aon
