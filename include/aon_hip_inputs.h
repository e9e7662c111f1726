/* Extension header of the libaon_hip C ABI: the ray gradients of a FROZEN vanilla network.
 *
 * Why a header of its own: include/aon_hip.h is pinned by tables in the test suite (every entry point that takes a stream is a guard-band
 * case of tests/test_hip_extents.py, every backward is a row of tests/test_bwd_call_cpu.py, every declared name is bound by the Python
 * package's main signature table).  Entry points added here get the same discipline from their own tests
 * (tests/test_vanilla_ray_grads_cpu.py, tests/test_hip_vanilla_ray_grads.py) and are bound through a table of their own
 * (_lib._EXT_SIGS).  The library exports them like every other symbol; the ABI version is unchanged (additive).
 */
#ifndef AON_HIP_INPUTS_H
#define AON_HIP_INPUTS_H

#include "aon_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* dL/d rays_o, dL/d rays_d and dL/d viewdirs, (n_rays, 3) fp32 each, overwritten, summed over the levels, of the training loss behind
 * aon_render_fwd_train* -- the network's parameters get NO gradient (a camera pose refined against a trained NeRF).  The call is
 * aon_render_bwd_ex without its weight-gradient stage: compositing backward and backward chain as there (same gradient planes), then two
 * ordinary launches on `stream`.  The sample positions are x_i = rays_o + t_i rays_d with t as DATA (coarse t depends on near / far only,
 * the fine t is detached by the reference); per-ray near / far get no gradient.  g_rays_d also carries the term through |rays_d| in the
 * compositing's interval lengths.
 * params_*_host: HOST arrays of the 24 DEVICE pointers of aon_pack_vanilla_mlp's order; entries 0, 10 and 16 (pts_linears.0.weight,
 * pts_linears.5.weight, views_linear.0.weight: the weights an encoding enters through) are read in their own nn.Linear layouts, the others
 * may be NULL.  rg: every member non-NULL; rg->rays_o and rg->viewdirs are the forward's.  opts: the forward's (every degree set
 * aon_render_fwd_train_ex accepts is served).
 * AON_E_INVALID before any launch: rg or a member of it NULL, a NULL level pointer or entry 0 / 10 / 16, forward and transposed streams
 * packed in different forms, and everything aon_render_bwd_ex refuses of the common arguments.  AON_E_WORKSPACE: workspace smaller than
 * aon_train_workspace_bytes_ex(), scratch smaller than aon_train_scratch_bytes_inputs_vanilla() (d_raw, gradient planes and one 128-byte
 * record per sample of the levels in use; no weight-gradient workspace).
 * Every sum over a ray's samples is fp64 in a fixed order (no atomics): a ray's gradients are the same bits on every run and do not depend
 * on which other rays share the call. */
int64_t aon_train_scratch_bytes_inputs_vanilla(int64_t n_rays, int num_levels, const aon_render_opts* opts);
int aon_render_bwd_inputs(const void* packed_bwd_coarse, const void* packed_fwd_coarse, const void* packed_bwd_fine,
                          const void* packed_fwd_fine, const float* rays_d, int64_t n_rays, int white_bkgd, int num_levels,
                          const float* const* g_rgb_host, const float* const* g_acc_host, const float* const* g_depth_host,
                          const float* const* params_coarse_host, const float* const* params_fine_host, void* workspace,
                          int64_t workspace_bytes, void* scratch, int64_t scratch_bytes, void* stream, const aon_render_opts* opts,
                          const aon_ray_grads* rg);

#ifdef __cplusplus
}
#endif

#endif /* AON_HIP_INPUTS_H */
