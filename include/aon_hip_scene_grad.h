/* Extension header of the libaon_hip C ABI: gradients through scenes.
 *
 * A header of its own for the reason include/aon_hip_scene.h gives: the four existing headers are pinned name for name by tables in the
 * test suite.  The entry point declared here gets the same discipline from its own tests (tests/test_scene_grad_cpu.py,
 * tests/test_hip_scene_grad.py) and is bound through a table of its own (_lib._SCENE_GRAD_SIGS).  The library exports it like every other
 * symbol; the ABI version is unchanged (additive).
 *
 * The one stage of a scene that had no backward is the merged composite.  Every stage around it (aon_art_mlp_fwd_train, aon_art_bwd_chain,
 * aon_art_wgrad) works on an arbitrary block of rays, and a scene's per-object pair segment is such a block: with this call the gradients of
 * a scene's outputs reach every object's codes and the network weights.  t, slot and the world direction's norm are data: no gradient
 * reaches them (no pose gradients).
 */
#ifndef AON_HIP_SCENE_GRAD_H
#define AON_HIP_SCENE_GRAD_H

#include "aon_hip_scene.h"

#ifdef __cplusplus
extern "C" {
#endif

/* aon_scene_composite_bwd: the backward of aon_scene_composite on the same raw (pairs, s, 4), t_vals (pairs, s), slot (n, k), rays_d (n, 3),
 * white_bkgd, act and opts.  Upstream gradients g_rgb (n, 3), g_acc (n,), g_depth (n,), g_obj_acc (n, k); the last three may each be NULL,
 * meaning zero.  With the forward's names, over the samples of ray r's live lists in ascending (t, object, i), rank j:
 *   f_j = 1 - alpha_j + 1e-10,  T_j = prod_{m<j} f_m,  w_j = alpha_j T_j
 *   gw_j = g_rgb . c_j + g_acc - [white_bkgd] sum(g_rgb) + t_j g_depth + g_obj_acc[r, object of j]
 *   dL/dalpha_j = T_j gw_j - Sfx_j / f_j,  Sfx_j = sum_{m>j} w_m gw_m
 *   d raw_sigma = dL/dalpha . delta exp(-sigma delta) . sigma'(raw),  d raw_c = w g_rgb_c . c'(raw_c)
 * the activations and their derivatives as aon_composite_bwd takes them for `act`.  Evaluated in fp64 on the fp32 inputs (delta, the norm
 * and raw + sigma_bias in fp32, as the forward forms them) and rounded to fp32 once per output; both scans in a fixed order, no atomics: the
 * same bits on every run, and a ray's rows depend on its own pairs only.  The last sample of every list (delta = 0) and a sentinel record
 * (0, 0, 0, -inf) get exact zeros.
 * d_raw (pairs, s, 4): the rows of the pairs that `slot` names are written, every other row is left alone (zero the buffer first where the
 * rest is read).  A slot entry outside [0, pairs) is dead, as in the forward.
 * One launch on `stream`, one wavefront per ray; n == 0 or pairs == 0: success without a launch.
 * Refused before any launch, in this order: sizes (n < 0, pairs < 0, k outside [1, 16], s < 2, k * s > 4096, act outside [0, 2]); a null
 * pointer (raw, t_vals, slot, rays_d, g_rgb, d_raw); raw, then d_raw, not 16-byte aligned (AON_E_INVALID each). */
int aon_scene_composite_bwd(const float* raw, const float* t_vals, const int32_t* slot, const float* rays_d, const float* g_rgb,
                            const float* g_acc, const float* g_depth, const float* g_obj_acc, int64_t n, int k, int64_t pairs, int s,
                            int white_bkgd, int act, const aon_render_opts* opts, float* d_raw, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* AON_HIP_SCENE_GRAD_H */
