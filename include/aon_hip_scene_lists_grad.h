/* Extension header of the libaon_hip C ABI: gradients through scenes with a backdrop -- the backward of the
 * per-list merged composite of include/aon_hip_scene_lists.h.
 *
 * A header of its own for the reason include/aon_hip_scene.h gives: the earlier headers are pinned name for name by tables in the test
 * suite.  The entry point declared here gets the same discipline from its own tests (tests/test_scene_lists_grad_cpu.py,
 * tests/test_hip_scene_lists_grad.py) and is bound through a table of its own (_lib._SCENE_LISTS_GRAD_SIGS).  The library exports it like
 * every other symbol; the ABI version is unchanged (additive).  aon_scene_composite_bwd and its kernel are untouched: this is a second
 * kernel beside it (csrc/aon_scene_lists_grad.hip), and every scene without a backdrop keeps its code path and bits.
 */
#ifndef AON_HIP_SCENE_LISTS_GRAD_H
#define AON_HIP_SCENE_LISTS_GRAD_H

#include "aon_hip_scene_lists.h"

#ifdef __cplusplus
extern "C" {
#endif

/* aon_scene_composite_lists_bwd: the backward of aon_scene_composite_lists on the same raw (pairs, s, 4), t_vals (pairs, s), slot (n, k),
 * rays_d (n, 3), white_bkgd and lists_host (k records, a HOST array read before the call returns).  It is aon_scene_composite_bwd
 * (include/aon_hip_scene_grad.h) with the record of a sample's list deciding two things:
 *   the activation and its derivative: act 0 / 1 / 2 with the list's own rgb_scale, rgb_shift, sigma_bias, xs = fl(raw + sigma_bias) in
 *     fp32 and the softplus threshold 20, as aon_composite_bwd takes them;
 *   the last interval: delta_{s-1} = 0, or with open_end the forward's 1e10f N as the forward forms it: N = sqrt((x x + y y) + z z), then
 *     the product, each rounded on its own in fp32.
 * Everything else is aon_scene_composite_bwd's contract, word for word.  Upstream gradients g_rgb (n, 3), g_acc (n,), g_depth (n,),
 * g_obj_acc (n, k) indexed by the list; the last three may each be NULL, meaning zero.  Over the samples of ray r's live lists in
 * ascending (t, list, i), rank j:
 *   f_j = 1 - alpha_j + 1e-10,  T_j = prod_{m<j} f_m,  w_j = alpha_j T_j
 *   gw_j = g_rgb . c_j + g_acc - [white_bkgd] sum(g_rgb) + t_j g_depth + g_obj_acc[r, list of j]
 *   dL/dalpha_j = T_j gw_j - Sfx_j / f_j,  Sfx_j = sum_{m>j} w_m gw_m
 *   d raw_sigma = dL/dalpha . delta exp(-sigma delta) . sigma'(raw),  d raw_c = w g_rgb_c . c'(raw_c)
 * Evaluated in fp64 on the fp32 inputs (delta, the norm and raw + sigma_bias in fp32, as the forward forms them) and rounded to fp32 once
 * per output; both scans in a fixed rank order, no atomics: the same bits on every run, and a ray's rows depend on its own lists only.
 * A factor that is exactly zero (w, or d alpha / d raw_sigma) gives +0: the last sample of a CLOSED list and a sentinel record
 * (0, 0, 0, -inf) get exact zeros.  The last sample of an OPEN list gets a real gradient: its colour entries are w g_rgb c', its density
 * entry is +0 wherever exp(-sigma 1e10 N) underflows to 0 or sigma' = 0, and the finite value of the formula otherwise (up to about
 * 1e10 |gw|: it fits fp32).  With k closed lists of one act and one set of scalars every bit of d_raw is aon_scene_composite_bwd's.
 * d_raw (pairs, s, 4): the rows of the pairs that `slot` names are written, every other row is left alone (zero the buffer first where the
 * rest is read).  A slot entry outside [0, pairs) is dead, as in the forward.
 * One launch on `stream`, one wavefront per ray; n == 0 or pairs == 0: success without a launch.
 * Refused before any launch, in this order: sizes (n < 0, pairs < 0, k outside [1, 16], s < 2, k * s > 4096); a null pointer (raw, t_vals,
 * slot, rays_d, g_rgb, lists_host, d_raw); a record with act outside [0, 2] or open_end outside {0, 1}; raw, then d_raw, not 16-byte
 * aligned (AON_E_INVALID each). */
int aon_scene_composite_lists_bwd(const float* raw, const float* t_vals, const int32_t* slot, const float* rays_d, const float* g_rgb,
                                  const float* g_acc, const float* g_depth, const float* g_obj_acc, int64_t n, int k, int64_t pairs, int s,
                                  int white_bkgd, const aon_scene_list* lists_host, float* d_raw, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* AON_HIP_SCENE_LISTS_GRAD_H */
