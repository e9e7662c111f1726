/* Extension header of the libaon_hip C ABI: the merged composite of a scene whose sample lists each carry their own activation and end
 * rule -- what a vanilla NeRF standing behind the articulated objects as the static backdrop needs.
 *
 * A header of its own for the reason include/aon_hip_scene.h gives: the earlier headers are pinned name for name by tables in the test
 * suite.  The entry point declared here gets the same discipline from its own tests (tests/test_scene_lists_cpu.py,
 * tests/test_hip_scene_lists.py) and is bound through a table of its own (_lib._SCENE_LISTS_SIGS).  The library exports it like every other
 * symbol; the ABI version is unchanged (additive).  Inference only.  aon_scene_composite and its kernel are untouched: this is a second
 * kernel beside it (csrc/aon_scene_lists.hip).
 */
#ifndef AON_HIP_SCENE_LISTS_H
#define AON_HIP_SCENE_LISTS_H

#include "aon_hip_scene.h"

#ifdef __cplusplus
extern "C" {
#endif

/* How the samples of ONE list (one column of slot) are read. */
typedef struct aon_scene_list {
  int   act;         /* 0 none, 1 vanilla (relu, sigmoid), 2 articulated (softplus(raw + sigma_bias), sigmoid * rgb_scale - rgb_shift) */
  float rgb_scale, rgb_shift, sigma_bias;   /* read for act 2 only */
  int   open_end;    /* 0: delta_{S-1} = 0 (a list ends where its box ends); 1: delta_{S-1} = 1e10 * N (helper.py:163-167) */
} aon_scene_list;

/* aon_scene_composite_lists: aon_scene_composite (include/aon_hip_scene.h) with `act` / `opts` replaced by one record per list.  raw
 * (pairs, s, 4) and t_vals (pairs, s) in the rows slot (n, k) names; per live list j of ray r (N = |rays_d[r]|, the WORLD direction) and
 * with lists_host[j]: sigma_i and rgb_i by that record's act and scalars, delta_i = (t_{i+1} - t_i) N for i < s - 1 and
 * delta_{s-1} = 0 or, with open_end, 1e10 N; alpha_i = 1 - exp(-sigma_i delta_i).  The open interval is formed in fp32 the way the
 * one-object composite forms it: N = sqrt((x x + y y) + z z), then (1e10f * N), then sigma * that product, each operation rounded on its
 * own, in that order; the closed intervals are ((t_{i+1} - t_i) * N), then sigma * that.  So an open list is opaque from its last
 * sample on wherever that sample has density, also when samples of other lists lie behind it: those get T <= 1e-10 of the formula.
 * Everything else is aon_scene_composite's contract, word for word: all samples of the ray's live lists in ascending order of the key
 * (t, list, i): T_1 = 1, T_{j+1} = T_j (1 - alpha_j + 1e-10), w_j = alpha_j T_j;  rgb = sum w_j rgb_j (+ 1 - acc with white_bkgd),
 * acc = sum w_j, depth = sum w_j t_j, obj_acc[r, j] = sum over list j's samples of w, weights[p, i] = w of that sample (both nullable).
 * A ray without a live list gets the background colour: rgb 1 or 0, acc = depth = obj_acc = 0.  rgb (n, 3), acc / depth (n,),
 * obj_acc (n, k), weights (pairs, s).  With k lists of act a, one set of scalars and open_end = 0, every output is bit for bit
 * aon_scene_composite's with that act and those opts.
 * lists_host: HOST array of k records, read before the call returns (they travel by value in the kernel arguments).
 * One launch on `stream`, one wavefront per ray, no atomics.  pairs == 0: raw / t_vals may be NULL and every ray gets the background.
 * Refused before any launch, in this order: sizes (n < 0, pairs < 0, k outside [1, 16], s < 2, k * s > 4096); a null pointer
 * (lists_host included); a record with act outside [0, 2] or open_end outside {0, 1}; raw not 16-byte aligned (AON_E_INVALID each). */
int aon_scene_composite_lists(const float* raw, const float* t_vals, const int32_t* slot, const float* rays_d, int64_t n, int k,
                              int64_t pairs, int s, int white_bkgd, const aon_scene_list* lists_host, float* rgb, float* acc, float* depth,
                              float* obj_acc, float* weights, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* AON_HIP_SCENE_LISTS_H */
