/* Extension header of the libaon_hip C ABI: occupancy grids for scenes -- the MLP stage of a scene level with every
 * sample in an empty cell of its object's grid skipped.
 *
 * A header of its own for the reason include/aon_hip_scene.h gives: that header, include/aon_hip.h and include/aon_hip_inputs.h are pinned
 * name for name by tables in the test suite.  The entry points declared here get the same discipline from their own tests
 * (tests/test_scene_occ_cpu.py, tests/test_hip_scene_occ.py) and are bound through a table of their own (_lib._SCENE_OCC_SIGS).  The library
 * exports them like every other symbol; the ABI version is unchanged (additive).
 */
#ifndef AON_HIP_SCENE_OCC_H
#define AON_HIP_SCENE_OCC_H

#include "aon_hip_scene.h"

#ifdef __cplusplus
extern "C" {
#endif

/* aon_scene_art_mlp_fwd_occ: aon_art_mlp_fwd on every object segment of the pair rows aon_scene_pairs laid out (object j's rows are
 * starts_host[j] .. starts_host[j + 1] - 1, its per-call block smalls_host[j]), with an optional occupancy grid per object, given in the
 * OBJECT's frame -- the frame of pair_o / pair_d and of the object's box.
 *
 * Sample i of pair row p lies at x = pair_o[p] + t_vals[p, i] * pair_d[p] (multiply, then add, each rounded: the MLP kernel's own bits) and
 * is looked up in its object's grid by the rule of aon_render_fwd_occ (include/aon_hip.h), operation for operation: cell
 * floor((x_a - lo_a) / step_a) per axis in fp32 with IEEE division, clamped to cells_a - 1; a coordinate outside [lo_a, lo_a + cells_a step_a]
 * or NaN is empty.  An empty sample's record is (0, 0, 0, -inf) -- zero density under the articulated activation, zero weight in
 * aon_scene_composite and aon_sample_pdf_n -- and the MLP never runs on it; every other record holds the bits aon_art_mlp_fwd writes.
 * An object whose grids_host entry is NULL is dense: the ordinary launch of aon_art_mlp_fwd on its segment.
 *
 * smalls_host / grids_host / starts_host: HOST arrays (k, k and k + 1 entries), read before the call returns, as are the aon_occupancy
 * records.  pair_o / pair_d / pair_v (pairs, 3), t_vals (pairs, s), raw (pairs, s, 4) with pairs = starts_host[k]; rows of raw from `pairs` on
 * are not written.  occupied_dev: device (k,) int64 or NULL; the samples of object j that ran through the MLP are ADDED to occupied_dev[j]
 * (a dense object adds all of its segment's samples), so the caller zeroes it where a frame begins.
 * workspace: device, aon_scene_occ_workspace_bytes(pairs, k, s) bytes (0 for arguments the call refuses), 256-byte aligned: the sample lists
 * (4 bytes per sample), tile counts and offsets (a tile is 1,024 samples of one object) and k counters, in 256-byte aligned pieces.  Of the
 * list of object j, at byte 4 * starts_host[j] * s, only the entries below its count are written.
 * Stream-ordered, no synchronisation: mark, one-workgroup scan and emit (three launches whatever k is, none when no object with rows has a
 * grid and occupied_dev is NULL), then one MLP launch per object with rows, whose pass count is read from device memory.  No atomics: the
 * same bits on every run.  starts_host[k] == 0: success, nothing launched, nothing written.
 * Refused before any launch, in this order:
 *   1. k outside [1, 16] or s < 1;
 *   2. starts_host NULL or not ascending from starts_host[0] = 0;
 *   3. starts_host[k] * s > 2^31 - 1;
 *   4. a null pointer: packed, smalls_host, grids_host, pair_o, pair_d, pair_v, t_vals, raw, workspace, or smalls_host[j] of an object with rows;
 *   5. a grid with null bits, a cell count outside [1, 2^24] (or more than 2^40 cells), lo or step not finite, step <= 0;
 *   6. raw not 16-byte aligned or the workspace not 256-byte aligned;
 *   7. packed and the block of an object with rows made in different forms (aon_set_bottleneck_fold), or one of them unknown
 *      (AON_E_INVALID each);
 *   8. a workspace that is too small (AON_E_WORKSPACE). */
int64_t aon_scene_occ_workspace_bytes(int64_t pairs, int k, int s);
int aon_scene_art_mlp_fwd_occ(const void* packed, const void* const* smalls_host, const aon_occupancy* const* grids_host,
                              const int64_t* starts_host, const float* pair_o, const float* pair_d, const float* pair_v, const float* t_vals,
                              int k, int s, float* raw, int64_t* occupied_dev, void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* AON_HIP_SCENE_OCC_H */
