/* Extension header of the libaon_hip C ABI: scenes of several posed articulated objects in one frame.
 *
 * A header of its own for the reason include/aon_hip_inputs.h gives: include/aon_hip.h and include/aon_hip_inputs.h are pinned name for name
 * by tables in the test suite.  The entry points declared here get the same discipline from their own tests (tests/test_scene_cpu.py,
 * tests/test_hip_scene.py) and are bound through a table of their own (_lib._SCENE_SIGS).  The library exports them like every other symbol;
 * the ABI version is unchanged (additive).
 *
 * The two per-ray stages around the unchanged stage calls (aon_sample_along_rays_bounds, aon_art_mlp_fwd, aon_sample_pdf_n):
 *   aon_scene_pairs      pairs every world ray with the objects whose box it crosses and compacts the pairs, so that the samplers and the
 *                        MLP run on object-frame rays only where a ray meets an object;
 *   aon_scene_composite  merges the per-object sample lists of a ray by distance and composites them.
 * Inference only.  No atomics anywhere: every output is the same bits on every run, and a ray's outputs depend on its own pairs only.
 */
#ifndef AON_HIP_SCENE_H
#define AON_HIP_SCENE_H

#include "aon_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AON_SCENE_MAX_OBJECTS 16      /* K */
#define AON_SCENE_MAX_MERGED 4096     /* K * S: the merged list of one ray lives in 14 bytes of LDS per sample (56 KiB at the limit) */

/* One placed object: the rigid object-to-world pose x_world = R x_object + centre (no scale: a ray's parameter t is the same distance in
 * every frame) and the axis-aligned box [lo, hi] in the OBJECT's frame. */
typedef struct aon_scene_object {
  float rot[9];      /* R, row-major, orthonormal with det > 0 (the caller's to check: the library does not) */
  float centre[3];   /* the box frame's origin in world coordinates */
  float lo[3];
  float hi[3];
} aon_scene_object;

/* aon_scene_pairs: for world ray r and object k the object-frame ray is o' = R^T (o - c), d' = R^T d, v' = R^T v, component a evaluated in
 * fp32 as ((R[0][a] * (o_0 - c_0)) + R[1][a] * (o_1 - c_1)) + R[2][a] * (o_2 - c_2): separately rounded subtractions, multiplications and
 * additions in that order (d', v': the same without the subtraction).  near / far are aon_ray_limits_box's slab test, operation by
 * operation, on (o', d') and the object's box; the pair is LIVE iff raw far > near and, with negatives clamped to 0, still far > near (the
 * rule of aon_ray_limits' `live`, without its set-wide patching: a dead pair does not exist).
 * Live pairs are stored object-major (all of object 0's, then object 1's ...), inside an object by ascending ray index, without padding
 * between objects:
 *   offsets   (k + 1,) int64, device: object j's pairs are rows offsets[j] .. offsets[j + 1] - 1; offsets[k] = P, the number of pairs
 *   slot      (n, k) int32: the row of pair (r, j), or -1
 *   pair_ray  (P,) int32: the world ray of a row;  pair_o / pair_d / pair_v (P, 3);  pair_near / pair_far (P,), clamped
 * The per-pair arrays have the caller's capacity n * k rows; rows from P on are not written.  (The stage calls the rows feed ask no alignment
 * of a segment's first row, so there is none.)
 * objects_host: HOST array of k records, read before the call returns.  workspace: device, aon_scene_pairs_workspace_bytes(n, k) bytes,
 * 256-byte aligned.  Three launches on `stream` (classify, one-workgroup scan, emit); no synchronisation.  n == 0: success, offsets zeroed.
 * Refused before any launch, in this order: sizes (n < 0, k outside [1, 16], n * k > 2^31 - 1); a null pointer; a misaligned workspace
 * (AON_E_INVALID each); a workspace that is too small (AON_E_WORKSPACE). */
int64_t aon_scene_pairs_workspace_bytes(int64_t n, int k);
int aon_scene_pairs(const float* rays_o, const float* rays_d, const float* viewdirs, int64_t n, const aon_scene_object* objects_host, int k,
                    void* workspace, int64_t workspace_bytes, int64_t* offsets, int32_t* slot, int32_t* pair_ray, float* pair_o, float* pair_d,
                    float* pair_v, float* pair_near, float* pair_far, void* stream);

/* aon_scene_composite: raw (pairs, s, 4) records of the MLP entry points and t_vals (pairs, s), rows as aon_scene_pairs laid them out.  Per
 * live pair of ray r (N = |rays_d[r]|, the WORLD direction): sigma_i, rgb_i by `act` / `opts` as aon_composite_ex (no density noise),
 * delta_i = (t_{i+1} - t_i) N for i < s - 1 and delta_{s-1} = 0 (a list ends where its box ends), alpha_i = 1 - exp(-sigma_i delta_i).  All
 * samples of the ray's live lists in ascending order of the key (t, object, i): T_1 = 1, T_{j+1} = T_j (1 - alpha_j + 1e-10),
 * w_j = alpha_j T_j;  rgb = sum w_j rgb_j (+ 1 - acc with white_bkgd), acc = sum w_j, depth = sum w_j t_j,
 * obj_acc[r, k] = sum over object k's samples of w_j, weights[p, i] = w of that sample (both nullable).  A ray without a live pair gets the
 * background: rgb 1 or 0, acc = depth = obj_acc = 0.  rgb (n, 3), acc / depth (n,), obj_acc (n, k), weights (pairs, s).
 * One launch on `stream`, one wavefront per ray.  pairs == 0: raw / t_vals may be NULL and every ray gets the background.
 * Refused before any launch, in this order: sizes (n < 0, pairs < 0, k outside [1, 16], s < 2, k * s > 4096, act outside [0, 2]); a null
 * pointer; raw not 16-byte aligned (AON_E_INVALID each). */
int aon_scene_composite(const float* raw, const float* t_vals, const int32_t* slot, const float* rays_d, int64_t n, int k, int64_t pairs,
                        int s, int white_bkgd, int act, const aon_render_opts* opts, float* rgb, float* acc, float* depth, float* obj_acc,
                        float* weights, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* AON_HIP_SCENE_H */
