/* Extension header of the libaon_hip C ABI: gradients of a scene with respect to its objects' poses.
 *
 * A header of its own for the reason include/aon_hip_scene.h gives: the five existing headers are pinned name for name by tables in the
 * test suite.  The entry points declared here get the same discipline from their own tests (tests/test_scene_pose_cpu.py,
 * tests/test_hip_scene_pose.py) and are bound through a table of their own (_lib._SCENE_POSE_SIGS).  The library exports them like every
 * other symbol; the ABI version is unchanged (additive).
 *
 * Object k of a scene sees a world ray (o, d, v) as o' = R^T (o - c), d' = R^T d, v' = R^T v (aon_scene_pairs).  The backward chain of a
 * segment (aon_art_bwd_chain) leaves behind what the gradients with respect to (o', d', v') need:
 *   aon_art_ray_grads     turns the chain's outputs of ONE level of ONE block of rays into dL/d rays_o, dL/d rays_d, dL/d viewdirs;
 *   aon_scene_pose_grads  reduces the per-pair gradients of a scene to dL/d [R | c] of every object.
 * t, slot, the pairs' existence, near / far and the WORLD direction's norm are data.  A rigid R preserves |d|, and aon_scene_composite takes
 * its interval lengths from the world direction: the object-frame direction has no norm term here.
 */
#ifndef AON_HIP_SCENE_POSE_H
#define AON_HIP_SCENE_POSE_H

#include "aon_hip_scene_grad.h"

#ifdef __cplusplus
extern "C" {
#endif

/* aon_art_ray_grads: the ray gradients of a FROZEN articulated network at one level of one block of n_rays rays of s samples, from the
 * outputs of aon_art_bwd_chain on that block: dplanes (the gradient planes, np padded samples, step-major) and dxp (np, 4).  params: HOST
 * array of the level's 40 device pointers in the order of aon_pack_art_mlp (entries 0, deformations_linear.0.weight (128, 163), and 26,
 * views_linear.0.weight (128, 256 + V + 128), V = 3 + 6 deg_view, are read).  t_vals (n_rays, s), viewdirs (n_rays, 3): the block's own.
 * Per sample i of ray r, sample index r * s + i of the planes:
 *   g_x_i = dxp_i + W_d0[:, 0:3]^T dZ_d0,i    (per component ONE fp32 fmaf chain from 0 over the 128 features in ascending order, then one
 *                                              fp32 add of dxp_i), and the V view-encoding partials W_v0[:, 256 : 256 + V]^T dZ_v0,i likewise
 *   g_rays_o[r] = sum_i g_x_i        g_rays_d[r] = sum_i t_i g_x_i        (fp64, ascending i, rounded to fp32 once)
 *   g_viewdirs[r] = the summed partials (fp64, ascending i) pulled back through pos_enc(viewdirs, 0, deg_view) at the forward's rounded
 *                   arguments, in ascending column order, rounded to fp32 once.
 * g_rays_d is sum_i t_i g_x_i ALONE: where |d| scales the compositing's interval lengths (aon_composite, one object's own ray) the norm
 * term g_n d / |d| is the caller's to add (aon_art_render_bwd_inputs does); in a scene it does not exist.
 * g_rays_o, g_rays_d, g_viewdirs (n_rays, 3): overwritten.  records: device scratch of aon_art_ray_grads_record_bytes(n_rays, s) bytes
 * (128 per sample; -1 for n_rays < 0, s < 1 or more than 2^31 - 1 samples), overwritten.
 * Two launches on `stream` (per sample, then one wavefront per ray); no atomics, the same bits on every run, and a ray's three rows depend
 * on its own samples only.  s has no upper limit.  n_rays == 0: success without a launch, whatever the pointers.
 * Refused before any launch, in this order: sizes (n_rays < 0, s < 1, np < 0, deg_view outside [0, 4], n_rays * s > 2^31 - 1); then, with
 * n_rays > 0, a null pointer (dplanes, dxp, params, params[0], params[26], t_vals, viewdirs, records, an output); n_rays * s > np
 * (AON_E_INVALID each); record_bytes too small (AON_E_WORKSPACE); dplanes, then dxp, then records not 16-byte aligned (AON_E_INVALID). */
int64_t aon_art_ray_grads_record_bytes(int64_t n_rays, int s);
int aon_art_ray_grads(const float* dplanes, const float* dxp, const void* const* params, const float* t_vals, const float* viewdirs,
                      int64_t n_rays, int s, int64_t np, int deg_view, void* records, int64_t record_bytes, float* g_rays_o, float* g_rays_d,
                      float* g_viewdirs, void* stream);

/* aon_scene_pose_grads: rays_o / rays_d / viewdirs (n, 3) the WORLD rays, pair_ray (pairs,) and offsets (k + 1,) (device) as
 * aon_scene_pairs wrote them, objects_host the HOST array of k records that call took (read before this one returns), g_o / g_d / g_v
 * (pairs, 3) the gradients with respect to the pairs' object-frame origin, direction and view direction (aon_art_ray_grads on every
 * segment).  With (o, d, v) the world ray of pair p and s_i = fl(o_i - c_i), the fp32 subtraction the forward forms:
 *   g_R[i][a] = sum_p ( s_i g_o[p][a] + d_i g_d[p][a] + v_i g_v[p][a] )        g_c[i] = - sum_a R[i][a] sum_p g_o[p][a]
 * the plain derivative with respect to the 12 entries of [R | c]: no tangent-space projection.
 * g_pose (k, 12): row j = [g_R (9, row-major) | g_c (3)] of object j, overwritten; an object without pairs gets twelve exact zeros.
 * Order: fp64 throughout, every product of two fp32 values exact.  One workgroup of 256 threads per object, whatever `pairs` is.  With
 * q = p - offsets[j] the pair's position in its segment, thread q mod 256 adds the pair's term ((s_i g_o + d_i g_d) + v_i g_v) to its own
 * sum in ascending q; the 256 sums are then folded by a fixed tree (sum[u] += sum[u + h] for h = 128, 64, ... 1); g_c is formed from the
 * three folded sums of g_o in ascending a; every output is rounded to fp32 once.  No atomics: an object's row is a function of its own
 * pairs' rows only, the same bits on every run.  A segment is clamped to [0, pairs] and a pair whose ray lies outside [0, n) adds nothing.
 * One launch on `stream`.  pairs == 0: pair_ray, g_o, g_d, g_v and the rays may be NULL, and zeros are written.
 * Refused before any launch, in this order: sizes (n < 0, pairs < 0, k outside [1, 16]); a null pointer (offsets, objects_host, g_pose;
 * with pairs > 0 every other one too) (AON_E_INVALID each). */
int aon_scene_pose_grads(const float* rays_o, const float* rays_d, const float* viewdirs, int64_t n, const int32_t* pair_ray,
                         const int64_t* offsets, const aon_scene_object* objects_host, int k, int64_t pairs, const float* g_o, const float* g_d,
                         const float* g_v, float* g_pose, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* AON_HIP_SCENE_POSE_H */
