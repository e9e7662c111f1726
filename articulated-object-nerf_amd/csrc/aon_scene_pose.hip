// Gradients of a scene with respect to its objects' poses (include/aon_hip_scene_pose.h is the contract and
// tests/_scene_pose_ref.py an independent torch fp64 restatement).
//
//   aon_art_ray_grads      the C entry of aon_ray_grad.hip's stage-level launcher: ray_grad_sample_kernel on one segment, then the reduce
//                          without the norm term.
//   scene_pose_grad_kernel one workgroup of 256 threads per object.  Thread u walks the object's pairs q = u, u + 256, ... in ascending
//                          order and adds the pair's term to twelve fp64 sums of its own -- the nine entries of g_R and the three sums of
//                          g_o' -- which a fixed tree through LDS (24 KiB) then folds.  The launch geometry does not depend on the number of
//                          pairs, so the order of every sum is a function of the pair's position in its segment alone; no atomics.
//                          The fp64 rate does not matter here: a pair is 30 multiply-adds against 76 bytes read, and a frame has a few
//                          thousand pairs per object.
#include "../../include/aon_hip_scene_pose.h"
#include "aon_capi_util.h"
#include "aon_scene_merge.h"

using namespace aon::capi;

namespace aon {
namespace {

constexpr int kPoseThreads = 256;
constexpr int kPoseSums = 12;   // g_R (9, row-major), then sum_p g_o' (3)

struct ScenePoseObjects {   // by value in the kernel arguments, as aon_scene.hip's SceneObjects: nothing for the host to keep alive
  float rot[kMaxObj][9];
  float centre[kMaxObj][3];
};

struct ScenePoseArgs {
  const float* rays_o; const float* rays_d; const float* viewdirs;
  const int32_t* pair_ray; const int64_t* offsets;
  const float* g_o; const float* g_d; const float* g_v;
  float* g_pose;
  int64_t n, pairs;
  ScenePoseObjects objs;
};

__global__ __launch_bounds__(kPoseThreads) void scene_pose_grad_kernel(ScenePoseArgs a) {
  __shared__ double part[kPoseSums][kPoseThreads];
  const int k = (int)blockIdx.x, u = (int)threadIdx.x;
  int64_t begin = a.offsets[k], end = a.offsets[k + 1];
  begin = begin < 0 ? 0 : (begin > a.pairs ? a.pairs : begin);
  end = end < begin ? begin : (end > a.pairs ? a.pairs : end);
  const float c0 = a.objs.centre[k][0], c1 = a.objs.centre[k][1], c2 = a.objs.centre[k][2];
  double sum[kPoseSums];
#pragma unroll
  for (int j = 0; j < kPoseSums; ++j) sum[j] = 0.0;
  for (int64_t p = begin + u; p < end; p += kPoseThreads) {
    const int64_t ray = a.pair_ray[p];
    if (ray < 0 || ray >= a.n) continue;
    const double s[3] = {(double)__fsub_rn(a.rays_o[ray * 3], c0), (double)__fsub_rn(a.rays_o[ray * 3 + 1], c1),
                         (double)__fsub_rn(a.rays_o[ray * 3 + 2], c2)};
    const double d[3] = {(double)a.rays_d[ray * 3], (double)a.rays_d[ray * 3 + 1], (double)a.rays_d[ray * 3 + 2]};
    const double v[3] = {(double)a.viewdirs[ray * 3], (double)a.viewdirs[ray * 3 + 1], (double)a.viewdirs[ray * 3 + 2]};
    const double go[3] = {(double)a.g_o[p * 3], (double)a.g_o[p * 3 + 1], (double)a.g_o[p * 3 + 2]};
    const double gd[3] = {(double)a.g_d[p * 3], (double)a.g_d[p * 3 + 1], (double)a.g_d[p * 3 + 2]};
    const double gv[3] = {(double)a.g_v[p * 3], (double)a.g_v[p * 3 + 1], (double)a.g_v[p * 3 + 2]};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int b = 0; b < 3; ++b) sum[3 * i + b] += (s[i] * go[b] + d[i] * gd[b]) + v[i] * gv[b];
    }
#pragma unroll
    for (int b = 0; b < 3; ++b) sum[9 + b] += go[b];
  }
#pragma unroll
  for (int j = 0; j < kPoseSums; ++j) part[j][u] = sum[j];
  __syncthreads();
  for (int h = kPoseThreads / 2; h > 0; h >>= 1) {
    if (u < h) {
#pragma unroll
      for (int j = 0; j < kPoseSums; ++j) part[j][u] += part[j][u + h];
    }
    __syncthreads();
  }
  if (u < 9) {
    a.g_pose[(int64_t)k * 12 + u] = (float)part[u][0];
  } else if (u < 12) {
    const int i = u - 9;
    double acc = 0.0;
#pragma unroll
    for (int b = 0; b < 3; ++b) acc += (double)a.objs.rot[k][3 * i + b] * part[9 + b][0];
    a.g_pose[(int64_t)k * 12 + u] = (float)(-acc);
  }
}

}  // namespace
}  // namespace aon

extern "C" {

int64_t aon_art_ray_grads_record_bytes(int64_t n_rays, int s) {
  if (n_rays < 0 || s < 1 || n_rays > INT32_MAX / (int64_t)s) return -1;
  return aon::ray_grad_record_bytes(n_rays * s);
}

int aon_art_ray_grads(const float* dplanes, const float* dxp, const void* const* params, const float* t_vals, const float* viewdirs,
                      int64_t n_rays, int s, int64_t np, int deg_view, void* records, int64_t record_bytes, float* g_rays_o, float* g_rays_d,
                      float* g_viewdirs, void* stream) {
  if (n_rays < 0 || s < 1 || np < 0 || deg_view < 0 || deg_view > 4 || n_rays > INT32_MAX / (int64_t)s)
    return fail(AON_E_INVALID, "aon_art_ray_grads: bad size / view degree (s >= 1, 0 <= deg_view <= 4, n_rays * s <= 2^31 - 1)");
  if (n_rays == 0) return AON_OK;
  if (!dplanes || !dxp || !params || !params[aon::ap_deform_w(0)] || !params[aon::ap_view_w(0)] || !t_vals || !viewdirs || !records || !g_rays_o || !g_rays_d || !g_viewdirs)
    return fail(AON_E_INVALID, "aon_art_ray_grads: null pointer");
  if (n_rays * s > np) return fail(AON_E_INVALID, "aon_art_ray_grads: n_rays * s exceeds the planes' np samples");
  if (record_bytes < aon::ray_grad_record_bytes(n_rays * s)) return fail(AON_E_WORKSPACE, "aon_art_ray_grads: record scratch too small");
  if (reinterpret_cast<uintptr_t>(dplanes) & 15) return fail(AON_E_INVALID, "aon_art_ray_grads: dplanes must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(dxp) & 15) return fail(AON_E_INVALID, "aon_art_ray_grads: dxp must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(records) & 15) return fail(AON_E_INVALID, "aon_art_ray_grads: records must be 16-byte aligned");
  return check(aon::launch_art_ray_grads(dplanes, dxp, static_cast<const float*>(params[aon::ap_deform_w(0)]), static_cast<const float*>(params[aon::ap_view_w(0)]), t_vals, viewdirs,
                                         n_rays, s, deg_view, static_cast<float*>(records), g_rays_o, g_rays_d, g_viewdirs,
                                         static_cast<hipStream_t>(stream)), "aon_art_ray_grads");
}

int aon_scene_pose_grads(const float* rays_o, const float* rays_d, const float* viewdirs, int64_t n, const int32_t* pair_ray,
                         const int64_t* offsets, const aon_scene_object* objects_host, int k, int64_t pairs, const float* g_o, const float* g_d,
                         const float* g_v, float* g_pose, void* stream) {
  if (n < 0 || pairs < 0 || k < 1 || k > AON_SCENE_MAX_OBJECTS)
    return fail(AON_E_INVALID, "aon_scene_pose_grads: bad size / object count (1 <= k <= 16)");
  if (!offsets || !objects_host || !g_pose || (pairs > 0 && (!rays_o || !rays_d || !viewdirs || !pair_ray || !g_o || !g_d || !g_v)))
    return fail(AON_E_INVALID, "aon_scene_pose_grads: null pointer");
  aon::ScenePoseArgs a{rays_o, rays_d, viewdirs, pair_ray, offsets, g_o, g_d, g_v, g_pose, n, pairs, {}};
  for (int j = 0; j < k; ++j) {
    std::memcpy(a.objs.rot[j], objects_host[j].rot, sizeof(float) * 9);
    std::memcpy(a.objs.centre[j], objects_host[j].centre, sizeof(float) * 3);
  }
  aon::scene_pose_grad_kernel<<<dim3((unsigned)k), dim3(aon::kPoseThreads), 0, static_cast<hipStream_t>(stream)>>>(a);
  return check(hipGetLastError(), "aon_scene_pose_grads");
}

}  // extern "C"
