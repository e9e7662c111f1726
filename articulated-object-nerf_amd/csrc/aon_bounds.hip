// Per-ray near / far from a ray-box intersection (tests/_bounds_ref.py is an independent numpy copy):
// helper.get_ray_limits_box (helper.py:42-102) for a general axis-aligned box, and the fix-up of helper.get_ray_limits (helper.py:29-39)
// without the reference's host round trip (`torch.any(...).item()`).
//
//   ray_box_kernel           one thread per ray: 24 B read, 8 B written; per block the min(near) / max(far) over its VALID rays
//                            (far > near on the raw values; a NaN compares false) as one partial each, when the caller wants them;
//   ray_limits_reduce_kernel ONE block turns the partials into the set's min(near) / max(far) (min / max do not depend on order: the
//                            same bits on every run; 8 B per 256 rays read once, whatever the ray count);
//   ray_limits_finish_kernel patches its invalid rays with those two values when there is a valid ray at all, clamps negatives to 0
//                            and writes the optional `live` byte: the ray was valid AND far > near after the clamp.  (A box wholly behind the camera
//                            is "valid" to the reference and comes out as near = far = 0: not live.)
//
// Arithmetic, operation by operation as torch evaluates the reference on fp32 tensors: inv = 1 / d is one IEEE division; sign = inv < 0
// (d = -0.0 -> inv = -inf -> sign 1); t = (bound - o) * inv is a rounded subtraction, then a rounded multiplication (0 * inf = NaN when the
// origin lies on a face the ray is parallel to); the two rejections are the reference's comparisons (false for a NaN); torch.max / torch.min
// propagate NaN (fmaxf / fminf do not).  Equal operands (zeros of either sign) yield the first, as std::max / std::min do.
#include "aon_launch.h"

namespace aon {

constexpr int kBoxThreads = 256;

// (torch_max / torch_min: aon_common.h, shared with the scene pairs)

struct Box {
  float lo[3], hi[3];
};

// min / max of a block's values; every thread of the block calls it.  red: 2 * kBoxThreads / 64 floats
__device__ __forceinline__ void block_min_max(float& mn, float& mx, float* red) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    mn = __builtin_fminf(mn, __shfl_xor(mn, d));   // (no NaN gets here: only valid rays contribute)
    mx = __builtin_fmaxf(mx, __shfl_xor(mx, d));
  }
  constexpr int kWaves = kBoxThreads / 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { red[wave] = mn; red[kWaves + wave] = mx; }
  __syncthreads();
  mn = red[0]; mx = red[kWaves];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) {
    mn = __builtin_fminf(mn, red[w]);
    mx = __builtin_fmaxf(mx, red[kWaves + w]);
  }
}

__global__ __launch_bounds__(kBoxThreads) void ray_box_kernel(const float* __restrict__ rays_o, const float* __restrict__ rays_d, int64_t n, Box box,
                                                              float* __restrict__ near, float* __restrict__ far, float* __restrict__ part_min,
                                                              float* __restrict__ part_max) {
  __shared__ float red[2 * kBoxThreads / 64];
  const int64_t ray = (int64_t)blockIdx.x * kBoxThreads + threadIdx.x;
  float mn = __builtin_huge_valf(), mx = -__builtin_huge_valf();
  if (ray < n) {
    float t0[3], t1[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float o = rays_o[ray * 3 + a];
      const float inv = __fdiv_rn(1.0f, rays_d[ray * 3 + a]);
      const bool neg = inv < 0.f;
      t0[a] = __fmul_rn(__fsub_rn(neg ? box.hi[a] : box.lo[a], o), inv);
      t1[a] = __fmul_rn(__fsub_rn(neg ? box.lo[a] : box.hi[a], o), inv);
    }
    bool valid = !(t0[0] > t1[1] || t0[1] > t1[0]);
    float tmin = torch_max(t0[0], t0[1]), tmax = torch_min(t1[0], t1[1]);
    if (tmin > t1[2] || t0[2] > tmax) valid = false;
    tmin = torch_max(tmin, t0[2]);
    tmax = torch_min(tmax, t1[2]);
    if (!valid) { tmin = -1.0f; tmax = -2.0f; }
    near[ray] = tmin;
    far[ray] = tmax;
    if (tmax > tmin) { mn = tmin; mx = tmax; }
  }
  if (part_min) {   // (uniform over the grid)
    block_min_max(mn, mx, red);
    if (threadIdx.x == 0) { part_min[blockIdx.x] = mn; part_max[blockIdx.x] = mx; }
  }
}

// one block: set[0] = min over the partial minima, set[1] = max over the partial maxima (+inf / -inf when no ray is valid)
__global__ __launch_bounds__(kBoxThreads) void ray_limits_reduce_kernel(const float* __restrict__ part_min, const float* __restrict__ part_max,
                                                                        int64_t nparts, float* __restrict__ set) {
  __shared__ float red[2 * kBoxThreads / 64];
  float mn = __builtin_huge_valf(), mx = -__builtin_huge_valf();
  for (int64_t p = threadIdx.x; p < nparts; p += kBoxThreads) {
    mn = __builtin_fminf(mn, part_min[p]);
    mx = __builtin_fmaxf(mx, part_max[p]);
  }
  block_min_max(mn, mx, red);
  if (threadIdx.x == 0) { set[0] = mn; set[1] = mx; }
}

__global__ __launch_bounds__(kBoxThreads) void ray_limits_finish_kernel(float* __restrict__ near, float* __restrict__ far, uint8_t* __restrict__ live,
                                                                        int64_t n, const float* __restrict__ set) {
  const float mn = set[0], mx = set[1];
  const bool any = mx > mn;   // a valid ray has far > near, so max(far) > min(near); no valid ray: -inf > inf is false
  const int64_t ray = (int64_t)blockIdx.x * kBoxThreads + threadIdx.x;
  if (ray >= n) return;
  float a = near[ray], b = far[ray];
  const bool valid = b > a;
  if (!valid && any) { a = mn; b = mx; }
  if (a < 0.f) a = 0.f;
  if (b < 0.f) b = 0.f;
  near[ray] = a;
  far[ray] = b;
  if (live) live[ray] = (valid && b > a) ? 1 : 0;
}

int64_t ray_limits_workspace_bytes(int64_t n) {   // the set's min / max, then the two partial arrays, one float per block of rays each
  const int64_t blocks = (n + kBoxThreads - 1) / kBoxThreads;
  return 256 + (blocks * 4 + 255) / 256 * 256 * 2;
}

// ws == nullptr: the raw (-1, -2) form alone (helper.get_ray_limits_box); else the fixed-up form (helper.get_ray_limits) and `live`
hipError_t launch_ray_limits(const float* rays_o, const float* rays_d, int64_t n, const float* lo3, const float* hi3, float* near, float* far,
                             uint8_t* live, char* ws, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  Box box;
  for (int a = 0; a < 3; ++a) { box.lo[a] = lo3[a]; box.hi[a] = hi3[a]; }
  const int64_t blocks = (n + kBoxThreads - 1) / kBoxThreads;
  float* set = reinterpret_cast<float*>(ws);
  float* pmin = ws ? reinterpret_cast<float*>(ws + 256) : nullptr;
  float* pmax = ws ? reinterpret_cast<float*>(ws + 256 + (blocks * 4 + 255) / 256 * 256) : nullptr;
  ray_box_kernel<<<dim3((unsigned)blocks), dim3(kBoxThreads), 0, stream>>>(rays_o, rays_d, n, box, near, far, pmin, pmax);
  if (hipError_t e = hipGetLastError(); e != hipSuccess || !ws) return e;
  ray_limits_reduce_kernel<<<dim3(1), dim3(kBoxThreads), 0, stream>>>(pmin, pmax, blocks, set);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  ray_limits_finish_kernel<<<dim3((unsigned)blocks), dim3(kBoxThreads), 0, stream>>>(near, far, live, n, set);
  return hipGetLastError();
}

}  // namespace aon
