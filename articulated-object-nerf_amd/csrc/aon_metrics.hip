// Test-epoch image metrics: SSIM over a list of images of mixed sizes in two launches.  The reference: LitModel.ssim_each / .ssim
// (models/interface.py:102-111, :142-157), which run piqa's SSIM() with its defaults on each (pred, gt) pair clipped to [0,1]:
//   11-tap Gaussian window, sigma = 1.5 (weights exp(-(i-5)^2 / (2 sigma^2)), normalised to sum 1), "valid" filtering (no padding:
//   an (h-10) x (w-10) map per channel), c1 = 0.01^2, c2 = 0.03^2 (value range 1), and the uncentred statistics
//     mu = G(x), sigma_xx = G(x^2) - mu_x^2, sigma_xy = G(xy) - mu_x mu_y,
//     ss = (2 mu_x mu_y + c1) / (mu_x^2 + mu_y^2 + c1) * (2 sigma_xy + c2) / (sigma_xx + sigma_yy + c2);
//   an image's SSIM is the mean of ss over every valid pixel of all three channels.
//
// The window statistics are fp64: G(x^2) - mu_x^2 cancels on flat (white-background) regions against c2 = 9e-4, and fp32 statistics
// move a 640x480 render's SSIM by ~5e-5 depending on the summation order.  x^2, y^2 and xy of fp32 inputs are exact in fp64.
//
// Launch 1: one workgroup per 16 x 32 tile of output pixels of one image.  It stages the tile's inputs plus the 10-pixel halo in LDS
// (clipped on load, deinterleaved from HWC), runs the horizontal then the vertical pass of the five statistics per channel, and reduces
// its valid pixels to ONE fp64 partial in a fixed tree order.  Launch 2: one workgroup per image sums that image's partials in a fixed
// order and writes the mean.  No atomics: the same image gives the same bits on every run and in any batch (its tiles and partial
// offsets relative to the image are independent of the other images).
#include "aon_launch.h"

#include <cmath>

namespace aon {

constexpr int kSsimWin = 11;
constexpr int kSsimHalo = kSsimWin - 1;
constexpr int kSsimTH = 16, kSsimTW = 32;                                      // output pixels per workgroup
constexpr int kSsimInH = kSsimTH + kSsimHalo, kSsimInW = kSsimTW + kSsimHalo;  // 26 x 42 staged input pixels
constexpr int kSsimThreads = 256;
constexpr int kSsimMaxImages = 32;                                             // images per launch pair (the kernel-argument table)

struct SsimArgs {
  const float* x[kSsimMaxImages];       // predictions, (h, w, 3) fp32
  const float* y[kSsimMaxImages];       // targets, same shape
  int h[kSsimMaxImages], w[kSsimMaxImages], tiles_x[kSsimMaxImages];
  int blk_begin[kSsimMaxImages + 1];    // workgroups (= partials) of image i: [blk_begin[i], blk_begin[i + 1])
  int n;
  double g[kSsimWin];
  double* part;                         // this launch's partials
  float* out;                           // this launch's outputs
};

__device__ __forceinline__ float clip01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }   // NaN stays NaN, as torch.clip

__device__ __forceinline__ double block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
#pragma unroll
  for (int s = kSsimThreads / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}

__global__ void __launch_bounds__(kSsimThreads) ssim_tile_kernel(SsimArgs a) {
  __shared__ float sx[3][kSsimInH][kSsimInW], sy[3][kSsimInH][kSsimInW];
  __shared__ double hs[5][kSsimInH][kSsimTW];   // horizontal pass of one channel: G_h(x), G_h(y), G_h(x^2), G_h(y^2), G_h(xy)
  __shared__ double red[kSsimThreads];
  const int blk = blockIdx.x, tid = threadIdx.x;
  int img = 0;
  for (int i = 1; i < a.n; ++i)
    if (blk >= a.blk_begin[i]) img = i;
  const int local = blk - a.blk_begin[img];
  const int h = a.h[img], w = a.w[img];
  const int r0 = (local / a.tiles_x[img]) * kSsimTH, c0 = (local % a.tiles_x[img]) * kSsimTW;
  const float* x = a.x[img];
  const float* y = a.y[img];

  // stage: a row of the tile is kSsimInW * 3 consecutive floats of the HWC image; pixels beyond the image are 0 (they only reach
  // output pixels outside the valid map, which are not counted)
  constexpr int kRowLen = kSsimInW * 3;
  for (int e = tid; e < kSsimInH * kRowLen; e += kSsimThreads) {
    const int r = e / kRowLen, q = e - r * kRowLen;
    const int c = q / 3, ch = q - c * 3;
    const int gr = r0 + r, gc = c0 + c;
    float vx = 0.f, vy = 0.f;
    if (gr < h && gc < w) {
      const int64_t off = ((int64_t)gr * w + gc) * 3 + ch;
      vx = clip01(x[off]);
      vy = clip01(y[off]);
    }
    sx[ch][r][c] = vx;
    sy[ch][r][c] = vy;
  }
  __syncthreads();

  const double c1 = 0.01 * 0.01, c2 = 0.03 * 0.03;
  const int valid_r = min(kSsimTH, h - kSsimHalo - r0), valid_c = min(kSsimTW, w - kSsimHalo - c0);
  double acc = 0.0;
  for (int ch = 0; ch < 3; ++ch) {
    for (int e = tid; e < kSsimInH * kSsimTW; e += kSsimThreads) {
      const int r = e / kSsimTW, c = e - r * kSsimTW;
      double m1 = 0.0, m2 = 0.0, s11 = 0.0, s22 = 0.0, s12 = 0.0;
#pragma unroll
      for (int t = 0; t < kSsimWin; ++t) {
        const double u = sx[ch][r][c + t], v = sy[ch][r][c + t], g = a.g[t];
        m1 = fma(g, u, m1);
        m2 = fma(g, v, m2);
        s11 = fma(g, u * u, s11);
        s22 = fma(g, v * v, s22);
        s12 = fma(g, u * v, s12);
      }
      hs[0][r][c] = m1; hs[1][r][c] = m2; hs[2][r][c] = s11; hs[3][r][c] = s22; hs[4][r][c] = s12;
    }
    __syncthreads();
    for (int e = tid; e < kSsimTH * kSsimTW; e += kSsimThreads) {
      const int r = e / kSsimTW, c = e - r * kSsimTW;
      double mx = 0.0, my = 0.0, gxx = 0.0, gyy = 0.0, gxy = 0.0;
#pragma unroll
      for (int t = 0; t < kSsimWin; ++t) {
        const double g = a.g[t];
        mx = fma(g, hs[0][r + t][c], mx);
        my = fma(g, hs[1][r + t][c], my);
        gxx = fma(g, hs[2][r + t][c], gxx);
        gyy = fma(g, hs[3][r + t][c], gyy);
        gxy = fma(g, hs[4][r + t][c], gxy);
      }
      const double mxx = mx * mx, myy = my * my, mxy = mx * my;
      const double cs = (2.0 * (gxy - mxy) + c2) / ((gxx - mxx) + (gyy - myy) + c2);
      const double ss = (2.0 * mxy + c1) / (mxx + myy + c1) * cs;
      if (r < valid_r && c < valid_c) acc += ss;
    }
    __syncthreads();   // hs is rewritten by the next channel
  }
  const double s = block_sum(acc, red);
  if (tid == 0) a.part[blk] = s;
}

__global__ void __launch_bounds__(kSsimThreads) ssim_finish_kernel(SsimArgs a) {
  __shared__ double red[kSsimThreads];
  const int img = blockIdx.x;
  const int b = a.blk_begin[img], e = a.blk_begin[img + 1];
  double v = 0.0;
  for (int k = b + (int)threadIdx.x; k < e; k += kSsimThreads) v += a.part[k];
  const double s = block_sum(v, red);
  if (threadIdx.x == 0) a.out[img] = (float)(s / (3.0 * (double)(a.h[img] - kSsimHalo) * (double)(a.w[img] - kSsimHalo)));
}

static int64_t ssim_tiles(int h, int w) {
  return (int64_t)((h - kSsimHalo + kSsimTH - 1) / kSsimTH) * ((w - kSsimHalo + kSsimTW - 1) / kSsimTW);
}

// fp64 partials the caller's workspace holds for these images (h, w >= 11, validated by the caller)
int64_t ssim_workspace_bytes(int n, const int* h, const int* w) {
  int64_t tiles = 0;
  for (int i = 0; i < n; ++i) tiles += ssim_tiles(h[i], w[i]);
  return tiles * (int64_t)sizeof(double);
}

hipError_t launch_ssim(int n, const float* const* x, const float* const* y, const int* h, const int* w, double* part, float* out,
                       hipStream_t stream) {
  double g[kSsimWin], sum = 0.0;
  for (int t = 0; t < kSsimWin; ++t) {
    const double d = t - (kSsimWin - 1) / 2;
    g[t] = std::exp(-(d * d) / (2.0 * 1.5 * 1.5));
    sum += g[t];
  }
  for (int i0 = 0; i0 < n; i0 += kSsimMaxImages) {
    SsimArgs a{};
    a.n = n - i0 < kSsimMaxImages ? n - i0 : kSsimMaxImages;
    int blk = 0;
    for (int i = 0; i < a.n; ++i) {
      a.x[i] = x[i0 + i]; a.y[i] = y[i0 + i]; a.h[i] = h[i0 + i]; a.w[i] = w[i0 + i];
      a.tiles_x[i] = (a.w[i] - kSsimHalo + kSsimTW - 1) / kSsimTW;
      a.blk_begin[i] = blk;
      blk += (int)ssim_tiles(a.h[i], a.w[i]);
    }
    a.blk_begin[a.n] = blk;
    for (int t = 0; t < kSsimWin; ++t) a.g[t] = g[t] / sum;
    a.part = part;
    a.out = out + i0;
    ssim_tile_kernel<<<dim3(blk), dim3(kSsimThreads), 0, stream>>>(a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    ssim_finish_kernel<<<dim3(a.n), dim3(kSsimThreads), 0, stream>>>(a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    part += blk;
  }
  return hipSuccess;
}

}  // namespace aon
