// spz_metrics.hip — image metrics on the device (DESIGN §8 "Compare"; the contract is in include/spz_amd.h): PSNR,
// MSE, L1, max error and SSIM of two images, and the comparison of two packed streams over a set of views.
//
//   spz_metrics_tile_kernel        one workgroup per 32x16 output tile, 256 lanes.  Per channel: the tile and its
//                                  5-pixel halo of both images into LDS, clamped, zeros outside the image; a horizontal
//                                  11-tap pass writing the five window sums (a, b, a^2, b^2, ab) per row into LDS in
//                                  f64; a vertical 11-tap pass giving S per pixel (two pixels per lane), with d^2, |d|
//                                  and max |d| on the way.  The map (mean S over the channels) when asked; the tile's
//                                  partial sums to a slab, reduced across the workgroup in a fixed order.
//   spz_metrics_reduce_kernel      one workgroup: the slab in a fixed order, then the five results.  No float atomics.
//   spz_loss_tile_kernel           the same tile body (metrics_tile_body<true>): beside the partial sums, the three
//                                  derivative maps of S per channel (to the window mean of a, of a^2 and of ab) as nine
//                                  f64 planes.
//   spz_loss_reduce_kernel         the slab in the metrics' order, then L = (1 - lambda) l1 + lambda (1 - ssim), l1, ssim.
//   spz_loss_grad_kernel           one workgroup per 32x16 tile: each plane's tile and halo into LDS (zeros outside the
//                                  image), the same two 11-tap passes, then dL/da per pixel through the clamp's mask.
//   compare                        per view: render A, render B (render_view of spz_view_pass.hpp into grow-only
//                                  buffers), then the two kernels above.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "spz_amd.h"
#include "spz_common.hpp"
#include "spz_view_pass.hpp"

namespace spz_amd_detail {
namespace {

constexpr int kMtW = 32;                 // output tile width
constexpr int kMtH = 16;                 // output tile height
constexpr int kMtR = 5;                  // window radius
constexpr int kMtInW = kMtW + 2 * kMtR;  // 42
constexpr int kMtInH = kMtH + 2 * kMtR;  // 26
constexpr uint32_t kMtThreads = 256;
constexpr uint32_t kMtRedThreads = 256;
constexpr uint32_t kMtMaxSide = 16384;
constexpr double kC1 = 0.01 * 0.01;
constexpr double kC2 = 0.03 * 0.03;

struct MetricsWindow {
  double w[2 * kMtR + 1];
};

// w_k = exp(-(k - 5)^2 / (2 1.5^2)) / sum, the sum taken in k order.
MetricsWindow metrics_window() {
  MetricsWindow m;
  double e[2 * kMtR + 1], s = 0.0;
  for (int k = 0; k <= 2 * kMtR; ++k) {
    const double x = (double)(k - kMtR);
    e[k] = std::exp(-(x * x) / (2.0 * 1.5 * 1.5));
    s += e[k];
  }
  for (int k = 0; k <= 2 * kMtR; ++k) m.w[k] = e[k] / s;
  return m;
}

uint32_t metrics_tiles(uint32_t width, uint32_t height) {
  return ((width + kMtW - 1) / kMtW) * ((height + kMtH - 1) / kMtH);
}

// fminf(fmaxf(v, 0), 1) with NaN -> 0, written as compares so that no NaN operand reaches a min / max instruction.
__device__ __forceinline__ float clamp01(float v) {
  v = v > 0.0f ? v : 0.0f;
  return v < 1.0f ? v : 1.0f;
}

// S of one pixel and channel; every expression is symmetric in (a, b).
__device__ __forceinline__ double ssim_of(double ma, double mb, double maa, double mbb, double mab) {
  const double mu_ab = ma * mb, mu_aa = ma * ma, mu_bb = mb * mb;
  const double sa = maa - mu_aa, sb = mbb - mu_bb, sab = mab - mu_ab;
  return ((2.0 * mu_ab + kC1) * (2.0 * sab + kC2)) / ((mu_aa + mu_bb + kC1) * (sa + sb + kC2));
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long u = __shfl_xor(v, o);
    v = u > v ? u : v;
  }
  return v;
}

// The derivatives of one pixel's S (image loss): to the window mean of ab (P), of a^2 (Q), and the total one to the
// window mean of a (M), the variances' dependence on it included.
__device__ __forceinline__ void ssim_derivatives(double ma, double mb, double maa, double mbb, double mab, double s,
                                                 double *p, double *q, double *m) {
  const double mu_ab = ma * mb, mu_aa = ma * ma, mu_bb = mb * mb;
  const double sa = maa - mu_aa, sb = mbb - mu_bb, sab = mab - mu_ab;
  const double a1 = 2.0 * mu_ab + kC1, a2 = 2.0 * sab + kC2, b1 = mu_aa + mu_bb + kC1, b2 = sa + sb + kC2;
  const double b12 = b1 * b2;
  *p = (2.0 * a1) / b12;
  *q = -s / b2;
  *m = (2.0 * mb * (a2 - a1)) / b12 - (2.0 * ma * s) * (1.0 / b1 - 1.0 / b2);
}

// The tile pass of the metrics and of the image loss.  slab: 4 planes of `tiles` 8-byte words: sum d^2, sum |d|, sum S
// (all f64), max |d| (the u64 bits of the f64).  kLoss: dmaps gets nine planes of height x width f64, plane 3 c + {0: M,
// 1: Q, 2: P} of channel c; map is not used.
template <bool kLoss>
__device__ __forceinline__ void metrics_tile_body(const float *__restrict__ a, uint32_t ca, const float *__restrict__ b,
                                                  uint32_t cb, uint32_t width, uint32_t height, uint32_t tiles_x,
                                                  uint32_t tiles, const MetricsWindow &win, float *__restrict__ map,
                                                  double *__restrict__ dmaps, double *__restrict__ slab) {
  __shared__ float la[kMtInH][kMtInW];
  __shared__ float lb[kMtInH][kMtInW];
  __shared__ double hs[5][kMtInH][kMtW];
  __shared__ double part[3][kMtThreads / 64];
  __shared__ unsigned long long part_max[kMtThreads / 64];
  const uint32_t tid = threadIdx.x;
  const int x0 = (int)((blockIdx.x % tiles_x) * kMtW), y0 = (int)((blockIdx.x / tiles_x) * kMtH);
  const int W = (int)width, H = (int)height;
  const int px = (int)(tid % kMtW), py0 = (int)(tid / kMtW);  // this lane's pixels: (px, py0) and (px, py0 + 8)
  double s_px[2] = {0.0, 0.0};
  double sum_d2 = 0.0, sum_d1 = 0.0;
  unsigned long long max_d = 0;
  for (uint32_t c = 0; c < 3; ++c) {
    for (int i = (int)tid; i < kMtInH * kMtInW; i += kMtThreads) {
      const int r = i / kMtInW, q = i % kMtInW;
      const int gy = y0 - kMtR + r, gx = x0 - kMtR + q;
      float va = 0.0f, vb = 0.0f;
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
        const size_t p = (size_t)gy * width + (size_t)gx;
        va = clamp01(a[p * ca + c]);
        vb = clamp01(b[p * cb + c]);
      }
      la[r][q] = va;
      lb[r][q] = vb;
    }
    __syncthreads();
    for (int i = (int)tid; i < kMtInH * kMtW; i += kMtThreads) {
      const int r = i / kMtW, q = i % kMtW;
      double ma = 0.0, mb = 0.0, maa = 0.0, mbb = 0.0, mab = 0.0;
#pragma unroll
      for (int k = 0; k <= 2 * kMtR; ++k) {
        const double va = la[r][q + k], vb = lb[r][q + k], wk = win.w[k];
        ma += wk * va;
        mb += wk * vb;
        maa += wk * (va * va);
        mbb += wk * (vb * vb);
        mab += wk * (va * vb);
      }
      hs[0][r][q] = ma;
      hs[1][r][q] = mb;
      hs[2][r][q] = maa;
      hs[3][r][q] = mbb;
      hs[4][r][q] = mab;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int py = py0 + 8 * j;
      const int gx = x0 + px, gy = y0 + py;
      if (gx < W && gy < H) {
        double ma = 0.0, mb = 0.0, maa = 0.0, mbb = 0.0, mab = 0.0;
#pragma unroll
        for (int k = 0; k <= 2 * kMtR; ++k) {
          const double wk = win.w[k];
          ma += wk * hs[0][py + k][px];
          mb += wk * hs[1][py + k][px];
          maa += wk * hs[2][py + k][px];
          mbb += wk * hs[3][py + k][px];
          mab += wk * hs[4][py + k][px];
        }
        const double s_one = ssim_of(ma, mb, maa, mbb, mab);
        s_px[j] += s_one;
        if constexpr (kLoss) {
          double dp, dq, dm;
          ssim_derivatives(ma, mb, maa, mbb, mab, s_one, &dp, &dq, &dm);
          const size_t plane = (size_t)width * height, at = (size_t)gy * width + (size_t)gx;
          dmaps[(3u * c + 0u) * plane + at] = dm;
          dmaps[(3u * c + 1u) * plane + at] = dq;
          dmaps[(3u * c + 2u) * plane + at] = dp;
        }
        const double d = (double)la[py + kMtR][px + kMtR] - (double)lb[py + kMtR][px + kMtR];
        const double ad = fabs(d);
        sum_d2 += d * d;
        sum_d1 += ad;
        const unsigned long long bits = (unsigned long long)__double_as_longlong(ad);
        max_d = bits > max_d ? bits : max_d;
        if constexpr (!kLoss) {
          if (map != nullptr && c == 2) map[(size_t)gy * width + (size_t)gx] = (float)(s_px[j] / 3.0);
        }
      }
    }
    __syncthreads();  // the next channel overwrites la, lb and hs
  }
  // the workgroup's partials: across each wave, then the waves in order
  const double sum_s = wave_sum(s_px[0] + s_px[1]);
  sum_d2 = wave_sum(sum_d2);
  sum_d1 = wave_sum(sum_d1);
  max_d = wave_max(max_d);
  const uint32_t wave = tid / 64;
  if ((tid & 63u) == 0) {
    part[0][wave] = sum_d2;
    part[1][wave] = sum_d1;
    part[2][wave] = sum_s;
    part_max[wave] = max_d;
  }
  __syncthreads();
  if (tid == 0) {
    double t0 = part[0][0], t1 = part[1][0], t2 = part[2][0];
    unsigned long long m = part_max[0];
    for (uint32_t w = 1; w < kMtThreads / 64; ++w) {
      t0 += part[0][w];
      t1 += part[1][w];
      t2 += part[2][w];
      m = part_max[w] > m ? part_max[w] : m;
    }
    slab[blockIdx.x] = t0;
    slab[tiles + blockIdx.x] = t1;
    slab[2u * tiles + blockIdx.x] = t2;
    slab[3u * tiles + blockIdx.x] = __longlong_as_double((long long)m);
  }
}

}  // namespace

__global__ __launch_bounds__(kMtThreads) void spz_metrics_tile_kernel(const float *__restrict__ a, uint32_t ca,
                                                                      const float *__restrict__ b, uint32_t cb,
                                                                      uint32_t width, uint32_t height, uint32_t tiles_x,
                                                                      uint32_t tiles, MetricsWindow win,
                                                                      float *__restrict__ map, double *__restrict__ slab) {
  metrics_tile_body<false>(a, ca, b, cb, width, height, tiles_x, tiles, win, map, nullptr, slab);
}

__global__ __launch_bounds__(kMtThreads) void spz_loss_tile_kernel(const float *__restrict__ a, uint32_t ca,
                                                                   const float *__restrict__ b, uint32_t cb,
                                                                   uint32_t width, uint32_t height, uint32_t tiles_x,
                                                                   uint32_t tiles, MetricsWindow win,
                                                                   double *__restrict__ dmaps, double *__restrict__ slab) {
  metrics_tile_body<true>(a, ca, b, cb, width, height, tiles_x, tiles, win, nullptr, dmaps, slab);
}

namespace {

// The slab's three sums and its maximum, in a fixed order: each lane its strided entries, then a tree over the lanes.
// Lane 0 returns with the results.
__device__ __forceinline__ void reduce_slab(const double *__restrict__ slab, uint32_t tiles, double *sum_d2,
                                            double *sum_d1, double *sum_s, unsigned long long *max_d) {
  __shared__ double r0[kMtRedThreads], r1[kMtRedThreads], r2[kMtRedThreads];
  __shared__ unsigned long long rm[kMtRedThreads];
  const uint32_t tid = threadIdx.x;
  double t0 = 0.0, t1 = 0.0, t2 = 0.0;
  unsigned long long m = 0;
  for (uint32_t i = tid; i < tiles; i += kMtRedThreads) {
    t0 += slab[i];
    t1 += slab[tiles + i];
    t2 += slab[2u * tiles + i];
    const unsigned long long u = (unsigned long long)__double_as_longlong(slab[3u * tiles + i]);
    m = u > m ? u : m;
  }
  r0[tid] = t0;
  r1[tid] = t1;
  r2[tid] = t2;
  rm[tid] = m;
  __syncthreads();
  for (uint32_t s = kMtRedThreads / 2; s > 0; s >>= 1) {
    if (tid < s) {
      r0[tid] += r0[tid + s];
      r1[tid] += r1[tid + s];
      r2[tid] += r2[tid + s];
      rm[tid] = rm[tid + s] > rm[tid] ? rm[tid + s] : rm[tid];
    }
    __syncthreads();
  }
  *sum_d2 = r0[0];
  *sum_d1 = r1[0];
  *sum_s = r2[0];
  *max_d = rm[0];
}

}  // namespace

__global__ __launch_bounds__(kMtRedThreads) void spz_metrics_reduce_kernel(const double *__restrict__ slab,
                                                                           uint32_t tiles, double count,
                                                                           spz_amd_image_metrics *__restrict__ out) {
  double d2, d1, ss;
  unsigned long long md;
  reduce_slab(slab, tiles, &d2, &d1, &ss, &md);
  if (threadIdx.x == 0) {
    const double mse = d2 / count;
    out->mse = mse;
    out->psnr = mse == 0.0 ? __longlong_as_double(0x7ff0000000000000ll) : 10.0 * log10(1.0 / mse);
    out->ssim = ss / count;
    out->l1 = d1 / count;
    out->max_abs = __longlong_as_double((long long)md);
  }
}

// out[0] = L = (1 - lambda) l1 + lambda (1 - ssim), out[1] = l1, out[2] = ssim; l1 and ssim as the metrics give them.
__global__ __launch_bounds__(kMtRedThreads) void spz_loss_reduce_kernel(const double *__restrict__ slab, uint32_t tiles,
                                                                        double count, double lambda,
                                                                        double *__restrict__ out) {
  double d2, d1, ss;
  unsigned long long md;
  reduce_slab(slab, tiles, &d2, &d1, &ss, &md);
  if (threadIdx.x == 0) {
    const double l1 = d1 / count, ssim = ss / count;
    out[0] = (1.0 - lambda) * l1 + lambda * (1.0 - ssim);
    out[1] = l1;
    out[2] = ssim;
  }
}

// dL/da of one 32x16 tile.  Per channel, the three planes (M, Q, P) one after the other: the tile and its halo into LDS
// (zeros outside the image), the 11 taps along rows, then along columns at this lane's two pixels:
//   d ssim / d a = (g*M + 2 a g*Q + b g*P) / count on the clamped a, b;  the L1 part: sign(a - b) / count;
//   dL/da = ((1 - lambda) sign - lambda (g*M + 2 a g*Q + b g*P)) / count where 0 <= a <= 1 (the raw value), else 0.
// Every element of grad is written; a fourth channel gets 0.
__global__ __launch_bounds__(kMtThreads) void spz_loss_grad_kernel(const float *__restrict__ a, uint32_t ca,
                                                                   const float *__restrict__ b, uint32_t cb,
                                                                   uint32_t width, uint32_t height, uint32_t tiles_x,
                                                                   MetricsWindow win, const double *__restrict__ dmaps,
                                                                   double lambda, double count,
                                                                   float *__restrict__ grad) {
  __shared__ double lm[kMtInH][kMtInW];
  __shared__ double hs[kMtInH][kMtW];
  const uint32_t tid = threadIdx.x;
  const int x0 = (int)((blockIdx.x % tiles_x) * kMtW), y0 = (int)((blockIdx.x / tiles_x) * kMtH);
  const int W = (int)width, H = (int)height;
  const int px = (int)(tid % kMtW), py0 = (int)(tid / kMtW);  // this lane's pixels: (px, py0) and (px, py0 + 8)
  const size_t plane = (size_t)width * height;
  float g_out[2][3];
  for (uint32_t c = 0; c < 3; ++c) {
    double acc[2] = {0.0, 0.0};
    double va[2] = {0.0, 0.0}, vb[2] = {0.0, 0.0};
    bool pass[2] = {false, false};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int gx = x0 + px, gy = y0 + py0 + 8 * j;
      if (gx < W && gy < H) {
        const size_t p = (size_t)gy * width + (size_t)gx;
        const float ra = a[p * ca + c];
        pass[j] = ra >= 0.0f && ra <= 1.0f;  // false for NaN
        va[j] = (double)clamp01(ra);
        vb[j] = (double)clamp01(b[p * cb + c]);
      }
    }
    for (uint32_t m = 0; m < 3; ++m) {
      const double *__restrict__ src = dmaps + (3u * c + m) * plane;
      for (int i = (int)tid; i < kMtInH * kMtInW; i += kMtThreads) {
        const int r = i / kMtInW, q = i % kMtInW;
        const int gy = y0 - kMtR + r, gx = x0 - kMtR + q;
        lm[r][q] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? src[(size_t)gy * width + (size_t)gx] : 0.0;
      }
      __syncthreads();
      for (int i = (int)tid; i < kMtInH * kMtW; i += kMtThreads) {
        const int r = i / kMtW, q = i % kMtW;
        double t = 0.0;
#pragma unroll
        for (int k = 0; k <= 2 * kMtR; ++k) t += win.w[k] * lm[r][q + k];
        hs[r][q] = t;
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int py = py0 + 8 * j;
        double t = 0.0;
#pragma unroll
        for (int k = 0; k <= 2 * kMtR; ++k) t += win.w[k] * hs[py + k][px];
        acc[j] += m == 0 ? t : (m == 1 ? (2.0 * va[j]) * t : vb[j] * t);
      }
      __syncthreads();  // the next plane overwrites lm and hs
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const double d = va[j] - vb[j];
      const double sign = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
      g_out[j][c] = pass[j] ? (float)(((1.0 - lambda) * sign - lambda * acc[j]) / count) : 0.0f;
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int gx = x0 + px, gy = y0 + py0 + 8 * j;
    if (gx < W && gy < H) {
      const size_t p = (size_t)gy * width + (size_t)gx;
      if (ca == 4) {
        *reinterpret_cast<F32x4 *>(grad + p * 4u) = F32x4{g_out[j][0], g_out[j][1], g_out[j][2], 0.0f};
      } else {
        grad[p * 3u] = g_out[j][0];
        grad[p * 3u + 1u] = g_out[j][1];
        grad[p * 3u + 2u] = g_out[j][2];
      }
    }
  }
}

namespace {

int metrics_enqueue(const float *d_a, int channels_a, const float *d_b, int channels_b, int width, int height,
                    spz_amd_image_metrics *d_out, float *d_ssim_map, void *d_workspace, hipStream_t st) {
  const uint32_t w = (uint32_t)width, h = (uint32_t)height;
  const uint32_t tiles_x = (w + kMtW - 1) / kMtW;
  const uint32_t tiles = metrics_tiles(w, h);
  static const MetricsWindow win = metrics_window();
  auto *slab = static_cast<double *>(d_workspace);
  hipLaunchKernelGGL(spz_metrics_tile_kernel, dim3(tiles), dim3(kMtThreads), 0, st, d_a, (uint32_t)channels_a, d_b,
                     (uint32_t)channels_b, w, h, tiles_x, tiles, win, d_ssim_map, slab);
  SPZ_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(spz_metrics_reduce_kernel, dim3(1), dim3(kMtRedThreads), 0, st, slab, tiles,
                     3.0 * (double)w * (double)h, d_out);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

// The image loss's workspace: the slab, then the nine f64 planes.
uint64_t loss_slab_bytes(uint32_t w, uint32_t h) { return Workspace::aligned((uint64_t)metrics_tiles(w, h) * 32u); }

int loss_enqueue(const float *d_a, int channels_a, const float *d_b, int channels_b, int width, int height,
                 double lambda, double *d_loss, float *d_grad, void *d_workspace, hipStream_t st) {
  const uint32_t w = (uint32_t)width, h = (uint32_t)height;
  const uint32_t tiles_x = (w + kMtW - 1) / kMtW;
  const uint32_t tiles = metrics_tiles(w, h);
  static const MetricsWindow win = metrics_window();
  uint8_t *base = align_ws(d_workspace);
  auto *slab = reinterpret_cast<double *>(base);
  auto *dmaps = reinterpret_cast<double *>(base + loss_slab_bytes(w, h));
  const double count = 3.0 * (double)w * (double)h;
  hipLaunchKernelGGL(spz_loss_tile_kernel, dim3(tiles), dim3(kMtThreads), 0, st, d_a, (uint32_t)channels_a, d_b,
                     (uint32_t)channels_b, w, h, tiles_x, tiles, win, dmaps, slab);
  SPZ_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(spz_loss_reduce_kernel, dim3(1), dim3(kMtRedThreads), 0, st, slab, tiles, count, lambda, d_loss);
  SPZ_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(spz_loss_grad_kernel, dim3(tiles), dim3(kMtThreads), 0, st, d_a, (uint32_t)channels_a, d_b,
                     (uint32_t)channels_b, w, h, tiles_x, win, dmaps, lambda, count, d_grad);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

bool aligned_to(const void *p, uintptr_t k) { return (reinterpret_cast<uintptr_t>(p) & (k - 1)) == 0; }

// The device blocks of one compare call, grow-only, freed (after the stream) when it returns.
struct CompareBlocks {
  hipStream_t st = nullptr;
  uint8_t *ws = nullptr;     // the render's workspace
  uint64_t ws_cap = 0;
  float *img = nullptr;      // images A and B, one after the other
  uint64_t img_cap = 0;      // floats per image
  uint8_t *mws = nullptr;    // the metrics slab
  uint64_t mws_cap = 0;
  float *map = nullptr;
  uint64_t map_cap = 0;
  uint8_t *small = nullptr;  // total (8), status (4), then the views' metrics
  ~CompareBlocks() {
    if (st) (void)hipStreamSynchronize(st);
    for (void *p : {(void *)ws, (void *)img, (void *)mws, (void *)map, (void *)small}) {
      if (p) (void)hipFree(p);
    }
    if (st) (void)hipStreamDestroy(st);
  }
};

template <class T>
int grow(T **p, uint64_t *cap, uint64_t need, uint64_t elem) {
  if (need <= *cap) return SPZ_AMD_OK;
  if (*p) SPZ_HIP_TRY(hipFree(*p));
  *p = nullptr;
  *cap = 0;
  SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(p), need * elem));
  *cap = need;
  return SPZ_AMD_OK;
}

}  // namespace
}  // namespace spz_amd_detail

using namespace spz_amd_detail;

extern "C" {

int spz_amd_image_metrics_check(int width, int height, int channels_a, int channels_b) {
  if (width < 1 || height < 1 || (uint32_t)width > kMtMaxSide || (uint32_t)height > kMtMaxSide) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  if ((channels_a != 3 && channels_a != 4) || (channels_b != 3 && channels_b != 4)) return SPZ_AMD_ERR_INVALID_ARG;
  return SPZ_AMD_OK;
}

uint64_t spz_amd_image_metrics_workspace_bytes(int width, int height) {
  if (width < 1 || height < 1 || (uint32_t)width > kMtMaxSide || (uint32_t)height > kMtMaxSide) return 0;
  return (uint64_t)metrics_tiles((uint32_t)width, (uint32_t)height) * 32u;
}

int spz_amd_image_metrics_device(const float *d_a, int channels_a, const float *d_b, int channels_b, int width,
                                 int height, spz_amd_image_metrics *d_out, float *d_ssim_map, void *d_workspace,
                                 void *hip_stream) {
  int rc = spz_amd_image_metrics_check(width, height, channels_a, channels_b);
  if (rc != SPZ_AMD_OK) return rc;
  if (d_a == nullptr || d_b == nullptr || d_out == nullptr || d_workspace == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  if (!aligned_to(d_a, 4) || !aligned_to(d_b, 4) || !aligned_to(d_out, 8) || !aligned_to(d_workspace, 8) ||
      !aligned_to(d_ssim_map, 4)) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  return metrics_enqueue(d_a, channels_a, d_b, channels_b, width, height, d_out, d_ssim_map, d_workspace,
                         static_cast<hipStream_t>(hip_stream));
}

uint64_t spz_amd_image_loss_workspace_bytes(int width, int height) {
  if (width < 1 || height < 1 || (uint32_t)width > kMtMaxSide || (uint32_t)height > kMtMaxSide) return 0;
  return loss_slab_bytes((uint32_t)width, (uint32_t)height) + 9u * 8u * (uint64_t)width * (uint64_t)height + 256u;
}

int spz_amd_image_loss_device(const float *d_a, int channels_a, const float *d_b, int channels_b, int width, int height,
                              double lambda_dssim, double *d_loss, float *d_grad, void *d_workspace, void *hip_stream) {
  int rc = spz_amd_image_metrics_check(width, height, channels_a, channels_b);
  if (rc != SPZ_AMD_OK) return rc;
  if (!(lambda_dssim >= 0.0) || !(lambda_dssim <= 1.0)) return SPZ_AMD_ERR_INVALID_ARG;
  if (d_a == nullptr || d_b == nullptr || d_loss == nullptr || d_grad == nullptr || d_workspace == nullptr) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  if (!aligned_to(d_a, 4) || !aligned_to(d_b, 4) || !aligned_to(d_loss, 8) || !aligned_to(d_grad, 4)) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  return loss_enqueue(d_a, channels_a, d_b, channels_b, width, height, lambda_dssim, d_loss, d_grad, d_workspace,
                      static_cast<hipStream_t>(hip_stream));
}

int spz_amd_image_metrics_host(const float *h_a, int channels_a, const float *h_b, int channels_b, int width,
                               int height, int device, spz_amd_image_metrics *h_out, float *h_ssim_map) {
  int rc = spz_amd_image_metrics_check(width, height, channels_a, channels_b);
  if (rc != SPZ_AMD_OK) return rc;
  if (h_a == nullptr || h_b == nullptr || h_out == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  DeviceGuard guard;
  rc = guard.enter(device);
  if (rc != SPZ_AMD_OK) return rc;
  CompareBlocks k;
  SPZ_HIP_TRY(hipStreamCreateWithFlags(&k.st, hipStreamNonBlocking));
  const uint64_t px = (uint64_t)width * (uint64_t)height;
  const uint64_t bytes_a = px * (uint64_t)channels_a * 4u, bytes_b = px * (uint64_t)channels_b * 4u;
  const uint64_t o_b = Workspace::aligned(bytes_a), o_map = o_b + Workspace::aligned(bytes_b),
                 o_out = o_map + (h_ssim_map ? Workspace::aligned(px * 4u) : 0u), o_ws = o_out + 256u,
                 total = o_ws + spz_amd_image_metrics_workspace_bytes(width, height);
  SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&k.small), total));
  uint8_t *base = k.small;
  auto *d_a = reinterpret_cast<float *>(base);
  auto *d_b = reinterpret_cast<float *>(base + o_b);
  float *d_map = h_ssim_map ? reinterpret_cast<float *>(base + o_map) : nullptr;
  auto *d_out = reinterpret_cast<spz_amd_image_metrics *>(base + o_out);
  SPZ_HIP_TRY(hipMemcpyAsync(d_a, h_a, bytes_a, hipMemcpyHostToDevice, k.st));
  SPZ_HIP_TRY(hipMemcpyAsync(d_b, h_b, bytes_b, hipMemcpyHostToDevice, k.st));
  rc = metrics_enqueue(d_a, channels_a, d_b, channels_b, width, height, d_out, d_map, base + o_ws, k.st);
  if (rc != SPZ_AMD_OK) return rc;
  SPZ_HIP_TRY(hipMemcpyAsync(h_out, d_out, sizeof(spz_amd_image_metrics), hipMemcpyDeviceToHost, k.st));
  if (h_ssim_map) SPZ_HIP_TRY(hipMemcpyAsync(h_ssim_map, d_map, px * 4u, hipMemcpyDeviceToHost, k.st));
  SPZ_HIP_TRY(hipStreamSynchronize(k.st));
  return SPZ_AMD_OK;
}

int spz_amd_compare_host(const uint8_t *d_stream_a, size_t size_a, const spz_amd_header *hdr_a,
                         const uint8_t *d_stream_b, size_t size_b, const spz_amd_header *hdr_b,
                         const spz_amd_render_params *views, int num_views, int device,
                         spz_amd_image_metrics *h_metrics, float *h_ssim_maps, uint64_t *h_entries, float *h_ms,
                         int32_t *h_bad_view) {
  if (h_bad_view) *h_bad_view = -1;
  if (h_metrics == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  int rc = check_views(views, num_views, SPZ_AMD_COMPARE_MAX_VIEWS, h_bad_view);
  if (rc != SPZ_AMD_OK) return rc;
  rc = check_render_input(d_stream_a, size_a, hdr_a);
  if (rc != SPZ_AMD_OK) return rc;
  rc = check_render_input(d_stream_b, size_b, hdr_b);
  if (rc != SPZ_AMD_OK) return rc;
  DeviceGuard guard;
  rc = guard.enter(device);
  if (rc != SPZ_AMD_OK) return rc;
  CompareBlocks k;
  SPZ_HIP_TRY(hipStreamCreateWithFlags(&k.st, hipStreamNonBlocking));
  SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&k.small), 256u + (uint64_t)num_views * sizeof(spz_amd_image_metrics)));
  auto *d_total = reinterpret_cast<uint64_t *>(k.small);
  auto *d_status = reinterpret_cast<uint32_t *>(k.small + 8);
  auto *d_metrics = reinterpret_cast<spz_amd_image_metrics *>(k.small + 256u);
  const RenderSource src_a = packed_render_source(d_stream_a, size_a, hdr_a);
  const RenderSource src_b = packed_render_source(d_stream_b, size_b, hdr_b);
  double render_ms = 0.0, metrics_ms = 0.0;
  uint64_t map_off = 0;
  for (int v = 0; v < num_views; ++v) {
    const spz_amd_render_params &p = views[v];
    const uint64_t px = (uint64_t)p.width * p.height;
    auto fail = [&](int r) {
      if (h_bad_view) *h_bad_view = v;
      return r;
    };
    rc = grow(&k.img, &k.img_cap, 8u * px, 4u);  // two images of 4 floats per pixel
    if (rc != SPZ_AMD_OK) return rc;
    rc = grow(&k.mws, &k.mws_cap, spz_amd_image_metrics_workspace_bytes(p.width, p.height), 1u);
    if (rc != SPZ_AMD_OK) return rc;
    if (h_ssim_maps) {
      rc = grow(&k.map, &k.map_cap, px, 4u);
      if (rc != SPZ_AMD_OK) return rc;
    }
    float *img_a = k.img, *img_b = k.img + 4u * px;
    const auto t0 = std::chrono::steady_clock::now();
    uint64_t ea = 0, eb = 0;
    rc = render_view(&k.ws, &k.ws_cap, src_a, &p, d_total, d_status, img_a, k.st, &ea);
    if (rc != SPZ_AMD_OK) return fail(rc);
    rc = render_view(&k.ws, &k.ws_cap, src_b, &p, d_total, d_status, img_b, k.st, &eb);
    if (rc != SPZ_AMD_OK) return fail(rc);
    SPZ_HIP_TRY(hipStreamSynchronize(k.st));
    const auto t1 = std::chrono::steady_clock::now();
    render_ms += std::chrono::duration<double, std::milli>(t1 - t0).count();
    rc = metrics_enqueue(img_a, 4, img_b, 4, (int)p.width, (int)p.height, d_metrics + v,
                         h_ssim_maps ? k.map : nullptr, k.mws, k.st);
    if (rc != SPZ_AMD_OK) return fail(rc);
    if (h_ssim_maps) {
      SPZ_HIP_TRY(hipMemcpyAsync(h_ssim_maps + map_off, k.map, px * 4u, hipMemcpyDeviceToHost, k.st));
      map_off += px;
    }
    SPZ_HIP_TRY(hipStreamSynchronize(k.st));
    metrics_ms += ms_since(t1);
    if (h_entries) {
      h_entries[2 * v] = ea;
      h_entries[2 * v + 1] = eb;
    }
  }
  SPZ_HIP_TRY(hipMemcpyAsync(h_metrics, d_metrics, (size_t)num_views * sizeof(spz_amd_image_metrics),
                             hipMemcpyDeviceToHost, k.st));
  SPZ_HIP_TRY(hipStreamSynchronize(k.st));
  if (h_ms) {
    h_ms[0] = (float)render_ms;
    h_ms[1] = (float)metrics_ms;
  }
  return SPZ_AMD_OK;
}

}  // extern "C"
