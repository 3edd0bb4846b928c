// spz_image_tile.hpp — the tile passes the image metrics, the image loss (spz_metrics.hip) and the photo loss
// (spz_photo.hip) share: the window, the 32x16 tile with its 5-pixel halo, the two 11-tap passes, the slab and its
// reduction in a fixed order.  One body per pass, the three uses told apart at compile time, so that each keeps the
// operations, and with them the bits, it had on its own.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "spz_common.hpp"

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

constexpr int kTileMetrics = 0, kTileLoss = 1, kTilePhoto = 2;

struct MetricsWindow {
  double w[2 * kMtR + 1];
};

// w_k = exp(-(k - 5)^2 / (2 1.5^2)) / sum, the sum taken in k order.
inline MetricsWindow metrics_window() {
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

inline uint32_t metrics_tiles(uint32_t width, uint32_t height) {
  return ((width + kMtW - 1) / kMtW) * ((height + kMtH - 1) / kMtH);
}

inline bool aligned_to(const void *p, uintptr_t k) { return (reinterpret_cast<uintptr_t>(p) & (k - 1)) == 0; }

// What the photo loss adds to the image loss's passes: per-pixel weights (NULL: all 1) and the 3 x 4 exposure [M | o],
// row-major, from device memory (d_exposure) or by value (e); has_exposure == 0: the identity, nothing is multiplied.
struct PhotoArgs {
  const float *weight;
  const double *d_exposure;
  double e[12];
  int32_t has_exposure;
  int32_t pad;
};

// fminf(fmaxf(v, 0), 1) with NaN -> 0, written as compares so that no NaN operand reaches a min / max instruction.
__device__ __forceinline__ float clamp01(float v) {
  v = v > 0.0f ? v : 0.0f;
  return v < 1.0f ? v : 1.0f;
}

__device__ __forceinline__ double clamp01(double v) {
  v = v > 0.0 ? v : 0.0;
  return v < 1.0 ? v : 1.0;
}

// Channel c of the exposed pixel, unclamped: t = ((o_c + M_c0 a_0) + M_c1 a_1) + M_c2 a_2 in f64; the value itself
// without an exposure.  e: the 12 values.
__device__ __forceinline__ double photo_exposed(const float *__restrict__ px, uint32_t c, const double *e,
                                                bool has_exposure) {
  if (!has_exposure) return (double)px[c];
  return ((e[4u * c + 3u] + e[4u * c] * (double)px[0]) + e[4u * c + 1u] * (double)px[1]) +
         e[4u * c + 2u] * (double)px[2];
}

// The exposure of a launch into LDS (the caller synchronises before it reads).
__device__ __forceinline__ void photo_exposure_to_lds(const PhotoArgs &ph, double *ex) {
  if (threadIdx.x < 12u) ex[threadIdx.x] = ph.d_exposure != nullptr ? ph.d_exposure[threadIdx.x] : ph.e[threadIdx.x];
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

// The tile pass of the metrics, of the image loss and of the photo loss.  slab: 4 planes of `tiles` 8-byte words: sum
// d^2, sum |d|, sum S (all f64), max |d| (the u64 bits of the f64).  kTileLoss: dmaps gets nine planes of height x width
// f64, plane 3 c + {0: M, 1: Q, 2: P} of channel c; map is not used.  kTilePhoto: a is exposed (in f64) before the
// clamp; the sums of |d| and of S and the nine planes carry each pixel's weight w; plane 0 of the slab is sum w and
// plane 3 is 0.  With no weights and no exposure every product is by 1.0 and the loss's bits come out.
template <int kMode>
__device__ __forceinline__ void metrics_tile_body(const float *__restrict__ a, uint32_t ca, const float *__restrict__ b,
                                                  uint32_t cb, uint32_t width, uint32_t height, uint32_t tiles_x,
                                                  uint32_t tiles, const MetricsWindow &win, float *__restrict__ map,
                                                  double *__restrict__ dmaps, double *__restrict__ slab,
                                                  const PhotoArgs *photo) {
  constexpr bool kLoss = kMode != kTileMetrics, kPhoto = kMode == kTilePhoto;
  using ValueA = std::conditional_t<kPhoto, double, float>;
  __shared__ ValueA la[kMtInH][kMtInW];
  __shared__ float lb[kMtInH][kMtInW];
  __shared__ double hs[5][kMtInH][kMtW];
  __shared__ double part[3][kMtThreads / 64];
  __shared__ unsigned long long part_max[kMtThreads / 64];
  __shared__ double ex[12];
  const uint32_t tid = threadIdx.x;
  const int x0 = (int)((blockIdx.x % tiles_x) * kMtW), y0 = (int)((blockIdx.x / tiles_x) * kMtH);
  const int W = (int)width, H = (int)height;
  const int px = (int)(tid % kMtW), py0 = (int)(tid / kMtW);  // this lane's pixels: (px, py0) and (px, py0 + 8)
  double s_px[2] = {0.0, 0.0};
  double sum_d2 = 0.0, sum_d1 = 0.0;
  unsigned long long max_d = 0;
  double wj[2] = {1.0, 1.0};
  bool exposed = false;
  if constexpr (kPhoto) {
    exposed = photo->has_exposure != 0;
    if (exposed) photo_exposure_to_lds(*photo, ex);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int gx = x0 + px, gy = y0 + py0 + 8 * j;
      if (photo->weight != nullptr && gx < W && gy < H) {
        wj[j] = (double)clamp01(photo->weight[(size_t)gy * width + (size_t)gx]);
      }
    }
    __syncthreads();
  }
  for (uint32_t c = 0; c < 3; ++c) {
    for (int i = (int)tid; i < kMtInH * kMtInW; i += kMtThreads) {
      const int r = i / kMtInW, q = i % kMtInW;
      const int gy = y0 - kMtR + r, gx = x0 - kMtR + q;
      ValueA va = 0;
      float vb = 0.0f;
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
        const size_t p = (size_t)gy * width + (size_t)gx;
        if constexpr (kPhoto) {
          va = exposed ? clamp01(photo_exposed(a + p * ca, c, ex, true)) : (double)clamp01(a[p * ca + c]);
        } else {
          va = clamp01(a[p * ca + c]);
        }
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
          if constexpr (kPhoto) {
            dm *= wj[j];
            dq *= wj[j];
            dp *= wj[j];
          }
          dmaps[(3u * c + 0u) * plane + at] = dm;
          dmaps[(3u * c + 1u) * plane + at] = dq;
          dmaps[(3u * c + 2u) * plane + at] = dp;
        }
        const double d = (double)la[py + kMtR][px + kMtR] - (double)lb[py + kMtR][px + kMtR];
        const double ad = fabs(d);
        if constexpr (kPhoto) {
          if (c == 0) sum_d2 += wj[j];  // plane 0: sum w
          sum_d1 += wj[j] * ad;
        } else {
          sum_d2 += d * d;
          sum_d1 += ad;
          const unsigned long long bits = (unsigned long long)__double_as_longlong(ad);
          max_d = bits > max_d ? bits : max_d;
        }
        if constexpr (!kLoss) {
          if (map != nullptr && c == 2) map[(size_t)gy * width + (size_t)gx] = (float)(s_px[j] / 3.0);
        }
      }
    }
    __syncthreads();  // the next channel overwrites la, lb and hs
  }
  if constexpr (kPhoto) {
    s_px[0] *= wj[0];
    s_px[1] *= wj[1];
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

// dL/da of one 32x16 tile.  Per channel, the three planes (M, Q, P) one after the other: the tile and its halo into LDS
// (zeros outside the image), the 11 taps along rows, then along columns at this lane's two pixels:
//   d ssim / d a = (g*M + 2 a g*Q + b g*P) / count on the clamped a, b;  the L1 part: sign(a - b) / count;
//   dL/da = ((1 - lambda) sign - lambda (g*M + 2 a g*Q + b g*P)) / count where 0 <= a <= 1 (the raw value), else 0.
// Every element of grad is written; a fourth channel gets 0.
// kPhoto: a is the exposed value t, the planes carry their weights already, the sign is multiplied by this pixel's w,
// count = 3 W is read from *d_count (0: every gradient 0); with an exposure the three gated values go through M^T,
// and with eslab the 12 sums of the exposure's gradient go to it, one row of `tiles` per value: gate g' a_k for M_ck
// and gate g' for o_c, a closed gate or a non-finite a_k skipped.
template <bool kPhoto>
__device__ __forceinline__ void loss_grad_body(const float *__restrict__ a, uint32_t ca, const float *__restrict__ b,
                                               uint32_t cb, uint32_t width, uint32_t height, uint32_t tiles_x,
                                               const MetricsWindow &win, const double *__restrict__ dmaps,
                                               double lambda, double count, float *__restrict__ grad,
                                               const PhotoArgs *photo, const double *__restrict__ d_count,
                                               double *__restrict__ eslab) {
  __shared__ double lm[kMtInH][kMtInW];
  __shared__ double hs[kMtInH][kMtW];
  __shared__ double ex[12];
  __shared__ double epart[12][kMtThreads / 64];
  const uint32_t tid = threadIdx.x;
  const int x0 = (int)((blockIdx.x % tiles_x) * kMtW), y0 = (int)((blockIdx.x / tiles_x) * kMtH);
  const int W = (int)width, H = (int)height;
  const int px = (int)(tid % kMtW), py0 = (int)(tid / kMtW);  // this lane's pixels: (px, py0) and (px, py0 + 8)
  const size_t plane = (size_t)width * height;
  float g_out[2][3];
  double gd[2][3];
  bool open[2][3];
  double wj[2] = {1.0, 1.0};
  bool exposed = false;
  if constexpr (kPhoto) {
    count = *d_count;
    exposed = photo->has_exposure != 0;
    if (exposed) photo_exposure_to_lds(*photo, ex);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int gx = x0 + px, gy = y0 + py0 + 8 * j;
      if (photo->weight != nullptr && gx < W && gy < H) {
        wj[j] = (double)clamp01(photo->weight[(size_t)gy * width + (size_t)gx]);
      }
    }
    __syncthreads();
  }
  for (uint32_t c = 0; c < 3; ++c) {
    double acc[2] = {0.0, 0.0};
    double va[2] = {0.0, 0.0}, vb[2] = {0.0, 0.0};
    bool pass[2] = {false, false};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int gx = x0 + px, gy = y0 + py0 + 8 * j;
      if (gx < W && gy < H) {
        const size_t p = (size_t)gy * width + (size_t)gx;
        if constexpr (kPhoto) {
          if (exposed) {
            const double t = photo_exposed(a + p * ca, c, ex, true);
            pass[j] = t >= 0.0 && t <= 1.0;  // false for NaN
            va[j] = clamp01(t);
          } else {
            const float ra = a[p * ca + c];
            pass[j] = ra >= 0.0f && ra <= 1.0f;
            va[j] = (double)clamp01(ra);
          }
        } else {
          const float ra = a[p * ca + c];
          pass[j] = ra >= 0.0f && ra <= 1.0f;  // false for NaN
          va[j] = (double)clamp01(ra);
        }
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
      if constexpr (kPhoto) {
        open[j][c] = pass[j] && count != 0.0;
        gd[j][c] = open[j][c] ? (((1.0 - lambda) * sign) * wj[j] - lambda * acc[j]) / count : 0.0;
        g_out[j][c] = (float)gd[j][c];
      } else {
        g_out[j][c] = pass[j] ? (float)(((1.0 - lambda) * sign - lambda * acc[j]) / count) : 0.0f;
      }
    }
  }
  if constexpr (kPhoto) {
    double eg[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) eg[k] = 0.0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int gx = x0 + px, gy = y0 + py0 + 8 * j;
      if (gx < W && gy < H && (exposed || eslab != nullptr)) {
        const float *pxa = a + ((size_t)gy * width + (size_t)gx) * ca;
        const double ar[3] = {(double)pxa[0], (double)pxa[1], (double)pxa[2]};
        if (eslab != nullptr) {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            if (!open[j][c]) continue;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
              if (isfinite(ar[k])) eg[4 * c + k] += gd[j][c] * ar[k];
            }
            eg[4 * c + 3] += gd[j][c];
          }
        }
        if (exposed) {
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              if (open[j][c]) s += ex[4 * c + k] * gd[j][c];
            }
            g_out[j][k] = (float)s;
          }
        }
      }
    }
    if (eslab != nullptr) {
      const uint32_t tiles = gridDim.x;
#pragma unroll
      for (int k = 0; k < 12; ++k) {
        const double t = wave_sum(eg[k]);
        if ((tid & 63u) == 0) epart[k][tid / 64] = t;
      }
      __syncthreads();
      if (tid < 12u) {
        double t = epart[tid][0];
        for (uint32_t w = 1; w < kMtThreads / 64; ++w) t += epart[tid][w];
        eslab[tid * tiles + blockIdx.x] = t;
      }
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

}  // namespace
}  // namespace spz_amd_detail
