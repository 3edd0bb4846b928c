// spz_photo.hip — the photo loss: the image loss of a render against a photograph, with per-pixel weights and a 3 x 4
// exposure of the render (DESIGN §8 "Fit"; the contract is in include/spz_amd.h "photo loss").  The tile passes are the
// image loss's own (spz_image_tile.hpp), so that without weights and exposure its bits come out.
//
//   spz_photo_tile_kernel             metrics_tile_body<kTilePhoto>: a exposed in f64 and clamped on the way into LDS;
//                                     the sums of w |d|, w S and w to the slab; the nine planes times w.
//   spz_photo_reduce_kernel           the slab in the metrics' order; W = sum w; L, l1, ssim; 3 W for the next kernel.
//   spz_photo_grad_kernel             loss_grad_body<true>: dL/da' per pixel, through the gate and M^T to dL/da; the
//                                     tile's 12 partial sums of the exposure's gradient to a second slab.
//   spz_photo_exposure_reduce_kernel  one workgroup: that slab in a fixed order, 12 doubles out.  No float atomics.
//   spz_image_exposure_kernel         out = M a + o in f32, one lane per pixel.
//   spz_photo_exposure_adam_kernel    one workgroup, 12 lanes: an Adam step of one view's exposure in f64.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "spz_amd.h"
#include "spz_block_ops.hpp"
#include "spz_common.hpp"
#include "spz_image_tile.hpp"
#include "spz_photo_internal.hpp"

#pragma clang fp contract(off)

namespace spz_amd_detail {

__global__ __launch_bounds__(kMtThreads) void spz_photo_tile_kernel(const float *__restrict__ a, uint32_t ca,
                                                                    const float *__restrict__ b, uint32_t cb,
                                                                    uint32_t width, uint32_t height, uint32_t tiles_x,
                                                                    uint32_t tiles, MetricsWindow win, PhotoArgs photo,
                                                                    double *__restrict__ dmaps,
                                                                    double *__restrict__ slab) {
  metrics_tile_body<kTilePhoto>(a, ca, b, cb, width, height, tiles_x, tiles, win, nullptr, dmaps, slab, &photo);
}

// out[0] = L, out[1] = l1, out[2] = ssim over 3 W, W the slab's plane 0; W == 0: (0, 0, 1).  *count = 3 W.
__global__ __launch_bounds__(kMtRedThreads) void spz_photo_reduce_kernel(const double *__restrict__ slab, uint32_t tiles,
                                                                         double lambda, double *__restrict__ out,
                                                                         double *__restrict__ count_out) {
  double sw, d1, ss;
  unsigned long long md;
  reduce_slab(slab, tiles, &sw, &d1, &ss, &md);
  if (threadIdx.x == 0) {
    const double count = 3.0 * sw;
    *count_out = count;
    if (sw == 0.0) {
      out[0] = 0.0;
      out[1] = 0.0;
      out[2] = 1.0;
    } else {
      const double l1 = d1 / count, ssim = ss / count;
      out[0] = (1.0 - lambda) * l1 + lambda * (1.0 - ssim);
      out[1] = l1;
      out[2] = ssim;
    }
  }
}

__global__ __launch_bounds__(kMtThreads) void spz_photo_grad_kernel(const float *__restrict__ a, uint32_t ca,
                                                                    const float *__restrict__ b, uint32_t cb,
                                                                    uint32_t width, uint32_t height, uint32_t tiles_x,
                                                                    MetricsWindow win, PhotoArgs photo,
                                                                    const double *__restrict__ dmaps, double lambda,
                                                                    const double *__restrict__ count,
                                                                    float *__restrict__ grad,
                                                                    double *__restrict__ eslab) {
  loss_grad_body<true>(a, ca, b, cb, width, height, tiles_x, win, dmaps, lambda, 0.0, grad, &photo, count, eslab);
}

// The 12 rows of `tiles` partial sums, each in a fixed order: a lane its strided entries, then a tree over the lanes.
__global__ __launch_bounds__(kMtRedThreads) void spz_photo_exposure_reduce_kernel(const double *__restrict__ eslab,
                                                                                  uint32_t tiles,
                                                                                  double *__restrict__ out) {
  __shared__ double r[kMtRedThreads];
  static_assert(kMtRedThreads == kOpsBlock, "block_sum is over 256 threads");
  const uint32_t tid = threadIdx.x;
  for (uint32_t k = 0; k < 12u; ++k) {
    double t = 0.0;
    for (uint32_t i = tid; i < tiles; i += kMtRedThreads) t += eslab[k * tiles + i];
    t = block_sum(t, r);
    if (tid == 0) out[k] = t;
  }
}

struct ExposureF32 {
  float e[12];
};

__global__ __launch_bounds__(256) void spz_image_exposure_kernel(const float *in, uint32_t channels, ExposureF32 ex,
                                                                 unsigned long long pixels, float *out) {
  const unsigned long long p = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
  if (p >= pixels) return;
  const float *a = in + p * channels;
  const float a0 = a[0], a1 = a[1], a2 = a[2];
  const float a3 = channels == 4u ? a[3] : 0.0f;
  float *o = out + p * channels;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c] = ((ex.e[4 * c + 3] + ex.e[4 * c] * a0) + ex.e[4 * c + 1] * a1) + ex.e[4 * c + 2] * a2;
  if (channels == 4u) o[3] = a3;
}

struct ExposureAdam {
  double beta1, c1, beta2, c2, eps, r, s;
};

__global__ __launch_bounds__(64) void spz_photo_exposure_adam_kernel(double *__restrict__ e, const double *__restrict__ g,
                                                                     double *__restrict__ m, double *__restrict__ v,
                                                                     ExposureAdam k) {
  const uint32_t i = threadIdx.x;
  if (i >= 12u) return;
  const double gi = g[i];
  if (!isfinite(gi)) return;
  const double m1 = k.beta1 * m[i] + k.c1 * gi;
  const double v1 = k.beta2 * v[i] + (k.c2 * gi) * gi;
  const double den = sqrt(v1) / k.r + k.eps;
  e[i] = e[i] - k.s * (m1 / den);
  m[i] = m1;
  v[i] = v1;
}

namespace {

uint64_t photo_slab_bytes(uint32_t w, uint32_t h) { return Workspace::aligned((uint64_t)metrics_tiles(w, h) * 32u); }
uint64_t photo_planes_bytes(uint32_t w, uint32_t h) { return Workspace::aligned(72u * (uint64_t)w * (uint64_t)h); }

bool exposure_finite(const double *e) {
  for (int k = 0; k < 12; ++k) {
    if (!std::isfinite(e[k])) return false;
  }
  return true;
}

// The workspace: the slab, the nine f64 planes, 3 W, then the exposure gradient's slab.  The exposure from device
// memory, or by value from the host, or neither.
int photo_enqueue(const float *d_a, int channels_a, const float *d_b, int channels_b, const float *d_weight,
                  const double *d_exposure, const double *h_exposure, int width, int height, double lambda,
                  double *d_loss, float *d_grad, double *d_exposure_grad, void *d_workspace, hipStream_t st) {
  const uint32_t w = (uint32_t)width, h = (uint32_t)height;
  const uint32_t tiles_x = (w + kMtW - 1) / kMtW;
  const uint32_t tiles = metrics_tiles(w, h);
  static const MetricsWindow win = metrics_window();
  uint8_t *base = align_ws(d_workspace);
  auto *slab = reinterpret_cast<double *>(base);
  auto *dmaps = reinterpret_cast<double *>(base + photo_slab_bytes(w, h));
  auto *count = reinterpret_cast<double *>(base + photo_slab_bytes(w, h) + photo_planes_bytes(w, h));
  double *eslab = d_exposure_grad != nullptr ? count + 32 : nullptr;  // 256 bytes on
  PhotoArgs photo = {};
  photo.weight = d_weight;
  photo.d_exposure = d_exposure;
  photo.has_exposure = d_exposure != nullptr || h_exposure != nullptr;
  if (h_exposure != nullptr) std::memcpy(photo.e, h_exposure, sizeof(photo.e));
  hipLaunchKernelGGL(spz_photo_tile_kernel, dim3(tiles), dim3(kMtThreads), 0, st, d_a, (uint32_t)channels_a, d_b,
                     (uint32_t)channels_b, w, h, tiles_x, tiles, win, photo, dmaps, slab);
  SPZ_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(spz_photo_reduce_kernel, dim3(1), dim3(kMtRedThreads), 0, st, slab, tiles, lambda, d_loss, count);
  SPZ_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(spz_photo_grad_kernel, dim3(tiles), dim3(kMtThreads), 0, st, d_a, (uint32_t)channels_a, d_b,
                     (uint32_t)channels_b, w, h, tiles_x, win, photo, dmaps, lambda, count, d_grad, eslab);
  SPZ_HIP_TRY(hipGetLastError());
  if (eslab != nullptr) {
    hipLaunchKernelGGL(spz_photo_exposure_reduce_kernel, dim3(1), dim3(kMtRedThreads), 0, st, eslab, tiles,
                       d_exposure_grad);
    SPZ_HIP_TRY(hipGetLastError());
  }
  return SPZ_AMD_OK;
}

}  // namespace

int photo_loss_enqueue(const float *d_a, int channels_a, const float *d_b, int channels_b, const float *d_weight,
                       const double *d_exposure, int width, int height, double lambda, double *d_loss, float *d_grad,
                       double *d_exposure_grad, void *d_workspace, hipStream_t st) {
  return photo_enqueue(d_a, channels_a, d_b, channels_b, d_weight, d_exposure, nullptr, width, height, lambda,
                       d_loss, d_grad, d_exposure_grad, d_workspace, st);
}

int photo_exposure_adam_enqueue(double *d_exposure, const double *d_grad, double *d_m, double *d_v, int t, double lr,
                                double beta1, double beta2, double eps, hipStream_t st) {
  ExposureAdam k;
  k.beta1 = beta1;
  k.c1 = 1.0 - beta1;
  k.beta2 = beta2;
  k.c2 = 1.0 - beta2;
  k.eps = eps;
  k.r = std::sqrt(1.0 - std::pow(beta2, (double)t));
  k.s = lr / (1.0 - std::pow(beta1, (double)t));
  hipLaunchKernelGGL(spz_photo_exposure_adam_kernel, dim3(1), dim3(64), 0, st, d_exposure, d_grad, d_m, d_v, k);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

}  // namespace spz_amd_detail

using namespace spz_amd_detail;

extern "C" {

uint64_t spz_amd_photo_loss_workspace_bytes(int width, int height) {
  if (width < 1 || height < 1 || (uint32_t)width > kMtMaxSide || (uint32_t)height > kMtMaxSide) return 0;
  const uint32_t w = (uint32_t)width, h = (uint32_t)height;
  return photo_slab_bytes(w, h) + photo_planes_bytes(w, h) + 256u +
         Workspace::aligned(96u * (uint64_t)metrics_tiles(w, h)) + 256u;
}

int spz_amd_photo_loss_device(const float *d_a, int channels_a, const float *d_b, int channels_b, const float *d_weight,
                              const double *h_exposure, int width, int height, double lambda_dssim, double *d_loss,
                              float *d_grad, double *d_exposure_grad, void *d_workspace, void *hip_stream) {
  int rc = spz_amd_image_metrics_check(width, height, channels_a, channels_b);
  if (rc != SPZ_AMD_OK) return rc;
  if (!(lambda_dssim >= 0.0) || !(lambda_dssim <= 1.0)) return SPZ_AMD_ERR_INVALID_ARG;
  if (d_a == nullptr || d_b == nullptr || d_loss == nullptr || d_grad == nullptr || d_workspace == nullptr) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  if (h_exposure != nullptr && (d_exposure_grad == nullptr || !exposure_finite(h_exposure))) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  if (!aligned_to(d_a, 4) || !aligned_to(d_b, 4) || !aligned_to(d_weight, 4) || !aligned_to(d_loss, 8) ||
      !aligned_to(d_grad, 4) || !aligned_to(d_exposure_grad, 8)) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  return photo_enqueue(d_a, channels_a, d_b, channels_b, d_weight, nullptr, h_exposure, width, height, lambda_dssim,
                       d_loss, d_grad, d_exposure_grad, d_workspace, static_cast<hipStream_t>(hip_stream));
}

int spz_amd_image_exposure_device(const float *d_in, int channels, const double *h_exposure, int width, int height,
                                  float *d_out, void *hip_stream) {
  int rc = spz_amd_image_metrics_check(width, height, channels, channels);
  if (rc != SPZ_AMD_OK) return rc;
  if (d_in == nullptr || d_out == nullptr || h_exposure == nullptr || !exposure_finite(h_exposure)) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  if (!aligned_to(d_in, 4) || !aligned_to(d_out, 4)) return SPZ_AMD_ERR_INVALID_ARG;
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  ExposureF32 ex;
  for (int k = 0; k < 12; ++k) ex.e[k] = (float)h_exposure[k];
  const unsigned long long pixels = (unsigned long long)width * (unsigned long long)height;
  hipLaunchKernelGGL(spz_image_exposure_kernel, dim3((unsigned)((pixels + 255u) / 256u)), dim3(256), 0,
                     static_cast<hipStream_t>(hip_stream), d_in, (uint32_t)channels, ex, pixels, d_out);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

int spz_amd_photo_default_options(spz_amd_photo_options *options) {
  if (options == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  std::memset(options, 0, sizeof(*options));
  options->fit_exposure = 0;
  options->lr_exposure = 0.01;  // 3DGS's exposure_lr_init
  return SPZ_AMD_OK;
}

int spz_amd_photo_check(const spz_amd_photo_options *o) {
  if (o == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  if (o->fit_exposure != 0 && o->fit_exposure != 1) return SPZ_AMD_ERR_INVALID_ARG;
  if (!(o->lr_exposure >= 0.0) || !std::isfinite(o->lr_exposure)) return SPZ_AMD_ERR_INVALID_ARG;
  return SPZ_AMD_OK;
}

}  // extern "C"
