// spz_depth_loss.hip — the depth loss: a depth render against a measured depth map, and its gradient to the render
// (DESIGN §8 "Depth fit"; the contract is in include/spz_amd.h "depth loss").
//
//   spz_depth_loss_partial_kernel  one lane per pixel, f64 from the f32 values: the pixel's validity, its weight w and
//                                  w |e|; each workgroup's two sums by a fixed tree in LDS to its slot of the slab.
//   spz_depth_loss_reduce_kernel   one workgroup: the slab in a fixed order; L = sum w |e| / W_v and W_v out.
//   spz_depth_loss_grad_kernel     one lane per pixel: the same validity and e again, W_v read from device memory;
//                                  g_D to d_grad_depth (0 where invalid), g_alpha added to channel 3 of d_grad_image.
// No float atomics: a run repeats its bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "spz_amd.h"
#include "spz_common.hpp"
#include "spz_image_tile.hpp"

#pragma clang fp contract(off)

namespace spz_amd_detail {

constexpr uint32_t kDlThreads = 256;

struct DepthLossArgs {
  const float *depth;   // height x width x 2: channel 0 is read
  const float *image;   // height x width x 4: channel 3 is read
  const float *target;  // height x width
  const float *weight;  // may be null: all 1
  unsigned long long pixels;
  float min_alpha;
  int kind;
};

// One pixel's terms.  valid: w > 0, the target finite and > 0, alpha >= min_alpha in f32, D finite and > 0.
struct DepthLossPixel {
  double w, D, alpha, e;
  bool valid;
};

__device__ __forceinline__ DepthLossPixel depth_loss_pixel(const DepthLossArgs &a, unsigned long long p) {
  DepthLossPixel x;
  const float D = a.depth[p * 2u], alpha = a.image[p * 4u + 3u], t = a.target[p];
  const float w = a.weight != nullptr ? clamp01(a.weight[p]) : 1.0f;  // NaN -> 0, as the photo loss
  x.valid = w > 0.0f && t > 0.0f && t < __builtin_huge_valf() && alpha >= a.min_alpha && D > 0.0f &&
            D < __builtin_huge_valf();
  x.w = (double)w;
  x.D = (double)D;
  x.alpha = (double)alpha;
  x.e = 0.0;
  if (x.valid) x.e = a.kind == SPZ_AMD_DEPTH_L1 ? x.D / x.alpha - (double)t : x.alpha / x.D - 1.0 / (double)t;
  return x;
}

__global__ __launch_bounds__(kDlThreads) void spz_depth_loss_partial_kernel(const DepthLossArgs a,
                                                                            double *__restrict__ slab) {
  __shared__ double r[2][kDlThreads];
  const uint32_t tid = threadIdx.x;
  const unsigned long long p = (unsigned long long)blockIdx.x * kDlThreads + tid;
  double sw = 0.0, se = 0.0;
  if (p < a.pixels) {
    const DepthLossPixel x = depth_loss_pixel(a, p);
    if (x.valid) {
      sw = x.w;
      se = x.w * fabs(x.e);
    }
  }
  r[0][tid] = sw;
  r[1][tid] = se;
  __syncthreads();
  for (uint32_t s = kDlThreads / 2; s > 0; s >>= 1) {
    if (tid < s) {
      r[0][tid] += r[0][tid + s];
      r[1][tid] += r[1][tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    slab[2ull * blockIdx.x] = r[0][0];
    slab[2ull * blockIdx.x + 1ull] = r[1][0];
  }
}

// out[0] = L = sum w |e| / W_v (0 when W_v == 0), out[1] = W_v: a lane its strided slots, then a tree over the lanes.
__global__ __launch_bounds__(kDlThreads) void spz_depth_loss_reduce_kernel(const double *__restrict__ slab,
                                                                           uint32_t blocks, double *__restrict__ out) {
  __shared__ double r[2][kDlThreads];
  const uint32_t tid = threadIdx.x;
  double sw = 0.0, se = 0.0;
  for (uint32_t i = tid; i < blocks; i += kDlThreads) {
    sw += slab[2ull * i];
    se += slab[2ull * i + 1ull];
  }
  r[0][tid] = sw;
  r[1][tid] = se;
  __syncthreads();
  for (uint32_t s = kDlThreads / 2; s > 0; s >>= 1) {
    if (tid < s) {
      r[0][tid] += r[0][tid + s];
      r[1][tid] += r[1][tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    out[0] = r[0][0] == 0.0 ? 0.0 : r[1][0] / r[0][0];
    out[1] = r[0][0];
  }
}

// s = scale sign(e) w / W_v.  L1: g_D = s / alpha, g_alpha = -s D / alpha^2.  Inverse: g_D = -s alpha / D^2,
// g_alpha = s / D.  Each rounded once to f32.
__global__ __launch_bounds__(kDlThreads) void spz_depth_loss_grad_kernel(const DepthLossArgs a, double scale,
                                                                         const double *__restrict__ loss,
                                                                         float *__restrict__ grad_depth,
                                                                         float *__restrict__ grad_image) {
  const unsigned long long p = (unsigned long long)blockIdx.x * kDlThreads + threadIdx.x;
  if (p >= a.pixels) return;
  const DepthLossPixel x = depth_loss_pixel(a, p);
  const double Wv = loss[1];
  float gD = 0.0f, gA = 0.0f;
  if (x.valid && Wv > 0.0 && x.e != 0.0) {
    const double s = (scale * (x.e > 0.0 ? 1.0 : -1.0)) * x.w / Wv;
    if (a.kind == SPZ_AMD_DEPTH_L1) {
      gD = (float)(s / x.alpha);
      gA = (float)(-(s * x.D) / (x.alpha * x.alpha));
    } else {
      gD = (float)(-(s * x.alpha) / (x.D * x.D));
      gA = (float)(s / x.D);
    }
  }
  grad_depth[p] = gD;
  if (grad_image != nullptr) grad_image[p * 4u + 3u] = grad_image[p * 4u + 3u] + gA;
}

namespace {

uint32_t depth_loss_blocks(uint32_t w, uint32_t h) {
  return (uint32_t)(((uint64_t)w * h + kDlThreads - 1) / kDlThreads);
}

int depth_loss_enqueue(const float *d_depth, const float *d_image, const float *d_target, const float *d_weight,
                       int width, int height, int kind, float min_alpha, double scale, double *d_loss,
                       float *d_grad_depth, float *d_grad_image, void *d_workspace, hipStream_t st) {
  DepthLossArgs a = {};
  a.depth = d_depth;
  a.image = d_image;
  a.target = d_target;
  a.weight = d_weight;
  a.pixels = (unsigned long long)width * (unsigned long long)height;
  a.min_alpha = min_alpha;
  a.kind = kind;
  const uint32_t blocks = depth_loss_blocks((uint32_t)width, (uint32_t)height);
  auto *slab = reinterpret_cast<double *>(align_ws(d_workspace));
  hipLaunchKernelGGL(spz_depth_loss_partial_kernel, dim3(blocks), dim3(kDlThreads), 0, st, a, slab);
  SPZ_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(spz_depth_loss_reduce_kernel, dim3(1), dim3(kDlThreads), 0, st, slab, blocks, d_loss);
  SPZ_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(spz_depth_loss_grad_kernel, dim3(blocks), dim3(kDlThreads), 0, st, a, scale, d_loss, d_grad_depth,
                     d_grad_image);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

}  // namespace

}  // namespace spz_amd_detail

using namespace spz_amd_detail;

extern "C" {

uint64_t spz_amd_depth_loss_workspace_bytes(int width, int height) {
  if (width < 1 || height < 1 || (uint32_t)width > kMtMaxSide || (uint32_t)height > kMtMaxSide) return 0;
  // two doubles per workgroup, and room to align a caller's pointer up to 256
  return Workspace::aligned(16u * (uint64_t)depth_loss_blocks((uint32_t)width, (uint32_t)height)) + 256u;
}

int spz_amd_depth_loss_device(const float *d_depth, const float *d_image, const float *d_target, const float *d_weight,
                              int width, int height, int kind, float min_alpha, double scale, double *d_loss,
                              float *d_grad_depth, float *d_grad_image, void *d_workspace, void *hip_stream) {
  int rc = spz_amd_image_metrics_check(width, height, 4, 4);
  if (rc != SPZ_AMD_OK) return rc;
  if (kind != SPZ_AMD_DEPTH_L1 && kind != SPZ_AMD_DEPTH_INVERSE_L1) return SPZ_AMD_ERR_INVALID_ARG;
  if (!(min_alpha > 0.0f) || !(min_alpha <= 1.0f)) return SPZ_AMD_ERR_INVALID_ARG;
  if (!(scale >= 0.0) || !std::isfinite(scale)) return SPZ_AMD_ERR_INVALID_ARG;
  if (d_depth == nullptr || d_image == nullptr || d_target == nullptr || d_loss == nullptr || d_grad_depth == nullptr ||
      d_workspace == nullptr) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  if (!aligned_to(d_depth, 4) || !aligned_to(d_image, 4) || !aligned_to(d_target, 4) || !aligned_to(d_weight, 4) ||
      !aligned_to(d_loss, 8) || !aligned_to(d_grad_depth, 4) || !aligned_to(d_grad_image, 4)) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  return depth_loss_enqueue(d_depth, d_image, d_target, d_weight, width, height, kind, min_alpha, scale, d_loss,
                            d_grad_depth, d_grad_image, d_workspace, static_cast<hipStream_t>(hip_stream));
}

int spz_amd_depth_default_options(spz_amd_depth_options *options) {
  if (options == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  options->weight = 1.0;
  options->min_alpha = 0.5f;
  options->kind = SPZ_AMD_DEPTH_L1;
  return SPZ_AMD_OK;
}

int spz_amd_depth_check(const spz_amd_depth_options *o) {
  if (o == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  if (!(o->weight >= 0.0) || !std::isfinite(o->weight)) return SPZ_AMD_ERR_INVALID_ARG;
  if (!(o->min_alpha > 0.0f) || !(o->min_alpha <= 1.0f)) return SPZ_AMD_ERR_INVALID_ARG;
  if (o->kind != SPZ_AMD_DEPTH_L1 && o->kind != SPZ_AMD_DEPTH_INVERSE_L1) return SPZ_AMD_ERR_INVALID_ARG;
  return SPZ_AMD_OK;
}

}  // extern "C"
