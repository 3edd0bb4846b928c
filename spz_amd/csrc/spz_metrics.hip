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
//   spz_loss_tile_kernel           the same tile body (metrics_tile_body of spz_image_tile.hpp, which the photo loss of
//                                  spz_photo.hip shares as well): beside the partial sums, the three
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
#include "spz_image_tile.hpp"
#include "spz_view_pass.hpp"

namespace spz_amd_detail {

__global__ __launch_bounds__(kMtThreads) void spz_metrics_tile_kernel(const float *__restrict__ a, uint32_t ca,
                                                                      const float *__restrict__ b, uint32_t cb,
                                                                      uint32_t width, uint32_t height, uint32_t tiles_x,
                                                                      uint32_t tiles, MetricsWindow win,
                                                                      float *__restrict__ map, double *__restrict__ slab) {
  metrics_tile_body<kTileMetrics>(a, ca, b, cb, width, height, tiles_x, tiles, win, map, nullptr, slab, nullptr);
}

__global__ __launch_bounds__(kMtThreads) void spz_loss_tile_kernel(const float *__restrict__ a, uint32_t ca,
                                                                   const float *__restrict__ b, uint32_t cb,
                                                                   uint32_t width, uint32_t height, uint32_t tiles_x,
                                                                   uint32_t tiles, MetricsWindow win,
                                                                   double *__restrict__ dmaps, double *__restrict__ slab) {
  metrics_tile_body<kTileLoss>(a, ca, b, cb, width, height, tiles_x, tiles, win, nullptr, dmaps, slab, nullptr);
}

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

// dL/da of one 32x16 tile (loss_grad_body of spz_image_tile.hpp).
__global__ __launch_bounds__(kMtThreads) void spz_loss_grad_kernel(const float *__restrict__ a, uint32_t ca,
                                                                   const float *__restrict__ b, uint32_t cb,
                                                                   uint32_t width, uint32_t height, uint32_t tiles_x,
                                                                   MetricsWindow win, const double *__restrict__ dmaps,
                                                                   double lambda, double count,
                                                                   float *__restrict__ grad) {
  loss_grad_body<false>(a, ca, b, cb, width, height, tiles_x, win, dmaps, lambda, count, grad, nullptr, nullptr,
                        nullptr);
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
