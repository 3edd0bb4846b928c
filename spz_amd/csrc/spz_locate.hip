// spz_locate.hip — the pose of a camera in a scene, fitted to a picture (DESIGN §8 "Locate"; the contract is in
// include/spz_amd.h "locate").  Host code over the rasteriser's device entry points, the image loss and the view
// backward, and one small kernel:
//
//   spz_image_halve_kernel   the 2 x 2 box mean of an image, channels kept: one lane per output value, f32,
//                            ((top left + top right) + (bottom left + bottom right)) / 4.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "spz_amd.h"
#include "spz_common.hpp"
#include "spz_view_pass.hpp"

#pragma clang fp contract(off)

namespace spz_amd_detail {
namespace {

constexpr uint32_t kHalveBlock = 256;

__global__ __launch_bounds__(kHalveBlock) void spz_image_halve_kernel(const float *__restrict__ in, uint32_t channels,
                                                                       uint32_t width, uint32_t out_width,
                                                                       unsigned long long count, float *__restrict__ out) {
  const unsigned long long j = (unsigned long long)blockIdx.x * kHalveBlock + threadIdx.x;
  if (j >= count) return;
  const uint32_t ch = (uint32_t)(j % channels);
  const unsigned long long px = j / channels;
  const unsigned long long x = px % out_width, y = px / out_width;
  const unsigned long long row = (unsigned long long)width * channels;
  const float *a = in + (2u * y) * row + (2u * x) * channels + ch;
  out[j] = ((a[0] + a[channels]) + (a[row] + a[row + channels])) * 0.25f;
}

// Exp(w) of so(3) by Rodrigues' formula, row-major; below |w| = 1e-4 the series of sin t / t and (1 - cos t) / t^2.
void so3_exp(const double w[3], double E[9]) {
  const double t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  double A, B;
  if (t2 < 1e-8) {
    A = 1.0 - t2 / 6.0;
    B = 0.5 - t2 / 24.0;
  } else {
    const double t = std::sqrt(t2);
    A = std::sin(t) / t;
    B = (1.0 - std::cos(t)) / t2;
  }
  const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) {
      const double k2 = K[r * 3] * K[c] + K[r * 3 + 1] * K[3 + c] + K[r * 3 + 2] * K[6 + c];
      E[r * 3 + c] = (r == c ? 1.0 : 0.0) + A * K[r * 3 + c] + B * k2;
    }
  }
}

}  // namespace
}  // namespace spz_amd_detail

using namespace spz_amd_detail;

extern "C" {

int spz_amd_image_halve_device(const float *d_in, int channels, int width, int height, float *d_out, void *hip_stream) {
  int rc = spz_amd_image_metrics_check(width, height, channels, channels);
  if (rc != SPZ_AMD_OK) return rc;
  if ((width & 1) || (height & 1) || d_in == nullptr || d_out == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  const uint32_t ow = (uint32_t)width / 2u, oh = (uint32_t)height / 2u;
  const unsigned long long count = (unsigned long long)ow * oh * (unsigned)channels;
  hipLaunchKernelGGL(spz_image_halve_kernel, dim3((unsigned)((count + kHalveBlock - 1) / kHalveBlock)), dim3(kHalveBlock),
                     0, static_cast<hipStream_t>(hip_stream), d_in, (uint32_t)channels, (uint32_t)width, ow, count, d_out);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

int spz_amd_locate_default_options(spz_amd_locate_options *options) {
  if (options == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  std::memset(options, 0, sizeof(*options));
  options->iterations = 300;
  options->levels = 1;
  options->lambda_dssim = 0.2;
  options->lr_rotation = 2e-3;
  options->lr_translation = 2e-3;  // for a camera at unit distance: the layers above scale it
  options->lr_final_factor = 0.1;
  options->beta1 = 0.9;
  options->beta2 = 0.999;
  options->eps = 1e-15;
  return SPZ_AMD_OK;
}

int spz_amd_locate_check(const spz_amd_locate_options *o) {
  if (o == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  if (o->iterations < 0 || o->levels < 1 || o->levels > SPZ_AMD_LOCATE_MAX_LEVELS) return SPZ_AMD_ERR_INVALID_ARG;
  if (!(o->lambda_dssim >= 0.0) || !(o->lambda_dssim <= 1.0)) return SPZ_AMD_ERR_INVALID_ARG;
  if (!(o->lr_rotation >= 0.0) || !std::isfinite(o->lr_rotation)) return SPZ_AMD_ERR_INVALID_ARG;
  if (!(o->lr_translation >= 0.0) || !std::isfinite(o->lr_translation)) return SPZ_AMD_ERR_INVALID_ARG;
  if (!(o->lr_final_factor > 0.0) || !(o->lr_final_factor <= 1.0)) return SPZ_AMD_ERR_INVALID_ARG;
  if (!(o->beta1 >= 0.0) || !(o->beta1 < 1.0) || !(o->beta2 >= 0.0) || !(o->beta2 < 1.0)) return SPZ_AMD_ERR_INVALID_ARG;
  if (!(o->eps >= 0.0) || !std::isfinite(o->eps)) return SPZ_AMD_ERR_INVALID_ARG;
  return SPZ_AMD_OK;
}

int spz_amd_locate_level_params(const spz_amd_render_params *params, int level, spz_amd_render_params *out) {
  if (params == nullptr || out == nullptr || level < 0 || level >= SPZ_AMD_LOCATE_MAX_LEVELS) return SPZ_AMD_ERR_INVALID_ARG;
  const uint32_t f = 1u << level;
  if (params->width % f != 0u || params->height % f != 0u) return SPZ_AMD_ERR_INVALID_ARG;
  *out = *params;
  out->width = params->width / f;
  out->height = params->height / f;
  out->fx = params->fx / (float)f;  // exact: a power of two
  out->fy = params->fy / (float)f;
  out->cx = params->cx / (float)f;
  out->cy = params->cy / (float)f;
  return spz_amd_render_check_params(out);
}

int spz_amd_locate_twist_gradient(const double pose[12], const double view_grad[12], double twist_grad[6]) {
  if (pose == nullptr || view_grad == nullptr || twist_grad == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  double A[9];  // G_R R^T + G_t t^T
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) {
      A[r * 3 + c] = (view_grad[r * 4] * pose[c * 4] + view_grad[r * 4 + 1] * pose[c * 4 + 1] +
                      view_grad[r * 4 + 2] * pose[c * 4 + 2]) +
                     view_grad[r * 4 + 3] * pose[c * 4 + 3];
    }
  }
  twist_grad[0] = A[7] - A[5];
  twist_grad[1] = A[2] - A[6];
  twist_grad[2] = A[3] - A[1];
  for (int k = 0; k < 3; ++k) twist_grad[3 + k] = view_grad[k * 4 + 3];
  return SPZ_AMD_OK;
}

int spz_amd_locate_pose_step(const spz_amd_locate_options *options, int iteration, const double twist_grad[6],
                             double m[6], double v[6], double pose[12]) {
  int rc = spz_amd_locate_check(options);
  if (rc != SPZ_AMD_OK) return rc;
  if (twist_grad == nullptr || m == nullptr || v == nullptr || pose == nullptr || iteration < 0 ||
      iteration >= options->iterations) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  const double f = std::pow(options->lr_final_factor, (double)iteration / (double)options->iterations);
  const double b1 = options->beta1, b2 = options->beta2;
  const double k1 = 1.0 - std::pow(b1, (double)(iteration + 1)), k2 = 1.0 - std::pow(b2, (double)(iteration + 1));
  double d[6];
  for (int k = 0; k < 6; ++k) {
    const double g = twist_grad[k];
    m[k] = b1 * m[k] + (1.0 - b1) * g;
    v[k] = b2 * v[k] + (1.0 - b2) * g * g;
    const double lr = (k < 3 ? options->lr_rotation : options->lr_translation) * f;
    d[k] = m[k] == 0.0 ? 0.0 : -lr * (m[k] / k1) / (std::sqrt(v[k] / k2) + options->eps);  // 0 / 0 with eps = 0
  }
  double E[9];
  so3_exp(d, E);
  double next[12];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 4; ++c) next[r * 4 + c] = E[r * 3] * pose[c] + E[r * 3 + 1] * pose[4 + c] + E[r * 3 + 2] * pose[8 + c];
    next[r * 4 + 3] = next[r * 4 + 3] + d[3 + r];
  }
  std::memcpy(pose, next, sizeof(next));
  return SPZ_AMD_OK;
}

}  // extern "C"

namespace {

// The run of every entry: a packed stream (input.hdr set) or a float cloud already in device memory; the target in
// device memory, or in host memory (host_target) and uploaded once.
int locate_run(const RenderSource &input, const spz_amd_render_params *params, const float *target_in, bool host_target,
               int channels, const spz_amd_locate_options *options, int device, float *h_world_to_camera, double *h_history,
               spz_amd_image_metrics *h_before, spz_amd_image_metrics *h_after, int32_t *h_iterations, float *h_ms) {
  if (h_iterations) *h_iterations = 0;
  int rc = spz_amd_locate_check(options);
  if (rc != SPZ_AMD_OK) return rc;
  rc = spz_amd_render_check_params(params);
  if (rc != SPZ_AMD_OK) return rc;
  if (target_in == nullptr || h_world_to_camera == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  rc = spz_amd_image_metrics_check((int)params->width, (int)params->height, 4, channels);
  if (rc != SPZ_AMD_OK) return rc;
  const int iters = options->iterations, levels = options->levels;
  if (iters > 0 && h_history == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  std::vector<spz_amd_render_params> lp((size_t)levels);
  for (int k = 0; k < levels; ++k) {
    rc = spz_amd_locate_level_params(params, k, &lp[(size_t)k]);
    if (rc != SPZ_AMD_OK) return rc;
  }
  const uint64_t n = input.n;
  int deg = input.sh_degree, aa = input.antialiased;
  if (input.cloud == nullptr) {
    rc = check_render_input(input.d_stream, input.size, input.hdr);
    if (rc != SPZ_AMD_OK) return rc;
    deg = input.hdr->sh_degree;
    aa = input.hdr->flags & 1;
  } else {
    const int sd = sh_dim_for_degree(deg);
    if (sd < 0) return SPZ_AMD_ERR_INVALID_ARG;
    if (n > kMaxEntries) return SPZ_AMD_ERR_TOO_MANY_POINTS;
    const spz_amd_cloud_in *cl = input.cloud;
    if (n && (!cl->positions || !cl->scales || !cl->rotations || !cl->alphas || !cl->colors || (sd > 0 && !cl->sh))) {
      return SPZ_AMD_ERR_INVALID_ARG;
    }
  }
  DeviceGuard guard;
  rc = guard.enter(device);
  if (rc != SPZ_AMD_OK) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  PackedResultPtr c;  // the stream and the two allocations, freed on every return
  rc = packed_result_open(device, &c);
  if (rc != SPZ_AMD_OK) return rc;

  const uint64_t W = params->width, H = params->height;
  const uint64_t sd = (uint64_t)sh_dim_for_degree(deg);
  const uint64_t count[6] = {3u * n, 3u * n, 4u * n, n, 3u * n, 3u * sd * n};
  const bool decode = input.cloud == nullptr && iters > 0 && n > 0;
  WorkspaceOffsets o;
  uint64_t c_off[6];
  for (int k = 0; k < 6; ++k) c_off[k] = o.put(decode ? count[k] * 4u : 0u);
  std::vector<uint64_t> t_off((size_t)levels, 0);
  for (int k = 1; k < levels; ++k) t_off[(size_t)k] = o.put((W >> k) * (H >> k) * (uint64_t)channels * 4u);
  const uint64_t o_image = o.put(16u * W * H), o_grad = o.put(iters ? 16u * W * H : 0u),
                 o_lws = o.put(iters ? spz_amd_image_loss_workspace_bytes((int)W, (int)H) : 0u),
                 o_mws = o.put(spz_amd_image_metrics_workspace_bytes((int)W, (int)H)), o_small = o.put(16u),
                 o_loss = o.put(24u * (uint64_t)iters), o_metrics = o.put(2u * sizeof(spz_amd_image_metrics)),
                 o_rg = o.put(iters ? n * 36u : 0u), o_vg = o.put(12u * sizeof(double)),
                 o_vws = o.put(iters ? spz_amd_render_view_backward_workspace_bytes(n) : 0u),
                 o_target = o.put(host_target ? W * H * (uint64_t)channels * 4u : 0u);
  SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&c->block), o.off + 256u));
  uint8_t *raw = c->block;  // every section is 256-aligned from hipMalloc's base
  const float *d_target = target_in;
  if (host_target) {
    SPZ_HIP_TRY(hipMemcpyAsync(raw + o_target, target_in, W * H * (uint64_t)channels * 4u, hipMemcpyHostToDevice, c->st));
    d_target = reinterpret_cast<const float *>(raw + o_target);
  }
  auto *d_image = reinterpret_cast<float *>(raw + o_image);
  auto *d_grad = reinterpret_cast<float *>(raw + o_grad);
  auto *d_total = reinterpret_cast<uint64_t *>(raw + o_small);
  auto *d_status = reinterpret_cast<uint32_t *>(raw + o_small + 8u);
  auto *d_loss = reinterpret_cast<double *>(raw + o_loss);
  auto *d_metrics = reinterpret_cast<spz_amd_image_metrics *>(raw + o_metrics);
  auto *d_rg = reinterpret_cast<float *>(raw + o_rg);
  auto *d_vg = reinterpret_cast<double *>(raw + o_vg);
  auto target = [&](int k) { return k == 0 ? d_target : reinterpret_cast<const float *>(raw + t_off[(size_t)k]); };

  uint64_t cap = 0, total = 0;
  spz_amd_render_params cur = *params;  // the given view with the pose of the moment
  auto metrics = [&](spz_amd_image_metrics *d_out) {
    int r = render_view(&c->scratch, &cap, input, &cur, d_total, d_status, d_image, c->st, &total);
    if (r != SPZ_AMD_OK) return r;
    return spz_amd_image_metrics_device(d_image, 4, d_target, channels, (int)W, (int)H, d_out, nullptr, raw + o_mws, c->st);
  };
  rc = metrics(d_metrics);
  if (rc != SPZ_AMD_OK) return rc;
  SPZ_HIP_TRY(hipStreamSynchronize(c->st));
  const double before_ms = ms_since(t0);

  double pose[12];
  for (int k = 0; k < 12; ++k) pose[k] = params->world_to_camera[k];
  int ran = 0;
  if (iters > 0) {
    spz_amd_cloud_in cloud = {};
    if (decode) {
      float *a[6];
      for (int k = 0; k < 6; ++k) a[k] = count[k] ? reinterpret_cast<float *>(raw + c_off[k]) : nullptr;
      const spz_amd_cloud_out dec = {a[0], a[1], a[2], a[3], a[4], a[5]};
      rc = spz_amd_decode_device(input.d_stream, input.size, input.hdr, params->coord, &dec, c->st);
      if (rc != SPZ_AMD_OK) return rc;
      cloud = spz_amd_cloud_in{a[0], a[1], a[2], a[3], a[4], a[5]};
    } else if (input.cloud != nullptr) {
      cloud = *input.cloud;
    }
    for (int k = 1; k < levels; ++k) {  // the k-fold box mean of the target
      rc = spz_amd_image_halve_device(target(k - 1), channels, (int)(W >> (k - 1)), (int)(H >> (k - 1)),
                                      const_cast<float *>(target(k)), c->st);
      if (rc != SPZ_AMD_OK) return rc;
    }
    RenderSource src_f;
    src_f.cloud = &cloud;
    src_f.n = n;
    src_f.sh_degree = deg;
    src_f.antialiased = aa;
    double m[6] = {0, 0, 0, 0, 0, 0}, v[6] = {0, 0, 0, 0, 0, 0};
    const int per = iters / levels;
    bool stop = false;
    for (int k = levels - 1, i = 0; k >= 0 && !stop; --k) {
      const int until = k == 0 ? iters : i + per;  // the remainder goes to level 0
      spz_amd_render_params p = lp[(size_t)k];
      for (; i < until; ++i) {
        for (int e = 0; e < 12; ++e) p.world_to_camera[e] = (float)pose[e];
        rc = render_view(&c->scratch, &cap, src_f, &p, d_total, d_status, d_image, c->st, &total);
        if (rc != SPZ_AMD_OK) return rc;
        rc = spz_amd_image_loss_device(d_image, 4, target(k), channels, (int)p.width, (int)p.height, options->lambda_dssim,
                                       d_loss + 3 * (size_t)i, d_grad, raw + o_lws, c->st);
        if (rc != SPZ_AMD_OK) return rc;
        rc = spz_amd_render_records_backward_device(n, &p, total, d_grad, d_rg, d_status, c->scratch, c->st);
        if (rc != SPZ_AMD_OK) return rc;
        rc = spz_amd_render_view_backward_device(&cloud, n, deg, aa, &p, total, d_rg, d_vg, d_status, c->scratch,
                                                 raw + o_vws, c->st);
        if (rc != SPZ_AMD_OK) return rc;
        double G[12];
        SPZ_HIP_TRY(hipMemcpyAsync(G, d_vg, sizeof(G), hipMemcpyDeviceToHost, c->st));
        SPZ_HIP_TRY(hipStreamSynchronize(c->st));
        bool finite = true;
        for (int e = 0; e < 12; ++e) finite = finite && std::isfinite(G[e]);
        if (!finite) {
          stop = true;
          break;
        }
        double g[6];
        (void)spz_amd_locate_twist_gradient(pose, G, g);
        rc = spz_amd_locate_pose_step(options, i, g, m, v, pose);
        if (rc != SPZ_AMD_OK) return rc;
        ran = i + 1;
      }
    }
  }
  const double loop_ms = ms_since(t0) - before_ms;

  for (int e = 0; e < 12; ++e) cur.world_to_camera[e] = (float)pose[e];
  if (ran > 0) {
    rc = metrics(d_metrics + 1);
    if (rc != SPZ_AMD_OK) return rc;
  }
  spz_amd_image_metrics hm[2];
  SPZ_HIP_TRY(hipMemcpyAsync(hm, d_metrics, sizeof(hm), hipMemcpyDeviceToHost, c->st));
  std::vector<double> loss3(3u * (size_t)ran);
  if (ran) SPZ_HIP_TRY(hipMemcpyAsync(loss3.data(), d_loss, 24u * (size_t)ran, hipMemcpyDeviceToHost, c->st));
  SPZ_HIP_TRY(hipStreamSynchronize(c->st));
  if (h_before) *h_before = hm[0];
  if (h_after) *h_after = ran > 0 ? hm[1] : hm[0];
  for (int i = 0; i < iters; ++i) h_history[i] = i < ran ? loss3[3u * (size_t)i] : 0.0;
  for (int e = 0; e < 12; ++e) h_world_to_camera[e] = cur.world_to_camera[e];
  if (h_iterations) *h_iterations = ran;
  if (h_ms) {
    h_ms[0] = (float)before_ms;
    h_ms[1] = (float)loop_ms;
    h_ms[2] = (float)(ms_since(t0) - before_ms - loop_ms);
  }
  return SPZ_AMD_OK;
}

}  // namespace

extern "C" {

int spz_amd_locate_host(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr,
                        const spz_amd_render_params *params, const float *d_target, int channels,
                        const spz_amd_locate_options *options, int device, float *h_world_to_camera, double *h_history,
                        spz_amd_image_metrics *h_before, spz_amd_image_metrics *h_after, int32_t *h_iterations,
                        float *h_ms) {
  if (d_stream == nullptr || hdr == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  return locate_run(packed_render_source(d_stream, size, hdr), params, d_target, false, channels, options, device,
                    h_world_to_camera, h_history, h_before, h_after, h_iterations, h_ms);
}

int spz_amd_locate_image_host(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr,
                              const spz_amd_render_params *params, const float *h_target, int channels,
                              const spz_amd_locate_options *options, int device, float *h_world_to_camera,
                              double *h_history, spz_amd_image_metrics *h_before, spz_amd_image_metrics *h_after,
                              int32_t *h_iterations, float *h_ms) {
  if (d_stream == nullptr || hdr == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  return locate_run(packed_render_source(d_stream, size, hdr), params, h_target, true, channels, options, device,
                    h_world_to_camera, h_history, h_before, h_after, h_iterations, h_ms);
}

int spz_amd_locate_cloud_host(const spz_amd_cloud_in *d_cloud, uint64_t num_points, int sh_degree, int antialiased,
                              const spz_amd_render_params *params, const float *d_target, int channels,
                              const spz_amd_locate_options *options, int device, float *h_world_to_camera,
                              double *h_history, spz_amd_image_metrics *h_before, spz_amd_image_metrics *h_after,
                              int32_t *h_iterations, float *h_ms) {
  if (d_cloud == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  RenderSource src;
  src.cloud = d_cloud;
  src.n = num_points;
  src.sh_degree = sh_degree;
  src.antialiased = antialiased ? 1 : 0;
  return locate_run(src, params, d_target, false, channels, options, device, h_world_to_camera, h_history, h_before, h_after,
                    h_iterations, h_ms);
}

}  // extern "C"
