// spz_render_backward.hip — the gradients of one rendered view to a float cloud (DESIGN §8 "Render backward"; the
// contract is in include/spz_amd.h "render backward").  Reads the workspace as spz_amd_render_finish_device left it.
//
//   spz_render_blend_backward_kernel       the forward's geometry: one 256-lane workgroup per 16x16 tile, one pixel per
//                                          lane, the tile's records staged in LDS 256 at a time.  It walks the tile's
//                                          list twice, front to back both times: first the forward blend again, bit for
//                                          bit, for the pixel's final C and T; then the same loop in step across each
//                                          wave, forming every used pair's gradient to the record's nine floats from
//                                          the prefix and "what lies behind" = final - prefix.  The nine values are
//                                          summed over the wave by DPP, one lane per wave adds them into the batch's
//                                          LDS slots, and each non-zero slot value goes to the n x 9 record gradients
//                                          by one global f32 atomic.
//   spz_render_depth_blend_backward_kernel the same body (blend_backward_body, which both kernels instantiate) with the
//                                          depth sum of spz_render_depth_kernel in it ("render depth backward"; DESIGN
//                                          §8 "Depth fit"): the record's depth, less the depth of the tile's first
//                                          entry, rides in the .w of the staged rgb, D is blended beside the colour,
//                                          and a tenth value per used pair, dL/dz, goes to an array of its own (n
//                                          floats), so the n x 9 layout stays what the chain and the view backward
//                                          read.
//   spz_render_preprocess_backward_kernel  one lane per Gaussian, f64 like the forward preprocess: the forward's
//                                          intermediates again from the floats and the camera, then the chain from the
//                                          nine record gradients to positions, log scales, raw quaternion, alpha,
//                                          colour and sh.  Writes every output element once (zeros for an invisible
//                                          Gaussian and for sh above the used degree); no atomics.  With the depth
//                                          gradients given, dL/dp += R[2, :] dL/dz (z is the record's depth,
//                                          rounded to f32 straight through); without them every bit is as before.
//                                          The lane's work is preprocess_backward_one
//                                          (spz_preprocess_backward_core.hpp: host and device).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "spz_amd.h"
#include "spz_common.hpp"
#include "spz_preprocess_backward_core.hpp"
#include "spz_render_internal.hpp"

#pragma clang fp contract(off)

namespace spz_amd_detail {

struct BlendBackwardParams {
  const spz_amd_render_record *rec;
  const uint32_t *sorted_gid;
  const uint2 *ranges;
  const unsigned long long *total;
  const float *grad_image;  // height x width x 4
  float *rec_grad;          // n x 9, zeroed; added into
  unsigned long long max_entries;
  uint32_t width, height, tiles_x;
  float bg[3];
};

struct DepthBlendBackwardParams {
  BlendBackwardParams b;    // b.grad_image may be null: all zero
  const float *grad_depth;  // height x width: the gradient to channel 0 of the depth map
  float *depth_grad;        // n, zeroed; added into
};

// The body of both blend backward kernels: the colour one (kDepth false) and the one with the depth sum of
// spz_render_depth_kernel in it (kDepth true: "render depth backward").
//
// Colour.  power, a, T' and the three tests are the expressions of spz_render_blend_kernel, so both passes use the
// pairs the image used.  With I = C + T_final bg and alpha = 1 - T_final, g the pixel's gradient, and for a used pair i
// (T before it, w = T a, C_i the prefix that includes it):
//   dL/drgb_i = w g_rgb
//   dL/da_i   = T (g_rgb . rgb_i) - (g_rgb . (C_final - C_i) + tail) / (1 - a)
//   tail      = T_final (g_rgb . bg - g_alpha)
// a = min(0.99, opacity e^power) hands dL/da to opacity and power only where it does not clamp.
//
// Depth.  s_rgb[k].w carries the record's depth z, D += (T a) z beside the colour sums, and a tenth value per used
// pair.  With g_D the pixel's gradient to D, D_i the prefix that includes pair i and D_final the pixel's sum:
//   dL/dz_i = w g_D
//   dL/da_i = T (g_rgb . rgb_i + g_D z_i) - (g_rgb . (C_final - C_i) + g_D (D_final - D_i) + tail) / (1 - a)
// D_final - D_i is a difference of two long f32 sums of w z, and at camera depths far above the depth range of a tile's
// list it cancels most of their digits.  So both walks sum w (z - z0) instead, z0 the depth of the tile's first (nearest)
// entry: D = D' + z0 (1 - T_final), which is the same loss with z - z0 for z and g_alpha + g_D z0 for g_alpha:
//   dL/da_i = T (g_rgb . rgb_i + g_D (z_i - z0)) - (g_rgb . (C_final - C_i) + g_D (D'_final - D'_i) + tail') / (1 - a)
//   tail'   = T_final (g_rgb . bg - g_alpha - g_D z0)
// dL/dz_i is unchanged.  The tenth sum goes to an array of its own, so the n x 9 layout stays.
//
// The colour instance stages 0 in s_rgb[k].w, reads no depth, no z0 and no grad_depth, and reads grad_image without a
// null check; every depth term is added after the colour terms of its sum, so each instance rounds as its formula reads.
template <bool kDepth>
__device__ __forceinline__ void blend_backward_body(const BlendBackwardParams &p, const float *grad_depth,
                                                    float *depth_grad) {
  constexpr uint32_t kGrads = kDepth ? kRecGrads + 1 : kRecGrads;  // and the record's depth z
  __shared__ float2 s_xy[kBlendThreads];
  __shared__ float4 s_co[kBlendThreads];   // conic A, B, C, opacity
  __shared__ float4 s_rgb[kBlendThreads];  // rgb, z - z0 (0 without the depth)
  __shared__ float s_grad[kGrads][kBlendThreads];
  const unsigned long long total = *p.total;
  if (total > p.max_entries) return;
  const uint32_t t = threadIdx.x;
  const uint32_t u = blockIdx.x * kTile + (t % kTile), v = blockIdx.y * kTile + (t / kTile);
  const bool inside = u < p.width && v < p.height;
  uint32_t begin = 0, end = 0;
  if (total != 0ull) {
    const uint2 r = p.ranges[blockIdx.y * p.tiles_x + blockIdx.x];
    begin = r.x;
    end = r.y;
  }
  if (begin >= end) return;  // workgroup-uniform: nothing blends here
  const float fu = (float)u, fv = (float)v;
  float z0 = 0.0f;
  if constexpr (kDepth) z0 = p.rec[p.sorted_gid[begin]].depth;  // workgroup-uniform: the list is in depth order
  // the forward blend, for the pixel's final colour sum, depth sum (of z - z0) and T
  float T = 1.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, D = 0.0f;
  bool done = !inside;
  for (uint32_t base = begin; base < end; base += kBlendThreads) {
    // also the barrier between the previous batch's reads and this batch's writes
    if (__syncthreads_count(done ? 1 : 0) == (int)kBlendThreads) break;
    const uint32_t j = base + t;
    if (j < end) {
      const spz_amd_render_record &q = p.rec[p.sorted_gid[j]];
      s_xy[t] = make_float2(q.mean[0], q.mean[1]);
      s_co[t] = make_float4(q.conic[0], q.conic[1], q.conic[2], q.opacity);
      s_rgb[t] = make_float4(q.rgb[0], q.rgb[1], q.rgb[2], kDepth ? q.depth - z0 : 0.0f);
    }
    __syncthreads();
    const uint32_t cnt = (end - base) < kBlendThreads ? end - base : kBlendThreads;
    for (uint32_t k = 0; k < cnt && !done; ++k) {
      const float2 xy = s_xy[k];
      const float4 co = s_co[k];
      const float dx = fu - xy.x, dy = fv - xy.y;
      const float power = -0.5f * (co.x * dx * dx + co.z * dy * dy) - co.y * dx * dy;
      if (power > 0.0f) continue;
      const float a = fminf(0.99f, co.w * expf(power));
      if (a < 1.0f / 255.0f) continue;
      const float Tn = T * (1.0f - a);
      if (Tn < 1e-4f) {
        done = true;
        break;
      }
      const float4 rgbz = s_rgb[k];
      const float w = T * a;
      c0 = c0 + w * rgbz.x;
      c1 = c1 + w * rgbz.y;
      c2 = c2 + w * rgbz.z;
      if constexpr (kDepth) D = D + w * rgbz.w;
      T = Tn;
    }
  }
  const float f0 = c0, f1 = c1, f2 = c2, fD = D;
  float g0 = 0.0f, g1 = 0.0f, g2 = 0.0f, g3 = 0.0f, gD = 0.0f;
  if (inside) {
    const unsigned long long at = (unsigned long long)v * p.width + u;
    if (!kDepth || p.grad_image) {  // only the depth kernel's may be null
      const float *g = p.grad_image + at * 4u;
      g0 = g[0];
      g1 = g[1];
      g2 = g[2];
      g3 = g[3];
    }
    if constexpr (kDepth) gD = grad_depth[at];
  }
  // the background and the alpha channel, and with the depth z0 (1 - T_final)
  float tail = (g0 * p.bg[0] + g1 * p.bg[1] + g2 * p.bg[2]) - g3;
  if constexpr (kDepth) tail = tail - gD * z0;
  tail = T * tail;
  // the same walk again, in step across the wave (a stopped lane takes no more pairs)
  T = 1.0f;
  c0 = 0.0f;
  c1 = 0.0f;
  c2 = 0.0f;
  D = 0.0f;
  done = !inside;
  for (uint32_t base = begin; base < end; base += kBlendThreads) {
    // also the barrier between the previous batch's reads and this batch's writes
    if (__syncthreads_count(done ? 1 : 0) == (int)kBlendThreads) break;
    const uint32_t j = base + t;
    uint32_t gid = 0;
    if (j < end) {
      gid = p.sorted_gid[j];
      const spz_amd_render_record &q = p.rec[gid];
      s_xy[t] = make_float2(q.mean[0], q.mean[1]);
      s_co[t] = make_float4(q.conic[0], q.conic[1], q.conic[2], q.opacity);
      s_rgb[t] = make_float4(q.rgb[0], q.rgb[1], q.rgb[2], kDepth ? q.depth - z0 : 0.0f);
    }
#pragma unroll
    for (uint32_t e = 0; e < kGrads; ++e) s_grad[e][t] = 0.0f;
    __syncthreads();
    const uint32_t cnt = (end - base) < kBlendThreads ? end - base : kBlendThreads;
    for (uint32_t k = 0; k < cnt; ++k) {
      if (__ballot(!done) == 0ull) break;  // wave-uniform: every lane of the wave has stopped
      const float2 xy = s_xy[k];
      const float4 co = s_co[k];
      const float dx = fu - xy.x, dy = fv - xy.y;
      const float power = -0.5f * (co.x * dx * dx + co.z * dy * dy) - co.y * dx * dy;
      const float ex = expf(power);
      const float raw = co.w * ex;
      const float a = fminf(0.99f, raw);
      const float Tn = T * (1.0f - a);
      bool use = !done && !(power > 0.0f) && !(a < 1.0f / 255.0f);
      if (use && Tn < 1e-4f) {
        done = true;
        use = false;
      }
      if (__ballot(use) == 0ull) continue;  // wave-uniform
      float d[kGrads] = {};
      if (use) {
        const float4 rgbz = s_rgb[k];
        const float w = T * a;
        c0 = c0 + w * rgbz.x;
        c1 = c1 + w * rgbz.y;
        c2 = c2 + w * rgbz.z;
        float front = g0 * rgbz.x + g1 * rgbz.y + g2 * rgbz.z;
        float behind = g0 * (f0 - c0) + g1 * (f1 - c1) + g2 * (f2 - c2);
        if constexpr (kDepth) {
          D = D + w * rgbz.w;
          front = front + gD * rgbz.w;
          behind = behind + gD * (fD - D);
          d[kRecGrads] = w * gD;
        }
        behind = behind + tail;
        const float da = T * front - behind / (1.0f - a);
        d[6] = w * g0;
        d[7] = w * g1;
        d[8] = w * g2;
        if (!(raw > 0.99f)) {  // a is opacity e^power
          const float dp = da * raw;
          d[0] = dp * (co.x * dx + co.y * dy);
          d[1] = dp * (co.z * dy + co.y * dx);
          d[2] = dp * (-0.5f * dx * dx);
          d[3] = dp * (-(dx * dy));
          d[4] = dp * (-0.5f * dy * dy);
          d[5] = da * ex;
        }
        T = Tn;
      }
#pragma unroll
      for (uint32_t e = 0; e < kGrads; ++e) d[e] = wave_sum_f32(d[e]);
      if ((t & 63u) == 0u) {
#pragma unroll
        for (uint32_t e = 0; e < kGrads; ++e) atomicAdd(&s_grad[e][k], d[e]);
      }
    }
    __syncthreads();
    if (j < end) {
      float *o = p.rec_grad + (unsigned long long)gid * kRecGrads;
#pragma unroll
      for (uint32_t e = 0; e < kRecGrads; ++e) {
        const float s = s_grad[e][t];
        if (s != 0.0f) atomicAdd(o + e, s);
      }
      if constexpr (kDepth) {
        const float s = s_grad[kRecGrads][t];
        if (s != 0.0f) atomicAdd(depth_grad + gid, s);
      }
    }
  }
}

// The two entries keep their names and parameter blocks (the tools and the recorded profiles find them by name).
__global__ __launch_bounds__(kBlendThreads) void spz_render_blend_backward_kernel(const BlendBackwardParams p) {
  blend_backward_body<false>(p, nullptr, nullptr);
}

__global__ __launch_bounds__(kBlendThreads) void spz_render_depth_blend_backward_kernel(const DepthBlendBackwardParams pp) {
  blend_backward_body<true>(pp.b, pp.grad_depth, pp.depth_grad);
}

__global__ __launch_bounds__(kPreBlock) void spz_render_preprocess_backward_kernel(const PreprocessBackwardParams p) {
  const uint32_t i = blockIdx.x * kPreBlock + threadIdx.x;
  if (*p.total > p.max_entries) {
    if (i == 0u) *p.status = 1u;
    return;
  }
  if (i < p.n) preprocess_backward_one(p, i);
}

}  // namespace spz_amd_detail

using namespace spz_amd_detail;

namespace {

// render_backward_device (d_grad_depth null: the colour blend backward, d_grad_image required) and
// render_depth_backward_device (d_grad_depth given: the depth blend backward, d_grad_image may be null) are one
// sequence: clear the record gradients, the blend backward, the per-Gaussian chain.
int backward_impl(const spz_amd_cloud_in *d_cloud, uint64_t num_points, int sh_degree, int antialiased,
                  const spz_amd_render_params *params, uint64_t max_entries, const float *d_grad_image,
                  const float *d_grad_depth, bool depth, const spz_amd_cloud_grads *d_grads, float *d_record_grads,
                  float *d_depth_grads, uint32_t *d_status, const void *d_render_workspace, void *d_backward_workspace,
                  void *hip_stream) {
  int rc = check_params(params);
  if (rc != SPZ_AMD_OK) return rc;
  FloatSrc src;
  rc = cloud_source(d_cloud, num_points, sh_degree, &src);
  if (rc != SPZ_AMD_OK) return rc;
  if (max_entries > kMaxEntries) return SPZ_AMD_ERR_INVALID_ARG;
  if ((depth ? d_grad_depth : d_grad_image) == nullptr || d_grads == nullptr || d_status == nullptr ||
      d_render_workspace == nullptr || d_backward_workspace == nullptr) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  if (num_points && (!d_grads->positions || !d_grads->scales || !d_grads->rotations || !d_grads->alphas ||
                     !d_grads->colors || (src.sh_dim > 0 && !d_grads->sh))) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  const hipStream_t st = static_cast<hipStream_t>(hip_stream);
  SPZ_HIP_TRY(hipMemsetAsync(d_status, 0, sizeof(uint32_t), st));
  if (num_points == 0) return SPZ_AMD_OK;  // the total is 0 and there is nothing to write
  const RenderLayout wl = render_layout(num_points, max_entries);
  const uint8_t *base = align_ws(const_cast<void *>(d_render_workspace));
  uint8_t *bws = align_ws(d_backward_workspace);
  float *rec_grad = reinterpret_cast<float *>(bws);
  // the n depth gradients follow the n x 9 record gradients
  float *depth_grad = depth ? reinterpret_cast<float *>(bws + al(num_points * kRecGrads * sizeof(float))) : nullptr;
  SPZ_HIP_TRY(hipMemsetAsync(rec_grad, 0, num_points * kRecGrads * sizeof(float), st));
  if (depth) SPZ_HIP_TRY(hipMemsetAsync(depth_grad, 0, num_points * sizeof(float), st));
  BlendBackwardParams b = {};
  const dim3 grid = fill_blend_params(b, wl, base, base + wl.prefix, params, max_entries);
  b.grad_image = d_grad_image;
  b.rec_grad = rec_grad;
  if (depth) {
    DepthBlendBackwardParams db = {};
    db.b = b;
    db.grad_depth = d_grad_depth;
    db.depth_grad = depth_grad;
    hipLaunchKernelGGL(spz_render_depth_blend_backward_kernel, grid, dim3(kBlendThreads), 0, st, db);
  } else {
    hipLaunchKernelGGL(spz_render_blend_backward_kernel, grid, dim3(kBlendThreads), 0, st, b);
  }
  SPZ_HIP_TRY(hipGetLastError());
  PreprocessBackwardParams q = {};
  q.src = src;
  q.cam = make_cam(params, sh_degree, antialiased);
  q.rec = b.rec;
  q.rec_grad = rec_grad;
  q.total = b.total;
  q.max_entries = max_entries;
  q.positions = d_grads->positions;
  q.scales = d_grads->scales;
  q.rotations = d_grads->rotations;
  q.alphas = d_grads->alphas;
  q.colors = d_grads->colors;
  q.sh = d_grads->sh;
  q.rec_grad_out = d_record_grads;
  q.status = d_status;
  q.n = (uint32_t)num_points;
  q.depth_grad = depth_grad;
  q.depth_grad_out = depth ? d_depth_grads : nullptr;
  hipLaunchKernelGGL(spz_render_preprocess_backward_kernel, dim3((unsigned)((num_points + kPreBlock - 1) / kPreBlock)),
                     dim3(kPreBlock), 0, st, q);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

}  // namespace

extern "C" {

uint64_t spz_amd_render_backward_workspace_bytes(uint64_t num_points) {
  return al(num_points * kRecGrads * sizeof(float)) + 256u;  // room to align a caller's pointer up to 256
}

int spz_amd_render_backward_device(const spz_amd_cloud_in *d_cloud, uint64_t num_points, int sh_degree, int antialiased,
                                   const spz_amd_render_params *params, uint64_t max_entries, const float *d_image,
                                   const float *d_grad_image, const spz_amd_cloud_grads *d_grads, float *d_record_grads,
                                   uint32_t *d_status, const void *d_render_workspace, void *d_backward_workspace,
                                   void *hip_stream) {
  (void)d_image;  // the blend runs again instead: see the contract
  return backward_impl(d_cloud, num_points, sh_degree, antialiased, params, max_entries, d_grad_image, nullptr, false,
                       d_grads, d_record_grads, nullptr, d_status, d_render_workspace, d_backward_workspace, hip_stream);
}

uint64_t spz_amd_render_depth_backward_workspace_bytes(uint64_t num_points) {
  // the n x 9 record gradients, the n depth gradients, and room to align a caller's pointer up to 256
  return al(num_points * kRecGrads * sizeof(float)) + al(num_points * sizeof(float)) + 256u;
}

int spz_amd_render_depth_backward_device(const spz_amd_cloud_in *d_cloud, uint64_t num_points, int sh_degree,
                                         int antialiased, const spz_amd_render_params *params, uint64_t max_entries,
                                         const float *d_grad_image, const float *d_grad_depth,
                                         const spz_amd_cloud_grads *d_grads, float *d_record_grads, float *d_depth_grads,
                                         uint32_t *d_status, const void *d_render_workspace, void *d_backward_workspace,
                                         void *hip_stream) {
  return backward_impl(d_cloud, num_points, sh_degree, antialiased, params, max_entries, d_grad_image, d_grad_depth, true,
                       d_grads, d_record_grads, d_depth_grads, d_status, d_render_workspace, d_backward_workspace,
                       hip_stream);
}

}  // extern "C"

// ---- the blend half on its own ("render view backward": the pose fit needs no gradients to the cloud)
namespace spz_amd_detail {

// Zeroes the caller's n x 9 record gradients for the blend backward to add into; with the total above max_entries it
// sets the status instead and writes nothing, as the blend backward then adds nothing.
__global__ __launch_bounds__(kPreBlock) void spz_render_records_clear_kernel(float *__restrict__ rec_grad,
                                                                             unsigned long long count,
                                                                             const unsigned long long *total,
                                                                             unsigned long long max_entries,
                                                                             uint32_t *status) {
  const unsigned long long j = (unsigned long long)blockIdx.x * kPreBlock + threadIdx.x;
  if (*total > max_entries) {
    if (j == 0ull) *status = 1u;
    return;
  }
  if (j < count) rec_grad[j] = 0.0f;
}

}  // namespace spz_amd_detail

extern "C" {

int spz_amd_render_records_backward_device(uint64_t num_points, const spz_amd_render_params *params,
                                           uint64_t max_entries, const float *d_grad_image, float *d_record_grads,
                                           uint32_t *d_status, const void *d_render_workspace, void *hip_stream) {
  int rc = check_params(params);
  if (rc != SPZ_AMD_OK) return rc;
  if (num_points > kMaxEntries) return SPZ_AMD_ERR_TOO_MANY_POINTS;
  if (max_entries > kMaxEntries) return SPZ_AMD_ERR_INVALID_ARG;
  if (d_grad_image == nullptr || d_status == nullptr || d_render_workspace == nullptr ||
      (num_points && d_record_grads == nullptr)) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  const hipStream_t st = static_cast<hipStream_t>(hip_stream);
  SPZ_HIP_TRY(hipMemsetAsync(d_status, 0, sizeof(uint32_t), st));
  if (num_points == 0) return SPZ_AMD_OK;  // the total is 0 and there is nothing to write
  const RenderLayout wl = render_layout(num_points, max_entries);
  const uint8_t *base = align_ws(const_cast<void *>(d_render_workspace));
  BlendBackwardParams b = {};
  const dim3 grid = fill_blend_params(b, wl, base, base + wl.prefix, params, max_entries);
  b.grad_image = d_grad_image;
  b.rec_grad = d_record_grads;
  const unsigned long long count = (unsigned long long)num_points * kRecGrads;
  hipLaunchKernelGGL(spz_render_records_clear_kernel, dim3((unsigned)((count + kPreBlock - 1) / kPreBlock)),
                     dim3(kPreBlock), 0, st, d_record_grads, count, b.total, max_entries, d_status);
  SPZ_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(spz_render_blend_backward_kernel, grid, dim3(kBlendThreads), 0, st, b);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

}  // extern "C"
