// spz_render_view_backward.hip — the gradient of one rendered view to its camera [R | t] (DESIGN §8 "Locate"; the
// contract is in include/spz_amd.h "render view backward").  Reads the records and the total of a finished render
// workspace and the n x 9 record gradients of the blend backward.
//
//   spz_render_view_backward_kernel   one lane per Gaussian runs view_backward_one (spz_view_backward_core.hpp) in f64
//                                     and holds that Gaussian's 12 contributions.  They are summed over the wave with
//                                     64-lane shuffles (a fixed tree), over the workgroup's four waves through LDS in
//                                     wave order, and the workgroup stores one row of 12 doubles.  No atomics.
//   spz_render_view_reduce_kernel     one workgroup of 64 x 12 lanes: lane (g, e) adds entry e of the rows g, g + 64,
//                                     g + 128, ... in that order, then lane e adds the 64 group sums in group order.
// Both orders depend on n alone, so the same record gradients give the same bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "spz_amd.h"
#include "spz_common.hpp"
#include "spz_render_internal.hpp"
#include "spz_view_backward_core.hpp"

#pragma clang fp contract(off)

namespace spz_amd_detail {
namespace {

constexpr uint32_t kViewBlock = 256;
constexpr uint32_t kViewWaves = kViewBlock / 64;
constexpr uint32_t kReduceGroups = 64;
constexpr uint32_t kReduceBlock = kReduceGroups * kViewGrads;  // 768

// The sum of an f64 over the 64 lanes of a wave (every lane active), valid in lane 0: a fixed tree of shuffles.
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_down(v, d, 64);
  return v;
}

__global__ __launch_bounds__(kViewBlock) void spz_render_view_backward_kernel(const ViewBackwardParams p) {
  __shared__ double s_part[kViewWaves][kViewGrads];
  if (*p.total > p.max_entries) {  // workgroup-uniform
    if (blockIdx.x == 0u && threadIdx.x == 0u) *p.status = 1u;
    return;
  }
  const uint32_t i = blockIdx.x * kViewBlock + threadIdx.x;
  double c[kViewGrads];
  if (i < p.n) {
    view_backward_one(p, i, c);
  } else {
#pragma unroll
    for (uint32_t e = 0; e < kViewGrads; ++e) c[e] = 0.0;
  }
#pragma unroll
  for (uint32_t e = 0; e < kViewGrads; ++e) c[e] = wave_sum_f64(c[e]);
  if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
    for (uint32_t e = 0; e < kViewGrads; ++e) s_part[threadIdx.x >> 6][e] = c[e];
  }
  __syncthreads();
  if (threadIdx.x < kViewGrads) {
    double s = s_part[0][threadIdx.x];
#pragma unroll
    for (uint32_t w = 1; w < kViewWaves; ++w) s = s + s_part[w][threadIdx.x];
    p.partials[(unsigned long long)blockIdx.x * kViewGrads + threadIdx.x] = s;
  }
}

__global__ __launch_bounds__(kReduceBlock) void spz_render_view_reduce_kernel(const double *__restrict__ partials,
                                                                              uint32_t rows,
                                                                              const unsigned long long *total,
                                                                              unsigned long long max_entries,
                                                                              double *__restrict__ view_grad) {
  __shared__ double s_sum[kReduceBlock];
  if (*total > max_entries) return;  // the first kernel has set the status; nothing is written
  const uint32_t t = threadIdx.x;  // group t / 12, entry t % 12: row g's entry e is flat element g * 12 + e
  const unsigned long long count = (unsigned long long)rows * kViewGrads;
  double s = 0.0;
  for (unsigned long long j = t; j < count; j += kReduceBlock) s = s + partials[j];
  s_sum[t] = s;
  __syncthreads();
  if (t < kViewGrads) {
    double r = s_sum[t];
    for (uint32_t g = 1; g < kReduceGroups; ++g) r = r + s_sum[g * kViewGrads + t];
    view_grad[t] = r;
  }
}

inline uint64_t view_rows(uint64_t n) { return (n + kViewBlock - 1) / kViewBlock; }

}  // namespace
}  // namespace spz_amd_detail

using namespace spz_amd_detail;

extern "C" {

uint64_t spz_amd_render_view_backward_workspace_bytes(uint64_t num_points) {
  return al(view_rows(num_points) * kViewGrads * sizeof(double)) + 256u;  // room to align a caller's pointer up to 256
}

int spz_amd_render_view_backward_device(const spz_amd_cloud_in *d_cloud, uint64_t num_points, int sh_degree,
                                        int antialiased, const spz_amd_render_params *params, uint64_t max_entries,
                                        const float *d_record_grads, double *d_view_grad, uint32_t *d_status,
                                        const void *d_render_workspace, void *d_workspace, void *hip_stream) {
  int rc = check_params(params);
  if (rc != SPZ_AMD_OK) return rc;
  FloatSrc src;
  rc = cloud_source(d_cloud, num_points, sh_degree, &src);
  if (rc != SPZ_AMD_OK) return rc;
  if (max_entries > kMaxEntries) return SPZ_AMD_ERR_INVALID_ARG;
  if (d_view_grad == nullptr || d_status == nullptr || d_render_workspace == nullptr || d_workspace == nullptr ||
      (reinterpret_cast<uintptr_t>(d_view_grad) & 7u) != 0u) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  if (num_points && d_record_grads == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  const hipStream_t st = static_cast<hipStream_t>(hip_stream);
  SPZ_HIP_TRY(hipMemsetAsync(d_status, 0, sizeof(uint32_t), st));
  if (num_points == 0) {  // the total is 0 and no Gaussian contributes
    SPZ_HIP_TRY(hipMemsetAsync(d_view_grad, 0, kViewGrads * sizeof(double), st));
    return SPZ_AMD_OK;
  }
  const RenderLayout wl = render_layout(num_points, max_entries);
  const uint8_t *base = align_ws(const_cast<void *>(d_render_workspace));
  ViewBackwardParams q = {};
  q.src = src;
  q.cam = make_cam(params, sh_degree, antialiased);
  q.rec = reinterpret_cast<const spz_amd_render_record *>(base + wl.rec);
  q.rec_grad = d_record_grads;
  q.total = reinterpret_cast<const unsigned long long *>(base + wl.total);
  q.max_entries = max_entries;
  q.partials = reinterpret_cast<double *>(align_ws(d_workspace));
  q.status = d_status;
  q.n = (uint32_t)num_points;
  const uint32_t rows = (uint32_t)view_rows(num_points);
  hipLaunchKernelGGL(spz_render_view_backward_kernel, dim3(rows), dim3(kViewBlock), 0, st, q);
  SPZ_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(spz_render_view_reduce_kernel, dim3(1), dim3(kReduceBlock), 0, st, q.partials, rows, q.total,
                     max_entries, d_view_grad);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

}  // extern "C"
