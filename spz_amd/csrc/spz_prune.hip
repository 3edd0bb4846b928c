// spz_prune.hip — significance pruning of a packed stream (DESIGN §8 "Prune"; the contract is in include/spz_amd.h):
// every Gaussian's blend weight summed (and maximised) over a set of views, the least significant dropped, the rest
// written as the filter's subset.
//
//   per view                       prepare_view (spz_view_pass.hpp: prepare, the total read back, the workspace
//                                  grown), then spz_amd_render_score_device (spz_render.hip's spz_render_score_kernel)
//                                  adding into the u64 sums and f32 maxima.
//   spz_prune_key_kernel           keep_count / keep_fraction: the complement of the score as radix keys (u64 sum: two
//                                  planes, 8 digits; the f32 max's bits: one plane, 4 digits), so the stable ascending
//                                  sort (spz_sort_internal.hpp) ranks by score descending, then input index.
//   spz_prune_top_kernel           mask[order[r]] = 1 for the first K ranks.
//   spz_prune_threshold_kernel     min_score: mask[j] = score_j >= s, the sum as q 2^-24 in f64.
//   (subset)                       select_subset_masked (spz_filter.hip): the filter's select and subset at the
//                                  input's degree.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "spz_amd.h"
#include "spz_common.hpp"
#include "spz_sort_internal.hpp"
#include "spz_view_pass.hpp"

namespace spz_amd_detail {
namespace {

constexpr uint32_t kPrBlock = 256;

}  // namespace

__global__ __launch_bounds__(kPrBlock) void spz_prune_key_kernel(const unsigned long long *sum, const uint32_t *max_bits,
                                                                 uint32_t n, uint32_t *k0, uint32_t *k1) {
  const uint32_t i = blockIdx.x * kPrBlock + threadIdx.x;
  if (i >= n) return;
  if (sum) {
    const unsigned long long k = ~sum[i];
    k0[i] = (uint32_t)k;
    k1[i] = (uint32_t)(k >> 32);
  } else {
    k0[i] = ~max_bits[i];
  }
}

__global__ __launch_bounds__(kPrBlock) void spz_prune_top_kernel(const uint32_t *order, uint32_t k, uint8_t *mask) {
  const uint32_t r = blockIdx.x * kPrBlock + threadIdx.x;
  if (r < k) mask[order[r]] = 1u;
}

__global__ __launch_bounds__(kPrBlock) void spz_prune_threshold_kernel(const unsigned long long *sum, const float *wmax,
                                                                       uint32_t n, double s, uint8_t *mask) {
  const uint32_t i = blockIdx.x * kPrBlock + threadIdx.x;
  if (i >= n) return;
  const double v = sum ? (double)sum[i] * 0x1p-24 : (double)wmax[i];
  mask[i] = v >= s ? 1u : 0u;
}

}  // namespace spz_amd_detail

using namespace spz_amd_detail;

extern "C" {

int spz_amd_prune_keep_count(uint64_t num_points, int rule, double rule_value, uint64_t *k) {
  if (k == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  if (rule == SPZ_AMD_PRUNE_KEEP_COUNT) {
    if (!(rule_value >= 0.0) || !(rule_value <= (double)num_points) || rule_value != std::floor(rule_value)) {
      return SPZ_AMD_ERR_INVALID_ARG;
    }
    *k = (uint64_t)rule_value;
    return SPZ_AMD_OK;
  }
  if (rule == SPZ_AMD_PRUNE_KEEP_FRACTION) {
    if (!(rule_value >= 0.0) || !(rule_value <= 1.0)) return SPZ_AMD_ERR_INVALID_ARG;
    const double c = std::ceil(rule_value * (double)num_points);
    *k = c >= (double)num_points ? num_points : (uint64_t)c;
    return SPZ_AMD_OK;
  }
  return SPZ_AMD_ERR_INVALID_ARG;
}

int spz_amd_prune_open(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr,
                       const spz_amd_render_params *views, int num_views, int score_kind, int rule, double rule_value,
                       int device, void **ctx, uint64_t *h_out_bytes, uint64_t *h_kept, uint8_t *h_mask,
                       uint64_t *h_weight_sum, float *h_weight_max, float *h_ms, int32_t *h_bad_view) {
  if (h_bad_view) *h_bad_view = -1;
  if (ctx == nullptr || h_out_bytes == nullptr || d_stream == nullptr || hdr == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  *ctx = nullptr;
  *h_out_bytes = 0;
  int rc = check_views(views, num_views, SPZ_AMD_PRUNE_MAX_VIEWS, h_bad_view);
  if (rc != SPZ_AMD_OK) return rc;
  if (score_kind != SPZ_AMD_PRUNE_SCORE_SUM && score_kind != SPZ_AMD_PRUNE_SCORE_MAX) return SPZ_AMD_ERR_INVALID_ARG;
  rc = check_render_input(d_stream, size, hdr);
  if (rc != SPZ_AMD_OK) return rc;
  const uint64_t n = hdr->num_points;
  uint64_t keep = 0;
  if (rule == SPZ_AMD_PRUNE_MIN_SCORE) {
    if (!std::isfinite(rule_value)) return SPZ_AMD_ERR_INVALID_ARG;
  } else {
    rc = spz_amd_prune_keep_count(n, rule, rule_value, &keep);
    if (rc != SPZ_AMD_OK) return rc;
  }
  DeviceGuard guard;
  rc = guard.enter(device);
  if (rc != SPZ_AMD_OK) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  PackedResultPtr c;
  rc = packed_result_open(device, &c);
  if (rc != SPZ_AMD_OK) return rc;
  const SortLayout sl = sort_layout(n);
  WorkspaceOffsets o;
  const uint64_t o_sum = o.put(n * 8u), o_max = o.put(n * 4u), o_small = o.put(16u), o_mask = o.put(n),
                 o_idx = o.put(n * 4u), o_order = o.put(n * 4u), o_sort = o.put(n ? sl.bytes : 0u),
                 o_fws = o.put(spz_amd_filter_workspace_bytes(n));
  SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&c->block), o.off));
  uint8_t *raw = c->block;  // every section is 256-aligned from hipMalloc's base
  auto *d_sum = reinterpret_cast<uint64_t *>(raw + o_sum);
  auto *d_max = reinterpret_cast<float *>(raw + o_max);
  auto *d_total = reinterpret_cast<uint64_t *>(raw + o_small);
  auto *d_status = reinterpret_cast<uint32_t *>(raw + o_small + 8u);
  uint8_t *d_mask = raw + o_mask;
  auto *d_idx = reinterpret_cast<uint32_t *>(raw + o_idx);
  auto *d_order = reinterpret_cast<uint32_t *>(raw + o_order);
  if (n) {
    SPZ_HIP_TRY(hipMemsetAsync(d_sum, 0, n * 8u, c->st));
    SPZ_HIP_TRY(hipMemsetAsync(d_max, 0, n * 4u, c->st));
  }
  // the views: prepare, the total, the workspace, the score
  const RenderSource src = packed_render_source(d_stream, size, hdr);
  uint64_t cap = 0, total = 0;
  for (int v = 0; v < num_views; ++v) {
    rc = prepare_view(&c->scratch, &cap, src, &views[v], d_total, c->st, &total);
    if (rc == SPZ_AMD_OK) {
      rc = spz_amd_render_score_device(n, &views[v], total, nullptr, d_sum, d_max, d_status, c->scratch, c->st);
    }
    if (rc != SPZ_AMD_OK) {
      if (h_bad_view) *h_bad_view = v;
      return rc;
    }
  }
  SPZ_HIP_TRY(hipStreamSynchronize(c->st));
  const double score_ms = ms_since(t0);
  // the rank and the keep mask
  const bool by_sum = score_kind == SPZ_AMD_PRUNE_SCORE_SUM;
  const unsigned blocks = (unsigned)((n + kPrBlock - 1) / kPrBlock);
  if (n) {
    if (rule == SPZ_AMD_PRUNE_MIN_SCORE) {
      hipLaunchKernelGGL(spz_prune_threshold_kernel, dim3(blocks), dim3(kPrBlock), 0, c->st,
                         by_sum ? reinterpret_cast<const unsigned long long *>(d_sum) : nullptr, d_max, (uint32_t)n,
                         rule_value, d_mask);
      SPZ_HIP_TRY(hipGetLastError());
    } else if (keep == 0 || keep == n) {
      SPZ_HIP_TRY(hipMemsetAsync(d_mask, keep ? 1 : 0, n, c->st));
    } else {
      uint8_t *sws = align_ws(raw + o_sort);
      auto *k0 = reinterpret_cast<uint32_t *>(sws + sl.planes_off[0][0]);
      auto *k1 = reinterpret_cast<uint32_t *>(sws + sl.planes_off[0][1]);
      hipLaunchKernelGGL(spz_prune_key_kernel, dim3(blocks), dim3(kPrBlock), 0, c->st,
                         by_sum ? reinterpret_cast<const unsigned long long *>(d_sum) : nullptr,
                         reinterpret_cast<const uint32_t *>(d_max), (uint32_t)n, k0, k1);
      SPZ_HIP_TRY(hipGetLastError());
      rc = radix_passes((uint32_t)n, by_sum ? 8u : 4u, d_order, sws, sl, c->st);
      if (rc != SPZ_AMD_OK) return rc;
      SPZ_HIP_TRY(hipMemsetAsync(d_mask, 0, n, c->st));
      hipLaunchKernelGGL(spz_prune_top_kernel, dim3((unsigned)((keep + kPrBlock - 1) / kPrBlock)), dim3(kPrBlock), 0,
                         c->st, d_order, (uint32_t)keep, d_mask);
      SPZ_HIP_TRY(hipGetLastError());
    }
  }
  SPZ_HIP_TRY(hipStreamSynchronize(c->st));
  const double rank_ms = ms_since(t0) - score_ms;
  uint64_t kept = 0;
  rc = select_subset_masked(d_stream, size, hdr, d_mask, d_idx, raw + o_fws, c.get(), &kept);
  if (rc != SPZ_AMD_OK) return rc;
  if (h_mask && n) SPZ_HIP_TRY(hipMemcpyAsync(h_mask, d_mask, n, hipMemcpyDeviceToHost, c->st));
  if (h_weight_sum && n) SPZ_HIP_TRY(hipMemcpyAsync(h_weight_sum, d_sum, n * 8u, hipMemcpyDeviceToHost, c->st));
  if (h_weight_max && n) SPZ_HIP_TRY(hipMemcpyAsync(h_weight_max, d_max, n * 4u, hipMemcpyDeviceToHost, c->st));
  SPZ_HIP_TRY(hipStreamSynchronize(c->st));
  if (h_ms) {
    h_ms[0] = (float)score_ms;
    h_ms[1] = (float)rank_ms;
    h_ms[2] = (float)(ms_since(t0) - score_ms - rank_ms);
  }
  if (h_kept) *h_kept = kept;
  *h_out_bytes = c->out_bytes;
  // the render's workspace is not needed by fetch: free it now
  SPZ_HIP_TRY(hipFree(c->scratch));
  c->scratch = nullptr;
  *ctx = c.release();
  return SPZ_AMD_OK;
}

int spz_amd_prune_fetch(void *ctx, uint8_t *h_out) { return packed_result_fetch(ctx, h_out); }

const uint8_t *spz_amd_prune_device_data(void *ctx) { return packed_result_device_data(ctx); }

void spz_amd_prune_close(void *ctx) { packed_result_close(ctx); }

}  // extern "C"
