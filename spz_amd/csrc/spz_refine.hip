// spz_refine.hip — fitting a packed stream to a target over views (DESIGN §8 "Refine"; the contract is in
// include/spz_amd.h): the Adam step over a float cloud and the loop from a stream to a stream.  The image loss and its
// gradient are beside the metrics kernels (spz_metrics.hip), whose window and tile pass they share.
//
//   spz_adam_step_kernel           one launch for all trained arrays.  Every array is cut into 16-byte units from the
//                                  first 16-aligned parameter address, with up to three scalar elements before and
//                                  after; a workgroup belongs to one array (a table of first workgroups in the kernel
//                                  arguments), a lane takes one unit: g, m, v, p in, m', v', p' out, in f32, one
//                                  rounding per operation.  Non-finite p or g: the element is left alone and counted
//                                  (one vector integer atomic per workgroup that has any).
//   refine                         decode A; per view the target (B rendered) and the "before" metrics; per iteration
//                                  render_view (spz_view_pass.hpp), spz_amd_image_loss_device,
//                                  spz_amd_render_backward_device on the same workspace and total, the Adam step; then
//                                  the trained sections encoded over a copy of A's bytes and the "after" metrics of
//                                  that stream.
//   refine images                  (DESIGN §8 "Fit") the same loop with the targets given, not rendered: the photo loss
//                                  of spz_photo.hip with each view's weights and, when they are fitted, its exposure
//                                  read from device memory, and that exposure's own Adam step on the device; "after"
//                                  through the fitted exposure.
//   refine images with depth       (DESIGN §8 "Depth fit") a view with a depth map: spz_amd_render_depth_device for the
//                                  finish, the photo loss, spz_amd_depth_loss_device adding into its gradient, and
//                                  spz_amd_render_depth_backward_device; the depth error of A and of the output.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "spz_amd.h"
#include "spz_common.hpp"
#include "spz_densify_internal.hpp"
#include "spz_photo_internal.hpp"
#include "spz_view_pass.hpp"

namespace spz_amd_detail {
namespace {

constexpr uint32_t kAdBlock = 256;

// One trained array of the launch: n4 16-byte units from element `head`, then the elements after them; the array's
// workgroups begin at `first_block`.
struct AdamSegment {
  float *p, *m, *v;
  const float *g;
  unsigned long long count;  // elements
  unsigned long long n4;     // 16-byte units
  uint32_t head;             // scalar elements in front of the units, 0..3
  uint32_t first_block;
  float s;                   // lr / (1 - beta1^t)
  uint32_t pad;
};

struct AdamLaunch {
  AdamSegment seg[6];
  uint32_t n_seg;
  float beta1, c1, beta2, c2, eps, r;
};

__device__ __forceinline__ bool finite_bits(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// torch's form of Adam on one element; false (and nothing changed) when p or g is not finite.
__device__ __forceinline__ bool adam_one(float &p, float g, float &m, float &v, const AdamLaunch &a, float s) {
  if (!finite_bits(p) || !finite_bits(g)) return false;
  const float m1 = a.beta1 * m + a.c1 * g;
  const float v1 = a.beta2 * v + (a.c2 * g) * g;
  const float den = sqrtf(v1) / a.r + a.eps;
  p = p - s * (m1 / den);
  m = m1;
  v = v1;
  return true;
}

}  // namespace

__global__ __launch_bounds__(kAdBlock) void spz_adam_step_kernel(AdamLaunch a, uint32_t *__restrict__ skipped) {
  __shared__ uint32_t part[kAdBlock / 64];
  uint32_t k = 0;
  while (k + 1 < a.n_seg && blockIdx.x >= a.seg[k + 1].first_block) ++k;  // uniform: a workgroup has one array
  const AdamSegment &sg = a.seg[k];
  const unsigned long long u = (unsigned long long)(blockIdx.x - sg.first_block) * kAdBlock + threadIdx.x;
  const unsigned long long n_scalar = sg.count - 4ull * sg.n4;  // head + tail, at most 6
  uint32_t bad = 0;
  if (u < sg.n4) {
    const unsigned long long e = sg.head + 4ull * u;
    F32x4 p = *reinterpret_cast<const F32x4 *>(sg.p + e);
    const F32x4 g = *reinterpret_cast<const F32x4 *>(sg.g + e);
    F32x4 m = *reinterpret_cast<const F32x4 *>(sg.m + e);
    F32x4 v = *reinterpret_cast<const F32x4 *>(sg.v + e);
    bad += adam_one(p.x, g.x, m.x, v.x, a, sg.s) ? 0u : 1u;
    bad += adam_one(p.y, g.y, m.y, v.y, a, sg.s) ? 0u : 1u;
    bad += adam_one(p.z, g.z, m.z, v.z, a, sg.s) ? 0u : 1u;
    bad += adam_one(p.w, g.w, m.w, v.w, a, sg.s) ? 0u : 1u;
    if (bad != 4u) {  // (untouched elements are written back with the bits that were read)
      *reinterpret_cast<F32x4 *>(sg.p + e) = p;
      *reinterpret_cast<F32x4 *>(sg.m + e) = m;
      *reinterpret_cast<F32x4 *>(sg.v + e) = v;
    }
  } else if (u - sg.n4 < n_scalar) {
    const unsigned long long s = u - sg.n4;
    const unsigned long long e = s < sg.head ? s : 4ull * sg.n4 + s;
    float p = sg.p[e], m = sg.m[e], v = sg.v[e];
    if (adam_one(p, sg.g[e], m, v, a, sg.s)) {
      sg.p[e] = p;
      sg.m[e] = m;
      sg.v[e] = v;
    } else {
      bad = 1u;
    }
  }
  for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o);
  if ((threadIdx.x & 63u) == 0) part[threadIdx.x / 64] = bad;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (uint32_t w = 0; w < kAdBlock / 64; ++w) t += part[w];
    if (t) atomicAdd(skipped, t);
  }
}

namespace {

bool finite_f(float x) { return std::isfinite(x); }

int adam_check_scalars(const spz_amd_adam_scalars &s) {
  if (!finite_f(s.beta1) || !finite_f(s.c1) || !finite_f(s.beta2) || !finite_f(s.c2) || !finite_f(s.eps) ||
      !finite_f(s.r) || !(s.r > 0.0f) || !(s.eps >= 0.0f)) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  for (int k = 0; k < 6; ++k) {
    if (!finite_f(s.s[k])) return SPZ_AMD_ERR_INVALID_ARG;
  }
  return SPZ_AMD_OK;
}

// The element counts of the six arrays in the order of spz_amd_cloud_in.
void cloud_counts(uint64_t n, int sh_degree, uint64_t count[6]) {
  const uint64_t sd = (uint64_t)sh_dim_for_degree(sh_degree);
  const uint64_t c[6] = {3u * n, 3u * n, 4u * n, n, 3u * n, n * sd * 3u};
  for (int k = 0; k < 6; ++k) count[k] = c[k];
}

float *grads_field(const spz_amd_cloud_grads *c, int k) {
  float *const f[6] = {c->positions, c->scales, c->rotations, c->alphas, c->colors, c->sh};
  return f[k];
}

int adam_enqueue(const spz_amd_cloud_grads *d_params, const spz_amd_cloud_grads *d_grads, const spz_amd_cloud_grads *d_m,
                 const spz_amd_cloud_grads *d_v, uint64_t num_points, int sh_degree, unsigned train_mask,
                 const spz_amd_adam_scalars &sc, uint32_t *d_skipped, hipStream_t st) {
  uint64_t count[6];
  cloud_counts(num_points, sh_degree, count);
  AdamLaunch a = {};
  a.beta1 = sc.beta1;
  a.c1 = sc.c1;
  a.beta2 = sc.beta2;
  a.c2 = sc.c2;
  a.eps = sc.eps;
  a.r = sc.r;
  uint64_t blocks = 0;
  for (int k = 0; k < 6; ++k) {
    if (((train_mask >> k) & 1u) == 0u || count[k] == 0) continue;
    AdamSegment &sg = a.seg[a.n_seg++];
    sg.p = grads_field(d_params, k);
    sg.g = grads_field(d_grads, k);
    sg.m = grads_field(d_m, k);
    sg.v = grads_field(d_v, k);
    sg.count = count[k];
    const uint64_t to16 = ((16u - (reinterpret_cast<uintptr_t>(sg.p) & 15u)) & 15u) / 4u;
    sg.head = (uint32_t)(to16 < count[k] ? to16 : count[k]);
    sg.n4 = (count[k] - sg.head) / 4u;
    sg.first_block = (uint32_t)blocks;
    sg.s = sc.s[k];
    const uint64_t units = sg.n4 + (count[k] - 4u * sg.n4);
    blocks += (units + kAdBlock - 1) / kAdBlock;
  }
  if (a.n_seg == 0) return SPZ_AMD_OK;
  if (blocks > 0x7fffffffull) return SPZ_AMD_ERR_TOO_MANY_POINTS;
  hipLaunchKernelGGL(spz_adam_step_kernel, dim3((unsigned)blocks), dim3(kAdBlock), 0, st, a, d_skipped);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

int adam_check_args(const spz_amd_cloud_grads *d_params, const spz_amd_cloud_grads *d_grads, const spz_amd_cloud_grads *d_m,
                    const spz_amd_cloud_grads *d_v, uint64_t num_points, int sh_degree, unsigned train_mask,
                    const spz_amd_adam_scalars &sc, const uint32_t *d_skipped) {
  if (d_params == nullptr || d_grads == nullptr || d_m == nullptr || d_v == nullptr || d_skipped == nullptr) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  if (sh_degree < 0 || sh_degree > 3) return SPZ_AMD_ERR_SH_DEGREE;
  if (train_mask == 0u || train_mask > SPZ_AMD_TRAIN_ALL || !aligned4(d_skipped)) return SPZ_AMD_ERR_INVALID_ARG;
  if (num_points > kMaxEntries) return SPZ_AMD_ERR_TOO_MANY_POINTS;
  int rc = adam_check_scalars(sc);
  if (rc != SPZ_AMD_OK) return rc;
  uint64_t count[6];
  cloud_counts(num_points, sh_degree, count);
  for (int k = 0; k < 6; ++k) {
    if (((train_mask >> k) & 1u) == 0u || count[k] == 0) continue;
    for (const spz_amd_cloud_grads *c : {d_params, d_grads, d_m, d_v}) {
      const float *f = grads_field(c, k);
      if (f == nullptr || !aligned4(f)) return SPZ_AMD_ERR_INVALID_ARG;
    }
  }
  return SPZ_AMD_OK;
}

// The float cloud, its gradients and moments: four times the six arrays, each array 256-aligned in one allocation.
struct CloudSet {
  spz_amd_cloud_grads p, g, m, v;
  uint64_t moments_off = 0, moments_bytes = 0;  // m and v are contiguous: one memset
};

spz_amd_cloud_grads cloud_at(uint8_t *base, const uint64_t off[6], const uint64_t count[6]) {
  auto f = [&](int k) { return count[k] ? reinterpret_cast<float *>(base + off[k]) : nullptr; };
  return spz_amd_cloud_grads{f(0), f(1), f(2), f(3), f(4), f(5)};
}

}  // namespace
}  // namespace spz_amd_detail

using namespace spz_amd_detail;

extern "C" {

int spz_amd_adam_scalars_of(int t, const double lr[6], double beta1, double beta2, double eps,
                            spz_amd_adam_scalars *out) {
  if (out == nullptr || lr == nullptr || t < 1) return SPZ_AMD_ERR_INVALID_ARG;
  if (!(beta1 >= 0.0) || !(beta1 < 1.0) || !(beta2 >= 0.0) || !(beta2 < 1.0) || !(eps >= 0.0) || !std::isfinite(eps)) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  for (int k = 0; k < 6; ++k) {
    if (!std::isfinite(lr[k]) || lr[k] < 0.0) return SPZ_AMD_ERR_INVALID_ARG;
  }
  const double bc1 = 1.0 - std::pow(beta1, (double)t), bc2 = 1.0 - std::pow(beta2, (double)t);
  out->beta1 = (float)beta1;
  out->c1 = (float)(1.0 - beta1);
  out->beta2 = (float)beta2;
  out->c2 = (float)(1.0 - beta2);
  out->eps = (float)eps;
  out->r = (float)std::sqrt(bc2);
  for (int k = 0; k < 6; ++k) out->s[k] = (float)(lr[k] / bc1);
  return adam_check_scalars(*out);
}

int spz_amd_adam_step_device(const spz_amd_cloud_grads *d_params, const spz_amd_cloud_grads *d_grads,
                             const spz_amd_cloud_grads *d_m, const spz_amd_cloud_grads *d_v, uint64_t num_points,
                             int sh_degree, unsigned train_mask, spz_amd_adam_scalars scalars, uint32_t *d_skipped,
                             void *hip_stream) {
  int rc = adam_check_args(d_params, d_grads, d_m, d_v, num_points, sh_degree, train_mask, scalars, d_skipped);
  if (rc != SPZ_AMD_OK) return rc;
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  return adam_enqueue(d_params, d_grads, d_m, d_v, num_points, sh_degree, train_mask, scalars, d_skipped,
                      static_cast<hipStream_t>(hip_stream));
}

int spz_amd_refine_default_options(spz_amd_refine_options *options) {
  if (options == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  std::memset(options, 0, sizeof(*options));
  options->iterations = 0;
  options->train_mask = SPZ_AMD_TRAIN_ALL;
  options->lambda_dssim = 0.2;
  options->lr[0] = 1.6e-4;  // times the scene's extent: the layers above scale it
  options->lr[1] = 5e-3;
  options->lr[2] = 1e-3;
  options->lr[3] = 5e-2;
  options->lr[4] = 2.5e-3;
  options->lr[5] = 2.5e-3 / 20.0;
  options->beta1 = 0.9;
  options->beta2 = 0.999;
  options->eps = 1e-15;
  return SPZ_AMD_OK;
}

int spz_amd_refine_check(const spz_amd_refine_options *o) {
  if (o == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  if (o->iterations < 0 || o->train_mask == 0u || o->train_mask > SPZ_AMD_TRAIN_ALL) return SPZ_AMD_ERR_INVALID_ARG;
  if (!(o->lambda_dssim >= 0.0) || !(o->lambda_dssim <= 1.0)) return SPZ_AMD_ERR_INVALID_ARG;
  spz_amd_adam_scalars sc;
  return spz_amd_adam_scalars_of(1, o->lr, o->beta1, o->beta2, o->eps, &sc);
}

}  // extern "C"

namespace {

// What the densify entry reports beside refine_open's results.
struct DensifyReport {
  uint64_t *h_num_points;
  spz_amd_densify_round *h_rounds;
  int rounds_capacity;
  int *h_num_rounds;
  uint32_t *h_origin;
};

// The targets of spz_amd_refine_images_open: given, not rendered.  Every pointer is the caller's.
struct PhotoTargets {
  const float *const *d_targets;  // num_views images of `channels` floats per pixel
  const float *const *d_weights;  // NULL, or num_views weight maps, any of them NULL
  int channels;
  const spz_amd_photo_options *options;
  double *h_exposures;            // may be NULL: 12 doubles per view out
  // "refine images with depth": all NULL for spz_amd_refine_images_open
  const float *const *d_depths = nullptr;        // NULL, or num_views depth maps, any of them NULL
  const spz_amd_depth_options *depth = nullptr;  // required with the depth entries
  double *h_depth_history = nullptr;             // may be NULL: iterations doubles out
  double *h_depth_error = nullptr;               // may be NULL: 2 doubles per view out
};

// The loop of the three entries: spz_amd_refine_open (densify == nullptr), spz_amd_refine_densify_open, and
// spz_amd_refine_images_open (photo != nullptr: there is no stream B, the targets are the caller's images).
int refine_run(const uint8_t *d_stream_a, size_t size_a, const spz_amd_header *hdr_a, const uint8_t *d_stream_b,
               size_t size_b, const spz_amd_header *hdr_b, const spz_amd_render_params *views, int num_views,
               const spz_amd_refine_options *options, const spz_amd_densify_options *densify, int device, void **ctx,
               uint64_t *h_out_bytes, double *h_history, spz_amd_image_metrics *h_before, spz_amd_image_metrics *h_after,
               uint64_t *h_skipped, float *h_ms, int32_t *h_bad_view, const DensifyReport &rep,
               const PhotoTargets *photo = nullptr) {
  if (h_bad_view) *h_bad_view = -1;
  if (rep.h_num_points) *rep.h_num_points = 0;
  if (rep.h_num_rounds) *rep.h_num_rounds = 0;
  if (ctx == nullptr || h_out_bytes == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  *ctx = nullptr;
  *h_out_bytes = 0;
  int rc = spz_amd_refine_check(options);
  if (rc != SPZ_AMD_OK) return rc;
  if (options->iterations > 0 && h_history == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  rc = check_views(views, num_views, SPZ_AMD_REFINE_MAX_VIEWS, h_bad_view);
  if (rc != SPZ_AMD_OK) return rc;
  spz_amd_layout lay_a, lay_b;
  rc = check_packed_stream(d_stream_a, size_a, hdr_a, &lay_a);
  if (rc != SPZ_AMD_OK) return rc;
  const int tch = photo ? photo->channels : 4;  // the targets' channels
  bool fit = false;
  bool any_depth = false;  // some view has a depth map
  if (photo != nullptr) {
    rc = spz_amd_photo_check(photo->options);
    if (rc != SPZ_AMD_OK) return rc;
    if (photo->depth != nullptr) {
      rc = spz_amd_depth_check(photo->depth);
      if (rc != SPZ_AMD_OK) return rc;
    } else if (photo->d_depths != nullptr) {
      return SPZ_AMD_ERR_INVALID_ARG;
    }
    if (photo->d_targets == nullptr || (tch != 3 && tch != 4)) return SPZ_AMD_ERR_INVALID_ARG;
    for (int v = 0; v < num_views; ++v) {
      const float *w = photo->d_weights ? photo->d_weights[v] : nullptr;
      const float *dm = photo->d_depths ? photo->d_depths[v] : nullptr;
      any_depth = any_depth || dm != nullptr;
      if (photo->d_targets[v] == nullptr || (reinterpret_cast<uintptr_t>(photo->d_targets[v]) & 3u) != 0 ||
          (reinterpret_cast<uintptr_t>(w) & 3u) != 0 || (reinterpret_cast<uintptr_t>(dm) & 3u) != 0 ||
          spz_amd_image_metrics_check((int)views[v].width, (int)views[v].height, 4, tch) != SPZ_AMD_OK) {
        if (h_bad_view) *h_bad_view = v;
        return SPZ_AMD_ERR_INVALID_ARG;
      }
    }
    fit = photo->options->fit_exposure != 0 && options->iterations > 0;
    hdr_b = hdr_a;  // (only its count is read below)
  } else {
    rc = check_packed_stream(d_stream_b, size_b, hdr_b, &lay_b);
    if (rc != SPZ_AMD_OK) return rc;
  }
  if (hdr_a->num_points > kMaxEntries || hdr_b->num_points > kMaxEntries) return SPZ_AMD_ERR_TOO_MANY_POINTS;
  const uint64_t n = hdr_a->num_points;
  const int deg = hdr_a->sh_degree, aa = hdr_a->flags & 1, coord = views[0].coord;
  const int iters = options->iterations;
  unsigned mask = options->train_mask;
  if (deg == 0) mask &= ~32u;  // nothing to train there
  // what the encode kernel writes: versions 2 and 3, positions at 12 fractional bits
  if (iters > 0 && (hdr_a->version == 1 || ((mask & 1u) && hdr_a->fractional_bits != 12))) return SPZ_AMD_ERR_UNSUPPORTED;
  // densify: the thresholds once, every buffer at the capacity the cloud may grow to
  spz_amd_densify_limits lim = {};
  uint64_t cap_n = n;
  bool dn = false;
  if (densify != nullptr) {
    rc = spz_amd_densify_check(densify);
    if (rc != SPZ_AMD_OK) return rc;
    if (densify->interval > 0) {
      rc = spz_amd_densify_thresholds(densify, views, num_views, &lim);
      if (rc != SPZ_AMD_OK) return rc;
      if ((mask & 3u) != 3u || (densify->opacity_reset_interval > 0 && (mask & 8u) == 0u)) return SPZ_AMD_ERR_INVALID_ARG;
      if (photo != nullptr && densify->max_points == 0) return SPZ_AMD_ERR_INVALID_ARG;  // no target count to take
      const uint64_t mp = densify->max_points ? densify->max_points : hdr_b->num_points;
      if (mp > kMaxEntries) return SPZ_AMD_ERR_TOO_MANY_POINTS;
      if (mp < n) return SPZ_AMD_ERR_INVALID_ARG;
      dn = iters > 0;
      if (dn) cap_n = mp;
    }
  }
  DeviceGuard guard;
  rc = guard.enter(device);
  if (rc != SPZ_AMD_OK) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  PackedResultPtr c;
  rc = packed_result_open(device, &c);
  if (rc != SPZ_AMD_OK) return rc;

  // the block: four clouds, the targets, the image and its gradient, the two small workspaces, the results
  uint64_t count[6];
  cloud_counts(cap_n, deg, count);
  uint64_t max_px = 0, loss_ws = 0, metrics_ws = 0, depth_ws = 0;
  std::vector<uint64_t> target_off((size_t)num_views);
  for (int v = 0; v < num_views; ++v) {
    const uint64_t px = (uint64_t)views[v].width * views[v].height;
    max_px = px > max_px ? px : max_px;
    const uint64_t lw = photo ? spz_amd_photo_loss_workspace_bytes((int)views[v].width, (int)views[v].height)
                              : spz_amd_image_loss_workspace_bytes((int)views[v].width, (int)views[v].height);
    const uint64_t mw = spz_amd_image_metrics_workspace_bytes((int)views[v].width, (int)views[v].height);
    const uint64_t dw = any_depth ? spz_amd_depth_loss_workspace_bytes((int)views[v].width, (int)views[v].height) : 0u;
    loss_ws = lw > loss_ws ? lw : loss_ws;
    metrics_ws = mw > metrics_ws ? mw : metrics_ws;
    depth_ws = dw > depth_ws ? dw : depth_ws;
  }
  WorkspaceOffsets o;
  uint64_t off[4][6];
  for (int s = 0; s < 4; ++s) {
    for (int k = 0; k < 6; ++k) off[s][k] = o.put(count[k] * 4u);
  }
  for (int v = 0; v < num_views; ++v) {  // (given targets are used in place)
    target_off[(size_t)v] = o.put(photo ? 0u : 16u * (uint64_t)views[v].width * views[v].height);
  }
  // a fitted exposure per view: 12 values and their two moments, each kind contiguous; then one gradient
  const uint64_t o_exposure = o.put(fit ? 3u * 96u * (uint64_t)num_views + 96u : 0u);
  const uint64_t o_image = o.put(16u * max_px), o_grad = o.put(16u * max_px), o_lws = o.put(iters ? loss_ws : 0u),
                 o_mws = o.put(metrics_ws), o_small = o.put(16u), o_loss = o.put(24u * (uint64_t)iters),
                 o_metrics = o.put(2u * (uint64_t)num_views * sizeof(spz_amd_image_metrics)),
                 o_bws = o.put(!iters       ? 0u
                               : any_depth ? spz_amd_render_depth_backward_workspace_bytes(cap_n)
                                           : spz_amd_render_backward_workspace_bytes(cap_n));
  // with depth maps: the depth render, the gradient to its channel 0, the depth loss's workspace, L_depth and W_v per
  // iteration, and per view the two depth errors (each L and W_v)
  const uint64_t o_depth = o.put(any_depth ? 8u * max_px : 0u), o_gdepth = o.put(any_depth ? 4u * max_px : 0u),
                 o_dws = o.put(depth_ws), o_dloss = o.put(any_depth ? 16u * (uint64_t)iters : 0u),
                 o_derr = o.put(any_depth ? 32u * (uint64_t)num_views : 0u);
  uint64_t off_alt[3][6] = {};
  for (int s = 0; s < 3; ++s) {
    for (int k = 0; k < 6; ++k) off_alt[s][k] = o.put(dn ? count[k] * 4u : 0u);
  }
  const uint64_t o_accum = o.put(dn ? cap_n * 4u : 0u), o_denom = o.put(dn ? cap_n * 4u : 0u),
                 o_action = o.put(dn ? cap_n : 0u), o_parent = o.put(dn ? cap_n * 4u : 0u),
                 o_child = o.put(dn ? cap_n : 0u), o_origin0 = o.put(dn ? cap_n * 4u : 0u),
                 o_origin1 = o.put(dn ? cap_n * 4u : 0u), o_rg = o.put(dn ? cap_n * 36u : 0u),
                 o_counts = o.put(dn ? 64u : 0u), o_pws = o.put(dn ? spz_amd_densify_plan_workspace_bytes(cap_n) : 0u);
  SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&c->block), o.off));
  uint8_t *raw = c->block;  // every section is 256-aligned from hipMalloc's base
  CloudSet cs;
  cs.p = cloud_at(raw, off[0], count);
  cs.g = cloud_at(raw, off[1], count);
  cs.m = cloud_at(raw, off[2], count);
  cs.v = cloud_at(raw, off[3], count);
  cs.moments_off = off[2][0];
  cs.moments_bytes = target_off[0] - off[2][0];
  CloudSet alt;  // the apply's destinations: parameters and both moments
  if (dn) {
    alt.p = cloud_at(raw, off_alt[0], count);
    alt.m = cloud_at(raw, off_alt[1], count);
    alt.v = cloud_at(raw, off_alt[2], count);
  }
  auto *d_accum = reinterpret_cast<float *>(raw + o_accum);
  auto *d_denom = reinterpret_cast<uint32_t *>(raw + o_denom);
  auto *d_parent = reinterpret_cast<uint32_t *>(raw + o_parent);
  uint32_t *d_origin[2] = {reinterpret_cast<uint32_t *>(raw + o_origin0), reinterpret_cast<uint32_t *>(raw + o_origin1)};
  const uint32_t *origin_cur = nullptr;  // nullptr: no round yet, the identity
  auto *d_rg = reinterpret_cast<float *>(raw + o_rg);
  auto *d_counts = reinterpret_cast<uint64_t *>(raw + o_counts);
  uint64_t n_cur = n;
  std::vector<spz_amd_densify_round> rounds;
  auto *d_image = reinterpret_cast<float *>(raw + o_image);
  auto *d_grad = reinterpret_cast<float *>(raw + o_grad);
  auto *d_total = reinterpret_cast<uint64_t *>(raw + o_small);
  auto *d_status = reinterpret_cast<uint32_t *>(raw + o_small + 8u);
  auto *d_skipped = reinterpret_cast<uint32_t *>(raw + o_small + 12u);
  auto *d_loss = reinterpret_cast<double *>(raw + o_loss);
  auto *d_metrics = reinterpret_cast<spz_amd_image_metrics *>(raw + o_metrics);
  auto target = [&](int v) {
    return photo ? photo->d_targets[v] : reinterpret_cast<const float *>(raw + target_off[(size_t)v]);
  };
  auto weight = [&](int v) { return photo && photo->d_weights ? photo->d_weights[v] : nullptr; };
  auto depth_map = [&](int v) { return any_depth ? photo->d_depths[v] : nullptr; };
  auto *d_depth = reinterpret_cast<float *>(raw + o_depth);
  auto *d_gdepth = reinterpret_cast<float *>(raw + o_gdepth);
  auto *d_dloss = reinterpret_cast<double *>(raw + o_dloss);
  auto *d_derr = reinterpret_cast<double *>(raw + o_derr);
  // view v's exposure at d_exposure + 12 v, its moments 12 V and 24 V doubles on, the gradient after them all
  auto *d_exposure = reinterpret_cast<double *>(raw + o_exposure);
  double *d_exposure_grad = d_exposure + 36u * (size_t)num_views;
  std::vector<double> exposures(12u * (size_t)num_views, 0.0);
  for (int v = 0; v < num_views; ++v) exposures[12u * (size_t)v] = exposures[12u * (size_t)v + 5u] = exposures[12u * (size_t)v + 10u] = 1.0;
  std::vector<int> visits((size_t)num_views, 0);
  auto fail = [&](int v, int r) {
    if (h_bad_view) *h_bad_view = v;
    return r;
  };
  SPZ_HIP_TRY(hipMemsetAsync(d_skipped, 0, 4, c->st));

  // the output begins as A's bytes
  SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&c->out_block), lay_a.total_bytes));
  SPZ_HIP_TRY(hipMemcpyAsync(c->out_block, d_stream_a, lay_a.total_bytes, hipMemcpyDeviceToDevice, c->st));
  c->out = c->out_block;
  c->out_bytes = lay_a.total_bytes;

  // targets and the "before" metrics
  uint64_t cap = 0, total = 0;
  const RenderSource src_a = packed_render_source(d_stream_a, size_a, hdr_a);
  auto render = [&](const RenderSource &src, const spz_amd_render_params *p, float *d_out) {
    return render_view(&c->scratch, &cap, src, p, d_total, d_status, d_out, c->st, &total);
  };
  // render_view with the depth blend for the second stage: the same image, and d_depth
  auto render_with_depth = [&](const RenderSource &src, const spz_amd_render_params *p, float *d_out) {
    const int r = prepare_view(&c->scratch, &cap, src, p, d_total, c->st, &total);
    if (r != SPZ_AMD_OK) return r;
    return spz_amd_render_depth_device(src.n, p, total, d_out, d_depth, nullptr, d_status, c->scratch, c->st);
  };
  // view v's depth error (L and W_v, scale 1) of the depth render in d_image and d_depth, into slot `which` (0: A, 1:
  // the output stream)
  auto depth_error = [&](int v, int which) {
    const spz_amd_render_params &p = views[v];
    return spz_amd_depth_loss_device(d_depth, d_image, depth_map(v), weight(v), (int)p.width, (int)p.height,
                                     photo->depth->kind, photo->depth->min_alpha, 1.0,
                                     d_derr + 2u * (2u * (size_t)v + (size_t)which), d_gdepth, nullptr, raw + o_dws,
                                     c->st);
  };
  for (int v = 0; v < num_views; ++v) {
    const spz_amd_render_params &p = views[v];
    if (photo == nullptr) {
      const RenderSource src_b = packed_render_source(d_stream_b, size_b, hdr_b);
      rc = render(src_b, &p, reinterpret_cast<float *>(raw + target_off[(size_t)v]));
      if (rc != SPZ_AMD_OK) return fail(v, rc);
    }
    rc = depth_map(v) ? render_with_depth(src_a, &p, d_image) : render(src_a, &p, d_image);
    if (rc != SPZ_AMD_OK) return fail(v, rc);
    rc = spz_amd_image_metrics_device(d_image, 4, target(v), tch, (int)p.width, (int)p.height, d_metrics + v, nullptr,
                                      raw + o_mws, c->st);
    if (rc != SPZ_AMD_OK) return fail(v, rc);
    if (depth_map(v)) {
      rc = depth_error(v, 0);
      if (rc != SPZ_AMD_OK) return fail(v, rc);
    }
  }
  if (fit) {
    SPZ_HIP_TRY(hipMemsetAsync(d_exposure, 0, 3u * 96u * (size_t)num_views + 96u, c->st));
    SPZ_HIP_TRY(hipMemcpyAsync(d_exposure, exposures.data(), 96u * (size_t)num_views, hipMemcpyHostToDevice, c->st));
  }
  SPZ_HIP_TRY(hipStreamSynchronize(c->st));
  const double before_ms = ms_since(t0);

  // the iterations
  if (iters > 0) {
    const spz_amd_cloud_out dec = {cs.p.positions, cs.p.scales, cs.p.rotations, cs.p.alphas, cs.p.colors, cs.p.sh};
    rc = spz_amd_decode_device(d_stream_a, size_a, hdr_a, coord, &dec, c->st);
    if (rc != SPZ_AMD_OK) return rc;
    if (cs.moments_bytes) SPZ_HIP_TRY(hipMemsetAsync(raw + cs.moments_off, 0, cs.moments_bytes, c->st));
    spz_amd_cloud_in cloud = {cs.p.positions, cs.p.scales, cs.p.rotations, cs.p.alphas, cs.p.colors, cs.p.sh};
    if (dn && cap_n) SPZ_HIP_TRY(hipMemsetAsync(raw + o_accum, 0, o_action - o_accum, c->st));  // accum and denom
    RenderSource src_f;
    src_f.cloud = &cloud;
    src_f.n = n;
    src_f.sh_degree = deg;
    src_f.antialiased = aa;
    for (int i = 0; i < iters; ++i) {
      const int v = i % num_views;
      const spz_amd_render_params &p = views[v];
      const bool with_depth = depth_map(v) != nullptr && photo->depth->weight > 0.0;
      rc = with_depth ? render_with_depth(src_f, &p, d_image) : render(src_f, &p, d_image);
      if (rc != SPZ_AMD_OK) return fail(v, rc);
      if (photo != nullptr) {
        rc = photo_loss_enqueue(d_image, 4, target(v), tch, weight(v), fit ? d_exposure + 12u * (size_t)v : nullptr,
                                (int)p.width, (int)p.height, options->lambda_dssim, d_loss + 3 * (size_t)i, d_grad,
                                fit ? d_exposure_grad : nullptr, raw + o_lws, c->st);
      } else {
        rc = spz_amd_image_loss_device(d_image, 4, target(v), 4, (int)p.width, (int)p.height, options->lambda_dssim,
                                       d_loss + 3 * (size_t)i, d_grad, raw + o_lws, c->st);
      }
      if (rc != SPZ_AMD_OK) return fail(v, rc);
      if (fit) {  // the exposure's own step: the image gradient above was formed with the values before it
        double *e = d_exposure + 12u * (size_t)v;
        rc = photo_exposure_adam_enqueue(e, d_exposure_grad, e + 12u * (size_t)num_views, e + 24u * (size_t)num_views,
                                         ++visits[(size_t)v], photo->options->lr_exposure, options->beta1,
                                         options->beta2, options->eps, c->st);
        if (rc != SPZ_AMD_OK) return rc;
      }
      const bool gather_stats = dn && i >= densify->from_iter && i < densify->until_iter;
      if (with_depth) {  // the depth term: its gradient to alpha joins the photo loss's d_grad
        rc = spz_amd_depth_loss_device(d_depth, d_image, depth_map(v), weight(v), (int)p.width, (int)p.height,
                                       photo->depth->kind, photo->depth->min_alpha, photo->depth->weight,
                                       d_dloss + 2 * (size_t)i, d_gdepth, d_grad, raw + o_dws, c->st);
        if (rc != SPZ_AMD_OK) return fail(v, rc);
        rc = spz_amd_render_depth_backward_device(&cloud, n_cur, deg, aa, &p, total, d_grad, d_gdepth, &cs.g,
                                                  gather_stats && n_cur ? d_rg : nullptr, nullptr, d_status, c->scratch,
                                                  raw + o_bws, c->st);
      } else {
        rc = spz_amd_render_backward_device(&cloud, n_cur, deg, aa, &p, total, d_image, d_grad, &cs.g,
                                            gather_stats && n_cur ? d_rg : nullptr, d_status, c->scratch, raw + o_bws,
                                            c->st);
      }
      if (rc != SPZ_AMD_OK) return fail(v, rc);
      if (gather_stats && n_cur) {  // the records are the front of the render workspace
        rc = spz_amd_densify_accumulate_device(reinterpret_cast<const spz_amd_render_record *>(align_ws(c->scratch)),
                                               d_rg, n_cur, p.width, p.height, d_accum, d_denom, c->st);
        if (rc != SPZ_AMD_OK) return rc;
      }
      if (n_cur) {
        spz_amd_adam_scalars sc;
        rc = spz_amd_adam_scalars_of(i + 1, options->lr, options->beta1, options->beta2, options->eps, &sc);
        if (rc != SPZ_AMD_OK) return rc;
        rc = adam_enqueue(&cs.p, &cs.g, &cs.m, &cs.v, n_cur, deg, mask, sc, d_skipped, c->st);
        if (rc != SPZ_AMD_OK) return rc;
      }
      if (gather_stats && (i + 1) % densify->interval == 0) {
        uint64_t counts[5] = {};
        rc = spz_amd_densify_plan_host(d_accum, d_denom, cs.p.scales, cs.p.alphas, n_cur, &lim, cap_n, cap_n,
                                       raw + o_action, d_parent, raw + o_child, d_counts, raw + o_pws, counts, c->st);
        if (rc != SPZ_AMD_OK) return rc;
        const uint64_t n_new = counts[0];
        if (n_new > cap_n) return SPZ_AMD_ERR_CAPACITY;  // (the plan's bound says it cannot be)
        rc = spz_amd_densify_apply_device(&cs.p, &cs.m, &cs.v, &alt.p, &alt.m, &alt.v, d_parent, raw + o_child, n_cur,
                                          n_new, cap_n, deg, densify->seed, (uint32_t)rounds.size(), c->st);
        if (rc != SPZ_AMD_OK) return rc;
        uint32_t *origin_next = d_origin[origin_cur == d_origin[0] ? 1 : 0];
        rc = densify_gather_u32(origin_cur, d_parent, n_cur, n_new, origin_next, c->st);
        if (rc != SPZ_AMD_OK) return rc;
        origin_cur = origin_next;
        std::swap(cs.p, alt.p);
        std::swap(cs.m, alt.m);
        std::swap(cs.v, alt.v);
        cloud = spz_amd_cloud_in{cs.p.positions, cs.p.scales, cs.p.rotations, cs.p.alphas, cs.p.colors, cs.p.sh};
        if (cap_n) SPZ_HIP_TRY(hipMemsetAsync(raw + o_accum, 0, o_action - o_accum, c->st));
        rounds.push_back(spz_amd_densify_round{i, 0, counts[1], counts[2], counts[3], counts[4], n_new});
        n_cur = n_new;
        src_f.n = n_cur;
      }
      if (dn && densify->opacity_reset_interval > 0 && (i + 1) % densify->opacity_reset_interval == 0) {
        rc = spz_amd_densify_reset_opacity_device(cs.p.alphas, cs.m.alphas, cs.v.alphas, n_cur, c->st);
        if (rc != SPZ_AMD_OK) return rc;
      }
    }
    if (dn) {
      // the output at the new count: A's bytes gathered through the origin map, the header's count replaced
      spz_amd_layout lay_o;
      rc = spz_amd_stream_layout(n_cur, deg, (int)hdr_a->version, &lay_o);
      if (rc != SPZ_AMD_OK) return rc;
      if (origin_cur != nullptr) {
        SPZ_HIP_TRY(hipStreamSynchronize(c->st));
        SPZ_HIP_TRY(hipFree(c->out_block));
        c->out_block = nullptr;
        c->out = nullptr;
        SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&c->out_block), lay_o.total_bytes));
        c->out = c->out_block;
        c->out_bytes = lay_o.total_bytes;
        rc = spz_amd_subset_device(d_stream_a, size_a, hdr_a, origin_cur, n_cur, -1, c->out_block, lay_o.total_bytes,
                                   c->st);
        if (rc != SPZ_AMD_OK) return rc;
      }
    }
    // the trained sections over the copy of A's bytes, from the views' frame back to the file's
    const unsigned sec_of[6] = {1u << SPZ_AMD_SEC_POSITIONS, 1u << SPZ_AMD_SEC_SCALES, 1u << SPZ_AMD_SEC_ROTATIONS,
                                1u << SPZ_AMD_SEC_ALPHAS,    1u << SPZ_AMD_SEC_COLORS, 1u << SPZ_AMD_SEC_SH};
    unsigned sections = 0;
    for (int k = 0; k < 6; ++k) sections |= ((mask >> k) & 1u) ? sec_of[k] : 0u;
    if (n_cur && sections) {
      rc = spz_amd_encode_shard_sections_device(&cloud, 0, n_cur, n_cur, deg, aa, coord, (int)hdr_a->version, 0, sections,
                                                c->out_block, c->out_bytes, c->st);
      if (rc != SPZ_AMD_OK) return rc;
    }
  }
  if (fit) {
    SPZ_HIP_TRY(hipMemcpyAsync(exposures.data(), d_exposure, 96u * (size_t)num_views, hipMemcpyDeviceToHost, c->st));
  }
  SPZ_HIP_TRY(hipStreamSynchronize(c->st));
  const double loop_ms = ms_since(t0) - before_ms;

  // the "after" metrics: of the output stream
  spz_amd_header hdr_o = *hdr_a;
  hdr_o.num_points = (uint32_t)n_cur;
  RenderSource src_o = packed_render_source(c->out_block, c->out_bytes, &hdr_o);
  for (int v = 0; v < num_views; ++v) {
    const spz_amd_render_params &p = views[v];
    if (iters == 0) break;
    rc = depth_map(v) ? render_with_depth(src_o, &p, d_image) : render(src_o, &p, d_image);
    if (rc != SPZ_AMD_OK) return fail(v, rc);
    if (depth_map(v)) {
      rc = depth_error(v, 1);
      if (rc != SPZ_AMD_OK) return fail(v, rc);
    }
    if (fit) {  // the file is judged through the exposure fitted for this photograph
      rc = spz_amd_image_exposure_device(d_image, 4, exposures.data() + 12u * (size_t)v, (int)p.width, (int)p.height,
                                         d_image, c->st);
      if (rc != SPZ_AMD_OK) return fail(v, rc);
    }
    rc = spz_amd_image_metrics_device(d_image, 4, target(v), tch, (int)p.width, (int)p.height,
                                      d_metrics + num_views + v, nullptr, raw + o_mws, c->st);
    if (rc != SPZ_AMD_OK) return fail(v, rc);
  }
  if (photo != nullptr && photo->h_exposures != nullptr) {
    std::memcpy(photo->h_exposures, exposures.data(), 96u * (size_t)num_views);
  }
  const size_t mbytes = (size_t)num_views * sizeof(spz_amd_image_metrics);
  if (h_before) SPZ_HIP_TRY(hipMemcpyAsync(h_before, d_metrics, mbytes, hipMemcpyDeviceToHost, c->st));
  if (h_after) {
    SPZ_HIP_TRY(hipMemcpyAsync(h_after, iters ? d_metrics + num_views : d_metrics, mbytes, hipMemcpyDeviceToHost, c->st));
  }
  std::vector<double> loss3(3u * (size_t)iters);
  if (iters) SPZ_HIP_TRY(hipMemcpyAsync(loss3.data(), d_loss, 24u * (size_t)iters, hipMemcpyDeviceToHost, c->st));
  std::vector<double> dloss2(any_depth ? 2u * (size_t)iters : 0u), derr4(any_depth ? 4u * (size_t)num_views : 0u);
  if (any_depth) {
    if (iters) SPZ_HIP_TRY(hipMemcpyAsync(dloss2.data(), d_dloss, 16u * (size_t)iters, hipMemcpyDeviceToHost, c->st));
    SPZ_HIP_TRY(hipMemcpyAsync(derr4.data(), d_derr, 32u * (size_t)num_views, hipMemcpyDeviceToHost, c->st));
  }
  uint32_t skipped = 0;
  SPZ_HIP_TRY(hipMemcpyAsync(&skipped, d_skipped, 4, hipMemcpyDeviceToHost, c->st));
  if (rep.h_origin && origin_cur && n_cur) {
    SPZ_HIP_TRY(hipMemcpyAsync(rep.h_origin, origin_cur, 4u * n_cur, hipMemcpyDeviceToHost, c->st));
  }
  SPZ_HIP_TRY(hipStreamSynchronize(c->st));
  if (rep.h_origin && !origin_cur) {
    for (uint64_t k = 0; k < n_cur; ++k) rep.h_origin[k] = (uint32_t)k;
  }
  if (rep.h_num_points) *rep.h_num_points = n_cur;
  if (rep.h_num_rounds) *rep.h_num_rounds = (int)rounds.size();
  for (size_t k = 0; rep.h_rounds && k < rounds.size() && (int)k < rep.rounds_capacity; ++k) rep.h_rounds[k] = rounds[k];
  for (int i = 0; i < iters; ++i) {
    const bool with_depth = depth_map(i % num_views) != nullptr && photo->depth->weight > 0.0;
    const double l_depth = with_depth ? dloss2[2u * (size_t)i] : 0.0;
    h_history[i] = with_depth ? loss3[3u * (size_t)i] + photo->depth->weight * l_depth : loss3[3u * (size_t)i];
    if (photo && photo->h_depth_history) photo->h_depth_history[i] = l_depth;
  }
  for (int v = 0; photo && photo->h_depth_error && v < num_views; ++v) {
    const bool has = depth_map(v) != nullptr;
    photo->h_depth_error[2 * v] = has ? derr4[4u * (size_t)v] : -1.0;
    photo->h_depth_error[2 * v + 1] = has ? derr4[4u * (size_t)v + (iters ? 2u : 0u)] : -1.0;
  }
  if (h_skipped) *h_skipped = skipped;
  if (h_ms) {
    h_ms[0] = (float)before_ms;
    h_ms[1] = (float)loop_ms;
    h_ms[2] = (float)(ms_since(t0) - before_ms - loop_ms);
  }
  *h_out_bytes = c->out_bytes;
  // fetch needs the output alone
  SPZ_HIP_TRY(hipFree(c->scratch));
  c->scratch = nullptr;
  SPZ_HIP_TRY(hipFree(c->block));
  c->block = nullptr;
  *ctx = c.release();
  return SPZ_AMD_OK;
}

}  // namespace

extern "C" {

int spz_amd_refine_open(const uint8_t *d_stream_a, size_t size_a, const spz_amd_header *hdr_a,
                        const uint8_t *d_stream_b, size_t size_b, const spz_amd_header *hdr_b,
                        const spz_amd_render_params *views, int num_views, const spz_amd_refine_options *options,
                        int device, void **ctx, uint64_t *h_out_bytes, double *h_history,
                        spz_amd_image_metrics *h_before, spz_amd_image_metrics *h_after, uint64_t *h_skipped, float *h_ms,
                        int32_t *h_bad_view) {
  return refine_run(d_stream_a, size_a, hdr_a, d_stream_b, size_b, hdr_b, views, num_views, options, nullptr, device,
                    ctx, h_out_bytes, h_history, h_before, h_after, h_skipped, h_ms, h_bad_view,
                    DensifyReport{nullptr, nullptr, 0, nullptr, nullptr});
}

int spz_amd_refine_densify_open(const uint8_t *d_stream_a, size_t size_a, const spz_amd_header *hdr_a,
                                const uint8_t *d_stream_b, size_t size_b, const spz_amd_header *hdr_b,
                                const spz_amd_render_params *views, int num_views, const spz_amd_refine_options *options,
                                const spz_amd_densify_options *densify, int device, void **ctx, uint64_t *h_out_bytes,
                                double *h_history, spz_amd_image_metrics *h_before, spz_amd_image_metrics *h_after,
                                uint64_t *h_skipped, float *h_ms, int32_t *h_bad_view, uint64_t *h_num_points,
                                spz_amd_densify_round *h_rounds, int rounds_capacity, int *h_num_rounds,
                                uint32_t *h_origin) {
  if (rounds_capacity < 0 || (rounds_capacity > 0 && h_rounds == nullptr)) {
    if (h_bad_view) *h_bad_view = -1;
    if (ctx) *ctx = nullptr;
    if (h_out_bytes) *h_out_bytes = 0;
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  return refine_run(d_stream_a, size_a, hdr_a, d_stream_b, size_b, hdr_b, views, num_views, options, densify, device,
                    ctx, h_out_bytes, h_history, h_before, h_after, h_skipped, h_ms, h_bad_view,
                    DensifyReport{h_num_points, h_rounds, rounds_capacity, h_num_rounds, h_origin});
}

int spz_amd_refine_images_depth_open(const uint8_t *d_stream_a, size_t size_a, const spz_amd_header *hdr_a,
                                     const spz_amd_render_params *views, int num_views, const float *const *d_targets,
                                     int channels, const float *const *d_weights, const float *const *d_depth_targets,
                                     const spz_amd_depth_options *depth, const spz_amd_refine_options *options,
                                     const spz_amd_photo_options *photo, const spz_amd_densify_options *densify,
                                     int device, void **ctx, uint64_t *h_out_bytes, double *h_history,
                                     spz_amd_image_metrics *h_before, spz_amd_image_metrics *h_after,
                                     uint64_t *h_skipped, float *h_ms, int32_t *h_bad_view, uint64_t *h_num_points,
                                     spz_amd_densify_round *h_rounds, int rounds_capacity, int *h_num_rounds,
                                     uint32_t *h_origin, double *h_exposures, double *h_depth_history,
                                     double *h_depth_error) {
  if (rounds_capacity < 0 || (rounds_capacity > 0 && h_rounds == nullptr) || depth == nullptr) {
    if (h_bad_view) *h_bad_view = -1;
    if (ctx) *ctx = nullptr;
    if (h_out_bytes) *h_out_bytes = 0;
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  PhotoTargets targets = {d_targets, d_weights, channels, photo, h_exposures};
  targets.d_depths = d_depth_targets;
  targets.depth = depth;
  targets.h_depth_history = h_depth_history;
  targets.h_depth_error = h_depth_error;
  return refine_run(d_stream_a, size_a, hdr_a, nullptr, 0, nullptr, views, num_views, options, densify, device, ctx,
                    h_out_bytes, h_history, h_before, h_after, h_skipped, h_ms, h_bad_view,
                    DensifyReport{h_num_points, h_rounds, rounds_capacity, h_num_rounds, h_origin}, &targets);
}

int spz_amd_refine_images_open(const uint8_t *d_stream_a, size_t size_a, const spz_amd_header *hdr_a,
                               const spz_amd_render_params *views, int num_views, const float *const *d_targets,
                               int channels, const float *const *d_weights, const spz_amd_refine_options *options,
                               const spz_amd_photo_options *photo, const spz_amd_densify_options *densify, int device,
                               void **ctx, uint64_t *h_out_bytes, double *h_history, spz_amd_image_metrics *h_before,
                               spz_amd_image_metrics *h_after, uint64_t *h_skipped, float *h_ms, int32_t *h_bad_view,
                               uint64_t *h_num_points, spz_amd_densify_round *h_rounds, int rounds_capacity,
                               int *h_num_rounds, uint32_t *h_origin, double *h_exposures) {
  if (rounds_capacity < 0 || (rounds_capacity > 0 && h_rounds == nullptr)) {
    if (h_bad_view) *h_bad_view = -1;
    if (ctx) *ctx = nullptr;
    if (h_out_bytes) *h_out_bytes = 0;
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  const PhotoTargets targets = {d_targets, d_weights, channels, photo, h_exposures};
  return refine_run(d_stream_a, size_a, hdr_a, nullptr, 0, nullptr, views, num_views, options, densify, device, ctx,
                    h_out_bytes, h_history, h_before, h_after, h_skipped, h_ms, h_bad_view,
                    DensifyReport{h_num_points, h_rounds, rounds_capacity, h_num_rounds, h_origin}, &targets);
}

}  // extern "C"

namespace {

// refine_images_host_open (depth_entry false: h_depths and depth are NULL) and refine_images_depth_host_open: the
// images, weight maps and depth maps uploaded, then the device form.
int images_host_open(const uint8_t *d_stream_a, size_t size_a, const spz_amd_header *hdr_a,
                     const spz_amd_render_params *views, int num_views, const float *const *h_targets, int channels,
                     const float *const *h_weights, const float *const *h_depths, const spz_amd_depth_options *depth,
                     bool depth_entry, const spz_amd_refine_options *options, const spz_amd_photo_options *photo,
                     const spz_amd_densify_options *densify, int device, void **ctx, uint64_t *h_out_bytes,
                     double *h_history, spz_amd_image_metrics *h_before, spz_amd_image_metrics *h_after,
                     uint64_t *h_skipped, float *h_ms, int32_t *h_bad_view, uint64_t *h_num_points,
                     spz_amd_densify_round *h_rounds, int rounds_capacity, int *h_num_rounds, uint32_t *h_origin,
                     double *h_exposures, double *h_depth_history, double *h_depth_error) {
  if (h_bad_view) *h_bad_view = -1;
  if (ctx) *ctx = nullptr;
  if (h_out_bytes) *h_out_bytes = 0;
  int rc = check_views(views, num_views, SPZ_AMD_REFINE_MAX_VIEWS, h_bad_view);
  if (rc != SPZ_AMD_OK) return rc;
  if (h_targets == nullptr || (channels != 3 && channels != 4)) return SPZ_AMD_ERR_INVALID_ARG;
  if (spz_amd_refine_check(options) != SPZ_AMD_OK || spz_amd_photo_check(photo) != SPZ_AMD_OK || rounds_capacity < 0 ||
      (rounds_capacity > 0 && h_rounds == nullptr) || (depth_entry && spz_amd_depth_check(depth) != SPZ_AMD_OK)) {
    return SPZ_AMD_ERR_INVALID_ARG;  // before anything is uploaded
  }
  spz_amd_layout lay_a;
  rc = check_packed_stream(d_stream_a, size_a, hdr_a, &lay_a);
  if (rc != SPZ_AMD_OK) return rc;
  WorkspaceOffsets o;
  std::vector<uint64_t> t_off((size_t)num_views), w_off((size_t)num_views), z_off((size_t)num_views);
  for (int v = 0; v < num_views; ++v) {
    if (h_targets[v] == nullptr) {
      if (h_bad_view) *h_bad_view = v;
      return SPZ_AMD_ERR_INVALID_ARG;
    }
    const uint64_t px = (uint64_t)views[v].width * views[v].height;
    t_off[(size_t)v] = o.put(4u * (uint64_t)channels * px);
    w_off[(size_t)v] = o.put(h_weights && h_weights[v] ? 4u * px : 0u);
    z_off[(size_t)v] = o.put(h_depths && h_depths[v] ? 4u * px : 0u);
  }
  DeviceGuard guard;
  rc = guard.enter(device);
  if (rc != SPZ_AMD_OK) return rc;
  struct Block {
    uint8_t *p = nullptr;
    ~Block() {
      if (p) (void)hipFree(p);
    }
  } block;
  SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&block.p), o.off ? o.off : 256u));
  std::vector<const float *> d_targets((size_t)num_views), d_weights((size_t)num_views, nullptr),
      d_depths((size_t)num_views, nullptr);
  for (int v = 0; v < num_views; ++v) {
    const uint64_t px = (uint64_t)views[v].width * views[v].height;
    d_targets[(size_t)v] = reinterpret_cast<const float *>(block.p + t_off[(size_t)v]);
    SPZ_HIP_TRY(hipMemcpy(block.p + t_off[(size_t)v], h_targets[v], 4u * (uint64_t)channels * px, hipMemcpyHostToDevice));
    if (h_weights && h_weights[v]) {
      d_weights[(size_t)v] = reinterpret_cast<const float *>(block.p + w_off[(size_t)v]);
      SPZ_HIP_TRY(hipMemcpy(block.p + w_off[(size_t)v], h_weights[v], 4u * px, hipMemcpyHostToDevice));
    }
    if (h_depths && h_depths[v]) {
      d_depths[(size_t)v] = reinterpret_cast<const float *>(block.p + z_off[(size_t)v]);
      SPZ_HIP_TRY(hipMemcpy(block.p + z_off[(size_t)v], h_depths[v], 4u * px, hipMemcpyHostToDevice));
    }
  }
  // (the loop blocks, so the images outlive it)
  if (depth_entry) {
    return spz_amd_refine_images_depth_open(d_stream_a, size_a, hdr_a, views, num_views, d_targets.data(), channels,
                                            h_weights ? d_weights.data() : nullptr, h_depths ? d_depths.data() : nullptr,
                                            depth, options, photo, densify, device, ctx, h_out_bytes, h_history, h_before,
                                            h_after, h_skipped, h_ms, h_bad_view, h_num_points, h_rounds, rounds_capacity,
                                            h_num_rounds, h_origin, h_exposures, h_depth_history, h_depth_error);
  }
  return spz_amd_refine_images_open(d_stream_a, size_a, hdr_a, views, num_views, d_targets.data(), channels,
                                    h_weights ? d_weights.data() : nullptr, options, photo, densify, device, ctx,
                                    h_out_bytes, h_history, h_before, h_after, h_skipped, h_ms, h_bad_view, h_num_points,
                                    h_rounds, rounds_capacity, h_num_rounds, h_origin, h_exposures);
}

}  // namespace

extern "C" {

int spz_amd_refine_images_host_open(const uint8_t *d_stream_a, size_t size_a, const spz_amd_header *hdr_a,
                                    const spz_amd_render_params *views, int num_views, const float *const *h_targets,
                                    int channels, const float *const *h_weights, const spz_amd_refine_options *options,
                                    const spz_amd_photo_options *photo, const spz_amd_densify_options *densify,
                                    int device, void **ctx, uint64_t *h_out_bytes, double *h_history,
                                    spz_amd_image_metrics *h_before, spz_amd_image_metrics *h_after, uint64_t *h_skipped,
                                    float *h_ms, int32_t *h_bad_view, uint64_t *h_num_points,
                                    spz_amd_densify_round *h_rounds, int rounds_capacity, int *h_num_rounds,
                                    uint32_t *h_origin, double *h_exposures) {
  return images_host_open(d_stream_a, size_a, hdr_a, views, num_views, h_targets, channels, h_weights, nullptr, nullptr,
                          false, options, photo, densify, device, ctx, h_out_bytes, h_history, h_before, h_after,
                          h_skipped, h_ms, h_bad_view, h_num_points, h_rounds, rounds_capacity, h_num_rounds, h_origin,
                          h_exposures, nullptr, nullptr);
}

int spz_amd_refine_images_depth_host_open(const uint8_t *d_stream_a, size_t size_a, const spz_amd_header *hdr_a,
                                          const spz_amd_render_params *views, int num_views,
                                          const float *const *h_targets, int channels, const float *const *h_weights,
                                          const float *const *h_depth_targets, const spz_amd_depth_options *depth,
                                          const spz_amd_refine_options *options, const spz_amd_photo_options *photo,
                                          const spz_amd_densify_options *densify, int device, void **ctx,
                                          uint64_t *h_out_bytes, double *h_history, spz_amd_image_metrics *h_before,
                                          spz_amd_image_metrics *h_after, uint64_t *h_skipped, float *h_ms,
                                          int32_t *h_bad_view, uint64_t *h_num_points, spz_amd_densify_round *h_rounds,
                                          int rounds_capacity, int *h_num_rounds, uint32_t *h_origin,
                                          double *h_exposures, double *h_depth_history, double *h_depth_error) {
  return images_host_open(d_stream_a, size_a, hdr_a, views, num_views, h_targets, channels, h_weights, h_depth_targets,
                          depth, true, options, photo, densify, device, ctx, h_out_bytes, h_history, h_before, h_after,
                          h_skipped, h_ms, h_bad_view, h_num_points, h_rounds, rounds_capacity, h_num_rounds, h_origin,
                          h_exposures, h_depth_history, h_depth_error);
}

int spz_amd_refine_fetch(void *ctx, uint8_t *h_out) { return packed_result_fetch(ctx, h_out); }

const uint8_t *spz_amd_refine_device_data(void *ctx) { return packed_result_device_data(ctx); }

void spz_amd_refine_close(void *ctx) { packed_result_close(ctx); }

}  // extern "C"
