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
//
// The six open entries share one path: an entry fills a RefineRequest and a RefineOutputs; reset() and plan() refuse on
// the host, before any HIP call, and derive every fact once; layout() cuts the one allocation into typed RefineBuffers;
// RefineRun is the loop as small functions over that state.  The host forms upload and join at refine_run.
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
  spz_amd_cloud_grads p = {}, g = {}, m = {}, v = {};
};

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

// What the caller of one of the six open entries gives.  An entry fills this and a RefineOutputs; nothing below the
// entries reads an argument list.
struct RefineRequest {
  const uint8_t *d_stream_a;
  size_t size_a;
  const spz_amd_header *hdr_a;
  const uint8_t *d_stream_b;  // the stream the targets are rendered from: not read when they are given
  size_t size_b;
  const spz_amd_header *hdr_b;
  const spz_amd_render_params *views;
  int num_views;
  const spz_amd_refine_options *options;
  const spz_amd_densify_options *densify;  // NULL or interval 0: off
  int device;
  bool given = false;  // "refine images": the targets are the caller's num_views images of `channels` floats a pixel
  const spz_amd_photo_options *photo = nullptr;
  const float *const *targets = nullptr;
  int channels = 4;
  const float *const *weights = nullptr;  // NULL, or num_views weight maps, any of them NULL
  bool depth_entry = false;               // "refine images with depth": depth is required
  const spz_amd_depth_options *depth = nullptr;
  const float *const *depths = nullptr;  // NULL, or num_views depth maps, any of them NULL
  bool on_host = false;  // the host forms before their upload: targets, weights and depths point to host memory
};

// Every place a result goes, in the order of the entries' arguments.  All but ctx and h_out_bytes may be NULL.
struct RefineOutputs {
  void **ctx;
  uint64_t *h_out_bytes;
  double *h_history;
  spz_amd_image_metrics *h_before, *h_after;
  uint64_t *h_skipped;
  float *h_ms;
  int32_t *h_bad_view;
  uint64_t *h_num_points = nullptr;  // densify's report
  spz_amd_densify_round *h_rounds = nullptr;
  int rounds_capacity = 0;
  int *h_num_rounds = nullptr;
  uint32_t *h_origin = nullptr;
  double *h_exposures = nullptr, *h_depth_history = nullptr, *h_depth_error = nullptr;  // 12 V, iterations, 2 V doubles
};

// What every entry does first: no refusal leaves an output as the caller had it.
void reset(const RefineOutputs &o) {
  if (o.ctx) *o.ctx = nullptr;
  if (o.h_out_bytes) *o.h_out_bytes = 0;
  if (o.h_bad_view) *o.h_bad_view = -1;
  if (o.h_num_points) *o.h_num_points = 0;
  if (o.h_num_rounds) *o.h_num_rounds = 0;
}

// What follows from a request, derived once.
struct RefinePlan {
  spz_amd_layout lay_a;
  // A's points; those of the stream the targets are rendered from (A's when they are given); the most the cloud may
  // grow to (n unless rounds run)
  uint64_t n = 0, n_target = 0, cap_n = 0;
  int deg = 0, aa = 0, coord = 0, iters = 0;
  int tch = 4;             // the targets' channels
  unsigned mask = 0;       // the trained arrays (without sh at degree 0: nothing to train there)
  bool fit = false;        // an exposure per view is fitted
  bool any_depth = false;  // some view has a depth map
  bool densify = false;    // densify rounds run
  spz_amd_densify_limits lim = {};
  uint64_t max_px = 0, loss_ws = 0, metrics_ws = 0, depth_ws = 0;  // the largest view's pixels and workspaces
};

// The given targets: the photo and depth options, then per view the image, its weight map and its depth map.
int plan_given(const RefineRequest &rq, const RefineOutputs &out, RefinePlan *pl) {
  int rc = spz_amd_photo_check(rq.photo);
  if (rc != SPZ_AMD_OK) return rc;
  if (rq.depth_entry) {
    rc = spz_amd_depth_check(rq.depth);
    if (rc != SPZ_AMD_OK) return rc;
  }
  if (rq.targets == nullptr || (rq.channels != 3 && rq.channels != 4)) return SPZ_AMD_ERR_INVALID_ARG;
  for (int v = 0; v < rq.num_views; ++v) {
    const float *w = rq.weights ? rq.weights[v] : nullptr;
    const float *dm = rq.depths ? rq.depths[v] : nullptr;
    pl->any_depth = pl->any_depth || dm != nullptr;
    // (device memory is read as floats; the host forms copy from theirs)
    const bool readable = rq.on_host || (aligned4(rq.targets[v]) && aligned4(w) && aligned4(dm));
    if (rq.targets[v] == nullptr || !readable ||
        spz_amd_image_metrics_check((int)rq.views[v].width, (int)rq.views[v].height, 4, rq.channels) != SPZ_AMD_OK) {
      if (out.h_bad_view) *out.h_bad_view = v;
      return SPZ_AMD_ERR_INVALID_ARG;
    }
  }
  pl->fit = rq.photo->fit_exposure != 0 && rq.options->iterations > 0;
  return SPZ_AMD_OK;
}

// Densify: the thresholds once, and the capacity every buffer gets.
int plan_densify(const RefineRequest &rq, RefinePlan *pl) {
  const spz_amd_densify_options *d = rq.densify;
  pl->cap_n = pl->n;
  if (d == nullptr) return SPZ_AMD_OK;
  int rc = spz_amd_densify_check(d);
  if (rc != SPZ_AMD_OK || d->interval <= 0) return rc;
  rc = spz_amd_densify_thresholds(d, rq.views, rq.num_views, &pl->lim);
  if (rc != SPZ_AMD_OK) return rc;
  if ((pl->mask & 3u) != 3u || (d->opacity_reset_interval > 0 && (pl->mask & 8u) == 0u)) return SPZ_AMD_ERR_INVALID_ARG;
  if (rq.given && d->max_points == 0) return SPZ_AMD_ERR_INVALID_ARG;  // no target count to take
  const uint64_t mp = d->max_points ? d->max_points : pl->n_target;
  if (mp > kMaxEntries) return SPZ_AMD_ERR_TOO_MANY_POINTS;
  if (mp < pl->n) return SPZ_AMD_ERR_INVALID_ARG;
  pl->densify = pl->iters > 0;
  if (pl->densify) pl->cap_n = mp;
  return SPZ_AMD_OK;
}

// Every refusal that needs no device, in one order for the six entries, and the plan.  No HIP call.
int plan(const RefineRequest &rq, const RefineOutputs &out, RefinePlan *pl) {
  int rc = spz_amd_refine_check(rq.options);
  if (rc != SPZ_AMD_OK) return rc;
  if (rq.options->iterations > 0 && out.h_history == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  rc = check_views(rq.views, rq.num_views, SPZ_AMD_REFINE_MAX_VIEWS, out.h_bad_view);
  if (rc != SPZ_AMD_OK) return rc;
  rc = check_packed_stream(rq.d_stream_a, rq.size_a, rq.hdr_a, &pl->lay_a);
  if (rc != SPZ_AMD_OK) return rc;
  if (rq.given) {
    rc = plan_given(rq, out, pl);
    pl->tch = rq.channels;
  } else {
    spz_amd_layout lay_b;
    rc = check_packed_stream(rq.d_stream_b, rq.size_b, rq.hdr_b, &lay_b);
  }
  if (rc != SPZ_AMD_OK) return rc;
  pl->n = rq.hdr_a->num_points;
  pl->n_target = rq.given ? pl->n : rq.hdr_b->num_points;
  if (pl->n > kMaxEntries || pl->n_target > kMaxEntries) return SPZ_AMD_ERR_TOO_MANY_POINTS;
  pl->deg = rq.hdr_a->sh_degree;
  pl->aa = rq.hdr_a->flags & 1;
  pl->coord = rq.views[0].coord;
  pl->iters = rq.options->iterations;
  pl->mask = rq.options->train_mask & (pl->deg == 0 ? ~32u : ~0u);
  // what the encode kernel writes: versions 2 and 3, positions at 12 fractional bits
  if (pl->iters > 0 && (rq.hdr_a->version == 1 || ((pl->mask & 1u) && rq.hdr_a->fractional_bits != 12))) {
    return SPZ_AMD_ERR_UNSUPPORTED;
  }
  rc = plan_densify(rq, pl);
  if (rc != SPZ_AMD_OK) return rc;
  auto raise = [](uint64_t *most, uint64_t x) { *most = x > *most ? x : *most; };
  for (int v = 0; v < rq.num_views; ++v) {
    const int w = (int)rq.views[v].width, h = (int)rq.views[v].height;
    raise(&pl->max_px, (uint64_t)rq.views[v].width * rq.views[v].height);
    raise(&pl->loss_ws, rq.given ? spz_amd_photo_loss_workspace_bytes(w, h) : spz_amd_image_loss_workspace_bytes(w, h));
    raise(&pl->metrics_ws, spz_amd_image_metrics_workspace_bytes(w, h));
    raise(&pl->depth_ws, pl->any_depth ? spz_amd_depth_loss_workspace_bytes(w, h) : 0u);
  }
  return SPZ_AMD_OK;
}

// The sections of the loop's one allocation as typed pointers.  Whether a section is needed is decided in layout()
// and nowhere else.
struct RefineBuffers {
  uint64_t bytes = 0;  // the allocation
  uint64_t count[6];   // the elements of the six arrays at capacity
  CloudSet cs;         // the float cloud, its gradients and its two moments
  uint8_t *moments;    // m and v are contiguous: one memset of moments_bytes
  uint64_t moments_bytes;
  std::vector<float *> rendered;  // per view the target rendered from B (given targets are used in place)
  // a fitted exposure per view: view v's 12 values at exposure + 12 v, its moments 12 V and 24 V doubles on, and after
  // them all one gradient
  double *exposure, *exposure_grad;
  float *image, *grad;  // the render and the loss's gradient to it
  uint8_t *loss_ws, *metrics_ws, *backward_ws;
  uint64_t *total;
  uint32_t *status, *skipped;
  double *loss;                      // L, l1 and ssim per iteration
  spz_amd_image_metrics *metrics;    // "before" per view, then "after" per view
  // with depth maps: the depth render, the gradient to its channel 0, the depth loss's workspace, L_depth and W_v per
  // iteration, and per view the two depth errors (each L and W_v)
  float *depth, *gdepth;
  uint8_t *depth_ws;
  double *dloss, *derr;
  // with densify: the apply's destinations (parameters and both moments), the statistics (accum and denom contiguous:
  // one memset of stats_bytes), the plan's outputs, the two origin maps, the record gradients
  CloudSet alt;
  float *accum, *rg;
  uint32_t *denom, *parent, *origin[2];
  uint64_t stats_bytes, *counts;
  uint8_t *action, *child, *plan_ws;
};

// Sections one after the other, each 256-aligned from the allocation's base; without a base (raw NULL) only the sizes.
struct Carver {
  uint8_t *raw;
  WorkspaceOffsets o;
  template <class T = uint8_t>
  T *take(uint64_t bytes) {
    const uint64_t at = o.put(bytes);
    return raw ? reinterpret_cast<T *>(raw + at) : nullptr;
  }
  spz_amd_cloud_grads cloud(const uint64_t count[6], bool on = true) {  // the six arrays; NULL for an empty one
    float *f[6];
    for (int k = 0; k < 6; ++k) {
      float *p = take<float>(on ? count[k] * 4u : 0u);
      f[k] = on && count[k] ? p : nullptr;
    }
    return spz_amd_cloud_grads{f[0], f[1], f[2], f[3], f[4], f[5]};
  }
};

// layout(rq, pl, NULL).bytes is the allocation; layout(rq, pl, its base) binds the pointers.
RefineBuffers layout(const RefineRequest &rq, const RefinePlan &pl, uint8_t *raw) {
  RefineBuffers b;
  Carver c{raw, {}};
  const uint64_t nv = (uint64_t)rq.num_views, iters = (uint64_t)pl.iters, cap = pl.densify ? pl.cap_n : 0u;
  const uint64_t depth_px = pl.any_depth ? pl.max_px : 0u;
  cloud_counts(pl.cap_n, pl.deg, b.count);
  b.cs.p = c.cloud(b.count);
  b.cs.g = c.cloud(b.count);
  const uint64_t moments_at = c.o.off;
  b.moments = c.take(0u);
  b.cs.m = c.cloud(b.count);
  b.cs.v = c.cloud(b.count);
  b.moments_bytes = c.o.off - moments_at;
  b.rendered.resize((size_t)nv);
  for (uint64_t v = 0; v < nv; ++v) {
    b.rendered[(size_t)v] = c.take<float>(rq.given ? 0u : 16u * (uint64_t)rq.views[v].width * rq.views[v].height);
  }
  b.exposure = c.take<double>(pl.fit ? 3u * 96u * nv + 96u : 0u);
  b.exposure_grad = b.exposure ? b.exposure + 36u * nv : nullptr;
  b.image = c.take<float>(16u * pl.max_px);
  b.grad = c.take<float>(16u * pl.max_px);
  b.loss_ws = c.take(iters ? pl.loss_ws : 0u);
  b.metrics_ws = c.take(pl.metrics_ws);
  uint8_t *small = c.take(16u);
  b.total = reinterpret_cast<uint64_t *>(small);
  b.status = small ? reinterpret_cast<uint32_t *>(small + 8u) : nullptr;
  b.skipped = small ? reinterpret_cast<uint32_t *>(small + 12u) : nullptr;
  b.loss = c.take<double>(24u * iters);
  b.metrics = c.take<spz_amd_image_metrics>(2u * nv * sizeof(spz_amd_image_metrics));
  b.backward_ws = c.take(!iters          ? 0u
                         : pl.any_depth ? spz_amd_render_depth_backward_workspace_bytes(pl.cap_n)
                                        : spz_amd_render_backward_workspace_bytes(pl.cap_n));
  b.depth = c.take<float>(8u * depth_px);
  b.gdepth = c.take<float>(4u * depth_px);
  b.depth_ws = c.take(pl.depth_ws);
  b.dloss = c.take<double>(pl.any_depth ? 16u * iters : 0u);
  b.derr = c.take<double>(pl.any_depth ? 32u * nv : 0u);
  b.alt.p = c.cloud(b.count, pl.densify);
  b.alt.m = c.cloud(b.count, pl.densify);
  b.alt.v = c.cloud(b.count, pl.densify);
  const uint64_t stats_at = c.o.off;
  b.accum = c.take<float>(cap * 4u);
  b.denom = c.take<uint32_t>(cap * 4u);
  b.stats_bytes = c.o.off - stats_at;
  b.action = c.take(cap);
  b.parent = c.take<uint32_t>(cap * 4u);
  b.child = c.take(cap);
  b.origin[0] = c.take<uint32_t>(cap * 4u);
  b.origin[1] = c.take<uint32_t>(cap * 4u);
  b.rg = c.take<float>(cap * 36u);
  b.counts = c.take<uint64_t>(pl.densify ? 64u : 0u);
  b.plan_ws = c.take(pl.densify ? spz_amd_densify_plan_workspace_bytes(pl.cap_n) : 0u);
  b.bytes = c.o.off;
  return b;
}

spz_amd_cloud_in as_input(const spz_amd_cloud_grads &c) {
  return spz_amd_cloud_in{c.positions, c.scales, c.rotations, c.alphas, c.colors, c.sh};
}

// One run of the loop (DESIGN §8 "Refine", "Densify", "Fit", "Depth fit"): the result, the buffers, and what changes
// from step to step.  Every function enqueues on the result's stream; the four that wait for it say so.
struct RefineRun {
  const RefineRequest &rq;
  const RefinePlan &pl;
  const RefineOutputs &out;
  PackedResult *c;
  RefineBuffers b;
  uint64_t ws_cap = 0, total = 0;  // the render workspace's size and the last prepared view's pair count
  uint64_t n_cur = 0;              // the cloud's count now
  spz_amd_cloud_in cloud = {};     // b.cs.p, as the render reads it
  const uint32_t *origin_cur = nullptr;  // NULL: no round yet, the identity
  std::vector<spz_amd_densify_round> rounds;
  std::vector<double> exposures;  // the host's copy: the identity until the loop has fitted them
  std::vector<int> visits;        // the exposure steps a view has had

  RefineRun(const RefineRequest &rq_, const RefinePlan &pl_, const RefineOutputs &out_, PackedResult *c_)
      : rq(rq_), pl(pl_), out(out_), c(c_), n_cur(pl_.n), exposures(12u * (size_t)rq_.num_views, 0.0),
        visits((size_t)rq_.num_views, 0) {
    for (size_t v = 0; v < (size_t)rq.num_views; ++v) {
      exposures[12u * v] = exposures[12u * v + 5u] = exposures[12u * v + 10u] = 1.0;
    }
  }

  const spz_amd_render_params &view(int v) const { return rq.views[v]; }
  const float *target(int v) const { return rq.given ? rq.targets[v] : b.rendered[(size_t)v]; }
  const float *weight(int v) const { return rq.given && rq.weights ? rq.weights[v] : nullptr; }
  const float *depth_map(int v) const { return pl.any_depth ? rq.depths[v] : nullptr; }
  int fail(int v, int rc) const {
    if (out.h_bad_view) *out.h_bad_view = v;
    return rc;
  }

  // The block and, as A's bytes to begin with, the output.
  int allocate() {
    SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&c->block), layout(rq, pl, nullptr).bytes));
    b = layout(rq, pl, c->block);
    SPZ_HIP_TRY(hipMemsetAsync(b.skipped, 0, 4, c->st));
    SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&c->out_block), pl.lay_a.total_bytes));
    SPZ_HIP_TRY(hipMemcpyAsync(c->out_block, rq.d_stream_a, pl.lay_a.total_bytes, hipMemcpyDeviceToDevice, c->st));
    c->out = c->out_block;
    c->out_bytes = pl.lay_a.total_bytes;
    return SPZ_AMD_OK;
  }

  // View v of `src` into d_out; with_depth: the depth blend for the second stage: the same image, and b.depth.
  int render(const RenderSource &src, int v, bool with_depth, float *d_out) {
    if (!with_depth) return render_view(&c->scratch, &ws_cap, src, &view(v), b.total, b.status, d_out, c->st, &total);
    const int rc = prepare_view(&c->scratch, &ws_cap, src, &view(v), b.total, c->st, &total);
    if (rc != SPZ_AMD_OK) return rc;
    return spz_amd_render_depth_device(src.n, &view(v), total, d_out, b.depth, nullptr, b.status, c->scratch, c->st);
  }

  // Depth: view v's depth loss of the depth render in b.image and b.depth against its map (L and W_v into d_out), its
  // gradient to the depth channel into b.gdepth and, times `scale`, to alpha added into d_grad_image (may be NULL).
  int depth_loss(int v, double scale, double *d_out, float *d_grad_image) {
    return spz_amd_depth_loss_device(b.depth, b.image, depth_map(v), weight(v), (int)view(v).width, (int)view(v).height,
                                     rq.depth->kind, rq.depth->min_alpha, scale, d_out, b.gdepth, d_grad_image,
                                     b.depth_ws, c->st);
  }
  // The depth term of iteration i, joining the photo loss's gradient; the depth error of A (slot 0) or the output (1).
  int depth_term(int i, int v) { return depth_loss(v, rq.depth->weight, b.dloss + 2 * (size_t)i, b.grad); }
  int depth_error(int v, int slot) { return depth_loss(v, 1.0, b.derr + 4u * (size_t)v + 2u * (size_t)slot, nullptr); }

  // "before" (slot 0: src is A) and "after" (slot 1: src is the output stream, judged through the exposure fitted for
  // the photograph): view v's metrics and, with a depth map, its depth error.  The depth error of the output goes in
  // front of the exposure, which rewrites the image in place; A's has nothing to wait for and follows the metrics.
  int measure(int v, const RenderSource &src, int slot) {
    const bool z = depth_map(v) != nullptr;
    const int w = (int)view(v).width, h = (int)view(v).height;
    int rc = render(src, v, z, b.image);
    if (rc == SPZ_AMD_OK && z && slot == 1) rc = depth_error(v, 1);
    if (rc == SPZ_AMD_OK && pl.fit && slot == 1) {
      rc = spz_amd_image_exposure_device(b.image, 4, exposures.data() + 12u * (size_t)v, w, h, b.image, c->st);
    }
    if (rc == SPZ_AMD_OK) {
      spz_amd_image_metrics *d_out = b.metrics + (size_t)slot * (size_t)rq.num_views + v;
      rc = spz_amd_image_metrics_device(b.image, 4, target(v), pl.tch, w, h, d_out, nullptr, b.metrics_ws, c->st);
    }
    if (rc == SPZ_AMD_OK && z && slot == 0) rc = depth_error(v, 0);
    return rc;
  }

  // The targets where they are rendered, "before", and the exposures at the identity with zero moments.  Waits.
  int before() {
    const RenderSource src_a = packed_render_source(rq.d_stream_a, rq.size_a, rq.hdr_a);
    for (int v = 0; v < rq.num_views; ++v) {
      int rc = SPZ_AMD_OK;
      if (!rq.given) {
        const RenderSource src_b = packed_render_source(rq.d_stream_b, rq.size_b, rq.hdr_b);
        rc = render(src_b, v, false, b.rendered[(size_t)v]);
      }
      if (rc == SPZ_AMD_OK) rc = measure(v, src_a, 0);
      if (rc != SPZ_AMD_OK) return fail(v, rc);
    }
    if (pl.fit) {
      const size_t nv = (size_t)rq.num_views;
      SPZ_HIP_TRY(hipMemsetAsync(b.exposure, 0, 3u * 96u * nv + 96u, c->st));
      SPZ_HIP_TRY(hipMemcpyAsync(b.exposure, exposures.data(), 96u * nv, hipMemcpyHostToDevice, c->st));
    }
    SPZ_HIP_TRY(hipStreamSynchronize(c->st));
    return SPZ_AMD_OK;
  }

  // A decoded into the float cloud in the views' frame; zero moments and statistics.
  int decode() {
    const spz_amd_cloud_grads &p = b.cs.p;
    const spz_amd_cloud_out dec = {p.positions, p.scales, p.rotations, p.alphas, p.colors, p.sh};
    const int rc = spz_amd_decode_device(rq.d_stream_a, rq.size_a, rq.hdr_a, pl.coord, &dec, c->st);
    if (rc != SPZ_AMD_OK) return rc;
    if (b.moments_bytes) SPZ_HIP_TRY(hipMemsetAsync(b.moments, 0, b.moments_bytes, c->st));
    cloud = as_input(b.cs.p);
    if (pl.densify && pl.cap_n) SPZ_HIP_TRY(hipMemsetAsync(b.accum, 0, b.stats_bytes, c->st));
    return SPZ_AMD_OK;
  }

  int forward(int v, bool with_depth) {
    RenderSource src;
    src.cloud = &cloud;
    src.n = n_cur;
    src.sh_degree = pl.deg;
    src.antialiased = pl.aa;
    return render(src, v, with_depth, b.image);
  }

  // Iteration i's loss of the render against view v's target (L, l1, ssim into b.loss) and its gradient into b.grad.
  // Photo: given targets take the photo loss of spz_photo.hip, with the view's weights and, when they are fitted, its
  // exposure read from device memory and that exposure's gradient.
  int loss(int i, int v) {
    const int w = (int)view(v).width, h = (int)view(v).height;
    double *d_loss = b.loss + 3 * (size_t)i;
    if (!rq.given) {
      return spz_amd_image_loss_device(b.image, 4, target(v), 4, w, h, rq.options->lambda_dssim, d_loss, b.grad,
                                       b.loss_ws, c->st);
    }
    return photo_loss_enqueue(b.image, 4, target(v), pl.tch, weight(v), pl.fit ? b.exposure + 12u * (size_t)v : nullptr,
                              w, h, rq.options->lambda_dssim, d_loss, b.grad, pl.fit ? b.exposure_grad : nullptr,
                              b.loss_ws, c->st);
  }

  // Exposure: view v's own Adam step on the device.  The image gradient was formed with the values before it.
  int exposure_step(int v) {
    const size_t nv = (size_t)rq.num_views;
    double *e = b.exposure + 12u * (size_t)v;
    return photo_exposure_adam_enqueue(e, b.exposure_grad, e + 12u * nv, e + 24u * nv, ++visits[(size_t)v],
                                       rq.photo->lr_exposure, rq.options->beta1, rq.options->beta2, rq.options->eps,
                                       c->st);
  }

  // The gradients of the cloud from b.grad (and b.gdepth); with_stats: also the record gradients densify accumulates.
  int backward(int v, bool with_depth, bool with_stats) {
    float *d_rg = with_stats ? b.rg : nullptr;
    if (with_depth) {
      return spz_amd_render_depth_backward_device(&cloud, n_cur, pl.deg, pl.aa, &view(v), total, b.grad, b.gdepth, &b.cs.g,
                                                  d_rg, nullptr, b.status, c->scratch, b.backward_ws, c->st);
    }
    return spz_amd_render_backward_device(&cloud, n_cur, pl.deg, pl.aa, &view(v), total, b.image, b.grad, &b.cs.g, d_rg,
                                          b.status, c->scratch, b.backward_ws, c->st);
  }

  // Densify's statistics of view v.  The records are the front of the render workspace.
  int accumulate(int v) {
    return spz_amd_densify_accumulate_device(reinterpret_cast<const spz_amd_render_record *>(align_ws(c->scratch)), b.rg,
                                             n_cur, view(v).width, view(v).height, b.accum, b.denom, c->st);
  }

  int adam(int i) {
    spz_amd_adam_scalars sc;
    const spz_amd_refine_options &o = *rq.options;
    const int rc = spz_amd_adam_scalars_of(i + 1, o.lr, o.beta1, o.beta2, o.eps, &sc);
    if (rc != SPZ_AMD_OK) return rc;
    return adam_enqueue(&b.cs.p, &b.cs.g, &b.cs.m, &b.cs.v, n_cur, pl.deg, pl.mask, sc, b.skipped, c->st);
  }

  // Densify: one round after iteration i.  The plan (which waits for its counts), the apply into the other set of
  // parameters and moments, the origin map through the plan's parents, fresh statistics.
  int densify_round(int i) {
    uint64_t counts[5] = {};
    int rc = spz_amd_densify_plan_host(b.accum, b.denom, b.cs.p.scales, b.cs.p.alphas, n_cur, &pl.lim, pl.cap_n, pl.cap_n,
                                       b.action, b.parent, b.child, b.counts, b.plan_ws, counts, c->st);
    if (rc != SPZ_AMD_OK) return rc;
    const uint64_t n_new = counts[0];
    if (n_new > pl.cap_n) return SPZ_AMD_ERR_CAPACITY;  // (the plan's bound says it cannot be)
    rc = spz_amd_densify_apply_device(&b.cs.p, &b.cs.m, &b.cs.v, &b.alt.p, &b.alt.m, &b.alt.v, b.parent, b.child, n_cur,
                                      n_new, pl.cap_n, pl.deg, rq.densify->seed, (uint32_t)rounds.size(), c->st);
    if (rc != SPZ_AMD_OK) return rc;
    uint32_t *origin_next = b.origin[origin_cur == b.origin[0] ? 1 : 0];
    rc = densify_gather_u32(origin_cur, b.parent, n_cur, n_new, origin_next, c->st);
    if (rc != SPZ_AMD_OK) return rc;
    origin_cur = origin_next;
    std::swap(b.cs.p, b.alt.p);
    std::swap(b.cs.m, b.alt.m);
    std::swap(b.cs.v, b.alt.v);
    cloud = as_input(b.cs.p);
    if (pl.cap_n) SPZ_HIP_TRY(hipMemsetAsync(b.accum, 0, b.stats_bytes, c->st));
    rounds.push_back(spz_amd_densify_round{i, 0, counts[1], counts[2], counts[3], counts[4], n_new});
    n_cur = n_new;
    return SPZ_AMD_OK;
  }

  int reset_opacity() {
    return spz_amd_densify_reset_opacity_device(b.cs.p.alphas, b.cs.m.alphas, b.cs.v.alphas, n_cur, c->st);
  }

  // Iteration i, as DESIGN §8 has it.
  int iterate(int i) {
    const int v = i % rq.num_views;
    const spz_amd_densify_options *d = rq.densify;
    const bool with_depth = depth_map(v) != nullptr && rq.depth->weight > 0.0;
    const bool gather = pl.densify && i >= d->from_iter && i < d->until_iter;
    int rc = forward(v, with_depth);
    if (rc == SPZ_AMD_OK) rc = loss(i, v);
    if (rc != SPZ_AMD_OK) return fail(v, rc);
    if (pl.fit) rc = exposure_step(v);
    if (rc != SPZ_AMD_OK) return rc;
    if (with_depth) rc = depth_term(i, v);
    if (rc == SPZ_AMD_OK) rc = backward(v, with_depth, gather && n_cur);
    if (rc != SPZ_AMD_OK) return fail(v, rc);
    if (gather && n_cur) rc = accumulate(v);
    if (rc == SPZ_AMD_OK && n_cur) rc = adam(i);
    if (rc == SPZ_AMD_OK && gather && (i + 1) % d->interval == 0) rc = densify_round(i);
    if (rc == SPZ_AMD_OK && pl.densify && d->opacity_reset_interval > 0 && (i + 1) % d->opacity_reset_interval == 0) {
      rc = reset_opacity();
    }
    return rc;
  }

  // The output stream: after a round A's bytes gathered through the origin map at the new count (waits, to free the
  // copy of A), then the trained sections encoded over it, from the views' frame back to the file's.
  int write_output() {
    if (origin_cur != nullptr) {
      spz_amd_layout lay_o;
      int rc = spz_amd_stream_layout(n_cur, pl.deg, (int)rq.hdr_a->version, &lay_o);
      if (rc != SPZ_AMD_OK) return rc;
      SPZ_HIP_TRY(hipStreamSynchronize(c->st));
      SPZ_HIP_TRY(hipFree(c->out_block));
      c->out_block = nullptr;
      c->out = nullptr;
      SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&c->out_block), lay_o.total_bytes));
      c->out = c->out_block;
      c->out_bytes = lay_o.total_bytes;
      rc = spz_amd_subset_device(rq.d_stream_a, rq.size_a, rq.hdr_a, origin_cur, n_cur, -1, c->out_block,
                                 lay_o.total_bytes, c->st);
      if (rc != SPZ_AMD_OK) return rc;
    }
    const unsigned sec_of[6] = {1u << SPZ_AMD_SEC_POSITIONS, 1u << SPZ_AMD_SEC_SCALES, 1u << SPZ_AMD_SEC_ROTATIONS,
                                1u << SPZ_AMD_SEC_ALPHAS,    1u << SPZ_AMD_SEC_COLORS, 1u << SPZ_AMD_SEC_SH};
    unsigned sections = 0;
    for (int k = 0; k < 6; ++k) sections |= ((pl.mask >> k) & 1u) ? sec_of[k] : 0u;
    if (n_cur == 0 || sections == 0) return SPZ_AMD_OK;
    return spz_amd_encode_shard_sections_device(&cloud, 0, n_cur, n_cur, pl.deg, pl.aa, pl.coord, (int)rq.hdr_a->version,
                                                0, sections, c->out_block, c->out_bytes, c->st);
  }

  // The iterations and the output, and the fitted exposures to the host.  Waits.
  int loop() {
    int rc = pl.iters > 0 ? decode() : SPZ_AMD_OK;
    for (int i = 0; rc == SPZ_AMD_OK && i < pl.iters; ++i) rc = iterate(i);
    if (rc == SPZ_AMD_OK && pl.iters > 0) rc = write_output();
    if (rc != SPZ_AMD_OK) return rc;
    if (pl.fit) {
      SPZ_HIP_TRY(hipMemcpyAsync(exposures.data(), b.exposure, 96u * (size_t)rq.num_views, hipMemcpyDeviceToHost, c->st));
    }
    SPZ_HIP_TRY(hipStreamSynchronize(c->st));
    return SPZ_AMD_OK;
  }

  // "after": of the output stream.  Without an iteration it is "before".
  int after() {
    spz_amd_header hdr_o = *rq.hdr_a;
    hdr_o.num_points = (uint32_t)n_cur;
    const RenderSource src_o = packed_render_source(c->out_block, c->out_bytes, &hdr_o);
    for (int v = 0; pl.iters > 0 && v < rq.num_views; ++v) {
      const int rc = measure(v, src_o, 1);
      if (rc != SPZ_AMD_OK) return fail(v, rc);
    }
    return SPZ_AMD_OK;
  }

  // Every result to where the caller wants it (all but the three laps and ctx).  Waits.
  int report() {
    const size_t nv = (size_t)rq.num_views, iters = (size_t)pl.iters;
    if (out.h_exposures) std::memcpy(out.h_exposures, exposures.data(), 96u * nv);
    const size_t mbytes = nv * sizeof(spz_amd_image_metrics);
    if (out.h_before) SPZ_HIP_TRY(hipMemcpyAsync(out.h_before, b.metrics, mbytes, hipMemcpyDeviceToHost, c->st));
    if (out.h_after) {
      SPZ_HIP_TRY(hipMemcpyAsync(out.h_after, iters ? b.metrics + nv : b.metrics, mbytes, hipMemcpyDeviceToHost, c->st));
    }
    std::vector<double> loss3(3u * iters);
    if (iters) SPZ_HIP_TRY(hipMemcpyAsync(loss3.data(), b.loss, 24u * iters, hipMemcpyDeviceToHost, c->st));
    std::vector<double> dloss2(pl.any_depth ? 2u * iters : 0u), derr4(pl.any_depth ? 4u * nv : 0u);
    if (pl.any_depth) {
      if (iters) SPZ_HIP_TRY(hipMemcpyAsync(dloss2.data(), b.dloss, 16u * iters, hipMemcpyDeviceToHost, c->st));
      SPZ_HIP_TRY(hipMemcpyAsync(derr4.data(), b.derr, 32u * nv, hipMemcpyDeviceToHost, c->st));
    }
    uint32_t skipped = 0;
    SPZ_HIP_TRY(hipMemcpyAsync(&skipped, b.skipped, 4, hipMemcpyDeviceToHost, c->st));
    if (out.h_origin && origin_cur && n_cur) {
      SPZ_HIP_TRY(hipMemcpyAsync(out.h_origin, origin_cur, 4u * n_cur, hipMemcpyDeviceToHost, c->st));
    }
    SPZ_HIP_TRY(hipStreamSynchronize(c->st));
    for (uint64_t k = 0; out.h_origin && !origin_cur && k < n_cur; ++k) out.h_origin[k] = (uint32_t)k;
    if (out.h_num_points) *out.h_num_points = n_cur;
    if (out.h_num_rounds) *out.h_num_rounds = (int)rounds.size();
    for (size_t k = 0; out.h_rounds && k < rounds.size() && (int)k < out.rounds_capacity; ++k) out.h_rounds[k] = rounds[k];
    for (size_t i = 0; i < iters; ++i) {  // the history is the loss that was minimised: with the depth term where it was
      const bool with_depth = depth_map((int)(i % nv)) != nullptr && rq.depth->weight > 0.0;
      const double l_depth = with_depth ? dloss2[2u * i] : 0.0;
      out.h_history[i] = with_depth ? loss3[3u * i] + rq.depth->weight * l_depth : loss3[3u * i];
      if (out.h_depth_history) out.h_depth_history[i] = l_depth;
    }
    for (size_t v = 0; out.h_depth_error && v < nv; ++v) {
      const bool has = depth_map((int)v) != nullptr;
      out.h_depth_error[2 * v] = has ? derr4[4u * v] : -1.0;
      out.h_depth_error[2 * v + 1] = has ? derr4[4u * v + (iters ? 2u : 0u)] : -1.0;
    }
    if (out.h_skipped) *out.h_skipped = skipped;
    return SPZ_AMD_OK;
  }
};

// A planned request on its device: the three laps of h_ms are "before", the loop, and "after" with the report.
int refine_run(const RefineRequest &rq, const RefinePlan &pl, const RefineOutputs &out) {
  DeviceGuard guard;
  int rc = guard.enter(rq.device);
  if (rc != SPZ_AMD_OK) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  PackedResultPtr c;
  rc = packed_result_open(rq.device, &c);
  if (rc != SPZ_AMD_OK) return rc;
  RefineRun run(rq, pl, out, c.get());
  rc = run.allocate();
  if (rc == SPZ_AMD_OK) rc = run.before();
  if (rc != SPZ_AMD_OK) return rc;
  const double before_ms = ms_since(t0);
  rc = run.loop();
  if (rc != SPZ_AMD_OK) return rc;
  const double loop_ms = ms_since(t0) - before_ms;
  rc = run.after();
  if (rc == SPZ_AMD_OK) rc = run.report();
  if (rc != SPZ_AMD_OK) return rc;
  if (out.h_ms) {
    out.h_ms[0] = (float)before_ms;
    out.h_ms[1] = (float)loop_ms;
    out.h_ms[2] = (float)(ms_since(t0) - before_ms - loop_ms);
  }
  // fetch needs the output alone
  SPZ_HIP_TRY(hipFree(c->scratch));
  c->scratch = nullptr;
  SPZ_HIP_TRY(hipFree(c->block));
  c->block = nullptr;
  *out.h_out_bytes = c->out_bytes;
  *out.ctx = c.release();
  return SPZ_AMD_OK;
}

// Every entry's beginning: the outputs reset, the one check of the outputs themselves, the plan.
int refine_begin(const RefineRequest &rq, const RefineOutputs &out, RefinePlan *pl) {
  reset(out);
  if (out.ctx == nullptr || out.h_out_bytes == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  if (out.rounds_capacity < 0 || (out.rounds_capacity > 0 && out.h_rounds == nullptr)) return SPZ_AMD_ERR_INVALID_ARG;
  return plan(rq, out, pl);
}

int refine_open(const RefineRequest &rq, const RefineOutputs &out) {
  RefinePlan pl;
  const int rc = refine_begin(rq, out, &pl);
  return rc != SPZ_AMD_OK ? rc : refine_run(rq, pl, out);
}

// The host forms: planned (and refused) before anything is uploaded; then the images, weight maps and depth maps in one
// block of device memory, and the same run.  The run blocks, so the block outlives it.
int refine_host_open(RefineRequest rq, const RefineOutputs &out) {
  RefinePlan pl;
  rq.on_host = true;
  int rc = refine_begin(rq, out, &pl);
  if (rc != SPZ_AMD_OK) return rc;
  const size_t nv = (size_t)rq.num_views;
  const float *const *host[3] = {rq.targets, rq.weights, rq.depths};
  std::vector<const float *> dev[3];
  std::vector<uint64_t> at(3u * nv), bytes(3u * nv);
  WorkspaceOffsets o;
  for (size_t v = 0; v < nv; ++v) {
    const uint64_t px = (uint64_t)rq.views[v].width * rq.views[v].height;
    for (size_t k = 0; k < 3; ++k) {
      bytes[3u * v + k] = host[k] && host[k][v] ? 4u * px * (k == 0 ? (uint64_t)rq.channels : 1u) : 0u;
      at[3u * v + k] = o.put(bytes[3u * v + k]);
    }
  }
  DeviceGuard guard;
  rc = guard.enter(rq.device);
  if (rc != SPZ_AMD_OK) return rc;
  struct Block {
    uint8_t *p = nullptr;
    ~Block() {
      if (p) (void)hipFree(p);
    }
  } block;
  SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&block.p), o.off ? o.off : 256u));
  for (size_t k = 0; k < 3; ++k) dev[k].assign(nv, nullptr);
  for (size_t v = 0; v < nv; ++v) {
    for (size_t k = 0; k < 3; ++k) {
      if (bytes[3u * v + k] == 0) continue;
      dev[k][v] = reinterpret_cast<const float *>(block.p + at[3u * v + k]);
      SPZ_HIP_TRY(hipMemcpy(block.p + at[3u * v + k], host[k][v], bytes[3u * v + k], hipMemcpyHostToDevice));
    }
  }
  rq.targets = dev[0].data();
  rq.weights = rq.weights ? dev[1].data() : nullptr;
  rq.depths = rq.depths ? dev[2].data() : nullptr;
  rq.on_host = false;
  return refine_run(rq, pl, out);
}

}  // namespace

extern "C" {

int spz_amd_refine_open(const uint8_t *d_stream_a, size_t size_a, const spz_amd_header *hdr_a,
                        const uint8_t *d_stream_b, size_t size_b, const spz_amd_header *hdr_b,
                        const spz_amd_render_params *views, int num_views, const spz_amd_refine_options *options,
                        int device, void **ctx, uint64_t *h_out_bytes, double *h_history,
                        spz_amd_image_metrics *h_before, spz_amd_image_metrics *h_after, uint64_t *h_skipped, float *h_ms,
                        int32_t *h_bad_view) {
  const RefineRequest rq = {d_stream_a, size_a, hdr_a, d_stream_b, size_b, hdr_b, views, num_views, options, nullptr, device};
  return refine_open(rq, RefineOutputs{ctx, h_out_bytes, h_history, h_before, h_after, h_skipped, h_ms, h_bad_view});
}

int spz_amd_refine_densify_open(const uint8_t *d_stream_a, size_t size_a, const spz_amd_header *hdr_a,
                                const uint8_t *d_stream_b, size_t size_b, const spz_amd_header *hdr_b,
                                const spz_amd_render_params *views, int num_views, const spz_amd_refine_options *options,
                                const spz_amd_densify_options *densify, int device, void **ctx, uint64_t *h_out_bytes,
                                double *h_history, spz_amd_image_metrics *h_before, spz_amd_image_metrics *h_after,
                                uint64_t *h_skipped, float *h_ms, int32_t *h_bad_view, uint64_t *h_num_points,
                                spz_amd_densify_round *h_rounds, int rounds_capacity, int *h_num_rounds,
                                uint32_t *h_origin) {
  const RefineRequest rq = {d_stream_a, size_a, hdr_a, d_stream_b, size_b, hdr_b, views, num_views, options, densify, device};
  return refine_open(rq, RefineOutputs{ctx, h_out_bytes, h_history, h_before, h_after, h_skipped, h_ms, h_bad_view,
                                       h_num_points, h_rounds, rounds_capacity, h_num_rounds, h_origin});
}

int spz_amd_refine_images_open(const uint8_t *d_stream_a, size_t size_a, const spz_amd_header *hdr_a,
                               const spz_amd_render_params *views, int num_views, const float *const *d_targets,
                               int channels, const float *const *d_weights, const spz_amd_refine_options *options,
                               const spz_amd_photo_options *photo, const spz_amd_densify_options *densify, int device,
                               void **ctx, uint64_t *h_out_bytes, double *h_history, spz_amd_image_metrics *h_before,
                               spz_amd_image_metrics *h_after, uint64_t *h_skipped, float *h_ms, int32_t *h_bad_view,
                               uint64_t *h_num_points, spz_amd_densify_round *h_rounds, int rounds_capacity,
                               int *h_num_rounds, uint32_t *h_origin, double *h_exposures) {
  const RefineRequest rq = {d_stream_a, size_a, hdr_a, nullptr, 0, nullptr, views, num_views, options, densify, device,
                            true, photo, d_targets, channels, d_weights};
  return refine_open(rq, RefineOutputs{ctx, h_out_bytes, h_history, h_before, h_after, h_skipped, h_ms, h_bad_view,
                                       h_num_points, h_rounds, rounds_capacity, h_num_rounds, h_origin, h_exposures});
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
  const RefineRequest rq = {d_stream_a, size_a, hdr_a, nullptr, 0, nullptr, views, num_views, options, densify, device,
                            true, photo, d_targets, channels, d_weights, true, depth, d_depth_targets};
  return refine_open(rq, RefineOutputs{ctx, h_out_bytes, h_history, h_before, h_after, h_skipped, h_ms, h_bad_view,
                                       h_num_points, h_rounds, rounds_capacity, h_num_rounds, h_origin, h_exposures,
                                       h_depth_history, h_depth_error});
}

int spz_amd_refine_images_host_open(const uint8_t *d_stream_a, size_t size_a, const spz_amd_header *hdr_a,
                                    const spz_amd_render_params *views, int num_views, const float *const *h_targets,
                                    int channels, const float *const *h_weights, const spz_amd_refine_options *options,
                                    const spz_amd_photo_options *photo, const spz_amd_densify_options *densify,
                                    int device, void **ctx, uint64_t *h_out_bytes, double *h_history,
                                    spz_amd_image_metrics *h_before, spz_amd_image_metrics *h_after, uint64_t *h_skipped,
                                    float *h_ms, int32_t *h_bad_view, uint64_t *h_num_points,
                                    spz_amd_densify_round *h_rounds, int rounds_capacity, int *h_num_rounds,
                                    uint32_t *h_origin, double *h_exposures) {
  const RefineRequest rq = {d_stream_a, size_a, hdr_a, nullptr, 0, nullptr, views, num_views, options, densify, device,
                            true, photo, h_targets, channels, h_weights};
  return refine_host_open(rq, RefineOutputs{ctx, h_out_bytes, h_history, h_before, h_after, h_skipped, h_ms, h_bad_view,
                                            h_num_points, h_rounds, rounds_capacity, h_num_rounds, h_origin, h_exposures});
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
  const RefineRequest rq = {d_stream_a, size_a, hdr_a, nullptr, 0, nullptr, views, num_views, options, densify, device,
                            true, photo, h_targets, channels, h_weights, true, depth, h_depth_targets};
  return refine_host_open(rq, RefineOutputs{ctx, h_out_bytes, h_history, h_before, h_after, h_skipped, h_ms, h_bad_view,
                                            h_num_points, h_rounds, rounds_capacity, h_num_rounds, h_origin, h_exposures,
                                            h_depth_history, h_depth_error});
}

int spz_amd_refine_fetch(void *ctx, uint8_t *h_out) { return packed_result_fetch(ctx, h_out); }

const uint8_t *spz_amd_refine_device_data(void *ctx) { return packed_result_device_data(ctx); }

void spz_amd_refine_close(void *ctx) { packed_result_close(ctx); }

}  // extern "C"

