// spz_densify.hip — 3DGS's adaptive density control over a float cloud and its Adam moments (DESIGN §8 "Densify"; the
// contract is in include/spz_amd.h): the gradient statistic, the decision, and the compaction that rewrites the cloud
// and both moments at a new count.  Every kernel streams over wave64 with one thread per Gaussian, row or float; there
// are no float atomics, and integer counts go through one vector atomic per workgroup that has any.
//
//   spz_densify_accumulate_kernel  one thread per Gaussian: 9 + 12 floats in, accum and denom updated.
//   plan                           classify (action, the sort key g or NaN, the culled count); the stable descending
//                                  argsort of the keys, which ranks the candidates in front of everything else; grant
//                                  (rank < budget keeps its action, else keep); the output counts summed per workgroup,
//                                  one workgroup scanning those sums (each thread a run of them, as the filter's
//                                  compaction does), then every workgroup scanning its own 256 and writing its rows of
//                                  the parent and child lists.
//   spz_densify_apply_kernel       one launch for the 18 arrays: a workgroup belongs to one of the six kinds (a table of
//                                  first workgroups in the kernel arguments, as the Adam step has); a lane takes one
//                                  output float of the parameters and both moments, the parent looked up once; rotations
//                                  go as 16-byte rows and positions as rows, because a split child's position needs the
//                                  whole parent.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "spz_amd.h"
#include "spz_block_ops.hpp"
#include "spz_common.hpp"
#include "spz_densify_internal.hpp"

#pragma clang fp contract(off)

namespace spz_amd_detail {
namespace {

constexpr uint32_t kDnBlock = kOpsBlock;  // 256: block_sum is written for it
constexpr uint32_t kDnScanBlock = 1024;

__device__ __forceinline__ bool finite_bits(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ uint32_t outputs_of(uint32_t action) { return action == 3u ? 0u : (action == 0u ? 1u : 2u); }

struct PlanParams {
  const float *accum;
  const uint32_t *denom;
  const float *scales, *alphas;
  float *key;
  const uint32_t *order;
  unsigned long long *tile_counts;
  uint8_t *action;
  uint32_t *parent;
  uint8_t *child;
  unsigned long long *counts;  // n', cloned, split, culled, refused
  uint32_t n;
  uint32_t use_max_scale;
  float grad_threshold, log_dense, alpha_min, log_max_scale;
  unsigned long long max_points, list_capacity;
};

// One kind of array of the apply launch: `units` threads from workgroup first_block on.
struct ApplySegment {
  const float *sp, *sm, *sv;
  float *dp, *dm, *dv;
  unsigned long long units;
  uint32_t width;  // floats per point
  uint32_t kind;   // 0 positions (a row per thread), 1 scales, 2 rotations (a row per thread), 3 the rest
  uint32_t first_block;
  uint32_t pad;
};

struct ApplyLaunch {
  ApplySegment seg[6];
  uint32_t n_seg;
  uint32_t n_src;
  const uint32_t *parent;
  const uint8_t *child;
  const float *scales, *rotations;  // the source parameters a split child's position reads
  unsigned long long key0;          // sm(seed ^ round)
  float log16;                      // (float)log(1.6)
};

__host__ __device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
  unsigned long long z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

}  // namespace

__global__ __launch_bounds__(kDnBlock) void spz_densify_accumulate_kernel(const spz_amd_render_record *__restrict__ rec,
                                                                          const float *__restrict__ rg, uint32_t n,
                                                                          float half_w, float half_h,
                                                                          float *__restrict__ accum,
                                                                          uint32_t *__restrict__ denom) {
  const unsigned long long i = (unsigned long long)blockIdx.x * kDnBlock + threadIdx.x;
  if (i >= n) return;
  if (!finite_bits(rec[i].depth)) return;
  const float a = rg[i * 9u] * half_w, b = rg[i * 9u + 1u] * half_h;
  const float s = a * a + b * b;
  const float norm = sqrtf(s);
  if (finite_bits(norm)) accum[i] = accum[i] + norm;
  denom[i] = denom[i] + 1u;
}

__global__ __launch_bounds__(kDnBlock) void spz_densify_classify_kernel(const PlanParams p) {
  __shared__ unsigned long long s[kDnBlock];
  const unsigned long long i = (unsigned long long)blockIdx.x * kDnBlock + threadIdx.x;
  unsigned long long culled = 0;
  if (i < p.n) {
    const float ms = fmaxf(fmaxf(p.scales[i * 3u], p.scales[i * 3u + 1u]), p.scales[i * 3u + 2u]);
    const float alpha = p.alphas[i];
    const bool cull = (alpha < p.alpha_min) || (p.use_max_scale != 0u && ms > p.log_max_scale);
    const uint32_t d = p.denom[i];
    float g = d > 0u ? p.accum[i] / (float)d : 0.0f;
    g = g != g ? 0.0f : g;
    const bool cand = !cull && g >= p.grad_threshold;
    p.action[i] = (uint8_t)(cull ? 3u : (cand ? (ms > p.log_dense ? 2u : 1u) : 0u));
    p.key[i] = cand ? g : __uint_as_float(0x7fc00000u);  // NaN sorts behind every candidate
    culled = cull ? 1ull : 0ull;
  }
  const unsigned long long t = block_sum(culled, s);
  if (threadIdx.x == 0 && t) atomicAdd(p.counts + 3, t);
}

// Thread r owns the Gaussian of rank r: the candidates are ranks 0 .. candidates - 1 in descending g.
__global__ __launch_bounds__(kDnBlock) void spz_densify_grant_kernel(const PlanParams p) {
  __shared__ unsigned long long s[kDnBlock];
  const unsigned long long r = (unsigned long long)blockIdx.x * kDnBlock + threadIdx.x;
  unsigned long long packed = 0;  // cloned | split << 16 | refused << 32 (each at most 256 per workgroup)
  if (r < p.n) {
    const unsigned long long left = (unsigned long long)p.n - p.counts[3];
    const unsigned long long budget = p.max_points > left ? p.max_points - left : 0ull;
    uint32_t i = p.order[r];
    i = i < p.n ? i : p.n - 1u;
    const uint32_t a = p.action[i];
    if (a == 1u || a == 2u) {
      if (r < budget) {
        packed = a == 1u ? 1ull : (1ull << 16);
      } else {
        p.action[i] = 0;
        packed = 1ull << 32;
      }
    }
  }
  const unsigned long long t = block_sum(packed, s);
  if (threadIdx.x == 0 && t) {
    if (t & 0xffffull) atomicAdd(p.counts + 1, t & 0xffffull);
    if ((t >> 16) & 0xffffull) atomicAdd(p.counts + 2, (t >> 16) & 0xffffull);
    if (t >> 32) atomicAdd(p.counts + 4, t >> 32);
  }
}

__global__ __launch_bounds__(kDnBlock) void spz_densify_tile_count_kernel(const PlanParams p) {
  __shared__ unsigned long long s[kDnBlock];
  const unsigned long long i = (unsigned long long)blockIdx.x * kDnBlock + threadIdx.x;
  const unsigned long long c = i < p.n ? outputs_of(p.action[i]) : 0u;
  const unsigned long long t = block_sum(c, s);
  if (threadIdx.x == 0) p.tile_counts[blockIdx.x] = t;
}

// counts[0 .. tiles) -> exclusive offsets in place; *total = their sum.  One workgroup; thread t owns a contiguous run
// of ceil(tiles / 1024) counts (the second level of the scan begins above 1024 tiles = 262 144 Gaussians).
__global__ __launch_bounds__(kDnScanBlock) void spz_densify_tile_scan_kernel(unsigned long long *counts, uint32_t tiles,
                                                                             unsigned long long *total) {
  __shared__ unsigned long long part[kDnScanBlock];
  const unsigned long long sum = block_scan_owned_runs<unsigned long long, kDnScanBlock>(
      tiles, part, [&](uint32_t k) { return counts[k]; },
      [&](uint32_t k, unsigned long long before) { counts[k] = before; });
  if (threadIdx.x == 0) *total = sum;
}

__global__ __launch_bounds__(kDnBlock) void spz_densify_emit_kernel(const PlanParams p) {
  __shared__ unsigned long long s[kDnBlock];
  const unsigned long long i = (unsigned long long)blockIdx.x * kDnBlock + threadIdx.x;
  const uint32_t a = i < p.n ? p.action[i] : 3u;
  const uint32_t c = outputs_of(a);
  const unsigned long long at = p.tile_counts[blockIdx.x] + block_exclusive_scan<unsigned long long>(c, s);
  if (c >= 1u && at < p.list_capacity) {
    p.parent[at] = (uint32_t)i;
    p.child[at] = (uint8_t)(a == 2u ? 2u : 0u);
  }
  if (c == 2u && at + 1u < p.list_capacity) {
    p.parent[at + 1u] = (uint32_t)i;
    p.child[at + 1u] = (uint8_t)(a == 2u ? 3u : 1u);
  }
}

namespace {

// The position of split child `ch` (2 or 3) of parent i: p + R(q / |q|) (exp(ls) (.) z), in f64; the parent's where
// any axis does not come out finite.
__device__ __forceinline__ void split_position(const ApplyLaunch &a, const ApplySegment &sg, uint32_t i, uint32_t ch,
                                               float out[3]) {
  const unsigned long long i3 = (unsigned long long)i * 3u, i4 = (unsigned long long)i * 4u;
  const float p0 = sg.sp[i3], p1 = sg.sp[i3 + 1u], p2 = sg.sp[i3 + 2u];
  double qx = a.rotations[i4], qy = a.rotations[i4 + 1u], qz = a.rotations[i4 + 2u], qw = a.rotations[i4 + 3u];
  const double qn = sqrt(qx * qx + qy * qy + qz * qz + qw * qw);
  qx /= qn;
  qy /= qn;
  qz /= qn;
  qw /= qn;
  const double Rq[9] = {1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy),
                        2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx),
                        2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)};
  const unsigned long long key = splitmix64(a.key0 + (unsigned long long)i);
  double sz[3];
#pragma unroll
  for (uint32_t j = 0; j < 3; ++j) {
    const unsigned long long ra = splitmix64(key + 2ull * j + 1ull), rb = splitmix64(key + 2ull * j + 2ull);
    const double u1 = (double)((ra >> 11) + 1ull) * 0x1p-53, u2 = (double)(rb >> 11) * 0x1p-53;
    const double r = sqrt(-2.0 * log(u1));
    const double ang = 6.283185307179586 * u2;
    const double z = ch == 2u ? r * cos(ang) : r * sin(ang);
    sz[j] = exp((double)a.scales[i3 + j]) * z;
  }
  const float c0 = (float)((double)p0 + (Rq[0] * sz[0] + Rq[1] * sz[1] + Rq[2] * sz[2]));
  const float c1 = (float)((double)p1 + (Rq[3] * sz[0] + Rq[4] * sz[1] + Rq[5] * sz[2]));
  const float c2 = (float)((double)p2 + (Rq[6] * sz[0] + Rq[7] * sz[1] + Rq[8] * sz[2]));
  const bool ok = finite_bits(c0) && finite_bits(c1) && finite_bits(c2);
  out[0] = ok ? c0 : p0;
  out[1] = ok ? c1 : p1;
  out[2] = ok ? c2 : p2;
}

}  // namespace

__global__ __launch_bounds__(kDnBlock) void spz_densify_apply_kernel(const ApplyLaunch a) {
  uint32_t k = 0;
  while (k + 1 < a.n_seg && blockIdx.x >= a.seg[k + 1].first_block) ++k;  // uniform: a workgroup has one kind
  const ApplySegment &sg = a.seg[k];
  const unsigned long long u = (unsigned long long)(blockIdx.x - sg.first_block) * kDnBlock + threadIdx.x;
  if (u >= sg.units) return;
  if (sg.kind == 0u || sg.kind == 2u) {  // a row per thread
    uint32_t i = a.parent[u];
    i = i < a.n_src ? i : a.n_src - 1u;
    const uint32_t ch = a.child[u];
    if (sg.kind == 2u) {
      const unsigned long long s4 = (unsigned long long)i * 4u, d4 = u * 4u;
      const F32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
      *reinterpret_cast<F32x4 *>(sg.dp + d4) = *reinterpret_cast<const F32x4 *>(sg.sp + s4);
      *reinterpret_cast<F32x4 *>(sg.dm + d4) = ch == 0u ? *reinterpret_cast<const F32x4 *>(sg.sm + s4) : zero;
      *reinterpret_cast<F32x4 *>(sg.dv + d4) = ch == 0u ? *reinterpret_cast<const F32x4 *>(sg.sv + s4) : zero;
    } else {
      const unsigned long long s3 = (unsigned long long)i * 3u, d3 = u * 3u;
      float pos[3];
      if (ch >= 2u) {
        split_position(a, sg, i, ch, pos);
      } else {
        pos[0] = sg.sp[s3];
        pos[1] = sg.sp[s3 + 1u];
        pos[2] = sg.sp[s3 + 2u];
      }
#pragma unroll
      for (uint32_t c = 0; c < 3; ++c) {
        sg.dp[d3 + c] = pos[c];
        sg.dm[d3 + c] = ch == 0u ? sg.sm[s3 + c] : 0.0f;
        sg.dv[d3 + c] = ch == 0u ? sg.sv[s3 + c] : 0.0f;
      }
    }
    return;
  }
  const unsigned long long row = u / sg.width;
  const uint32_t col = (uint32_t)(u - row * sg.width);
  uint32_t i = a.parent[row];
  i = i < a.n_src ? i : a.n_src - 1u;
  const uint32_t ch = a.child[row];
  const unsigned long long s = (unsigned long long)i * sg.width + col;
  float v = sg.sp[s];
  if (sg.kind == 1u && ch >= 2u) v = v - a.log16;
  sg.dp[u] = v;
  sg.dm[u] = ch == 0u ? sg.sm[s] : 0.0f;
  sg.dv[u] = ch == 0u ? sg.sv[s] : 0.0f;
}

__global__ __launch_bounds__(kDnBlock) void spz_densify_reset_kernel(float *__restrict__ alphas, float *__restrict__ m,
                                                                     float *__restrict__ v, uint32_t n, float ceiling) {
  const unsigned long long i = (unsigned long long)blockIdx.x * kDnBlock + threadIdx.x;
  if (i >= n) return;
  const float a = alphas[i];
  if (a > ceiling) alphas[i] = ceiling;  // NaN: left alone
  if (m != nullptr) m[i] = 0.0f;
  if (v != nullptr) v[i] = 0.0f;
}

__global__ __launch_bounds__(kDnBlock) void spz_densify_gather_u32_kernel(const uint32_t *__restrict__ src,
                                                                          const uint32_t *__restrict__ parent,
                                                                          uint32_t n_src, uint32_t n_new,
                                                                          uint32_t *__restrict__ dst) {
  const unsigned long long k = (unsigned long long)blockIdx.x * kDnBlock + threadIdx.x;
  if (k >= n_new) return;
  uint32_t i = parent[k];
  i = i < n_src ? i : n_src - 1u;
  dst[k] = src == nullptr ? i : src[i];
}

int densify_gather_u32(const uint32_t *d_src, const uint32_t *d_parent, uint64_t n_src, uint64_t n_new, uint32_t *d_dst,
                       hipStream_t st) {
  if (n_new == 0) return SPZ_AMD_OK;
  if (d_parent == nullptr || d_dst == nullptr || n_src == 0 || n_src > kMaxEntries || n_new > kMaxEntries) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  hipLaunchKernelGGL(spz_densify_gather_u32_kernel, dim3((unsigned)((n_new + kDnBlock - 1) / kDnBlock)), dim3(kDnBlock),
                     0, st, d_src, d_parent, (uint32_t)n_src, (uint32_t)n_new, d_dst);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

namespace {

bool aligned_to(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0; }

struct PlanLayout {
  uint64_t tiles, key, order, tile_counts, sort, bytes;
};

PlanLayout plan_layout(uint64_t n) {
  PlanLayout w = {};
  w.tiles = (n + kDnBlock - 1) / kDnBlock;
  WorkspaceOffsets o;
  w.key = o.put(n * 4u);
  w.order = o.put(n * 4u);
  w.tile_counts = o.put(w.tiles * 8u);
  w.sort = o.put(spz_amd_sort_workspace_bytes(n));
  w.bytes = o.bytes();
  return w;
}

uint64_t plan_list_bound(uint64_t n, uint64_t max_points) {
  const uint64_t grown = max_points > n ? max_points : n;
  return 2u * n < grown ? 2u * n : grown;
}

int plan_check(const float *d_accum, const uint32_t *d_denom, const float *d_scales, const float *d_alphas, uint64_t n,
               const spz_amd_densify_limits *lim, uint64_t max_points, uint64_t list_capacity, const uint8_t *d_action,
               const uint32_t *d_parent, const uint8_t *d_child, const uint64_t *d_counts, const void *d_workspace) {
  if (lim == nullptr || d_counts == nullptr || !aligned_to(d_counts, 8)) return SPZ_AMD_ERR_INVALID_ARG;
  if (n > kMaxEntries || max_points > kMaxEntries) return SPZ_AMD_ERR_TOO_MANY_POINTS;
  if (std::isnan(lim->grad_threshold) || std::isnan(lim->log_dense) || std::isnan(lim->alpha_min) ||
      (lim->use_max_scale && std::isnan(lim->log_max_scale))) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  if (n == 0) return SPZ_AMD_OK;
  if (d_accum == nullptr || d_denom == nullptr || d_scales == nullptr || d_alphas == nullptr || d_action == nullptr ||
      d_parent == nullptr || d_child == nullptr || d_workspace == nullptr) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  if (!aligned_to(d_accum, 4) || !aligned_to(d_denom, 4) || !aligned_to(d_scales, 4) || !aligned_to(d_alphas, 4) ||
      !aligned_to(d_parent, 4)) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  if (list_capacity < plan_list_bound(n, max_points)) return SPZ_AMD_ERR_CAPACITY;
  return SPZ_AMD_OK;
}

int plan_enqueue(const float *d_accum, const uint32_t *d_denom, const float *d_scales, const float *d_alphas, uint64_t n,
                 const spz_amd_densify_limits *lim, uint64_t max_points, uint64_t list_capacity, uint8_t *d_action,
                 uint32_t *d_parent, uint8_t *d_child, uint64_t *d_counts, void *d_workspace, hipStream_t st) {
  int device = 0;
  int rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  SPZ_HIP_TRY(hipMemsetAsync(d_counts, 0, 5u * sizeof(uint64_t), st));
  if (n == 0) return SPZ_AMD_OK;
  const PlanLayout w = plan_layout(n);
  uint8_t *ws = align_ws(d_workspace);
  PlanParams p = {};
  p.accum = d_accum;
  p.denom = d_denom;
  p.scales = d_scales;
  p.alphas = d_alphas;
  p.key = reinterpret_cast<float *>(ws + w.key);
  p.order = reinterpret_cast<uint32_t *>(ws + w.order);
  p.tile_counts = reinterpret_cast<unsigned long long *>(ws + w.tile_counts);
  p.action = d_action;
  p.parent = d_parent;
  p.child = d_child;
  p.counts = reinterpret_cast<unsigned long long *>(d_counts);
  p.n = (uint32_t)n;
  p.use_max_scale = lim->use_max_scale ? 1u : 0u;
  p.grad_threshold = lim->grad_threshold;
  p.log_dense = lim->log_dense;
  p.alpha_min = lim->alpha_min;
  p.log_max_scale = lim->log_max_scale;
  p.max_points = max_points;
  p.list_capacity = list_capacity;
  const dim3 grid((unsigned)w.tiles), block(kDnBlock);
  hipLaunchKernelGGL(spz_densify_classify_kernel, grid, block, 0, st, p);
  SPZ_HIP_TRY(hipGetLastError());
  rc = spz_amd_argsort_f32_device(p.key, n, 1, reinterpret_cast<uint32_t *>(ws + w.order), ws + w.sort, st);
  if (rc != SPZ_AMD_OK) return rc;
  hipLaunchKernelGGL(spz_densify_grant_kernel, grid, block, 0, st, p);
  SPZ_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(spz_densify_tile_count_kernel, grid, block, 0, st, p);
  SPZ_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(spz_densify_tile_scan_kernel, dim3(1), dim3(kDnScanBlock), 0, st, p.tile_counts, (uint32_t)w.tiles,
                     p.counts);
  SPZ_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(spz_densify_emit_kernel, grid, block, 0, st, p);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

float *field(const spz_amd_cloud_grads *c, int k) {
  float *const f[6] = {c->positions, c->scales, c->rotations, c->alphas, c->colors, c->sh};
  return f[k];
}

bool finite_d(double x) { return std::isfinite(x); }

}  // namespace
}  // namespace spz_amd_detail

using namespace spz_amd_detail;

extern "C" {

int spz_amd_densify_default_options(spz_amd_densify_options *o) {
  if (o == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  std::memset(o, 0, sizeof(*o));
  o->interval = 0;  // off; 3DGS: 100
  o->from_iter = 500;
  o->until_iter = 15000;
  o->opacity_reset_interval = 0;  // off; 3DGS: 3000
  o->grad_threshold = 2e-4;
  o->percent_dense = 0.01;
  o->extent = 0.0;
  o->min_opacity = 0.005;
  o->max_scale = 0.0;
  o->max_points = 0;
  o->seed = 0;
  return SPZ_AMD_OK;
}

int spz_amd_densify_check(const spz_amd_densify_options *o) {
  if (o == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  if (o->interval < 0 || o->from_iter < 0 || o->until_iter < 0 || o->opacity_reset_interval < 0) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  if (o->until_iter < o->from_iter) return SPZ_AMD_ERR_INVALID_ARG;
  for (double x : {o->grad_threshold, o->percent_dense, o->extent, o->min_opacity, o->max_scale}) {
    if (!finite_d(x) || x < 0.0) return SPZ_AMD_ERR_INVALID_ARG;
  }
  if (!(o->min_opacity > 0.0) || !(o->min_opacity < 1.0)) return SPZ_AMD_ERR_INVALID_ARG;
  if (o->interval > 0 && !(o->percent_dense > 0.0)) return SPZ_AMD_ERR_INVALID_ARG;
  return SPZ_AMD_OK;
}

int spz_amd_densify_thresholds(const spz_amd_densify_options *o, const spz_amd_render_params *views, int num_views,
                               spz_amd_densify_limits *out) {
  if (out == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  int rc = spz_amd_densify_check(o);
  if (rc != SPZ_AMD_OK) return rc;
  if (!(o->percent_dense > 0.0)) return SPZ_AMD_ERR_INVALID_ARG;
  double extent = o->extent;
  if (extent == 0.0) {
    if (views == nullptr || num_views < 1) return SPZ_AMD_ERR_INVALID_ARG;
    double mean[3] = {0.0, 0.0, 0.0};
    auto centre = [&](int v, double c[3]) {
      const float *m = views[v].world_to_camera;
      for (int k = 0; k < 3; ++k) {
        c[k] = -((double)m[k] * (double)m[3] + (double)m[4 + k] * (double)m[7] + (double)m[8 + k] * (double)m[11]);
      }
    };
    for (int v = 0; v < num_views; ++v) {
      double c[3];
      centre(v, c);
      for (int k = 0; k < 3; ++k) mean[k] += c[k];
    }
    for (int k = 0; k < 3; ++k) mean[k] /= (double)num_views;
    double far = 0.0;
    for (int v = 0; v < num_views; ++v) {
      double c[3];
      centre(v, c);
      const double dx = c[0] - mean[0], dy = c[1] - mean[1], dz = c[2] - mean[2];
      const double d = std::sqrt(dx * dx + dy * dy + dz * dz);
      far = d > far ? d : far;
    }
    extent = 1.1 * far;
    if (!(extent > 0.0) || !finite_d(extent)) return SPZ_AMD_ERR_INVALID_ARG;
  }
  std::memset(out, 0, sizeof(*out));
  out->extent = extent;
  out->grad_threshold = (float)o->grad_threshold;
  out->log_dense = (float)std::log(o->percent_dense * extent);
  out->alpha_min = (float)std::log(o->min_opacity / (1.0 - o->min_opacity));
  out->use_max_scale = o->max_scale > 0.0 ? 1 : 0;
  out->log_max_scale = o->max_scale > 0.0 ? (float)std::log(o->max_scale) : 0.0f;
  return SPZ_AMD_OK;
}

int spz_amd_densify_accumulate_device(const spz_amd_render_record *d_records, const float *d_record_grads, uint64_t n,
                                      uint32_t width, uint32_t height, float *d_accum, uint32_t *d_denom,
                                      void *hip_stream) {
  if (width < 1 || width > 16384 || height < 1 || height > 16384) return SPZ_AMD_ERR_INVALID_ARG;
  if (n > kMaxEntries) return SPZ_AMD_ERR_TOO_MANY_POINTS;
  if (n == 0) return SPZ_AMD_OK;
  if (d_records == nullptr || d_record_grads == nullptr || d_accum == nullptr || d_denom == nullptr ||
      !aligned_to(d_records, 4) || !aligned_to(d_record_grads, 4) || !aligned_to(d_accum, 4) || !aligned_to(d_denom, 4)) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  int device = 0;
  int rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  hipLaunchKernelGGL(spz_densify_accumulate_kernel, dim3((unsigned)((n + kDnBlock - 1) / kDnBlock)), dim3(kDnBlock), 0,
                     static_cast<hipStream_t>(hip_stream), d_records, d_record_grads, (uint32_t)n, 0.5f * (float)width,
                     0.5f * (float)height, d_accum, d_denom);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

uint64_t spz_amd_densify_plan_workspace_bytes(uint64_t n) { return n > kMaxEntries ? 0u : plan_layout(n).bytes; }

int spz_amd_densify_plan_device(const float *d_accum, const uint32_t *d_denom, const float *d_scales,
                                const float *d_alphas, uint64_t n, const spz_amd_densify_limits *limits,
                                uint64_t max_points, uint64_t list_capacity, uint8_t *d_action, uint32_t *d_parent,
                                uint8_t *d_child, uint64_t *d_counts, void *d_workspace, void *hip_stream) {
  const int rc = plan_check(d_accum, d_denom, d_scales, d_alphas, n, limits, max_points, list_capacity, d_action,
                            d_parent, d_child, d_counts, d_workspace);
  if (rc != SPZ_AMD_OK) return rc;
  return plan_enqueue(d_accum, d_denom, d_scales, d_alphas, n, limits, max_points, list_capacity, d_action, d_parent,
                      d_child, d_counts, d_workspace, static_cast<hipStream_t>(hip_stream));
}

int spz_amd_densify_plan_host(const float *d_accum, const uint32_t *d_denom, const float *d_scales, const float *d_alphas,
                              uint64_t n, const spz_amd_densify_limits *limits, uint64_t max_points,
                              uint64_t list_capacity, uint8_t *d_action, uint32_t *d_parent, uint8_t *d_child,
                              uint64_t *d_counts, void *d_workspace, uint64_t *h_counts, void *hip_stream) {
  if (h_counts == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  int rc = plan_check(d_accum, d_denom, d_scales, d_alphas, n, limits, max_points, list_capacity, d_action, d_parent,
                      d_child, d_counts, d_workspace);
  if (rc != SPZ_AMD_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  rc = plan_enqueue(d_accum, d_denom, d_scales, d_alphas, n, limits, max_points, list_capacity, d_action, d_parent,
                    d_child, d_counts, d_workspace, st);
  if (rc != SPZ_AMD_OK) return rc;
  SPZ_HIP_TRY(hipMemcpyAsync(h_counts, d_counts, 5u * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  SPZ_HIP_TRY(hipStreamSynchronize(st));
  return SPZ_AMD_OK;
}

int spz_amd_densify_apply_device(const spz_amd_cloud_grads *d_src_params, const spz_amd_cloud_grads *d_src_m,
                                 const spz_amd_cloud_grads *d_src_v, const spz_amd_cloud_grads *d_dst_params,
                                 const spz_amd_cloud_grads *d_dst_m, const spz_amd_cloud_grads *d_dst_v,
                                 const uint32_t *d_parent, const uint8_t *d_child, uint64_t n_src, uint64_t n_new,
                                 uint64_t dst_capacity, int sh_degree, uint64_t seed, uint32_t round, void *hip_stream) {
  if (d_src_params == nullptr || d_src_m == nullptr || d_src_v == nullptr || d_dst_params == nullptr ||
      d_dst_m == nullptr || d_dst_v == nullptr) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  if (sh_degree < 0 || sh_degree > 3) return SPZ_AMD_ERR_SH_DEGREE;
  if (n_src > kMaxEntries || n_new > kMaxEntries || dst_capacity > kMaxEntries) return SPZ_AMD_ERR_TOO_MANY_POINTS;
  if (n_new > dst_capacity) return SPZ_AMD_ERR_CAPACITY;
  if (n_new == 0) return SPZ_AMD_OK;
  if (n_src == 0 || d_parent == nullptr || d_child == nullptr || !aligned_to(d_parent, 4)) return SPZ_AMD_ERR_INVALID_ARG;
  const uint32_t width[6] = {3u, 3u, 4u, 1u, 3u, 3u * (uint32_t)sh_dim_for_degree(sh_degree)};
  const uint32_t kind[6] = {0u, 1u, 2u, 3u, 3u, 3u};
  ApplyLaunch a = {};
  uint64_t blocks = 0;
  for (int k : {5, 0, 1, 2, 4, 3}) {  // the largest first, so that the grid's tail is made of the small ones
    if (width[k] == 0) continue;
    ApplySegment &sg = a.seg[a.n_seg++];
    sg.sp = field(d_src_params, k);
    sg.sm = field(d_src_m, k);
    sg.sv = field(d_src_v, k);
    sg.dp = field(d_dst_params, k);
    sg.dm = field(d_dst_m, k);
    sg.dv = field(d_dst_v, k);
    for (const float *f : {sg.sp, sg.sm, sg.sv, (const float *)sg.dp, (const float *)sg.dm, (const float *)sg.dv}) {
      if (f == nullptr || !aligned_to(f, 4)) return SPZ_AMD_ERR_INVALID_ARG;
    }
    sg.width = width[k];
    sg.kind = kind[k];
    sg.units = (kind[k] == 0u || kind[k] == 2u) ? n_new : n_new * width[k];
    sg.first_block = (uint32_t)blocks;
    blocks += (sg.units + kDnBlock - 1) / kDnBlock;
  }
  if (blocks > 0x7fffffffull) return SPZ_AMD_ERR_TOO_MANY_POINTS;
  // segments must come in ascending first_block for the kernel's walk: they do, in the order they were added
  a.n_src = (uint32_t)n_src;
  a.parent = d_parent;
  a.child = d_child;
  a.scales = d_src_params->scales;
  a.rotations = d_src_params->rotations;
  a.key0 = splitmix64(seed ^ (uint64_t)round);
  a.log16 = (float)std::log(1.6);
  int device = 0;
  const int rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  hipLaunchKernelGGL(spz_densify_apply_kernel, dim3((unsigned)blocks), dim3(kDnBlock), 0,
                     static_cast<hipStream_t>(hip_stream), a);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

int spz_amd_densify_reset_opacity_device(float *d_alphas, float *d_alphas_m, float *d_alphas_v, uint64_t n,
                                         void *hip_stream) {
  if (n > kMaxEntries) return SPZ_AMD_ERR_TOO_MANY_POINTS;
  if (n == 0) return SPZ_AMD_OK;
  if (d_alphas == nullptr || !aligned_to(d_alphas, 4) || !aligned_to(d_alphas_m, 4) || !aligned_to(d_alphas_v, 4)) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  int device = 0;
  const int rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  hipLaunchKernelGGL(spz_densify_reset_kernel, dim3((unsigned)((n + kDnBlock - 1) / kDnBlock)), dim3(kDnBlock), 0,
                     static_cast<hipStream_t>(hip_stream), d_alphas, d_alphas_m, d_alphas_v, (uint32_t)n,
                     (float)std::log(0.01 / 0.99));
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

}  // extern "C"
