// spz_seed.hip — Gaussians from posed RGB-D views (DESIGN §8 "Seed"; the contract is in include/spz_amd.h "seed"): the
// valid depth samples of a view that the cloud built so far does not explain are lifted to Gaussians and appended.
//
//   spz_seed_select_kernel    one lane per lattice sample, 256 consecutive samples of the row-major lattice per block:
//                             depth, weight and colour tests first, then (when covering) the two rendered maps.  A flag
//                             byte per sample (bit 0 valid, bit 1 selected) and the block's two counts.  A pure
//                             streaming read: at stride 1 every plane is read coalesced, once.
//   spz_seed_offsets_kernel   one block: the exclusive scan of the blocks' selected counts (spz_block_ops.hpp's owned-run
//                             scan), the three totals (valid, appended, refused) into d_counts.
//   spz_seed_emit_kernel      the same blocks again: a selected sample's rank is its block's offset plus the block scan
//                             of the flags; rank < room writes the Gaussian at n + rank, the rest are the refused.  The
//                             block's ranks are consecutive, so its sh rows are zeroed by all lanes together.  No
//                             atomics: the scan fixes the order, and a run repeats its bytes.
//
// The host form (spz_amd_seed_open) keeps the float cloud in device memory, renders it for the cover test with the
// rasteriser's own prepare and depth blend (spz_view_pass.hpp), and encodes the appended points alone.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>

#include "spz_amd.h"
#include "spz_block_ops.hpp"
#include "spz_common.hpp"
#include "spz_render_internal.hpp"
#include "spz_view_pass.hpp"

#pragma clang fp contract(off)

namespace spz_amd_detail {
namespace {

constexpr uint32_t kSeedBlock = kOpsBlock;
constexpr uint32_t kSeedValid = 1u, kSeedSelected = 2u;

// The sample lattice of a view: lw x lh samples, sample (i, j) at pixel (stride i + stride / 2, stride j + stride / 2).
struct SeedLattice {
  uint32_t width, height, stride, lw, lh;
  uint32_t samples;  // lw lh <= 2^28
  uint32_t blocks;
};

inline SeedLattice seed_lattice(uint32_t width, uint32_t height, uint32_t stride) {
  SeedLattice l = {width, height, stride, 0u, 0u, 0u, 0u};
  const uint32_t half = stride / 2u;
  l.lw = width > half ? (width - half + stride - 1u) / stride : 0u;
  l.lh = height > half ? (height - half + stride - 1u) / stride : 0u;
  l.samples = l.lw * l.lh;
  l.blocks = (l.samples + kSeedBlock - 1u) / kSeedBlock;
  return l;
}

struct SeedLayout {
  uint64_t flags, sel, valid, offsets, bytes;
};

inline SeedLayout seed_layout(const SeedLattice &l) {
  SeedLayout s;
  WorkspaceOffsets o;
  s.flags = o.put(l.samples);
  s.sel = o.put(4ull * l.blocks);
  s.valid = o.put(4ull * l.blocks);
  s.offsets = o.put(8ull * l.blocks);
  s.bytes = o.bytes();
  return s;
}

// What the kernels read of the options and the view, widened once on the host.
struct SeedArgs {
  double R[9], t[3];
  double fx, fy, cx, cy;
  double scale_factor, tolerance;
  float near_plane, cover_alpha, alpha;
  uint32_t channels, sh3;  // image channels; sh floats per point
};

__device__ __forceinline__ bool finitef(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__global__ __launch_bounds__(kSeedBlock) void spz_seed_select_kernel(SeedLattice l, SeedArgs a,
                                                                     const float *__restrict__ image,
                                                                     const float *__restrict__ depth,
                                                                     const float *__restrict__ weights,
                                                                     const float *__restrict__ cover_image,
                                                                     const float *__restrict__ cover_depth,
                                                                     uint8_t *__restrict__ flags,
                                                                     uint32_t *__restrict__ block_sel,
                                                                     uint32_t *__restrict__ block_valid) {
  __shared__ unsigned long long s[kSeedBlock];
  const uint32_t sample = blockIdx.x * kSeedBlock + threadIdx.x;
  uint32_t flag = 0u;
  if (sample < l.samples) {
    const uint32_t j = sample / l.lw, i = sample - j * l.lw;
    const uint32_t u = l.stride * i + l.stride / 2u, v = l.stride * j + l.stride / 2u;
    const size_t pix = (size_t)v * l.width + u;
    const float d = depth[pix];
    bool ok = finitef(d) && d > a.near_plane;
    if (ok && weights != nullptr) ok = weights[pix] > 0.5f;
    if (ok) {
      const float *c = image + pix * a.channels;
      ok = finitef(c[0]) && finitef(c[1]) && finitef(c[2]);
    }
    if (ok) {
      flag = kSeedValid | kSeedSelected;
      if (cover_image != nullptr) {
        const float A = cover_image[pix * 4u + 3u];
        if (A >= a.cover_alpha) {
          const float e = cover_depth[pix * 2u] / A;
          const double diff = fabs((double)e - (double)d);
          if (diff <= a.tolerance * (double)d) flag = kSeedValid;
        }
      }
    }
    flags[sample] = (uint8_t)flag;
  }
  // both counts in one sum: each is at most 256
  const unsigned long long both = block_sum<unsigned long long>((flag & kSeedValid) | ((flag & kSeedSelected) << 15), s);
  if (threadIdx.x == 0u) {
    block_valid[blockIdx.x] = (uint32_t)(both & 0xffffu);
    block_sel[blockIdx.x] = (uint32_t)(both >> 16);
  }
}

// One block: the owned-run scan of the blocks' selected counts, whose total is the selected; each lane sums its run's
// valid counts on the storing walk.  d_counts: valid, appended = min(selected, room), refused = selected - appended.
__global__ __launch_bounds__(kSeedBlock) void spz_seed_offsets_kernel(const uint32_t *__restrict__ block_sel,
                                                                      const uint32_t *__restrict__ block_valid,
                                                                      uint32_t blocks, unsigned long long room,
                                                                      unsigned long long *__restrict__ offsets,
                                                                      unsigned long long *__restrict__ counts) {
  __shared__ unsigned long long s[kSeedBlock];
  unsigned long long valid = 0ull;
  const unsigned long long total = block_scan_owned_runs(
      blocks, s, [&](uint32_t b) { return (unsigned long long)block_sel[b]; },
      [&](uint32_t b, unsigned long long before) {
        offsets[b] = before;
        valid += block_valid[b];
      });
  valid = block_sum(valid, s);
  if (threadIdx.x == 0u) {
    const unsigned long long appended = total < room ? total : room;
    counts[0] = valid;
    counts[1] = appended;
    counts[2] = total - appended;
  }
}

__global__ __launch_bounds__(kSeedBlock) void spz_seed_emit_kernel(SeedLattice l, SeedArgs a,
                                                                   const float *__restrict__ image,
                                                                   const float *__restrict__ depth,
                                                                   const uint8_t *__restrict__ flags,
                                                                   const uint32_t *__restrict__ block_sel,
                                                                   const unsigned long long *__restrict__ offsets,
                                                                   unsigned long long n, unsigned long long room,
                                                                   float *__restrict__ positions, float *__restrict__ scales,
                                                                   float *__restrict__ rotations, float *__restrict__ alphas,
                                                                   float *__restrict__ colors, float *__restrict__ sh) {
  __shared__ unsigned long long s[kSeedBlock];
  const uint32_t count = block_sel[blockIdx.x];
  const unsigned long long first = offsets[blockIdx.x];
  if (count == 0u || first >= room) return;  // block-uniform
  const uint32_t sample = blockIdx.x * kSeedBlock + threadIdx.x;
  const bool selected = sample < l.samples && (flags[sample] & kSeedSelected) != 0u;
  const unsigned long long rank = first + block_exclusive_scan(selected ? 1ull : 0ull, s);
  if (a.sh3) {  // the block's rows n + first .. n + min(first + count, room), zeroed together
    const unsigned long long last = first + count < room ? first + count : room;
    float *row = sh + (n + first) * a.sh3;
    const unsigned long long floats = (last - first) * a.sh3;
    for (unsigned long long k = threadIdx.x; k < floats; k += kSeedBlock) row[k] = 0.0f;
  }
  if (!selected || rank >= room) return;
  const uint32_t j = sample / l.lw, i = sample - j * l.lw;
  const uint32_t u = l.stride * i + l.stride / 2u, v = l.stride * j + l.stride / 2u;
  const size_t pix = (size_t)v * l.width + u;
  const double z = (double)depth[pix];
  const double qx = (((double)u + 0.5 - a.cx) / a.fx) * z - a.t[0];
  const double qy = (((double)v + 0.5 - a.cy) / a.fy) * z - a.t[1];
  const double qz = z - a.t[2];
  const unsigned long long at = n + rank;
#pragma unroll
  for (uint32_t k = 0; k < 3u; ++k) {
    positions[at * 3u + k] = (float)((qx * a.R[k] + qy * a.R[3u + k]) + qz * a.R[6u + k]);
  }
  const float ls = (float)log((((a.scale_factor * (double)l.stride) * z) * 0.5) * (1.0 / a.fx + 1.0 / a.fy));
  const float *c = image + pix * a.channels;
#pragma unroll
  for (uint32_t k = 0; k < 3u; ++k) {
    scales[at * 3u + k] = ls;
    colors[at * 3u + k] = (float)(((double)c[k] - 0.5) / kC0);
  }
  F32x4 q = {0.0f, 0.0f, 0.0f, 1.0f};
  *reinterpret_cast<F32x4 *>(rotations + at * 4u) = q;
  alphas[at] = a.alpha;
}

SeedArgs seed_args(const spz_amd_render_params *p, const spz_amd_seed_options *o, int channels) {
  SeedArgs a = {};
  for (int r = 0; r < 3; ++r) {
    for (int k = 0; k < 3; ++k) a.R[r * 3 + k] = p->world_to_camera[r * 4 + k];
    a.t[r] = p->world_to_camera[r * 4 + 3];
  }
  a.fx = p->fx;
  a.fy = p->fy;
  a.cx = p->cx;
  a.cy = p->cy;
  a.scale_factor = o->scale_factor;
  a.tolerance = o->cover_tolerance;
  a.near_plane = p->near_plane;
  a.cover_alpha = o->cover_alpha;
  a.alpha = o->alpha;
  a.channels = (uint32_t)channels;
  a.sh3 = (uint32_t)sh_dim_for_degree(o->sh_degree) * 3u;
  return a;
}

}  // namespace
}  // namespace spz_amd_detail

using namespace spz_amd_detail;

extern "C" {

int spz_amd_seed_default_options(spz_amd_seed_options *options) {
  if (options == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  std::memset(options, 0, sizeof(*options));
  options->stride = 1u;
  options->scale_factor = 1.0f;
  options->alpha = 0.0f;
  options->cover_alpha = 0.5f;
  options->cover_tolerance = 0.05f;
  options->cover = 1;
  options->sh_degree = 0;
  return SPZ_AMD_OK;
}

int spz_amd_seed_check(const spz_amd_seed_options *o) {
  if (o == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  if (o->stride < 1u || o->stride > 64u) return SPZ_AMD_ERR_INVALID_ARG;
  if (!(o->scale_factor > 0.0f) || !std::isfinite(o->scale_factor)) return SPZ_AMD_ERR_INVALID_ARG;
  if (!std::isfinite(o->alpha)) return SPZ_AMD_ERR_INVALID_ARG;
  if (!(o->cover_alpha >= 0.0f) || !(o->cover_alpha <= 1.0f)) return SPZ_AMD_ERR_INVALID_ARG;
  if (!(o->cover_tolerance >= 0.0f) || !std::isfinite(o->cover_tolerance)) return SPZ_AMD_ERR_INVALID_ARG;
  if (o->cover != 0 && o->cover != 1) return SPZ_AMD_ERR_INVALID_ARG;
  if (o->sh_degree < 0 || o->sh_degree > 3) return SPZ_AMD_ERR_INVALID_ARG;
  return SPZ_AMD_OK;
}

uint64_t spz_amd_seed_samples(uint32_t width, uint32_t height, uint32_t stride) {
  if (width < 1u || width > kMaxSide || height < 1u || height > kMaxSide || stride < 1u || stride > 64u) return 0;
  return seed_lattice(width, height, stride).samples;
}

uint64_t spz_amd_seed_workspace_bytes(uint32_t width, uint32_t height, uint32_t stride) {
  if (width < 1u || width > kMaxSide || height < 1u || height > kMaxSide || stride < 1u || stride > 64u) return 0;
  return seed_layout(seed_lattice(width, height, stride)).bytes;
}

int spz_amd_seed_view_device(const spz_amd_cloud_out *d_cloud, uint64_t num_points, uint64_t capacity, int sh_degree,
                             const spz_amd_render_params *params, const spz_amd_seed_options *options,
                             const float *d_image, int channels, const float *d_depth, const float *d_weights,
                             const float *d_cover_image, const float *d_cover_depth, uint64_t *d_counts,
                             void *d_workspace, void *hip_stream) {
  int rc = spz_amd_seed_check(options);
  if (rc != SPZ_AMD_OK) return rc;
  rc = spz_amd_render_check_params(params);
  if (rc != SPZ_AMD_OK) return rc;
  if (d_cloud == nullptr || d_image == nullptr || d_depth == nullptr || d_counts == nullptr || d_workspace == nullptr) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  if (sh_degree != options->sh_degree || (channels != 3 && channels != 4)) return SPZ_AMD_ERR_INVALID_ARG;
  if ((d_cover_image == nullptr) != (d_cover_depth == nullptr)) return SPZ_AMD_ERR_INVALID_ARG;
  if (num_points > capacity) return SPZ_AMD_ERR_INVALID_ARG;
  if (capacity > kMaxEntries) return SPZ_AMD_ERR_TOO_MANY_POINTS;
  const bool room = capacity > num_points;
  if (room && (!d_cloud->positions || !d_cloud->scales || !d_cloud->rotations || !d_cloud->alphas || !d_cloud->colors ||
               (sh_degree > 0 && !d_cloud->sh))) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const SeedLattice l = seed_lattice(params->width, params->height, options->stride);
  if (l.samples == 0u) {  // a view narrower than half a stride: no sample, no launch
    SPZ_HIP_TRY(hipMemsetAsync(d_counts, 0, 24, st));
    return SPZ_AMD_OK;
  }
  const SeedLayout m = seed_layout(l);
  uint8_t *ws = align_ws(d_workspace);
  auto *d_sel = reinterpret_cast<uint32_t *>(ws + m.sel);
  auto *d_valid = reinterpret_cast<uint32_t *>(ws + m.valid);
  auto *d_offsets = reinterpret_cast<unsigned long long *>(ws + m.offsets);
  const SeedArgs a = seed_args(params, options, channels);
  const bool covering = options->cover != 0 && num_points > 0 && d_cover_image != nullptr;
  hipLaunchKernelGGL(spz_seed_select_kernel, dim3(l.blocks), dim3(kSeedBlock), 0, st, l, a, d_image, d_depth, d_weights,
                     covering ? d_cover_image : nullptr, covering ? d_cover_depth : nullptr, ws + m.flags, d_sel, d_valid);
  SPZ_HIP_TRY(hipGetLastError());
  const unsigned long long left = capacity - num_points;
  hipLaunchKernelGGL(spz_seed_offsets_kernel, dim3(1), dim3(kSeedBlock), 0, st, d_sel, d_valid, l.blocks, left, d_offsets,
                     reinterpret_cast<unsigned long long *>(d_counts));
  SPZ_HIP_TRY(hipGetLastError());
  if (!room) return SPZ_AMD_OK;  // every selected sample is refused: nothing to write
  // the grid is the lattice's, never the selection's: a view that selects nothing launches blocks that return at once
  hipLaunchKernelGGL(spz_seed_emit_kernel, dim3(l.blocks), dim3(kSeedBlock), 0, st, l, a, d_image, d_depth, ws + m.flags,
                     d_sel, d_offsets, (unsigned long long)num_points, left, d_cloud->positions, d_cloud->scales,
                     d_cloud->rotations, d_cloud->alphas, d_cloud->colors, d_cloud->sh);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

int spz_amd_seed_open(const spz_amd_render_params *views, int num_views, const spz_amd_seed_options *options,
                      const float *const *h_images, const int32_t *channels, const float *const *h_depths,
                      const float *const *h_weights, const uint8_t *d_base, size_t base_size,
                      const spz_amd_header *base_hdr, uint64_t max_points, int device, void **ctx,
                      uint64_t *h_out_bytes, uint64_t *h_counts, uint64_t *h_num_points, float *h_ms,
                      int32_t *h_bad_view) {
  if (h_bad_view) *h_bad_view = -1;
  if (ctx == nullptr || h_out_bytes == nullptr || h_images == nullptr || channels == nullptr || h_depths == nullptr) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  *ctx = nullptr;
  *h_out_bytes = 0;
  if (h_num_points) *h_num_points = 0;
  int rc = spz_amd_seed_check(options);
  if (rc != SPZ_AMD_OK) return rc;
  rc = check_views(views, num_views, SPZ_AMD_SEED_MAX_VIEWS, h_bad_view);
  if (rc != SPZ_AMD_OK) return rc;
  uint64_t pixels = 0, samples_sum = 0, ws_bytes = 0;
  for (int v = 0; v < num_views; ++v) {
    if (h_images[v] == nullptr || h_depths[v] == nullptr || (channels[v] != 3 && channels[v] != 4)) {
      if (h_bad_view) *h_bad_view = v;
      return SPZ_AMD_ERR_INVALID_ARG;
    }
    const uint64_t px = (uint64_t)views[v].width * views[v].height;
    pixels = px > pixels ? px : pixels;
    samples_sum += spz_amd_seed_samples(views[v].width, views[v].height, options->stride);
    const uint64_t w = spz_amd_seed_workspace_bytes(views[v].width, views[v].height, options->stride);
    ws_bytes = w > ws_bytes ? w : ws_bytes;
  }
  if (max_points > SPZ_AMD_REFERENCE_MAX_POINTS) return SPZ_AMD_ERR_TOO_MANY_POINTS;
  const uint64_t max_new = max_points ? max_points
                                      : (samples_sum < SPZ_AMD_REFERENCE_MAX_POINTS ? samples_sum
                                                                                    : SPZ_AMD_REFERENCE_MAX_POINTS);
  uint64_t n0 = 0;
  if (base_hdr != nullptr) {
    rc = check_render_input(d_base, base_size, base_hdr);
    if (rc != SPZ_AMD_OK) return rc;
    if ((int)base_hdr->sh_degree != options->sh_degree) return SPZ_AMD_ERR_SH_DEGREE;
    n0 = base_hdr->num_points;
  }
  const int deg = options->sh_degree, coord = views[0].coord;
  const uint64_t cap_n = n0 + max_new, sh3 = (uint64_t)sh_dim_for_degree(deg) * 3u;
  DeviceGuard guard;
  rc = guard.enter(device);
  if (rc != SPZ_AMD_OK) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  PackedResultPtr c;
  rc = packed_result_open(device, &c);
  if (rc != SPZ_AMD_OK) return rc;

  // the cloud at its capacity, one view's inputs and cover maps, the select's workspace, the small values
  WorkspaceOffsets o;
  const uint64_t o_pos = o.put(12u * cap_n), o_scl = o.put(12u * cap_n), o_rot = o.put(16u * cap_n),
                 o_alp = o.put(4u * cap_n), o_col = o.put(12u * cap_n), o_sh = o.put(4u * sh3 * cap_n),
                 o_image = o.put(16u * pixels), o_depth = o.put(4u * pixels), o_weight = o.put(4u * pixels),
                 o_cimage = o.put(16u * pixels), o_cdepth = o.put(8u * pixels), o_ws = o.put(ws_bytes),
                 o_small = o.put(64u);
  SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&c->block), o.bytes()));
  uint8_t *raw = align_ws(c->block);
  auto f = [&](uint64_t off) { return reinterpret_cast<float *>(raw + off); };
  const spz_amd_cloud_out cloud = {f(o_pos), f(o_scl), f(o_rot), f(o_alp), f(o_col), sh3 ? f(o_sh) : nullptr};
  const spz_amd_cloud_in cloud_in = {cloud.positions, cloud.scales, cloud.rotations, cloud.alphas, cloud.colors, cloud.sh};
  auto *d_total = reinterpret_cast<uint64_t *>(raw + o_small);
  auto *d_status = reinterpret_cast<uint32_t *>(raw + o_small + 8u);
  auto *d_counts = reinterpret_cast<uint64_t *>(raw + o_small + 16u);
  if (n0) {
    rc = spz_amd_decode_device(d_base, base_size, base_hdr, coord, &cloud, c->st);
    if (rc != SPZ_AMD_OK) return rc;
  }

  uint64_t n = n0, cap = 0, total = 0;
  if (options->cover != 0 && cap_n > 0) {
    // the render scratch's prepare part at the cloud's final capacity, once: prepare_view then grows it for entries
    // only, not on every view whose cloud has outgrown the last one's
    cap = spz_amd_render_workspace_bytes(cap_n, 0);
    SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&c->scratch), cap));
  }
  double render_ms = 0.0, seed_ms = 0.0;
  RenderSource src;
  src.cloud = &cloud_in;
  src.sh_degree = deg;
  for (int v = 0; v < num_views; ++v) {
    auto fail = [&](int r) {
      if (h_bad_view) *h_bad_view = v;
      return r;
    };
    const double a0 = ms_since(t0);
    const bool covering = options->cover != 0 && n > 0;
    if (covering) {
      spz_amd_render_params p = views[v];
      p.background[0] = p.background[1] = p.background[2] = 0.0f;
      p.max_sh_degree = deg;
      src.n = n;
      rc = prepare_view(&c->scratch, &cap, src, &p, d_total, c->st, &total);
      if (rc != SPZ_AMD_OK) return fail(rc);
      rc = spz_amd_render_depth_device(n, &p, total, f(o_cimage), f(o_cdepth), nullptr, d_status, c->scratch, c->st);
      if (rc != SPZ_AMD_OK) return fail(rc);
      SPZ_HIP_TRY(hipStreamSynchronize(c->st));
    }
    const double a1 = ms_since(t0);
    const uint64_t px = (uint64_t)views[v].width * views[v].height;
    SPZ_HIP_TRY(hipMemcpyAsync(f(o_image), h_images[v], 4u * px * (uint64_t)channels[v], hipMemcpyHostToDevice, c->st));
    SPZ_HIP_TRY(hipMemcpyAsync(f(o_depth), h_depths[v], 4u * px, hipMemcpyHostToDevice, c->st));
    const bool weighted = h_weights != nullptr && h_weights[v] != nullptr;
    if (weighted) SPZ_HIP_TRY(hipMemcpyAsync(f(o_weight), h_weights[v], 4u * px, hipMemcpyHostToDevice, c->st));
    rc = spz_amd_seed_view_device(&cloud, n, cap_n, deg, &views[v], options, f(o_image), channels[v], f(o_depth),
                                  weighted ? f(o_weight) : nullptr, covering ? f(o_cimage) : nullptr,
                                  covering ? f(o_cdepth) : nullptr, d_counts, raw + o_ws, c->st);
    if (rc != SPZ_AMD_OK) return fail(rc);
    uint64_t counts[3] = {0, 0, 0};
    SPZ_HIP_TRY(hipMemcpyAsync(counts, d_counts, sizeof(counts), hipMemcpyDeviceToHost, c->st));
    SPZ_HIP_TRY(hipStreamSynchronize(c->st));
    if (h_counts) std::memcpy(h_counts + 3u * (size_t)v, counts, sizeof(counts));
    n += counts[1];
    render_ms += a1 - a0;
    seed_ms += ms_since(t0) - a1;
  }
  if (c->scratch) {
    SPZ_HIP_TRY(hipFree(c->scratch));
    c->scratch = nullptr;
  }

  // the new points alone, under a header of their own
  const double e0 = ms_since(t0);
  const uint64_t added = n - n0;
  spz_amd_layout lay;
  rc = spz_amd_stream_layout(added, deg, 3, &lay);
  if (rc != SPZ_AMD_OK) return rc;
  SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&c->out_block), lay.total_bytes));
  const spz_amd_cloud_in tail = {cloud.positions + 3u * n0, cloud.scales + 3u * n0, cloud.rotations + 4u * n0,
                                 cloud.alphas + n0,         cloud.colors + 3u * n0, sh3 ? cloud.sh + sh3 * n0 : nullptr};
  rc = spz_amd_encode_device(&tail, added, deg, 0, coord, 3, c->out_block, lay.total_bytes, c->st);
  if (rc != SPZ_AMD_OK) return rc;
  SPZ_HIP_TRY(hipStreamSynchronize(c->st));
  SPZ_HIP_TRY(hipFree(c->block));
  c->block = nullptr;
  c->out = c->out_block;
  c->out_bytes = lay.total_bytes;
  *h_out_bytes = lay.total_bytes;
  if (h_num_points) *h_num_points = added;
  if (h_ms) {
    h_ms[0] = (float)render_ms;
    h_ms[1] = (float)seed_ms;
    h_ms[2] = (float)(ms_since(t0) - e0);
  }
  *ctx = c.release();
  return SPZ_AMD_OK;
}

int spz_amd_seed_fetch(void *ctx, uint8_t *h_out) { return packed_result_fetch(ctx, h_out); }
const uint8_t *spz_amd_seed_device_data(void *ctx) { return packed_result_device_data(ctx); }
void spz_amd_seed_close(void *ctx) { packed_result_close(ctx); }

}  // extern "C"
