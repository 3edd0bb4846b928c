// spz_render_internal.hpp — what the translation units of the rasteriser share (spz_render.hip: the forward and its
// scoring and depth blends; spz_render_backward.hip: the gradients): the tile geometry, the f64 camera, the float
// cloud's loader, 3DGS's sh constants, the wave sum of the blend backwards, the workspace layout of the prepare and
// entries parts, the fill of a blend kernel's common parameters, and the host-side argument checks.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "spz_amd.h"
#include "spz_common.hpp"
#include "spz_sort_internal.hpp"

#pragma clang fp contract(off)

namespace spz_amd_detail {

constexpr uint32_t kTile = 16;
constexpr uint32_t kBlendThreads = kTile * kTile;
constexpr uint32_t kMaxSide = 16384;
constexpr uint64_t kMaxTiles = (kMaxSide / kTile) * (kMaxSide / kTile);  // 2^20
constexpr uint32_t kPreBlock = 256;
constexpr uint32_t kScanBlock = 256;
constexpr uint32_t kScanPer = 4;
constexpr uint32_t kScanItems = kScanBlock * kScanPer;  // depth-ordered Gaussians per run of the count scan

// The camera, in f64 (every value is the f32 argument widened, or computed from them on the host).
struct RenderCam {
  double R[9], t[3], campos[3];
  double fx, fy, cx, cy, near_plane;
  double lim_x_pos, lim_x_neg, lim_y_pos, lim_y_neg;  // bounds of x/z and y/z in the Jacobian
  uint32_t width, height, tiles_x, tiles_y;
  uint32_t sh_coeffs;  // higher-band sh coefficients used: 0, 3, 8, 15
  uint32_t antialiased;
};

// One decoded Gaussian (the floats loadSpz returns).
struct Gauss {
  float p[3], s[3], q[4], alpha, col[3];
};

// A GaussianCloud's arrays in device memory.
struct FloatSrc {
  const float *positions, *scales, *rotations, *alphas, *colors, *sh;
  uint32_t sh_dim;
  __device__ __forceinline__ void load(uint32_t i, Gauss &g) const {
    const unsigned long long i3 = (unsigned long long)i * 3u, i4 = (unsigned long long)i * 4u;
#pragma unroll
    for (uint32_t a = 0; a < 3; ++a) {
      g.p[a] = positions[i3 + a];
      g.s[a] = scales[i3 + a];
      g.col[a] = colors[i3 + a];
    }
#pragma unroll
    for (uint32_t a = 0; a < 4; ++a) g.q[a] = rotations[i4 + a];
    g.alpha = alphas[i];
  }
  __device__ __forceinline__ float coeff(uint32_t i, uint32_t k, uint32_t c) const {
    return sh[(unsigned long long)i * sh_dim * 3u + k * 3u + c];
  }
};

// 3DGS's sh constants (forward.cu).
constexpr double kC0 = 0.28209479177387814;
constexpr double kC1 = 0.4886025119029199;
constexpr double kC2[5] = {1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792,
                           0.5462742152960396};
constexpr double kC3[7] = {-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154,
                           -0.4570457994644658, 1.445305721320277, -0.5900435899266435};

__device__ __forceinline__ double clampd(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The sum of an f32 over the 64 lanes of a wave (every lane active): within each row of 16 by DPP (quad xor 1, quad
// xor 2, half-row mirror, row mirror), then the four rows' values by readlane.  The result is wave-uniform.
__device__ __forceinline__ float wave_sum_f32(float v) {
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xb1, 0xf, 0xf, false));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4e, 0xf, 0xf, false));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xf, 0xf, false));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xf, 0xf, false));
  const int b = __float_as_int(v);
  return (__int_as_float(__builtin_amdgcn_readlane(b, 0)) + __int_as_float(__builtin_amdgcn_readlane(b, 16))) +
         (__int_as_float(__builtin_amdgcn_readlane(b, 32)) + __int_as_float(__builtin_amdgcn_readlane(b, 48)));
}

inline uint64_t al(uint64_t b) { return Workspace::aligned(b); }

// Workspace: [prepare part | depth sort] then [entries part] (absent for max_entries == 0).
struct RenderLayout {
  uint64_t runs;
  uint64_t rec, key, count, order, run_sums, total, sort_n, prefix;            // from the 256-aligned base
  uint64_t entry, eorder, sorted_gid, ranges, sort_m, entries;  // from the entries part's base
  SortLayout sl_n, sl_m;
  uint64_t bytes;
};

inline RenderLayout render_layout(uint64_t n, uint64_t m) {
  RenderLayout w = {};
  w.runs = (n + kScanItems - 1) / kScanItems;
  uint64_t off = 0;
  w.rec = off;
  off += al(n * sizeof(spz_amd_render_record));
  w.key = off;
  off += al(n * 4u);
  w.count = off;
  off += al(n * 4u);
  w.order = off;
  off += al(n * 4u);
  w.run_sums = off;
  off += al(w.runs * 8u);
  w.total = off;
  off += al(8u);
  w.sort_n = off;
  w.sl_n = sort_layout(n);
  off += n ? al(w.sl_n.bytes) : 0u;
  w.prefix = off;
  uint64_t e = 0;
  if (m) {
    w.entry = e;
    e += al(m * 8u);
    w.eorder = e;
    e += al(m * 4u);
    w.sorted_gid = e;
    e += al(m * 4u);
    w.ranges = e;
    e += al(kMaxTiles * 8u);
    w.sort_m = e;
    w.sl_m = sort_layout(m);
    e += al(w.sl_m.bytes);
  }
  w.entries = e;
  w.bytes = w.prefix + w.entries + 256u;  // room to align a caller's pointer up to 256
  return w;
}

// What the parameter blocks of the blend kernels have in common (BlendParams, ScoreParams, DepthParams,
// BlendBackwardParams): the records, the tile lists and the total from the workspace (base: the prepare part; ent: the
// entries part), the image's size and the background.  Returns the launch grid, one workgroup per tile.
template <class P>
inline dim3 fill_blend_params(P &b, const RenderLayout &wl, const uint8_t *base, const uint8_t *ent,
                              const spz_amd_render_params *params, uint64_t max_entries) {
  b.rec = reinterpret_cast<const spz_amd_render_record *>(base + wl.rec);
  b.sorted_gid = max_entries ? reinterpret_cast<const uint32_t *>(ent + wl.sorted_gid) : nullptr;
  b.ranges = max_entries ? reinterpret_cast<const uint2 *>(ent + wl.ranges) : nullptr;  // read only when the total is > 0
  b.total = reinterpret_cast<const unsigned long long *>(base + wl.total);
  b.max_entries = max_entries;
  b.width = params->width;
  b.height = params->height;
  b.tiles_x = (params->width + kTile - 1) / kTile;
  for (int k = 0; k < 3; ++k) b.bg[k] = params->background[k];
  return dim3(b.tiles_x, (params->height + kTile - 1) / kTile);
}

inline bool finite3(const float *v, int k) {
  for (int i = 0; i < k; ++i) {
    if (!std::isfinite(v[i])) return false;
  }
  return true;
}

inline int check_params(const spz_amd_render_params *p) {
  if (p == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  if (!finite3(p->world_to_camera, 12) || !finite3(p->background, 3)) return SPZ_AMD_ERR_INVALID_ARG;
  const float *m = p->world_to_camera;
  double R[9];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) R[r * 3 + c] = m[r * 4 + c];
  }
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) {
      const double d = R[i * 3] * R[j * 3] + R[i * 3 + 1] * R[j * 3 + 1] + R[i * 3 + 2] * R[j * 3 + 2];
      if (std::fabs(d - (i == j ? 1.0 : 0.0)) > 1e-4) return SPZ_AMD_ERR_INVALID_ARG;
    }
  }
  const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) +
                     R[2] * (R[3] * R[7] - R[4] * R[6]);
  if (!(det > 0.0)) return SPZ_AMD_ERR_INVALID_ARG;
  if (!std::isfinite(p->fx) || !std::isfinite(p->fy) || !(p->fx > 0.0f) || !(p->fy > 0.0f)) return SPZ_AMD_ERR_INVALID_ARG;
  if (!std::isfinite(p->cx) || !std::isfinite(p->cy)) return SPZ_AMD_ERR_INVALID_ARG;
  if (p->width < 1 || p->width > kMaxSide || p->height < 1 || p->height > kMaxSide) return SPZ_AMD_ERR_INVALID_ARG;
  if (!std::isfinite(p->near_plane) || !(p->near_plane > 0.0f)) return SPZ_AMD_ERR_INVALID_ARG;
  if (p->max_sh_degree < 0 || p->max_sh_degree > 3) return SPZ_AMD_ERR_INVALID_ARG;
  if (!valid_coord(p->coord)) return SPZ_AMD_ERR_INVALID_ARG;
  return SPZ_AMD_OK;
}

inline RenderCam make_cam(const spz_amd_render_params *p, int file_degree, int antialiased) {
  RenderCam c = {};
  for (int r = 0; r < 3; ++r) {
    for (int k = 0; k < 3; ++k) c.R[r * 3 + k] = p->world_to_camera[r * 4 + k];
    c.t[r] = p->world_to_camera[r * 4 + 3];
  }
  for (int k = 0; k < 3; ++k) c.campos[k] = -(c.R[k] * c.t[0] + c.R[3 + k] * c.t[1] + c.R[6 + k] * c.t[2]);
  c.fx = p->fx;
  c.fy = p->fy;
  c.cx = p->cx;
  c.cy = p->cy;
  c.near_plane = p->near_plane;
  const double W = p->width, H = p->height;
  c.lim_x_pos = (W - c.cx) / c.fx + 0.3 * W / c.fx;
  c.lim_x_neg = c.cx / c.fx + 0.3 * W / c.fx;
  c.lim_y_pos = (H - c.cy) / c.fy + 0.3 * H / c.fy;
  c.lim_y_neg = c.cy / c.fy + 0.3 * H / c.fy;
  c.width = p->width;
  c.height = p->height;
  c.tiles_x = (p->width + kTile - 1) / kTile;
  c.tiles_y = (p->height + kTile - 1) / kTile;
  const int deg = file_degree < p->max_sh_degree ? file_degree : p->max_sh_degree;
  c.sh_coeffs = (uint32_t)sh_dim_for_degree(deg);
  c.antialiased = antialiased ? 1u : 0u;
  return c;
}

inline int cloud_source(const spz_amd_cloud_in *cl, uint64_t n, int sh_degree, FloatSrc *src) {
  const int sd = sh_dim_for_degree(sh_degree);
  if (sd < 0 || cl == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  if (n > kMaxEntries) return SPZ_AMD_ERR_TOO_MANY_POINTS;
  if (n && (!cl->positions || !cl->scales || !cl->rotations || !cl->alphas || !cl->colors || (sd > 0 && !cl->sh))) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  *src = FloatSrc{cl->positions, cl->scales, cl->rotations, cl->alphas, cl->colors, cl->sh, (uint32_t)sd};
  return SPZ_AMD_OK;
}

}  // namespace spz_amd_detail
