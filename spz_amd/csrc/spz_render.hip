// spz_render.hip — a forward 3D Gaussian splat rasteriser (DESIGN §8 "Render"; the contract is in include/spz_amd.h).
// One pinhole view of a packed stream or of a float cloud, with no display attached.
//
//   spz_render_preprocess_kernel<Src>  one lane per Gaussian: decode (packed: the decode kernel's per-field helpers of
//                                      spz_quant.hpp / spz_common.hpp) or load (floats), project, the 2D covariance,
//                                      conic, radius, tile rectangle and sh colour in f64; writes the 48-byte record,
//                                      the tile count and the f32 depth key (+inf: invisible).
//   (depth order)                      spz_amd_argsort_f32_device over the depth keys: stable, so ties go by index.
//   spz_render_block_sums_kernel       the tile counts in depth order, summed per run of kScanItems.
//   spz_render_scan_sums_kernel        one workgroup: exclusive u64 scan of the run sums; the entry total.
//   spz_render_emit_kernel             the in-run scan again, then every Gaussian's (tile id, Gaussian) entries at its
//                                      offset, in depth order.  Nothing when the total is above max_entries (status 1).
//   spz_render_pad_kernel              sentinel keys after the total, so the sort may run over max_entries keys.
//   (tile order)                       radix_passes of spz_sort.hip over the tile ids: 1..3 stable 8-bit digits.
//   spz_render_ranges_kernel           the Gaussian of every sorted entry, and each tile's [start, end).  The entries
//                                      are (tile id, Gaussian) pairs, so each sorted one costs one random 8-byte read.
//   spz_render_blend_kernel            one 256-lane workgroup per 16x16 tile, one pixel per lane: the tile's records
//                                      staged in LDS 256 at a time, read by every lane at the same address (a
//                                      broadcast); the workgroup stops once every lane has stopped.
//   spz_render_score_kernel            the blend again, pixel for pixel, adding each used pair's weight T a into the
//                                      Gaussian's u64 sum (as rint(w 2^24)) and f32 max (spz_prune.hip uses it).
//   spz_render_depth_kernel            the blend again, pixel for pixel, adding each used pair's (T a) z into the pixel's
//                                      depth sum and taking the first Gaussian after which T < 0.5 as its median.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "spz_amd.h"
#include "spz_block_ops.hpp"
#include "spz_common.hpp"
#include "spz_kernel_params.hpp"
#include "spz_quant.hpp"
#include "spz_render_internal.hpp"
#include "spz_sort_internal.hpp"

#pragma clang fp contract(off)

namespace spz_amd_detail {
namespace {

static_assert(sizeof(spz_amd_render_record) == 48, "the record is 48 bytes");

// The packed stream: the decode kernel's per-field arithmetic, one Gaussian at a time.
struct PackedSrc {
  const uint8_t *positions, *alphas, *colors, *scales, *rotations, *sh;
  const float *tables;
  unsigned long long sh_mask;  // bit k * 3 + c: coefficient k channel c is negated
  float pos_scale;
  uint32_t version, sh_dim, flip_p, flip_q;
  __device__ __forceinline__ void load(uint32_t i, Gauss &g) const {
#pragma unroll
    for (uint32_t a = 0; a < 3; ++a) {
      g.p[a] = decode_position_axis(positions, i, a, version == 1u, pos_scale, flip_p);
      g.s[a] = scale_from_byte(scales[(unsigned long long)i * 3u + a]);
      g.col[a] = tables[kTableColorDec + colors[(unsigned long long)i * 3u + a]];
    }
    g.alpha = tables[kTableAlphaDec + alphas[i]];
    F32x4 r;
    if (version >= 3u) {
      const uint8_t *b = rotations + (unsigned long long)i * 4u;
      r = unpack_quat_smallest_three((uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) |
                                     ((uint32_t)b[3] << 24), flip_q);
    } else {
      const uint8_t *b = rotations + (unsigned long long)i * 3u;
      r = unpack_quat_first_three((uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16), flip_q);
    }
    g.q[0] = r.x;
    g.q[1] = r.y;
    g.q[2] = r.z;
    g.q[3] = r.w;
  }
  __device__ __forceinline__ float coeff(uint32_t i, uint32_t k, uint32_t c) const {
    const uint32_t e = k * 3u + c;
    return xor_sign(sh_from_byte(sh[(unsigned long long)i * sh_dim * 3u + e]), (uint32_t)(sh_mask >> e) & 1u);
  }
};

template <class Src>
__device__ __forceinline__ double sh_channel(const Src &src, uint32_t i, uint32_t c, double col, uint32_t nk, double x,
                                             double y, double z) {
  double r = kC0 * col;
  if (nk >= 3u) {
    r = r - kC1 * y * (double)src.coeff(i, 0, c) + kC1 * z * (double)src.coeff(i, 1, c) -
        kC1 * x * (double)src.coeff(i, 2, c);
  }
  if (nk >= 8u) {
    const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    r = r + kC2[0] * xy * (double)src.coeff(i, 3, c) + kC2[1] * yz * (double)src.coeff(i, 4, c) +
        kC2[2] * (2.0 * zz - xx - yy) * (double)src.coeff(i, 5, c) + kC2[3] * xz * (double)src.coeff(i, 6, c) +
        kC2[4] * (xx - yy) * (double)src.coeff(i, 7, c);
    if (nk >= 15u) {
      r = r + kC3[0] * y * (3.0 * xx - yy) * (double)src.coeff(i, 8, c) +
          kC3[1] * xy * z * (double)src.coeff(i, 9, c) +
          kC3[2] * y * (4.0 * zz - xx - yy) * (double)src.coeff(i, 10, c) +
          kC3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy) * (double)src.coeff(i, 11, c) +
          kC3[4] * x * (4.0 * zz - xx - yy) * (double)src.coeff(i, 12, c) +
          kC3[5] * z * (xx - yy) * (double)src.coeff(i, 13, c) +
          kC3[6] * x * (xx - 3.0 * yy) * (double)src.coeff(i, 14, c);
    }
  }
  r = r + 0.5;
  return r > 0.0 ? r : 0.0;
}

}  // namespace

template <class Src>
__global__ __launch_bounds__(kPreBlock) void spz_render_preprocess_kernel(const Src src, const RenderCam cam,
                                                                          uint32_t n, spz_amd_render_record *rec,
                                                                          float *depth_key, uint32_t *tile_count) {
  const uint32_t i = blockIdx.x * kPreBlock + threadIdx.x;
  if (i >= n) return;
  Gauss g;
  src.load(i, g);
  spz_amd_render_record o = {};
  o.depth = __builtin_huge_valf();
  uint32_t count = 0;
  const double px = g.p[0], py = g.p[1], pz = g.p[2];
  const double *R = cam.R;
  const double x = R[0] * px + R[1] * py + R[2] * pz + cam.t[0];
  const double y = R[3] * px + R[4] * py + R[5] * pz + cam.t[1];
  const double z = R[6] * px + R[7] * py + R[8] * pz + cam.t[2];
  bool visible = z > cam.near_plane;  // false for NaN too
  if (visible) {
    const double mx = cam.fx * x / z + cam.cx - 0.5, my = cam.fy * y / z + cam.cy - 0.5;
    // R_q of the normalised quaternion (x, y, z, w)
    double qx = g.q[0], qy = g.q[1], qz = g.q[2], qw = g.q[3];
    const double qn = sqrt(qx * qx + qy * qy + qz * qz + qw * qw);
    qx /= qn;
    qy /= qn;
    qz /= qn;
    qw /= qn;
    const double Rq[9] = {1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy),
                          2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx),
                          2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)};
    const double s0 = exp((double)g.s[0]), s1 = exp((double)g.s[1]), s2 = exp((double)g.s[2]);
    double M[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      M[r * 3 + 0] = Rq[r * 3 + 0] * s0;
      M[r * 3 + 1] = Rq[r * 3 + 1] * s1;
      M[r * 3 + 2] = Rq[r * 3 + 2] * s2;
    }
    double S[9];  // Sigma = M M^T
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) S[r * 3 + c] = M[r * 3 + 0] * M[c * 3 + 0] + M[r * 3 + 1] * M[c * 3 + 1] + M[r * 3 + 2] * M[c * 3 + 2];
    }
    const double tx = z * clampd(x / z, -cam.lim_x_neg, cam.lim_x_pos);
    const double ty = z * clampd(y / z, -cam.lim_y_neg, cam.lim_y_pos);
    const double J00 = cam.fx / z, J02 = -(cam.fx * tx) / (z * z);
    const double J11 = cam.fy / z, J12 = -(cam.fy * ty) / (z * z);
    double T[6];  // J R: row 0 = J00 R0 + J02 R2, row 1 = J11 R1 + J12 R2
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      T[c] = J00 * R[c] + J02 * R[6 + c];
      T[3 + c] = J11 * R[3 + c] + J12 * R[6 + c];
    }
    double TS[6];  // T Sigma
#pragma unroll
    for (int r = 0; r < 2; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) TS[r * 3 + c] = T[r * 3 + 0] * S[c] + T[r * 3 + 1] * S[3 + c] + T[r * 3 + 2] * S[6 + c];
    }
    double a = TS[0] * T[0] + TS[1] * T[1] + TS[2] * T[2];
    const double b = TS[0] * T[3] + TS[1] * T[4] + TS[2] * T[5];
    double c = TS[3] * T[3] + TS[4] * T[4] + TS[5] * T[5];
    const double det0 = a * c - b * b;
    a = a + 0.3;
    c = c + 0.3;
    const double det = a * c - b * b;
    visible = det > 0.0;
    if (visible) {
      double opacity = 1.0 / (1.0 + exp(-(double)g.alpha));
      if (cam.antialiased) opacity = opacity * sqrt((det0 > 0.0 ? det0 : 0.0) / det);
      const double ca = c / det, cb = -b / det, cc = a / det;
      const double mid = 0.5 * (a + c);
      const double disc = mid * mid - det;
      const double lam = mid + sqrt(disc > 0.1 ? disc : 0.1);
      const double radius = ceil(3.0 * sqrt(lam));
      // the opacity too: fminf(0.99f, NaN) is 0.99f, so a NaN alpha would blend as an opaque Gaussian
      visible = isfinite(mx) && isfinite(my) && isfinite(radius) && isfinite(ca) && isfinite(cb) && isfinite(cc) &&
                isfinite(opacity);
      if (visible) {
        const double tw = (double)cam.tiles_x, th = (double)cam.tiles_y;
        const double x0 = clampd(floor((mx - radius) / 16.0), 0.0, tw), x1 = clampd(floor((mx + radius + 15.0) / 16.0), 0.0, tw);
        const double y0 = clampd(floor((my - radius) / 16.0), 0.0, th), y1 = clampd(floor((my + radius + 15.0) / 16.0), 0.0, th);
        visible = x1 > x0 && y1 > y0;
        if (visible) {
          // direction from the camera centre, normalised
          double dx = px - cam.campos[0], dy = py - cam.campos[1], dz = pz - cam.campos[2];
          const double dn = sqrt(dx * dx + dy * dy + dz * dz);
          dx /= dn;
          dy /= dn;
          dz /= dn;
          o.mean[0] = (float)mx;
          o.mean[1] = (float)my;
          o.conic[0] = (float)ca;
          o.conic[1] = (float)cb;
          o.conic[2] = (float)cc;
          o.opacity = (float)opacity;
#pragma unroll
          for (uint32_t ch = 0; ch < 3; ++ch) {
            o.rgb[ch] = (float)sh_channel(src, i, ch, (double)g.col[ch], cam.sh_coeffs, dx, dy, dz);
          }
          o.depth = (float)z;
          o.rect[0] = (uint16_t)x0;
          o.rect[1] = (uint16_t)y0;
          o.rect[2] = (uint16_t)x1;
          o.rect[3] = (uint16_t)y1;
          count = (uint32_t)(x1 - x0) * (uint32_t)(y1 - y0);
        }
      }
    }
  }
  rec[i] = o;
  depth_key[i] = o.depth;
  tile_count[i] = count;
}

static_assert(kScanBlock == kOpsBlock, "the scans below run at the default block size");

__global__ __launch_bounds__(kScanBlock) void spz_render_block_sums_kernel(const uint32_t *order, const uint32_t *tile_count,
                                                                           uint32_t n, unsigned long long *run_sums) {
  __shared__ unsigned long long s[kScanBlock];
  const unsigned long long k0 = (unsigned long long)blockIdx.x * kScanItems + threadIdx.x * kScanPer;
  unsigned long long v = 0;
#pragma unroll
  for (uint32_t r = 0; r < kScanPer; ++r) {
    if (k0 + r < n) v += tile_count[order[k0 + r]];
  }
  unsigned long long sum;
  (void)block_exclusive_scan(v, s, &sum);
  if (threadIdx.x == 0) run_sums[blockIdx.x] = sum;
}

// One workgroup: run_sums[0 .. runs) -> exclusive prefixes in place; *total and *d_total = the sum.
__global__ __launch_bounds__(kScanBlock) void spz_render_scan_sums_kernel(unsigned long long *run_sums, uint32_t runs,
                                                                          unsigned long long *total,
                                                                          unsigned long long *d_total) {
  __shared__ unsigned long long s[kScanBlock];
  const unsigned long long sum = block_scan_owned_runs(
      runs, s, [&](uint32_t k) { return run_sums[k]; },
      [&](uint32_t k, unsigned long long before) { run_sums[k] = before; });
  if (threadIdx.x == 0) {
    *total = sum;
    *d_total = sum;
  }
}

struct EmitParams {
  const uint32_t *order, *tile_count;
  const spz_amd_render_record *rec;
  const unsigned long long *run_offsets, *total;
  uint2 *entry;       // (tile id, Gaussian)
  uint32_t *sort_key;  // the tile id again, in the sort's key plane
  uint32_t *status;
  unsigned long long max_entries;
  uint32_t n, tiles_x;
};

__global__ __launch_bounds__(kScanBlock) void spz_render_emit_kernel(const EmitParams p) {
  __shared__ unsigned long long s[kScanBlock];
  const unsigned long long total = *p.total;
  if (total > p.max_entries) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *p.status = 1u;
    return;
  }
  const unsigned long long k0 = (unsigned long long)blockIdx.x * kScanItems + threadIdx.x * kScanPer;
  uint32_t g[kScanPer], c[kScanPer];
  unsigned long long v = 0;
#pragma unroll
  for (uint32_t r = 0; r < kScanPer; ++r) {
    const bool ok = k0 + r < p.n;
    g[r] = ok ? p.order[k0 + r] : 0u;
    c[r] = ok ? p.tile_count[g[r]] : 0u;
    v += c[r];
  }
  unsigned long long off = p.run_offsets[blockIdx.x] + block_exclusive_scan(v, s);
#pragma unroll
  for (uint32_t r = 0; r < kScanPer; ++r) {
    if (c[r] == 0u) continue;
    if (off + c[r] > total) return;  // cannot happen with consistent counts; never write past the entries
    const spz_amd_render_record &q = p.rec[g[r]];
    const uint32_t x0 = q.rect[0], y0 = q.rect[1], x1 = q.rect[2], y1 = q.rect[3];
    for (uint32_t ty = y0; ty < y1; ++ty) {
      for (uint32_t tx = x0; tx < x1; ++tx) {
        const uint32_t key = ty * p.tiles_x + tx;
        p.entry[off] = make_uint2(key, g[r]);
        p.sort_key[off] = key;
        ++off;
      }
    }
  }
}

// Sort keys [total, max_entries) (every key when the total does not fit) = 0xffffffff: after every tile id.
__global__ __launch_bounds__(256) void spz_render_pad_kernel(const unsigned long long *total, uint32_t max_entries,
                                                             uint32_t *sort_key) {
  const unsigned long long t = *total;
  const uint32_t from = t > max_entries ? 0u : (uint32_t)t;
  for (uint32_t j = from + blockIdx.x * 256u + threadIdx.x; j < max_entries; j += gridDim.x * 256u) sort_key[j] = 0xffffffffu;
}

// One lane per sorted entry (one random 8-byte read each): its Gaussian, and the tile runs' bounds.  The neighbours' tile
// ids come through LDS; the two at the workgroup's edges are read again.
__global__ __launch_bounds__(256) void spz_render_ranges_kernel(const unsigned long long *total_p, uint32_t max_entries,
                                                                const uint32_t *order, const uint2 *entry,
                                                                uint32_t *sorted_gid, uint2 *ranges) {
  __shared__ uint32_t s_key[256 + 2];
  const unsigned long long total = *total_p;
  if (total > max_entries) return;
  const uint32_t m = (uint32_t)total;
  const uint32_t tid = threadIdx.x;
  const uint32_t j = blockIdx.x * 256u + tid;
  uint32_t t = 0xffffffffu;
  if (j < m) {
    const uint2 v = entry[order[j]];
    t = v.x;
    sorted_gid[j] = v.y;
  }
  s_key[tid + 1u] = t;
  if (tid == 0u) s_key[0] = (j > 0u && j - 1u < m) ? entry[order[j - 1u]].x : 0xffffffffu;
  if (tid == 255u) s_key[257] = (j + 1u < m) ? entry[order[j + 1u]].x : 0xffffffffu;
  __syncthreads();
  if (j < m) {
    if (j == 0u || s_key[tid] != t) ranges[t].x = j;
    if (j + 1u == m || s_key[tid + 2u] != t) ranges[t].y = j + 1u;
  }
}

struct BlendParams {
  const spz_amd_render_record *rec;
  const uint32_t *sorted_gid;
  const uint2 *ranges;
  const unsigned long long *total;
  float *image;
  unsigned long long max_entries;
  uint32_t width, height, tiles_x;
  float bg[3];
};

__global__ __launch_bounds__(kBlendThreads) void spz_render_blend_kernel(const BlendParams p) {
  __shared__ float2 s_xy[kBlendThreads];
  __shared__ float4 s_co[kBlendThreads];   // conic A, B, C, opacity
  __shared__ float4 s_rgb[kBlendThreads];
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
  const float fu = (float)u, fv = (float)v;
  float T = 1.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
  bool done = !inside;
  for (uint32_t base = begin; base < end; base += kBlendThreads) {
    // also the barrier between the previous batch's reads and this batch's writes
    if (__syncthreads_count(done ? 1 : 0) == (int)kBlendThreads) break;
    const uint32_t j = base + t;
    if (j < end) {
      const spz_amd_render_record &q = p.rec[p.sorted_gid[j]];
      s_xy[t] = make_float2(q.mean[0], q.mean[1]);
      s_co[t] = make_float4(q.conic[0], q.conic[1], q.conic[2], q.opacity);
      s_rgb[t] = make_float4(q.rgb[0], q.rgb[1], q.rgb[2], 0.0f);
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
      const float4 rgb = s_rgb[k];
      const float w = T * a;
      c0 = c0 + w * rgb.x;
      c1 = c1 + w * rgb.y;
      c2 = c2 + w * rgb.z;
      T = Tn;
    }
  }
  if (inside) {
    float *o = p.image + ((unsigned long long)v * p.width + u) * 4u;
    o[0] = c0 + T * p.bg[0];
    o[1] = c1 + T * p.bg[1];
    o[2] = c2 + T * p.bg[2];
    o[3] = 1.0f - T;
  }
}

namespace {

// Sum and max of a u32 over the 64 lanes of a wave (every lane active): within each row of 16 by DPP (quad xor 1, quad
// xor 2, half-row mirror, row mirror), then the four rows' values by readlane.  The results are wave-uniform.
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xb1, 0xf, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4e, 0xf, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, false);
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) + (uint32_t)__builtin_amdgcn_readlane((int)v, 16) +
         (uint32_t)__builtin_amdgcn_readlane((int)v, 32) + (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
}

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xb1, 0xf, 0xf, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4e, 0xf, 0xf, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, false));
  const uint32_t a = max((uint32_t)__builtin_amdgcn_readlane((int)v, 0), (uint32_t)__builtin_amdgcn_readlane((int)v, 16));
  const uint32_t b = max((uint32_t)__builtin_amdgcn_readlane((int)v, 32), (uint32_t)__builtin_amdgcn_readlane((int)v, 48));
  return max(a, b);
}

}  // namespace

struct ScoreParams {
  const spz_amd_render_record *rec;
  const uint32_t *sorted_gid;
  const uint2 *ranges;
  const unsigned long long *total;
  float *image;  // may be null
  unsigned long long *weight_sum;
  uint32_t *weight_max;  // the f32 bit patterns (non-negative, so they order as u32)
  unsigned long long max_entries;
  uint32_t width, height, tiles_x;
  float bg[3];
};

// The blend of spz_render_blend_kernel, pixel for pixel, plus each used (pixel, Gaussian) pair's weight w = T a.  The
// loop over a batch runs in step across the wave (a stopped lane takes no more pairs) so that each record's
// q = rint(w 2^24) and w are reduced over the wave by DPP; one lane per wave adds them into the batch's LDS slots
// (integer LDS atomics), and each slot that was used goes to the Gaussian's u64 sum and u32 max by one global integer
// atomic each.  Integer sums and maxima do not depend on the order, so the scores repeat their bits.
__global__ __launch_bounds__(kBlendThreads) void spz_render_score_kernel(const ScoreParams p) {
  __shared__ float2 s_xy[kBlendThreads];
  __shared__ float4 s_co[kBlendThreads];   // conic A, B, C, opacity
  __shared__ float4 s_rgb[kBlendThreads];
  __shared__ uint32_t s_sum[kBlendThreads], s_max[kBlendThreads];
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
  const float fu = (float)u, fv = (float)v;
  float T = 1.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
  bool done = !inside;
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
      s_rgb[t] = make_float4(q.rgb[0], q.rgb[1], q.rgb[2], 0.0f);
    }
    s_sum[t] = 0u;
    s_max[t] = 0u;
    __syncthreads();
    const uint32_t cnt = (end - base) < kBlendThreads ? end - base : kBlendThreads;
    for (uint32_t k = 0; k < cnt; ++k) {
      if (__ballot(!done) == 0ull) break;  // wave-uniform: every lane of the wave has stopped
      const float2 xy = s_xy[k];
      const float4 co = s_co[k];
      const float dx = fu - xy.x, dy = fv - xy.y;
      const float power = -0.5f * (co.x * dx * dx + co.z * dy * dy) - co.y * dx * dy;
      const float a = fminf(0.99f, co.w * expf(power));
      const float Tn = T * (1.0f - a);
      bool use = !done && !(power > 0.0f) && !(a < 1.0f / 255.0f);
      if (use && Tn < 1e-4f) {
        done = true;
        use = false;
      }
      const float w = T * a;
      if (use) {
        const float4 rgb = s_rgb[k];
        c0 = c0 + w * rgb.x;
        c1 = c1 + w * rgb.y;
        c2 = c2 + w * rgb.z;
        T = Tn;
      }
      if (__ballot(use) != 0ull) {  // wave-uniform
        const uint32_t qv = use ? (uint32_t)rintf(w * 16777216.0f) : 0u;
        const uint32_t wb = use ? __float_as_uint(w) : 0u;
        const uint32_t sq = wave_sum_u32(qv), mw = wave_max_u32(wb);
        if ((t & 63u) == 0u) {
          atomicAdd(&s_sum[k], sq);
          atomicMax(&s_max[k], mw);
        }
      }
    }
    __syncthreads();
    if (j < end && s_sum[t] != 0u) {
      atomicAdd(p.weight_sum + gid, (unsigned long long)s_sum[t]);
      atomicMax(p.weight_max + gid, s_max[t]);
    }
  }
  if (inside && p.image) {
    float *o = p.image + ((unsigned long long)v * p.width + u) * 4u;
    o[0] = c0 + T * p.bg[0];
    o[1] = c1 + T * p.bg[1];
    o[2] = c2 + T * p.bg[2];
    o[3] = 1.0f - T;
  }
}

struct DepthParams {
  const spz_amd_render_record *rec;
  const uint32_t *sorted_gid;
  const uint2 *ranges;
  const unsigned long long *total;
  float *image;     // may be null
  float *depth;     // height x width x 2: accumulated depth, median depth
  uint32_t *index;  // may be null: the median Gaussian
  unsigned long long max_entries;
  uint32_t width, height, tiles_x;
  float bg[3];
};

namespace {

constexpr uint32_t kNoIndex = 0xffffffffu;

// One pixel's state in the depth blend: the blend kernel's T and colour, the depth sum D and the median taken so far.
struct DepthPixel {
  float T = 1.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, D = 0.0f, median = __builtin_huge_valf();
  uint32_t index = kNoIndex;
  // A used pair: weight w = T a, the colour and depth sums, T = Tn, and the first Gaussian to bring T under 0.5.
  __device__ __forceinline__ void use(float a, float Tn, const float4 &rgbz, uint32_t gid) {
    const float w = T * a;
    c0 = c0 + w * rgbz.x;
    c1 = c1 + w * rgbz.y;
    c2 = c2 + w * rgbz.z;
    D = D + w * rgbz.w;
    T = Tn;
    if (index == kNoIndex && Tn < 0.5f) {
      median = rgbz.w;
      index = gid;
    }
  }
};

}  // namespace

// The blend of spz_render_blend_kernel, pixel for pixel, plus each used pair's depth: s_rgb[k].w carries the record's
// depth z and s_gid[k] its Gaussian.  D += (T a) z; the first used Gaussian after which T < 0.5 is the pixel's median.
__global__ __launch_bounds__(kBlendThreads) void spz_render_depth_kernel(const DepthParams p) {
  __shared__ float2 s_xy[kBlendThreads];
  __shared__ float4 s_co[kBlendThreads];   // conic A, B, C, opacity
  __shared__ float4 s_rgb[kBlendThreads];  // rgb, depth
  __shared__ uint32_t s_gid[kBlendThreads];
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
  const float fu = (float)u, fv = (float)v;
  DepthPixel px;
  bool done = !inside;
  for (uint32_t base = begin; base < end; base += kBlendThreads) {
    // also the barrier between the previous batch's reads and this batch's writes
    if (__syncthreads_count(done ? 1 : 0) == (int)kBlendThreads) break;
    const uint32_t j = base + t;
    if (j < end) {
      const uint32_t gid = p.sorted_gid[j];
      const spz_amd_render_record &q = p.rec[gid];
      s_xy[t] = make_float2(q.mean[0], q.mean[1]);
      s_co[t] = make_float4(q.conic[0], q.conic[1], q.conic[2], q.opacity);
      s_rgb[t] = make_float4(q.rgb[0], q.rgb[1], q.rgb[2], q.depth);
      s_gid[t] = gid;
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
      const float Tn = px.T * (1.0f - a);
      if (Tn < 1e-4f) {
        done = true;
        break;
      }
      px.use(a, Tn, s_rgb[k], s_gid[k]);
    }
  }
  if (inside) {
    const unsigned long long at = (unsigned long long)v * p.width + u;
    p.depth[at * 2u] = px.D;
    p.depth[at * 2u + 1u] = px.median;
    if (p.index) p.index[at] = px.index;
    if (p.image) {
      float *o = p.image + at * 4u;
      o[0] = px.c0 + px.T * p.bg[0];
      o[1] = px.c1 + px.T * p.bg[1];
      o[2] = px.c2 + px.T * p.bg[2];
      o[3] = 1.0f - px.T;
    }
  }
}

}  // namespace spz_amd_detail

namespace {

using namespace spz_amd_detail;

// Preprocess, depth order and count scan into the prepare part at `base` (256-aligned).
template <class Src>
int prepare_impl(const Src &src, uint64_t n, int file_degree, int antialiased, const spz_amd_render_params *params,
                 uint64_t *d_total, spz_amd_render_record *d_records, uint8_t *base, hipStream_t st) {
  const RenderLayout wl = render_layout(n, 0);
  const RenderCam cam = make_cam(params, file_degree, antialiased);
  auto *rec = reinterpret_cast<spz_amd_render_record *>(base + wl.rec);
  auto *key = reinterpret_cast<float *>(base + wl.key);
  auto *count = reinterpret_cast<uint32_t *>(base + wl.count);
  auto *order = reinterpret_cast<uint32_t *>(base + wl.order);
  auto *run_sums = reinterpret_cast<unsigned long long *>(base + wl.run_sums);
  auto *total = reinterpret_cast<unsigned long long *>(base + wl.total);
  if (n) {
    hipLaunchKernelGGL(spz_render_preprocess_kernel<Src>, dim3((unsigned)((n + kPreBlock - 1) / kPreBlock)),
                       dim3(kPreBlock), 0, st, src, cam, (uint32_t)n, rec, key, count);
    SPZ_HIP_TRY(hipGetLastError());
    const int rc = spz_amd_argsort_f32_device(key, n, 0, order, base + wl.sort_n, st);
    if (rc != SPZ_AMD_OK) return rc;
    hipLaunchKernelGGL(spz_render_block_sums_kernel, dim3((unsigned)wl.runs), dim3(kScanBlock), 0, st, order, count,
                       (uint32_t)n, run_sums);
    SPZ_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(spz_render_scan_sums_kernel, dim3(1), dim3(kScanBlock), 0, st, run_sums, (uint32_t)wl.runs, total,
                     reinterpret_cast<unsigned long long *>(d_total));
  SPZ_HIP_TRY(hipGetLastError());
  if (d_records && n) {
    SPZ_HIP_TRY(hipMemcpyAsync(d_records, rec, n * sizeof(spz_amd_render_record), hipMemcpyDeviceToDevice, st));
  }
  return SPZ_AMD_OK;
}

// Tile entries, their sort by tile id and the tile ranges (base: the prepare part; ent: the entries part).
int entries_impl(uint64_t n, const spz_amd_render_params *params, uint64_t m, uint32_t *d_status, uint8_t *base,
                 uint8_t *ent, hipStream_t st) {
  const RenderLayout wl = render_layout(n, m);
  const uint32_t tiles_x = (params->width + kTile - 1) / kTile, tiles_y = (params->height + kTile - 1) / kTile;
  const uint64_t tiles = (uint64_t)tiles_x * tiles_y;
  SPZ_HIP_TRY(hipMemsetAsync(d_status, 0, sizeof(uint32_t), st));
  const auto *total = reinterpret_cast<const unsigned long long *>(base + wl.total);
  if (n == 0) return SPZ_AMD_OK;  // the total is 0
  EmitParams e = {};
  e.order = reinterpret_cast<const uint32_t *>(base + wl.order);
  e.tile_count = reinterpret_cast<const uint32_t *>(base + wl.count);
  e.rec = reinterpret_cast<const spz_amd_render_record *>(base + wl.rec);
  e.run_offsets = reinterpret_cast<const unsigned long long *>(base + wl.run_sums);
  e.total = total;
  e.status = d_status;
  e.max_entries = m;
  e.n = (uint32_t)n;
  e.tiles_x = tiles_x;
  if (m) {
    e.entry = reinterpret_cast<uint2 *>(ent + wl.entry);
    e.sort_key = reinterpret_cast<uint32_t *>(ent + wl.sort_m + wl.sl_m.planes_off[0][0]);
  }
  hipLaunchKernelGGL(spz_render_emit_kernel, dim3((unsigned)wl.runs), dim3(kScanBlock), 0, st, e);
  SPZ_HIP_TRY(hipGetLastError());
  if (m == 0) return SPZ_AMD_OK;
  uint2 *ranges = reinterpret_cast<uint2 *>(ent + wl.ranges);
  SPZ_HIP_TRY(hipMemsetAsync(ranges, 0, tiles * sizeof(uint2), st));
  const unsigned grid = (unsigned)std::min<uint64_t>((m + 255) / 256, 8192);
  hipLaunchKernelGGL(spz_render_pad_kernel, dim3(grid), dim3(256), 0, st, total, (uint32_t)m, e.sort_key);
  SPZ_HIP_TRY(hipGetLastError());
  const uint32_t digits = tiles <= 256u ? 1u : (tiles <= 65536u ? 2u : 3u);
  uint32_t *eorder = reinterpret_cast<uint32_t *>(ent + wl.eorder);
  const int rc = radix_passes((uint32_t)m, digits, eorder, ent + wl.sort_m, wl.sl_m, st);
  if (rc != SPZ_AMD_OK) return rc;
  hipLaunchKernelGGL(spz_render_ranges_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, total, (uint32_t)m,
                     eorder, e.entry, reinterpret_cast<uint32_t *>(ent + wl.sorted_gid), ranges);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

int blend_impl(uint64_t n, const spz_amd_render_params *params, uint64_t m, float *d_image, uint8_t *base, uint8_t *ent,
               hipStream_t st) {
  const RenderLayout wl = render_layout(n, m);
  BlendParams b = {};
  const dim3 grid = fill_blend_params(b, wl, base, ent, params, m);
  b.image = d_image;
  hipLaunchKernelGGL(spz_render_blend_kernel, grid, dim3(kBlendThreads), 0, st, b);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

int score_impl(uint64_t n, const spz_amd_render_params *params, uint64_t m, float *d_image, uint64_t *d_weight_sum,
               float *d_weight_max, uint8_t *base, uint8_t *ent, hipStream_t st) {
  const RenderLayout wl = render_layout(n, m);
  ScoreParams b = {};
  const dim3 grid = fill_blend_params(b, wl, base, ent, params, m);
  b.image = d_image;
  b.weight_sum = reinterpret_cast<unsigned long long *>(d_weight_sum);
  b.weight_max = reinterpret_cast<uint32_t *>(d_weight_max);
  hipLaunchKernelGGL(spz_render_score_kernel, grid, dim3(kBlendThreads), 0, st, b);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

int depth_impl(uint64_t n, const spz_amd_render_params *params, uint64_t m, float *d_image, float *d_depth,
               uint32_t *d_index, uint8_t *base, uint8_t *ent, hipStream_t st) {
  const RenderLayout wl = render_layout(n, m);
  DepthParams b = {};
  const dim3 grid = fill_blend_params(b, wl, base, ent, params, m);
  b.image = d_image;
  b.depth = d_depth;
  b.index = d_index;
  hipLaunchKernelGGL(spz_render_depth_kernel, grid, dim3(kBlendThreads), 0, st, b);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

int packed_source(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, int coord, PackedSrc *src) {
  spz_amd_layout lay;
  const int rc = check_packed_stream(d_stream, size, hdr, &lay);
  if (rc != SPZ_AMD_OK) return rc;
  if (hdr->num_points > kMaxEntries) return SPZ_AMD_ERR_TOO_MANY_POINTS;
  *src = PackedSrc{};
  src->positions = d_stream + lay.offset[SPZ_AMD_SEC_POSITIONS];
  src->alphas = d_stream + lay.offset[SPZ_AMD_SEC_ALPHAS];
  src->colors = d_stream + lay.offset[SPZ_AMD_SEC_COLORS];
  src->scales = d_stream + lay.offset[SPZ_AMD_SEC_SCALES];
  src->rotations = d_stream + lay.offset[SPZ_AMD_SEC_ROTATIONS];
  src->sh = d_stream + lay.offset[SPZ_AMD_SEC_SH];
  src->version = hdr->version;
  const int sd = sh_dim_for_degree(hdr->sh_degree);
  src->sh_dim = (uint32_t)sd;
  const FlipMasks fm = flip_masks(SPZ_AMD_RUB, coord);
  src->flip_p = fm.p;
  src->flip_q = fm.q;
  for (int k = 0; k < sd; ++k) {
    if ((fm.sh15 >> k) & 1u) src->sh_mask |= 7ull << (3 * k);
  }
  src->pos_scale = (float)(1.0 / (double)(int32_t)(1u << (hdr->fractional_bits & 31)));
  return SPZ_AMD_OK;
}

// What a host form returns: the image alone (the blend kernel), or depth maps with an optional index and image (the
// depth kernel).
struct HostOut {
  float *rgba = nullptr;
  float *depth = nullptr;
  uint32_t *index = nullptr;
};

// The host forms: prepare into a block of their own, read the total, then the entries and the blend into a second.
template <class Prepare>
int render_host_impl(uint64_t n, const spz_amd_render_params *params, int device, const HostOut &out, uint64_t *h_entries,
                     float *h_ms, uint64_t upload_bytes, const Prepare &prepare) {
  struct Blocks {
    hipStream_t st = nullptr;
    void *a = nullptr, *b = nullptr;
    ~Blocks() {
      if (st) (void)hipStreamSynchronize(st);
      if (a) (void)hipFree(a);
      if (b) (void)hipFree(b);
      if (st) (void)hipStreamDestroy(st);
    }
  };
  DeviceGuard guard;
  int rc = guard.enter(device);
  if (rc != SPZ_AMD_OK) return rc;
  Blocks k;
  SPZ_HIP_TRY(hipStreamCreateWithFlags(&k.st, hipStreamNonBlocking));
  const RenderLayout wp = render_layout(n, 0);
  const uint64_t small = 256;  // total (8) + status (4)
  SPZ_HIP_TRY(hipMalloc(&k.a, wp.bytes + small + al(upload_bytes)));
  uint8_t *base = align_ws(k.a);
  uint8_t *tail = base + wp.prefix;
  auto *d_total = reinterpret_cast<uint64_t *>(tail);
  auto *d_status = reinterpret_cast<uint32_t *>(tail + 8);
  uint8_t *upload = tail + small;
  auto t0 = std::chrono::steady_clock::now();
  rc = prepare(base, d_total, upload, k.st, &t0);  // uploads (if any), then sets t0 and enqueues the preprocess
  if (rc != SPZ_AMD_OK) return rc;
  uint64_t total = 0;
  SPZ_HIP_TRY(hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, k.st));
  SPZ_HIP_TRY(hipStreamSynchronize(k.st));
  const double t_pre = ms_since(t0);
  if (total > kMaxEntries) return SPZ_AMD_ERR_CAPACITY;
  const RenderLayout wf = render_layout(n, total);
  const uint64_t pixels = (uint64_t)params->width * params->height;
  const uint64_t image_bytes = out.rgba ? pixels * 16u : 0u, depth_bytes = out.depth ? pixels * 8u : 0u, index_bytes = out.index ? pixels * 4u : 0u;
  SPZ_HIP_TRY(hipMalloc(&k.b, wf.entries + al(image_bytes) + al(depth_bytes) + al(index_bytes) + 256));
  uint8_t *ent = align_ws(k.b);
  float *d_image = reinterpret_cast<float *>(ent + wf.entries);
  float *d_depth = reinterpret_cast<float *>(ent + wf.entries + al(image_bytes));
  uint32_t *d_index = reinterpret_cast<uint32_t *>(ent + wf.entries + al(image_bytes) + al(depth_bytes));
  const auto t1 = std::chrono::steady_clock::now();
  rc = entries_impl(n, params, total, d_status, base, ent, k.st);
  if (rc != SPZ_AMD_OK) return rc;
  SPZ_HIP_TRY(hipStreamSynchronize(k.st));
  const double t_ent = ms_since(t1);
  const auto t2 = std::chrono::steady_clock::now();
  rc = out.depth ? depth_impl(n, params, total, out.rgba ? d_image : nullptr, d_depth, out.index ? d_index : nullptr,
                              base, ent, k.st)
                 : blend_impl(n, params, total, d_image, base, ent, k.st);
  if (rc != SPZ_AMD_OK) return rc;
  SPZ_HIP_TRY(hipStreamSynchronize(k.st));
  const double t_blend = ms_since(t2);
  if (out.rgba) SPZ_HIP_TRY(hipMemcpyAsync(out.rgba, d_image, image_bytes, hipMemcpyDeviceToHost, k.st));
  if (out.depth) SPZ_HIP_TRY(hipMemcpyAsync(out.depth, d_depth, depth_bytes, hipMemcpyDeviceToHost, k.st));
  if (out.index) SPZ_HIP_TRY(hipMemcpyAsync(out.index, d_index, index_bytes, hipMemcpyDeviceToHost, k.st));
  SPZ_HIP_TRY(hipStreamSynchronize(k.st));
  if (h_entries) *h_entries = total;
  if (h_ms) {
    h_ms[0] = (float)t_pre;
    h_ms[1] = (float)t_ent;
    h_ms[2] = (float)t_blend;
  }
  return SPZ_AMD_OK;
}

// render_host and render_depth_host: a stream in device memory.  has_output: the form's required output is there.
int packed_host(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, const spz_amd_render_params *params,
                int device, const HostOut &out, bool has_output, uint64_t *h_entries, float *h_ms) {
  int rc = check_params(params);
  if (rc != SPZ_AMD_OK) return rc;
  PackedSrc src;
  rc = packed_source(d_stream, size, hdr, params->coord, &src);
  if (rc != SPZ_AMD_OK) return rc;
  if (!has_output) return SPZ_AMD_ERR_INVALID_ARG;
  return render_host_impl(hdr->num_points, params, device, out, h_entries, h_ms, 0,
                          [&](uint8_t *base, uint64_t *d_total, uint8_t *, hipStream_t st,
                              std::chrono::steady_clock::time_point *) -> int {
                            int r = ensure_tables(device, &src.tables);
                            if (r != SPZ_AMD_OK) return r;
                            return prepare_impl(src, hdr->num_points, hdr->sh_degree, hdr->flags & 1, params, d_total,
                                                nullptr, base, st);
                          });
}

// render_cloud_host and render_depth_cloud_host: a cloud in host memory, uploaded first.
int cloud_host(const spz_amd_cloud_in *h_cloud, uint64_t num_points, int sh_degree, int antialiased,
               const spz_amd_render_params *params, int device, const HostOut &out, bool has_output,
               uint64_t *h_entries, float *h_ms) {
  int rc = check_params(params);
  if (rc != SPZ_AMD_OK) return rc;
  FloatSrc hs;
  rc = cloud_source(h_cloud, num_points, sh_degree, &hs);
  if (rc != SPZ_AMD_OK) return rc;
  if (!has_output) return SPZ_AMD_ERR_INVALID_ARG;
  const uint64_t fpp[6] = {3, 3, 4, 1, 3, (uint64_t)hs.sh_dim * 3u};
  uint64_t upload = 0;
  for (int f = 0; f < 6; ++f) upload += al(num_points * fpp[f] * 4u);
  return render_host_impl(num_points, params, device, out, h_entries, h_ms, upload,
                          [&](uint8_t *base, uint64_t *d_total, uint8_t *up, hipStream_t st,
                              std::chrono::steady_clock::time_point *t0) -> int {
                            const float *hp[6] = {hs.positions, hs.scales, hs.rotations, hs.alphas, hs.colors, hs.sh};
                            float *dp[6];
                            uint8_t *q = up;
                            for (int f = 0; f < 6; ++f) {
                              dp[f] = reinterpret_cast<float *>(q);
                              const uint64_t bytes = num_points * fpp[f] * 4u;
                              if (bytes) SPZ_HIP_TRY(hipMemcpyAsync(dp[f], hp[f], bytes, hipMemcpyHostToDevice, st));
                              q += al(bytes);
                            }
                            SPZ_HIP_TRY(hipStreamSynchronize(st));
                            *t0 = std::chrono::steady_clock::now();
                            const FloatSrc ds{dp[0], dp[1], dp[2], dp[3], dp[4], dp[5], hs.sh_dim};
                            return prepare_impl(ds, num_points, sh_degree, antialiased, params, d_total, nullptr,
                                                base, st);
                          });
}

}  // namespace

extern "C" {

int spz_amd_render_check_params(const spz_amd_render_params *params) { return check_params(params); }

uint64_t spz_amd_render_workspace_bytes(uint64_t num_points, uint64_t max_entries) {
  return render_layout(num_points, max_entries).bytes;
}

int spz_amd_render_prepare_packed_device(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr,
                                         const spz_amd_render_params *params, uint64_t *d_total,
                                         spz_amd_render_record *d_records, void *d_workspace, void *hip_stream) {
  int rc = check_params(params);
  if (rc != SPZ_AMD_OK) return rc;
  PackedSrc src;
  rc = packed_source(d_stream, size, hdr, params->coord, &src);
  if (rc != SPZ_AMD_OK) return rc;
  if (d_total == nullptr || d_workspace == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  rc = ensure_tables(device, &src.tables);
  if (rc != SPZ_AMD_OK) return rc;
  return prepare_impl(src, hdr->num_points, hdr->sh_degree, hdr->flags & 1, params, d_total, d_records,
                      align_ws(d_workspace), static_cast<hipStream_t>(hip_stream));
}

int spz_amd_render_prepare_cloud_device(const spz_amd_cloud_in *d_cloud, uint64_t num_points, int sh_degree,
                                        int antialiased, const spz_amd_render_params *params, uint64_t *d_total,
                                        spz_amd_render_record *d_records, void *d_workspace, void *hip_stream) {
  int rc = check_params(params);
  if (rc != SPZ_AMD_OK) return rc;
  FloatSrc src;
  rc = cloud_source(d_cloud, num_points, sh_degree, &src);
  if (rc != SPZ_AMD_OK) return rc;
  if (d_total == nullptr || d_workspace == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  return prepare_impl(src, num_points, sh_degree, antialiased, params, d_total, d_records, align_ws(d_workspace),
                      static_cast<hipStream_t>(hip_stream));
}

int spz_amd_render_finish_device(uint64_t num_points, const spz_amd_render_params *params, uint64_t max_entries,
                                 float *d_image, uint32_t *d_status, void *d_workspace, void *hip_stream) {
  int rc = check_params(params);
  if (rc != SPZ_AMD_OK) return rc;
  if (num_points > kMaxEntries || max_entries > kMaxEntries) return SPZ_AMD_ERR_INVALID_ARG;
  if (d_image == nullptr || d_status == nullptr || d_workspace == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  const hipStream_t st = static_cast<hipStream_t>(hip_stream);
  uint8_t *base = align_ws(d_workspace);
  uint8_t *ent = base + render_layout(num_points, 0).prefix;
  rc = entries_impl(num_points, params, max_entries, d_status, base, ent, st);
  if (rc != SPZ_AMD_OK) return rc;
  return blend_impl(num_points, params, max_entries, d_image, base, ent, st);
}

int spz_amd_render_score_device(uint64_t num_points, const spz_amd_render_params *params, uint64_t max_entries,
                                float *d_image, uint64_t *d_weight_sum, float *d_weight_max, uint32_t *d_status,
                                void *d_workspace, void *hip_stream) {
  int rc = check_params(params);
  if (rc != SPZ_AMD_OK) return rc;
  if (num_points > kMaxEntries || max_entries > kMaxEntries) return SPZ_AMD_ERR_INVALID_ARG;
  if (d_status == nullptr || d_workspace == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  if (num_points && (d_weight_sum == nullptr || d_weight_max == nullptr)) return SPZ_AMD_ERR_INVALID_ARG;
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  const hipStream_t st = static_cast<hipStream_t>(hip_stream);
  uint8_t *base = align_ws(d_workspace);
  uint8_t *ent = base + render_layout(num_points, 0).prefix;
  rc = entries_impl(num_points, params, max_entries, d_status, base, ent, st);
  if (rc != SPZ_AMD_OK) return rc;
  return score_impl(num_points, params, max_entries, d_image, d_weight_sum, d_weight_max, base, ent, st);
}

int spz_amd_render_host(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr,
                        const spz_amd_render_params *params, int device, float *h_rgba, uint64_t *h_entries,
                        float *h_ms) {
  HostOut out;
  out.rgba = h_rgba;
  return packed_host(d_stream, size, hdr, params, device, out, h_rgba != nullptr, h_entries, h_ms);
}

int spz_amd_render_cloud_host(const spz_amd_cloud_in *h_cloud, uint64_t num_points, int sh_degree, int antialiased,
                              const spz_amd_render_params *params, int device, float *h_rgba, uint64_t *h_entries,
                              float *h_ms) {
  HostOut out;
  out.rgba = h_rgba;
  return cloud_host(h_cloud, num_points, sh_degree, antialiased, params, device, out, h_rgba != nullptr, h_entries, h_ms);
}

int spz_amd_render_depth_device(uint64_t num_points, const spz_amd_render_params *params, uint64_t max_entries,
                                float *d_image, float *d_depth, uint32_t *d_index, uint32_t *d_status,
                                void *d_workspace, void *hip_stream) {
  int rc = check_params(params);
  if (rc != SPZ_AMD_OK) return rc;
  if (num_points > kMaxEntries) return SPZ_AMD_ERR_INVALID_ARG;
  if (d_depth == nullptr || d_status == nullptr || d_workspace == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  if (max_entries > kMaxEntries) return SPZ_AMD_ERR_CAPACITY;
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  const hipStream_t st = static_cast<hipStream_t>(hip_stream);
  uint8_t *base = align_ws(d_workspace);
  uint8_t *ent = base + render_layout(num_points, 0).prefix;
  rc = entries_impl(num_points, params, max_entries, d_status, base, ent, st);
  if (rc != SPZ_AMD_OK) return rc;
  return depth_impl(num_points, params, max_entries, d_image, d_depth, d_index, base, ent, st);
}

int spz_amd_render_depth_host(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr,
                              const spz_amd_render_params *params, int device, float *h_rgba, float *h_depth,
                              uint32_t *h_index, uint64_t *h_entries, float *h_ms) {
  HostOut out;
  out.rgba = h_rgba;
  out.depth = h_depth;
  out.index = h_index;
  return packed_host(d_stream, size, hdr, params, device, out, h_depth != nullptr, h_entries, h_ms);
}

int spz_amd_render_depth_cloud_host(const spz_amd_cloud_in *h_cloud, uint64_t num_points, int sh_degree,
                                    int antialiased, const spz_amd_render_params *params, int device, float *h_rgba,
                                    float *h_depth, uint32_t *h_index, uint64_t *h_entries, float *h_ms) {
  HostOut out;
  out.rgba = h_rgba;
  out.depth = h_depth;
  out.index = h_index;
  return cloud_host(h_cloud, num_points, sh_degree, antialiased, params, device, out, h_depth != nullptr, h_entries,
                    h_ms);
}

}  // extern "C"
