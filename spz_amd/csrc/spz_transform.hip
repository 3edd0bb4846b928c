// spz_transform.hip — place a scene: p -> s*R*p + t with the rotation applied to the quaternions and to the sh bands
// (DESIGN "Transform").  Two kernels over one parameter block (spz_amd_transform, built on the host in double by
// spz_amd_transform_params):
//
//   spz_transform_cloud_kernel   in place on a resident float cloud, one point per thread.
//   spz_transform_packed_kernel  packed stream -> v3 stream in one pass.  A flat tile list over the OUTPUT sections, as in
//                                spz_subset_kernel: positions / scales / rotations decode with the decoder's code
//                                (decode_position_axis, scale_from_byte, unpack_quat_*), are transformed and re-encoded
//                                with the encoder's (position_fixed, scale_to_byte_f, pack_quat_smallest_three); alpha
//                                and colour tiles (and scales when s == 1) are byte copies; sh tiles stage 256 point
//                                records through LDS so that the global loads and stores stay lane-contiguous, and each
//                                thread rotates one record (sh_from_byte, quantize_sh_f).  Positions whose new value
//                                does not fit the 24-bit field are counted: a ballot per wave, one atomic per wave.
// The per-point arithmetic and the packed point cores live in spz_xf.hpp, shared with spz_merge.hip.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "spz_amd.h"
#include "spz_common.hpp"
#include "spz_kernel_params.hpp"
#include "spz_quant.hpp"
#include "spz_xf.hpp"

#pragma clang fp contract(off)

namespace spz_amd_detail {
namespace {

constexpr uint32_t kXfBlock = 256;                 // threads; point tiles hold one point per thread
constexpr uint32_t kCopyUnroll = 4;
constexpr uint32_t kCopyTileBytes = kXfBlock * kCopyUnroll * 4u;
constexpr uint32_t kMaxShBytes = 45;               // 3 * 15 at degree 3
constexpr uint32_t kMagic = 0x5053474eu;           // load-spz.cc:132

enum XfKind : uint32_t { XF_POS = 0, XF_COPY, XF_SCALE, XF_ROT, XF_SH };

struct XfSec {
  const uint8_t *src;
  uint8_t *dst;
  unsigned long long bytes;   // output bytes of the section
  uint32_t kind;
  uint32_t tile_begin;
};

struct PackedXfParams {
  XfSec sec[SPZ_AMD_NUM_SECTIONS];
  uint32_t n_sec;
  uint32_t total_tiles;
  uint32_t num_points;
  uint32_t version;            // of the input
  uint32_t sh_bytes;           // 3 * dim of the (shared) degree
  float in_pos_scale;          // 1 / (1 << input fractionalBits)
  float out_pos_scale;         // 1 << fractional_bits
  unsigned long long *out_of_range;
  uint8_t *header_dst;
  uint32_t header_words[4];
  spz_amd_transform xf;
};

struct CloudXfParams {
  float *positions, *scales, *rotations, *sh;
  unsigned long long num_points;
  uint32_t sh_dim;
  spz_amd_transform xf;
};

// ---- packed tiles ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void copy_tile(const XfSec &q, uint32_t tl, bool scale, float ln_s) {
  const unsigned long long base = (unsigned long long)tl * kCopyTileBytes;
#pragma unroll
  for (uint32_t r = 0; r < kCopyUnroll; ++r) {
    const unsigned long long b0 = base + ((unsigned long long)r * kXfBlock + threadIdx.x) * 4ull;
    if (b0 >= q.bytes) break;
    const uint32_t n = (q.bytes - b0) < 4ull ? (uint32_t)(q.bytes - b0) : 4u;
    uint32_t w = 0;
    if (n == 4u) {
      w = *reinterpret_cast<const u32_a1 *>(q.src + b0);  // unaligned dword (section bases land on any byte)
    } else {
      for (uint32_t j = 0; j < n; ++j) w |= (uint32_t)q.src[b0 + j] << (8u * j);
    }
    if (scale) w = xf_scale_bytes(w, ln_s);
    if (n == 4u) {
      *reinterpret_cast<u32_a1 *>(q.dst + b0) = w;
    } else {
      for (uint32_t j = 0; j < n; ++j) q.dst[b0 + j] = (uint8_t)(w >> (8u * j));
    }
  }
}

__device__ __forceinline__ void position_tile(const PackedXfParams &p, const XfSec &q, uint32_t tl) {
  const unsigned long long i = (unsigned long long)tl * kXfBlock + threadIdx.x;
  const bool bad = i < p.num_points &&
                   xf_position_point(q.src, i, p.version == 1u, p.in_pos_scale, &p.xf, p.out_pos_scale, q.dst + i * 9ull);
  const unsigned long long ballot = __ballot(bad);
  if ((threadIdx.x & 63u) == 0u && ballot != 0ull && p.out_of_range != nullptr) {
    atomicAdd(p.out_of_range, (unsigned long long)__popcll(ballot));
  }
}

__device__ __forceinline__ void rotation_tile(const PackedXfParams &p, const XfSec &q, uint32_t tl) {
  const unsigned long long i = (unsigned long long)tl * kXfBlock + threadIdx.x;
  if (i >= p.num_points) return;
  *reinterpret_cast<u32_a1 *>(q.dst + i * 4ull) = xf_rotation_point(q.src, i, p.version, &p.xf);
}

// 256 records through LDS: coalesced dword loads of the tile's bytes, one record per thread, coalesced dword stores.
__device__ __forceinline__ void sh_tile(const PackedXfParams &p, const XfSec &q, uint32_t tl, uint8_t *lds) {
  const uint32_t rec = p.sh_bytes, dim = rec / 3u;
  const unsigned long long first = (unsigned long long)tl * kXfBlock;
  const unsigned long long left = p.num_points - first;
  const uint32_t pts = left < kXfBlock ? (uint32_t)left : kXfBlock;
  const uint32_t bytes = pts * rec;
  const uint8_t *src = q.src + first * rec;
  uint8_t *dst = q.dst + first * rec;
  for (uint32_t b = threadIdx.x * 4u; b < bytes; b += kXfBlock * 4u) {
    if (b + 4u <= bytes) {
      *reinterpret_cast<uint32_t *>(lds + b) = *reinterpret_cast<const u32_a1 *>(src + b);
    } else {
      for (uint32_t j = b; j < bytes; ++j) lds[j] = src[j];
    }
  }
  __syncthreads();
  if (threadIdx.x < pts) xf_sh_record(lds + threadIdx.x * rec, dim, dim, &p.xf);
  __syncthreads();
  for (uint32_t b = threadIdx.x * 4u; b < bytes; b += kXfBlock * 4u) {
    if (b + 4u <= bytes) {
      *reinterpret_cast<u32_a1 *>(dst + b) = *reinterpret_cast<const uint32_t *>(lds + b);
    } else {
      for (uint32_t j = b; j < bytes; ++j) dst[j] = lds[j];
    }
  }
}

}  // namespace

__global__ __launch_bounds__(kXfBlock) void spz_transform_packed_kernel(const PackedXfParams p) {
  __shared__ uint32_t lds_words[kXfBlock * kMaxShBytes / 4u];
  const uint32_t tile = blockIdx.x;
  if (tile == 0 && threadIdx.x < 16 && p.header_dst != nullptr) {
    p.header_dst[threadIdx.x] = (uint8_t)(p.header_words[threadIdx.x >> 2] >> ((threadIdx.x & 3u) * 8u));
  }
  if (tile >= p.total_tiles) return;
  uint32_t si = 0;
  for (uint32_t s = 1; s < p.n_sec; ++s) si = (tile >= p.sec[s].tile_begin) ? s : si;
  const XfSec &q = p.sec[si];
  const uint32_t tl = tile - q.tile_begin;
  switch (q.kind) {
    case XF_POS: position_tile(p, q, tl); break;
    case XF_COPY: copy_tile(q, tl, false, 0.0f); break;
    case XF_SCALE: copy_tile(q, tl, true, p.xf.ln_s); break;
    case XF_ROT: rotation_tile(p, q, tl); break;
    case XF_SH: sh_tile(p, q, tl, reinterpret_cast<uint8_t *>(lds_words)); break;
    default: break;
  }
}

__global__ __launch_bounds__(kXfBlock) void spz_transform_cloud_kernel(const CloudXfParams p) {
  const unsigned long long stride = (unsigned long long)gridDim.x * kXfBlock;
  for (unsigned long long i = (unsigned long long)blockIdx.x * kXfBlock + threadIdx.x; i < p.num_points; i += stride) {
    if (p.positions != nullptr && p.xf.apply_positions) {
      float *q = p.positions + i * 3ull;
      float v[3] = {q[0], q[1], q[2]};
      xf_position(p.xf, v);
      q[0] = v[0];
      q[1] = v[1];
      q[2] = v[2];
    }
    if (p.scales != nullptr && p.xf.apply_scales) {
      float *q = p.scales + i * 3ull;
      q[0] = fadd_sep(q[0], p.xf.ln_s);
      q[1] = fadd_sep(q[1], p.xf.ln_s);
      q[2] = fadd_sep(q[2], p.xf.ln_s);
    }
    if (p.rotations != nullptr && p.xf.apply_rotation) {
      F32x4 *q = reinterpret_cast<F32x4 *>(p.rotations + i * 4ull);
      *q = xf_rotation(p.xf, *q);
    }
    if (p.sh != nullptr && p.sh_dim > 0 && p.xf.apply_rotation) {
      float *r = p.sh + i * (3ull * p.sh_dim);
      for (uint32_t c = 0; c < 3; ++c) {
        float in[15], out[15];
#pragma unroll
        for (uint32_t k = 0; k < 15; ++k) in[k] = k < p.sh_dim ? r[3 * k + c] : 0.0f;
        xf_sh_channel(p.xf, p.sh_dim, in, out);
#pragma unroll
        for (uint32_t k = 0; k < 15; ++k) {
          if (k < p.sh_dim) r[3 * k + c] = out[k];
        }
      }
    }
  }
}

}  // namespace spz_amd_detail

namespace {

using namespace spz_amd_detail;

// ---- the parameter block, in double --------------------------------------------------------------------------------
double snap(double v) {
  if (std::fabs(v) < 1e-12) return 0.0;
  if (std::fabs(v - 1.0) < 1e-12) return 1.0;
  if (std::fabs(v + 1.0) < 1e-12) return -1.0;
  return v;
}

// The real-SH basis the 3DGS rasteriser evaluates (bands 1..3, its constants and signs), at the unit vector d.
void sh_basis(const double d[3], double y[15]) {
  const double x = d[0], yy = d[1], z = d[2];
  const double C1 = 0.4886025119029199;
  const double C2[5] = {1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396};
  const double C3[7] = {-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154,
                        -0.4570457994644658, 1.445305721320277, -0.5900435899266435};
  const double xx = x * x, y2 = yy * yy, zz = z * z;
  y[0] = -C1 * yy;
  y[1] = C1 * z;
  y[2] = -C1 * x;
  y[3] = C2[0] * x * yy;
  y[4] = C2[1] * yy * z;
  y[5] = C2[2] * (2.0 * zz - xx - y2);
  y[6] = C2[3] * x * z;
  y[7] = C2[4] * (xx - y2);
  y[8] = C3[0] * yy * (3.0 * xx - y2);
  y[9] = C3[1] * x * yy * z;
  y[10] = C3[2] * yy * (4.0 * zz - xx - y2);
  y[11] = C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * y2);
  y[12] = C3[4] * x * (4.0 * zz - xx - y2);
  y[13] = C3[5] * z * (xx - y2);
  y[14] = C3[6] * x * (xx - 3.0 * y2);
}

// D_l[k][m] = sum_q w_q Y_k(R^T d_q) Y_m(d_q) over 4-node Gauss-Legendre in cos(theta) x 8 equally spaced phi: exact for
// the degree-6 products of two bands <= 3, no linear solve.
void sh_rotation(const double R[3][3], double D[15][15]) {
  const double u[4] = {-0.8611363115940526, -0.3399810435848563, 0.3399810435848563, 0.8611363115940526};
  const double wu[4] = {0.3478548451374538, 0.6521451548625461, 0.6521451548625461, 0.3478548451374538};
  const double kPi = 3.14159265358979323846;
  for (int k = 0; k < 15; ++k)
    for (int m = 0; m < 15; ++m) D[k][m] = 0.0;
  for (int i = 0; i < 4; ++i) {
    const double st = std::sqrt(1.0 - u[i] * u[i]);
    for (int j = 0; j < 8; ++j) {
      const double phi = 2.0 * kPi * j / 8.0;
      const double d[3] = {st * std::cos(phi), st * std::sin(phi), u[i]};
      double rd[3];
      for (int a = 0; a < 3; ++a) rd[a] = R[0][a] * d[0] + R[1][a] * d[1] + R[2][a] * d[2];  // R^T d
      double yr[15], yd[15];
      sh_basis(rd, yr);
      sh_basis(d, yd);
      const double w = wu[i] * (2.0 * kPi / 8.0);
      for (int k = 0; k < 15; ++k)
        for (int m = 0; m < 15; ++m) D[k][m] += w * yr[k] * yd[m];
    }
  }
}

int transform_params(const double *rotation, const double *translation, double scale, int coord, spz_amd_transform *out) {
  if (out == nullptr || !valid_coord(coord)) return SPZ_AMD_ERR_INVALID_ARG;
  double q[4] = {0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0};
  if (rotation) std::memcpy(q, rotation, sizeof(q));
  if (translation) std::memcpy(t, translation, sizeof(t));
  double n2 = 0.0;
  for (double v : q) {
    if (!std::isfinite(v)) return SPZ_AMD_ERR_INVALID_ARG;
    n2 += v * v;
  }
  for (double v : t) {
    if (!std::isfinite(v) || !std::isfinite((float)v)) return SPZ_AMD_ERR_INVALID_ARG;
  }
  const float s32 = (float)scale;
  if (!std::isfinite(scale) || !(scale > 0.0) || !std::isfinite(s32) || !(s32 > 0.0f)) return SPZ_AMD_ERR_INVALID_ARG;
  const double norm = std::sqrt(n2);
  if (!(norm > 0.0) || !std::isfinite(norm)) return SPZ_AMD_ERR_INVALID_ARG;
  // into RUB: R = F R_c F, t = F t_c; the quaternion's vector part is an axial vector: det(F) F v
  const uint32_t fp = flip_masks(coord, SPZ_AMD_RUB).p;
  double f[3];
  for (int a = 0; a < 3; ++a) f[a] = ((fp >> a) & 1u) ? -1.0 : 1.0;
  const double det = f[0] * f[1] * f[2];
  double x = det * f[0] * q[0] / norm, y = det * f[1] * q[1] / norm, z = det * f[2] * q[2] / norm, w = q[3] / norm;
  if (w < 0.0) {  // q and -q are one rotation; w >= 0 makes the identity (0, 0, 0, 1)
    x = -x; y = -y; z = -z; w = -w;
  }
  double R[3][3] = {{1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w)},
                    {2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w)},
                    {2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)}};
  bool identity = true;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) {
      R[i][j] = snap(R[i][j]);
      identity = identity && R[i][j] == (i == j ? 1.0 : 0.0);
    }
  }
  double qr[4] = {snap(x), snap(y), snap(z), snap(w)};
  if (identity) qr[0] = qr[1] = qr[2] = 0.0, qr[3] = 1.0;
  double D[15][15];
  sh_rotation(R, D);
  spz_amd_transform o = {};
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) o.m[3 * i + j] = (float)(scale * R[i][j]);
    o.t[i] = (float)(f[i] * t[i]);
  }
  o.ln_s = (float)std::log(scale);
  for (int i = 0; i < 4; ++i) o.q[i] = (float)qr[i];
  for (int k = 0; k < 3; ++k)
    for (int m = 0; m < 3; ++m) o.d1[3 * k + m] = (float)snap(D[k][m]);
  for (int k = 0; k < 5; ++k)
    for (int m = 0; m < 5; ++m) o.d2[5 * k + m] = (float)snap(D[3 + k][3 + m]);
  for (int k = 0; k < 7; ++k)
    for (int m = 0; m < 7; ++m) o.d3[7 * k + m] = (float)snap(D[8 + k][8 + m]);
  o.apply_rotation = identity ? 0 : 1;
  o.apply_scales = scale != 1.0 ? 1 : 0;
  o.apply_positions = (identity && scale == 1.0 && o.t[0] == 0.0f && o.t[1] == 0.0f && o.t[2] == 0.0f) ? 0 : 1;
  *out = o;
  return SPZ_AMD_OK;
}

int packed_impl(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, const spz_amd_transform *xf, int fb,
                uint8_t *d_out, size_t capacity, uint64_t *d_out_of_range, void *hip_stream) {
  if (d_stream == nullptr || hdr == nullptr || xf == nullptr || d_out == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  if (fb < 0 || fb > 24) return SPZ_AMD_ERR_INVALID_ARG;
  if (hdr->version < 1 || hdr->version > 3) return SPZ_AMD_ERR_VERSION;
  if (hdr->sh_degree > 3) return SPZ_AMD_ERR_SH_DEGREE;
  spz_amd_layout in, out;
  int rc = spz_amd_stream_layout(hdr->num_points, hdr->sh_degree, (int)hdr->version, &in);
  if (rc != SPZ_AMD_OK) return rc;
  if (size < in.total_bytes) return SPZ_AMD_ERR_SHORT_STREAM;
  rc = spz_amd_stream_layout(hdr->num_points, hdr->sh_degree, 3, &out);
  if (rc != SPZ_AMD_OK) return rc;
  if (capacity < out.total_bytes) return SPZ_AMD_ERR_CAPACITY;
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  if (d_out_of_range) SPZ_HIP_TRY(hipMemsetAsync(d_out_of_range, 0, sizeof(uint64_t), st));
  PackedXfParams p = {};
  p.num_points = hdr->num_points;
  p.version = hdr->version;
  p.sh_bytes = out.bytes_per_point[SPZ_AMD_SEC_SH];
  // float scale = 1.0 / (1 << fractionalBits) (load-spz.cc:495); x86 masks the shift count to 5 bits
  p.in_pos_scale = (float)(1.0 / (double)(int32_t)(1u << (hdr->fractional_bits & 31)));
  p.out_pos_scale = (float)(1u << fb);
  p.out_of_range = reinterpret_cast<unsigned long long *>(d_out_of_range);
  p.xf = *xf;
  const uint64_t n = hdr->num_points;
  const uint64_t point_tiles = (n + kXfBlock - 1) / kXfBlock;
  // largest sections first, so that the tail of the grid is made of the small ones
  const int order[SPZ_AMD_NUM_SECTIONS] = {SPZ_AMD_SEC_SH, SPZ_AMD_SEC_POSITIONS, SPZ_AMD_SEC_ROTATIONS,
                                           SPZ_AMD_SEC_SCALES, SPZ_AMD_SEC_COLORS, SPZ_AMD_SEC_ALPHAS};
  unsigned long long tiles = 0;
  for (int s : order) {
    if (out.bytes[s] == 0) continue;
    XfSec &q = p.sec[p.n_sec++];
    q.src = d_stream + in.offset[s];
    q.dst = d_out + out.offset[s];
    q.bytes = out.bytes[s];
    q.tile_begin = (uint32_t)tiles;
    bool per_point = true;
    if (s == SPZ_AMD_SEC_POSITIONS) q.kind = XF_POS;
    else if (s == SPZ_AMD_SEC_ROTATIONS) q.kind = XF_ROT;
    else if (s == SPZ_AMD_SEC_SH) q.kind = XF_SH;
    else {
      q.kind = (s == SPZ_AMD_SEC_SCALES && xf->apply_scales) ? XF_SCALE : XF_COPY;
      per_point = false;
    }
    tiles += per_point ? point_tiles : (out.bytes[s] + kCopyTileBytes - 1) / kCopyTileBytes;
  }
  if (tiles > 0x7fffffffull) return SPZ_AMD_ERR_INVALID_ARG;
  p.total_tiles = (uint32_t)tiles;
  p.header_dst = d_out;
  p.header_words[0] = kMagic;
  p.header_words[1] = 3u;
  p.header_words[2] = hdr->num_points;
  p.header_words[3] = (uint32_t)hdr->sh_degree | ((uint32_t)fb << 8) | ((uint32_t)(hdr->flags & 1u) << 16);
  hipLaunchKernelGGL(spz_transform_packed_kernel, dim3(p.total_tiles > 0 ? p.total_tiles : 1u), dim3(kXfBlock), 0, st, p);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

int cloud_impl(float *pos, float *scales, float *rot, float *sh, uint64_t n, int sh_degree, const spz_amd_transform *xf,
               hipStream_t st) {
  const int sd = sh_dim_for_degree(sh_degree);
  if (sd < 0 || xf == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  if (n == 0) return SPZ_AMD_OK;
  CloudXfParams p = {};
  p.positions = pos;
  p.scales = scales;
  p.rotations = rot;
  p.sh = sd > 0 ? sh : nullptr;
  p.num_points = n;
  p.sh_dim = (uint32_t)sd;
  p.xf = *xf;
  const uint64_t blocks = (n + kXfBlock - 1) / kXfBlock;
  hipLaunchKernelGGL(spz_transform_cloud_kernel, dim3((unsigned)(blocks < 0x7fffffffull ? blocks : 0x7fffffffull)),
                     dim3(kXfBlock), 0, st, p);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

}  // namespace

extern "C" {

int spz_amd_transform_params(const double rotation[4], const double translation[3], double scale, int coord,
                             spz_amd_transform *out) {
  return transform_params(rotation, translation, scale, coord, out);
}

int spz_amd_transform_cloud_device(float *d_positions, float *d_scales, float *d_rotations, float *d_sh,
                                   uint64_t num_points, int sh_degree, const spz_amd_transform *xf, void *hip_stream) {
  if (num_points > 0) {
    int device = 0;
    const int rc = current_device(&device);
    if (rc != SPZ_AMD_OK) return rc;
  }
  return cloud_impl(d_positions, d_scales, d_rotations, d_sh, num_points, sh_degree, xf, static_cast<hipStream_t>(hip_stream));
}

int spz_amd_transform_packed_device(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr,
                                    const spz_amd_transform *xf, int fractional_bits, uint8_t *d_out, size_t capacity,
                                    uint64_t *d_out_of_range, void *hip_stream) {
  return packed_impl(d_stream, size, hdr, xf, fractional_bits, d_out, capacity, d_out_of_range, hip_stream);
}

int spz_amd_transform_open(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, const spz_amd_transform *xf,
                           int fractional_bits, int device, void **ctx, uint64_t *h_out_bytes, uint64_t *h_out_of_range,
                           float *h_ms) {
  if (ctx == nullptr || h_out_bytes == nullptr || h_out_of_range == nullptr || hdr == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  *ctx = nullptr;
  *h_out_bytes = 0;
  *h_out_of_range = 0;
  spz_amd_layout out;
  int rc = spz_amd_stream_layout(hdr->num_points, hdr->sh_degree, 3, &out);
  if (rc != SPZ_AMD_OK) return rc;
  DeviceGuard guard;
  rc = guard.enter(device);
  if (rc != SPZ_AMD_OK) return rc;
  PackedResultPtr c;
  rc = packed_result_open(device, &c);
  if (rc != SPZ_AMD_OK) return rc;
  const size_t stream_bytes = Workspace::aligned(out.total_bytes);
  SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&c->block), stream_bytes + 256));
  c->out = c->block;
  uint64_t *d_count = reinterpret_cast<uint64_t *>(c->block + stream_bytes);
  const auto t0 = std::chrono::steady_clock::now();
  rc = packed_impl(d_stream, size, hdr, xf, fractional_bits, c->out, out.total_bytes, d_count, c->st);
  if (rc != SPZ_AMD_OK) return rc;
  uint64_t h = 0;
  SPZ_HIP_TRY(hipMemcpyAsync(&h, d_count, sizeof(h), hipMemcpyDeviceToHost, c->st));
  SPZ_HIP_TRY(hipStreamSynchronize(c->st));
  if (h_ms) h_ms[0] = (float)ms_since(t0);
  c->out_bytes = out.total_bytes;
  *h_out_bytes = out.total_bytes;
  *h_out_of_range = h;
  *ctx = c.release();
  return SPZ_AMD_OK;
}

int spz_amd_transform_fetch(void *ctx, uint8_t *h_out) { return packed_result_fetch(ctx, h_out); }

const uint8_t *spz_amd_transform_device_data(void *ctx) { return packed_result_device_data(ctx); }

void spz_amd_transform_close(void *ctx) { packed_result_close(ctx); }

int spz_amd_transform_cloud_host(float *h_positions, float *h_scales, float *h_rotations, float *h_sh,
                                 uint64_t num_points, int sh_degree, const spz_amd_transform *xf, int device) {
  const int sd = sh_dim_for_degree(sh_degree);
  if (sd < 0 || xf == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  if (num_points == 0) return SPZ_AMD_OK;
  DeviceGuard guard;
  int rc = guard.enter(device);
  if (rc != SPZ_AMD_OK) return rc;
  const size_t fpp[4] = {3, 3, 4, (size_t)sd * 3};  // floats per point: positions, scales, rotations, sh
  float *hp[4] = {h_positions, h_scales, h_rotations, h_sh};
  size_t total = 0;
  for (int i = 0; i < 4; ++i) {
    if (hp[i] && fpp[i]) total += Workspace::aligned(num_points * fpp[i] * sizeof(float));
  }
  if (total == 0) return SPZ_AMD_OK;
  Workspace ws;
  rc = ws.open(device, total);
  if (rc != SPZ_AMD_OK) return rc;
  float *b[4] = {nullptr, nullptr, nullptr, nullptr};
  hipStream_t st = ws.pipe()->up;
  for (int i = 0; i < 4; ++i) {
    if (!hp[i] || !fpp[i]) continue;
    b[i] = static_cast<float *>(ws.take(num_points * fpp[i] * sizeof(float)));
    SPZ_HIP_TRY(hipMemcpyAsync(b[i], hp[i], num_points * fpp[i] * sizeof(float), hipMemcpyHostToDevice, st));
  }
  rc = cloud_impl(b[0], b[1], b[2], b[3], num_points, sh_degree, xf, st);
  if (rc != SPZ_AMD_OK) return rc;
  for (int i = 0; i < 4; ++i) {
    if (b[i]) SPZ_HIP_TRY(hipMemcpyAsync(hp[i], b[i], num_points * fpp[i] * sizeof(float), hipMemcpyDeviceToHost, st));
  }
  SPZ_HIP_TRY(hipStreamSynchronize(st));
  return SPZ_AMD_OK;
}

}  // extern "C"
