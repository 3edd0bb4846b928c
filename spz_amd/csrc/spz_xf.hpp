// spz_xf.hpp — the per-point arithmetic of a placement (DESIGN "Transform"): p -> s*R*p + t, l -> l + ln s,
// q -> q_R * q and the sh bands rotated with D1..D3, over the f32 parameter block of spz_amd_transform_params, and the
// packed-domain point cores built on it (decode with the decoder's code, place, encode with the encoder's).  Shared by
// spz_transform.hip (one stream -> one stream) and spz_merge.hip (K streams -> one stream), so that a placed input of
// a merge gets the bytes the transform gives it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "spz_amd.h"
#include "spz_common.hpp"
#include "spz_kernel_params.hpp"
#include "spz_quant.hpp"

#pragma clang fp contract(off)

namespace spz_amd_detail {
namespace {

typedef uint32_t u32_a1 __attribute__((aligned(1)));

// ---- the per-point arithmetic (every product and sum rounded on its own) ----------------------------------------
__device__ __forceinline__ void xf_position(const spz_amd_transform &x, float v[3]) {
  float o[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float s = fadd_sep(fadd_sep(fmul_sep(x.m[3 * i], v[0]), fmul_sep(x.m[3 * i + 1], v[1])), fmul_sep(x.m[3 * i + 2], v[2]));
    o[i] = fadd_sep(s, x.t[i]);
  }
  v[0] = o[0];
  v[1] = o[1];
  v[2] = o[2];
}

// q_R * q (Hamilton), a = q_R, b = q, (x, y, z, w); each sum left to right.
__device__ __forceinline__ F32x4 xf_rotation(const spz_amd_transform &x, F32x4 b) {
  const float ax = x.q[0], ay = x.q[1], az = x.q[2], aw = x.q[3];
  F32x4 o;
  o.x = fadd_sep(fadd_sep(fadd_sep(fmul_sep(aw, b.x), fmul_sep(ax, b.w)), fmul_sep(ay, b.z)), -fmul_sep(az, b.y));
  o.y = fadd_sep(fadd_sep(fadd_sep(fmul_sep(aw, b.y), -fmul_sep(ax, b.z)), fmul_sep(ay, b.w)), fmul_sep(az, b.x));
  o.z = fadd_sep(fadd_sep(fadd_sep(fmul_sep(aw, b.z), fmul_sep(ax, b.y)), -fmul_sep(ay, b.x)), fmul_sep(az, b.w));
  o.w = fadd_sep(fadd_sep(fadd_sep(fmul_sep(aw, b.w), -fmul_sep(ax, b.x)), -fmul_sep(ay, b.y)), -fmul_sep(az, b.z));
  return o;
}

// One band of one channel: out[m] = sum_k D[k][m] * in[k], k ascending from the k = 0 product.
template <int N>
__device__ __forceinline__ void xf_band(const float *D, const float *in, float *out) {
#pragma unroll
  for (int m = 0; m < N; ++m) {
    float acc = fmul_sep(D[m], in[0]);
#pragma unroll
    for (int k = 1; k < N; ++k) acc = fadd_sep(acc, fmul_sep(D[k * N + m], in[k]));
    out[m] = acc;
  }
}

// The bands 1..3 present in `dim` coefficients (3, 8 or 15), coefficient-major [coeff][rgb] records.
__device__ __forceinline__ void xf_sh_channel(const spz_amd_transform &x, uint32_t dim, const float *in, float *out) {
  xf_band<3>(x.d1, in, out);
  if (dim >= 8) xf_band<5>(x.d2, in + 3, out + 3);
  if (dim >= 15) xf_band<7>(x.d3, in + 8, out + 8);
}

__device__ __forceinline__ bool fits24(float r) { return r >= -8388608.0f && r <= 8388607.0f; }  // NaN: false

// ---- packed-domain point cores -----------------------------------------------------------------------------------
// Four log-scale bytes, each decoded, + ln_s, encoded.
__device__ __forceinline__ uint32_t xf_scale_bytes(uint32_t w, float ln_s) {
  uint32_t o = 0;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    const float v = fadd_sep(scale_from_byte((w >> (8u * j)) & 0xffu), ln_s);
    o |= (uint32_t)scale_to_byte_f(v) << (8u * j);
  }
  return o;
}

// Point i of a positions section (v1: float16, else 24-bit fixed at in_scale = 2^-fractionalBits) -> the 9 bytes at
// out_scale = 2^fractional_bits written to d; x == nullptr: no placement.  Returns true when a coordinate is not finite
// or does not fit the 24-bit field (its bytes wrap, as saveSpz's would).
__device__ __forceinline__ bool xf_position_point(const uint8_t *src, unsigned long long i, bool v1, float in_scale,
                                                  const spz_amd_transform *x, float out_scale, uint8_t *d) {
  float v[3];
#pragma unroll
  for (uint32_t a = 0; a < 3; ++a) v[a] = decode_position_axis(src, i, a, v1, in_scale, 0u);
  if (x != nullptr && x->apply_positions) xf_position(*x, v);
  bool bad = false;
#pragma unroll
  for (uint32_t a = 0; a < 3; ++a) {
    bad = bad || !fits24(round_half_away(v[a] * out_scale));
    const uint32_t f = (uint32_t)position_fixed(v[a], out_scale) & 0xffffffu;
    d[3 * a] = (uint8_t)f;
    d[3 * a + 1] = (uint8_t)(f >> 8);
    d[3 * a + 2] = (uint8_t)(f >> 16);
  }
  return bad;
}

// Point i of a rotations section (v3: smallest three, else first three) -> the v3 word; x == nullptr: no placement.
__device__ __forceinline__ uint32_t xf_rotation_point(const uint8_t *src, unsigned long long i, uint32_t version,
                                                      const spz_amd_transform *x) {
  F32x4 r;
  if (version >= 3u) {
    r = unpack_quat_smallest_three(*reinterpret_cast<const u32_a1 *>(src + i * 4ull), 0u);
  } else {
    const uint8_t *b = src + i * 3ull;
    r = unpack_quat_first_three((uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16), 0u);
  }
  if (x != nullptr && x->apply_rotation) r = xf_rotation(*x, r);
  return pack_quat_smallest_three(r, 0u);
}

// One sh record of `dim` coefficients in place (LDS): decoded, rotated when x rotates, re-quantised.  The first `keep`
// coefficients are written back (the others are left as they were).
__device__ __forceinline__ void xf_sh_record(uint8_t *r, uint32_t dim, uint32_t keep, const spz_amd_transform *x) {
#pragma unroll
  for (uint32_t c = 0; c < 3; ++c) {
    float in[15], out[15];
#pragma unroll
    for (uint32_t k = 0; k < 15; ++k) in[k] = k < dim ? sh_from_byte(r[3 * k + c]) : 0.0f;
    if (x != nullptr && x->apply_rotation) {
      xf_sh_channel(*x, dim, in, out);
    } else {
#pragma unroll
      for (uint32_t k = 0; k < 15; ++k) out[k] = in[k];
    }
#pragma unroll
    for (uint32_t k = 0; k < 15; ++k) {
      if (k < keep) r[3 * k + c] = (uint8_t)quantize_sh_f(out[k], k < 3u);  // elements 0..8: the degree-1 bucket
    }
  }
}

}  // namespace
}  // namespace spz_amd_detail
