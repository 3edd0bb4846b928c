// spz_quant.hpp — the exact per-value quantise / dequantise arithmetic of the device code: round-half-away and the
// x86 conversions, the sh and uint8 quantisers, and the quaternion encoders / decoders with their proven fast paths
// (spz_selftest_kernel).  Shared by spz_kernels.hip (encode / decode / gather / self test) and spz_transform.hip, so
// that a transformed stream is encoded and decoded by the same code as a saved one.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "spz_common.hpp"
#include "spz_kernel_params.hpp"

#pragma clang fp contract(off)

namespace spz_amd_detail {
namespace {

// ------------------------------------------------------------------------------------------
// Exact scalar helpers
// ------------------------------------------------------------------------------------------
// Keeps a product in a register of its own so that no later add can be contracted with it,
// whatever the compiler flags are.
__device__ __forceinline__ float fmul_sep(float a, float b) {
  float r = a * b;
  asm volatile("" : "+v"(r));
  return r;
}
__device__ __forceinline__ float fadd_sep(float a, float b) {
  float r = a + b;
  asm volatile("" : "+v"(r));
  return r;
}

// std::round: half away from zero, exact (load-spz.cc:74,78,284).
__device__ __forceinline__ float round_half_away(float x) {
  float t = __builtin_truncf(x);
  float d = __builtin_fabsf(x - t);  // exact
  float one = __builtin_copysignf(1.0f, x);
  return (d >= 0.5f) ? (t + one) : t;
}

// static_cast<int32_t>(float) as the reference's x86-64 build executes it (cvttss2si):
// NaN and out-of-range give 0x80000000.
__device__ __forceinline__ int32_t cvt_i32_x86(float r) {
  return (r >= -2147483648.0f && r < 2147483648.0f) ? (int32_t)r : (int32_t)0x80000000;
}

// static_cast<uint32_t>(float) as x86-64 gcc executes it: 64-bit cvttss2si, low 32 bits.
__device__ __forceinline__ uint32_t cvt_u32_x86(float r) {
  if (r > -9223372036854775808.0f && r < 9223372036854775808.0f) {
    return (uint32_t)(long long)r;
  }
  return 0u;
}

// toUint8 (load-spz.cc:74): static_cast<uint8_t>(clamp(round(x), 0, 255)), as a float in
// [0, 255].  std::clamp lets a NaN through and the x86 cast turns it into 0; fmaxf(NaN, 0) = 0
// gives the same.
__device__ __forceinline__ float to_uint8_f(float x) {
  float r = round_half_away(x);
  return __builtin_fminf(__builtin_fmaxf(r, 0.0f), 255.0f);
}
__device__ __forceinline__ uint32_t to_uint8(float x) { return (uint32_t)to_uint8_f(x); }

// quantizeSH (load-spz.cc:77-81) for bucket b in {8, 16}, as a float in [0, 255]:
//   q = (int)(round(128 x) + 128);  q = (q + b/2) / b * b;  clamp(q, 0, 255).
// With r = round(128 x) (an integer-valued float) and 128 a multiple of b,
//   (q + b/2) / b * b  ==  b * floor((r + b/2) / b) + 128   wherever q + b/2 >= 0,
// and every negative q + b/2 (C division truncates toward zero) ends <= 0 and clamps to 0, as
// does the floor form.  All products are by powers of two; the sums are exact below 2^24 and
// far outside the clamp range above it.  The reference's (int) cast is "integer indefinite"
// (INT_MIN -> clamps to 0) for NaN and once r + 128.0f reaches 2^31, i.e. from r = 2^31 - 128 up.
__device__ __forceinline__ float quantize_sh_f(float x, bool degree1) {
  const float inv_b = degree1 ? 0.125f : 0.0625f;
  const float b = degree1 ? 8.0f : 16.0f;
  float r = round_half_away(x * 128.0f);
  // exact products: a fused multiply-add rounds exactly like the separate operations here
  float k = __builtin_floorf(__builtin_fmaf(r, inv_b, 0.5f));
  float v = __builtin_fminf(__builtin_fmaxf(__builtin_fmaf(k, b, 128.0f), 0.0f), 255.0f);
  return (r < 2147483520.0f) ? v : 0.0f;
}

// Four values already in [0, 255] and integral -> one little-endian dword.
__device__ __forceinline__ uint32_t pack_u8x4(float a, float b, float c, float d) {
  uint32_t w = __builtin_amdgcn_cvt_pk_u8_f32(a, 0u, 0u);
  w = __builtin_amdgcn_cvt_pk_u8_f32(b, 1u, w);
  w = __builtin_amdgcn_cvt_pk_u8_f32(c, 2u, w);
  return __builtin_amdgcn_cvt_pk_u8_f32(d, 3u, w);
}

// The per-byte dequantisers of unpackGaussians and the quantisers of packGaussians that are one expression each.
// scales: b / 16.0f - 10.0f (load-spz.cc:506; the quotient is exact) and toUint8((s + 10.0f) * 16.0f) (:291).
__device__ __forceinline__ float scale_from_byte(uint32_t b) { return (float)b / 16.0f - 10.0f; }
__device__ __forceinline__ float scale_to_byte_f(float v) { return to_uint8_f(fadd_sep(v, 10.0f) * 16.0f); }
// sh: (b - 128) / 128 (load-spz.cc:83).
__device__ __forceinline__ float sh_from_byte(uint32_t b) { return ((float)b - 128.0f) / 128.0f; }
// positions: (int32)round(p * scale) (load-spz.cc:282-288; scale = 1 << fractionalBits, the product is exact); the
// caller keeps the low 24 bits.
__device__ __forceinline__ int32_t position_fixed(float v, float scale) { return cvt_i32_x86(round_half_away(v * scale)); }

constexpr float kSqrt1_2 = (float)0.707106781186547524401;  // load-spz.cc:46

// ------------------------------------------------------------------------------------------
// Correctly rounded divisions without the IEEE expansion's operand scaling.
//
// hipcc expands an f32 `a / b` into v_div_scale x2, v_rcp, five fma/mul, v_div_fmas, v_div_fixup
// (11 VALU operations); a quaternion costs seven of them.  Inside the exponent window where
// v_div_scale does not scale and v_div_fixup passes its operand through, the same arithmetic is
// (a) for the four quotients x_i / norm: ONE refined reciprocal shared by all four, then the
//     expansion's own two residual corrections (quat_quotient);
// (b) for the divisions by the constants 0.70710677f and 511.0f: reciprocal multiply + one fma
//     residual correction (div_by_const), which equals the IEEE quotient for every dividend that
//     is zero or in [2^-100, 2^126] — checked over ALL such floats by spz_selftest_kernel
//     (tests/test_gpu_parity.py::test_fast_divisions_exhaustive), as are (a) on 2^31 operand pairs
//     and sqrt_cr on every float of its window.
// Operands outside the window (quat_fast_ok) take the general forms below, unchanged from the
// reference-shaped arithmetic; both forms give identical bits wherever the fast one is used.
// ------------------------------------------------------------------------------------------
constexpr uint32_t kFastLoBits = 0x2b800000u;  // 2^-40
constexpr uint32_t kFastHiBits = 0x53800000u;  // 2^40

// Every component is zero or has 2^-40 <= |x| <= 2^40, and at least one is not zero: then no square
// under/overflows, norm is in [2^-40, 2^41], every quotient is zero or >= 2^-81 and every residual
// of the corrections below is exactly representable.
__device__ __forceinline__ bool quat_fast_ok(F32x4 r) {
  const uint32_t a0 = __float_as_uint(r.x) & 0x7fffffffu, a1 = __float_as_uint(r.y) & 0x7fffffffu;
  const uint32_t a2 = __float_as_uint(r.z) & 0x7fffffffu, a3 = __float_as_uint(r.w) & 0x7fffffffu;
  // a - 1 wraps a zero to 0xffffffff, so zeros pass the lower bound
  const uint32_t lo = min(min(a0 - 1u, a1 - 1u), min(a2 - 1u, a3 - 1u));
  const uint32_t hi = max(max(a0, a1), max(a2, a3));
  return lo >= kFastLoBits - 1u && hi <= kFastHiBits && hi != 0u;
}

// Correctly rounded sqrt for 2^-80 <= x <= 2^82 (no denormal scaling, no zero / inf fix-up): v_sqrt_f32
// is within one ulp, the two neighbours are tried with exact residuals (the IEEE expansion's own step).
__device__ __forceinline__ float sqrt_cr(float x) {
  const float s = __builtin_amdgcn_sqrtf(x);
  const float dn = __uint_as_float(__float_as_uint(s) - 1u);
  const float up = __uint_as_float(__float_as_uint(s) + 1u);
  const float r_dn = __builtin_fmaf(-dn, s, x);
  const float r_up = __builtin_fmaf(-up, s, x);
  float o = (r_dn <= 0.0f) ? dn : s;
  o = (r_up > 0.0f) ? up : o;
  return o;
}

// 1 / b refined once (v_rcp_f32 + one Newton step): the reciprocal the IEEE expansion uses.
__device__ __forceinline__ float refined_rcp(float b) {
  const float y0 = __builtin_amdgcn_rcpf(b);
  const float e = __builtin_fmaf(-b, y0, 1.0f);
  return __builtin_fmaf(e, y0, y0);
}

// a / b for a >= 0 (zero or >= 2^-100), b > 0, quotient zero or normal; y = refined_rcp(b).
__device__ __forceinline__ float quat_quotient(float a, float b, float y) {
  const float m = a * y;
  const float r0 = __builtin_fmaf(-b, m, a);
  const float q1 = __builtin_fmaf(r0, y, m);
  const float r1 = __builtin_fmaf(-b, q1, a);
  return __builtin_fmaf(r1, y, q1);
}

// x / c for a constant c with rc = RN(1 / c); x zero or in [2^-100, 2^126].
__device__ __forceinline__ float div_by_const(float x, float c, float rc) {
  const float m = x * rc;
  const float rem = __builtin_fmaf(-m, c, x);
  return __builtin_fmaf(rem, rc, m);
}
constexpr float kRcpSqrt1_2 = 1.0f / kSqrt1_2;
constexpr float kRcp511 = 1.0f / 511.0f;

struct Quat4 { float q0, q1, q2, q3; };

// normalized() (splat-types.cc:71-74) followed by the xyz flip (load-spz.cc:224-227), general operands.
__device__ __forceinline__ Quat4 normalized_flipped(F32x4 r, uint32_t flip_q) {
  float n2 = fadd_sep(fadd_sep(fadd_sep(fmul_sep(r.x, r.x), fmul_sep(r.y, r.y)), fmul_sep(r.z, r.z)),
                      fmul_sep(r.w, r.w));
  float norm = __builtin_sqrtf(n2);
  Quat4 q;
  q.q0 = xor_sign(r.x / norm, flip_q & 1u);
  q.q1 = xor_sign(r.y / norm, (flip_q >> 1) & 1u);
  q.q2 = xor_sign(r.z / norm, (flip_q >> 2) & 1u);
  q.q3 = r.w / norm;
  return q;
}

// The same for operands inside the quat_fast_ok window: same bits, 4 + 9 + 20 operations instead of 4 + 15 + 44.
__device__ __forceinline__ Quat4 normalized_flipped_fast(F32x4 r, uint32_t flip_q) {
  float n2 = fadd_sep(fadd_sep(fadd_sep(fmul_sep(r.x, r.x), fmul_sep(r.y, r.y)), fmul_sep(r.z, r.z)),
                      fmul_sep(r.w, r.w));
  const float norm = sqrt_cr(n2);
  const float y = refined_rcp(norm);
  const uint32_t sx = (__float_as_uint(r.x) >> 31) ^ (flip_q & 1u), sy = (__float_as_uint(r.y) >> 31) ^ ((flip_q >> 1) & 1u);
  const uint32_t sz = (__float_as_uint(r.z) >> 31) ^ ((flip_q >> 2) & 1u), sw = __float_as_uint(r.w) >> 31;
  Quat4 q;
  q.q0 = xor_sign(quat_quotient(__builtin_fabsf(r.x), norm, y), sx);
  q.q1 = xor_sign(quat_quotient(__builtin_fabsf(r.y), norm, y), sy);
  q.q2 = xor_sign(quat_quotient(__builtin_fabsf(r.z), norm, y), sz);
  q.q3 = xor_sign(quat_quotient(__builtin_fabsf(r.w), norm, y), sw);
  return q;
}

// The bit-field assembly of packQuaternionSmallestThree (load-spz.cc:229-254), general operands.
__device__ __forceinline__ uint32_t smallest_three_fields(Quat4 q) {
  const float q0 = q.q0, q1 = q.q1, q2 = q.q2, q3 = q.q3;
  // argmax |q|, strict >, first wins
  uint32_t iL = 0;
  float best = __builtin_fabsf(q0);
  if (__builtin_fabsf(q1) > best) { iL = 1; best = __builtin_fabsf(q1); }
  if (__builtin_fabsf(q2) > best) { iL = 2; best = __builtin_fabsf(q2); }
  if (__builtin_fabsf(q3) > best) { iL = 3; best = __builtin_fabsf(q3); }
  float qL = (iL == 0) ? q0 : (iL == 1) ? q1 : (iL == 2) ? q2 : q3;
  uint32_t negate = (qL < 0.0f) ? 1u : 0u;
  uint32_t comp = iL;
  const float qs[4] = {q0, q1, q2, q3};
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i) {
    uint32_t negbit = ((qs[i] < 0.0f) ? 1u : 0u) ^ negate;
    float m = fmul_sep(511.0f, __builtin_fabsf(qs[i]) / kSqrt1_2) + 0.5f;
    uint32_t mag = cvt_u32_x86(m);
    uint32_t next = (comp << 10) | (negbit << 9) | mag;
    comp = (i != iL) ? next : comp;
  }
  return comp;
}

// The same for |q_i| zero or in [2^-100, 2]: only the three kept components are quantised, the
// divisions by sqrt(1/2) are reciprocal multiplies with a residual correction, and 511 t + 0.5 < 2^31
// converts with one instruction.
__device__ __forceinline__ uint32_t smallest_three_fields_fast(Quat4 q) {
  const float a0 = __builtin_fabsf(q.q0), a1 = __builtin_fabsf(q.q1), a2 = __builtin_fabsf(q.q2), a3 = __builtin_fabsf(q.q3);
  uint32_t iL = 0;
  float best = a0;
  if (a1 > best) { iL = 1; best = a1; }
  if (a2 > best) { iL = 2; best = a2; }
  if (a3 > best) { iL = 3; best = a3; }
  const float qL = (iL == 0) ? q.q0 : (iL == 1) ? q.q1 : (iL == 2) ? q.q2 : q.q3;
  const uint32_t negate = (qL < 0.0f) ? 1u : 0u;
  // the components other than iL, in index order
  const float c0 = (iL == 0) ? q.q1 : q.q0;
  const float c1 = (iL <= 1) ? q.q2 : q.q1;
  const float c2 = (iL <= 2) ? q.q3 : q.q2;
  uint32_t comp = iL;
  const float cs[3] = {c0, c1, c2};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const uint32_t negbit = ((cs[i] < 0.0f) ? 1u : 0u) ^ negate;
    const float t = div_by_const(__builtin_fabsf(cs[i]), kSqrt1_2, kRcpSqrt1_2);
    const float m = fmul_sep(511.0f, t) + 0.5f;
    comp = (comp << 10) | (negbit << 9) | (uint32_t)m;
  }
  return comp;
}

// packQuaternionSmallestThree (load-spz.cc:216-255) incl. normalized() (splat-types.cc:71-74).
__device__ __forceinline__ uint32_t pack_quat_smallest_three(F32x4 r, uint32_t flip_q) {
#if SPZ_QUAT_FAST
  if (quat_fast_ok(r)) return smallest_three_fields_fast(normalized_flipped_fast(r, flip_q));
#endif
  return smallest_three_fields(normalized_flipped(r, flip_q));
}

// PARITY UNPINNED (no v2 encoder in the reference): upstream nianticlabs/spz v1.x
// first-three encoder — normalise, flip, scale by +-127.5 so that w >= 0, offset, toUint8.
__device__ __forceinline__ uint32_t pack_quat_first_three(F32x4 r, uint32_t flip_q) {
  Quat4 q;
#if SPZ_QUAT_FAST
  if (quat_fast_ok(r)) q = normalized_flipped_fast(r, flip_q);
  else
#endif
    q = normalized_flipped(r, flip_q);
  float s = (q.q3 < 0.0f) ? -127.5f : 127.5f;
  uint32_t b0 = to_uint8(fmul_sep(q.q0, s) + 127.5f);
  uint32_t b1 = to_uint8(fmul_sep(q.q1, s) + 127.5f);
  uint32_t b2 = to_uint8(fmul_sep(q.q2, s) + 127.5f);
  return b0 | (b1 << 8) | (b2 << 16);
}

// unpackQuaternionSmallestThree (load-spz.cc:347-381) followed by the flip pass.
template <bool FAST>
__device__ __forceinline__ F32x4 unpack_quat_smallest_three_t(uint32_t comp, uint32_t flip_q) {
  const uint32_t iL = comp >> 30;
  float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  float sum = 0.0f;
#pragma unroll
  for (int i = 3; i >= 0; --i) {
    const bool take = ((uint32_t)i != iL);
    uint32_t mag = comp & 511u;
    uint32_t neg = (comp >> 9) & 1u;
    // (sqrt1_2 * mag) / 511.f: the dividend is zero or in [0.707, 361.4] for the 512 magnitudes
    float c = fmul_sep(kSqrt1_2, (float)mag);
    if constexpr (FAST) c = div_by_const(c, 511.0f, kRcp511);
    else c = c / 511.0f;
    c = __uint_as_float(__float_as_uint(c) ^ (neg << 31));
    float s2 = sum + fmul_sep(c, c);
    v[i] = take ? c : 0.0f;
    sum = take ? s2 : sum;
    comp = take ? (comp >> 10) : comp;
  }
  // sqrt(1.0f - sum): ::sqrt(double) rounded to float == correctly rounded sqrtf; a negative
  // argument yields the x86 default NaN (sign bit set).
  float d = 1.0f - sum;
  float big = (d < 0.0f) ? __uint_as_float(0xffc00000u) : __builtin_sqrtf(d);
  float x = (iL == 0) ? big : v[0];
  float y = (iL == 1) ? big : v[1];
  float z = (iL == 2) ? big : v[2];
  float w = (iL == 3) ? big : v[3];
  F32x4 o;
  o.x = mul_pm1(x, flip_q & 1u);
  o.y = mul_pm1(y, (flip_q >> 1) & 1u);
  o.z = mul_pm1(z, (flip_q >> 2) & 1u);
  o.w = w;
  return o;
}
__device__ __forceinline__ F32x4 unpack_quat_smallest_three(uint32_t comp, uint32_t flip_q) {
  return unpack_quat_smallest_three_t<SPZ_QUAT_FAST != 0>(comp, flip_q);
}

// unpackQuaternionFirstThree (load-spz.cc:333-345) followed by the flip pass.
__device__ __forceinline__ F32x4 unpack_quat_first_three(uint32_t r3, uint32_t flip_q) {
  constexpr float k = 1.0f / 127.5f;
  float x = fmul_sep((float)(r3 & 0xffu), k) + (-1.0f);
  float y = fmul_sep((float)((r3 >> 8) & 0xffu), k) + (-1.0f);
  float z = fmul_sep((float)((r3 >> 16) & 0xffu), k) + (-1.0f);
  float sq = fadd_sep(fadd_sep(fmul_sep(x, x), fmul_sep(y, y)), fmul_sep(z, z));
  float d = 1.0f - sq;
  float m = (0.0f < d) ? d : 0.0f;  // std::max(0.0f, d)
  F32x4 o;
  o.x = xor_sign(x, flip_q & 1u);
  o.y = xor_sign(y, (flip_q >> 1) & 1u);
  o.z = xor_sign(z, (flip_q >> 2) & 1u);
  o.w = __builtin_sqrtf(m);
  return o;
}

}  // namespace
}  // namespace spz_amd_detail
