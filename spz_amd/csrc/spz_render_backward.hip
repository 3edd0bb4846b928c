// spz_render_backward.hip — the gradients of one rendered view to a float cloud (DESIGN §8 "Render backward"; the
// contract is in include/spz_amd.h "render backward").  Reads the workspace as spz_amd_render_finish_device left it.
//
//   spz_render_blend_backward_kernel       the forward's geometry: one 256-lane workgroup per 16x16 tile, one pixel per
//                                          lane, the tile's records staged in LDS 256 at a time.  It walks the tile's
//                                          list twice, front to back both times: first the forward blend again, bit for
//                                          bit, for the pixel's final C and T; then the same loop in step across each
//                                          wave, forming every used pair's gradient to the record's nine floats from
//                                          the prefix and "what lies behind" = final - prefix.  The nine values are
//                                          summed over the wave by DPP, one lane per wave adds them into the batch's
//                                          LDS slots, and each non-zero slot value goes to the n x 9 record gradients
//                                          by one global f32 atomic.
//   spz_render_depth_blend_backward_kernel the same body (blend_backward_body, which both kernels instantiate) with the
//                                          depth sum of spz_render_depth_kernel in it ("render depth backward"; DESIGN
//                                          §8 "Depth fit"): the record's depth, less the depth of the tile's first
//                                          entry, rides in the .w of the staged rgb, D is blended beside the colour,
//                                          and a tenth value per used pair, dL/dz, goes to an array of its own (n
//                                          floats), so the n x 9 layout stays what the chain and the view backward
//                                          read.
//   spz_render_preprocess_backward_kernel  one lane per Gaussian, f64 like the forward preprocess: the forward's
//                                          intermediates again from the floats and the camera, then the chain from the
//                                          nine record gradients to positions, log scales, raw quaternion, alpha,
//                                          colour and sh.  Writes every output element once (zeros for an invisible
//                                          Gaussian and for sh above the used degree); no atomics.  With the depth
//                                          gradients given, dL/dp += R[2, :] dL/dz (z is the record's depth,
//                                          rounded to f32 straight through); without them every bit is as before.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "spz_amd.h"
#include "spz_common.hpp"
#include "spz_render_internal.hpp"

#pragma clang fp contract(off)

namespace spz_amd_detail {
namespace {

constexpr uint32_t kRecGrads = 9;  // mean 2, conic 3, opacity 1, rgb 3: the record's first nine floats

}  // namespace

struct BlendBackwardParams {
  const spz_amd_render_record *rec;
  const uint32_t *sorted_gid;
  const uint2 *ranges;
  const unsigned long long *total;
  const float *grad_image;  // height x width x 4
  float *rec_grad;          // n x 9, zeroed; added into
  unsigned long long max_entries;
  uint32_t width, height, tiles_x;
  float bg[3];
};

struct DepthBlendBackwardParams {
  BlendBackwardParams b;    // b.grad_image may be null: all zero
  const float *grad_depth;  // height x width: the gradient to channel 0 of the depth map
  float *depth_grad;        // n, zeroed; added into
};

// The body of both blend backward kernels: the colour one (kDepth false) and the one with the depth sum of
// spz_render_depth_kernel in it (kDepth true: "render depth backward").
//
// Colour.  power, a, T' and the three tests are the expressions of spz_render_blend_kernel, so both passes use the
// pairs the image used.  With I = C + T_final bg and alpha = 1 - T_final, g the pixel's gradient, and for a used pair i
// (T before it, w = T a, C_i the prefix that includes it):
//   dL/drgb_i = w g_rgb
//   dL/da_i   = T (g_rgb . rgb_i) - (g_rgb . (C_final - C_i) + tail) / (1 - a)
//   tail      = T_final (g_rgb . bg - g_alpha)
// a = min(0.99, opacity e^power) hands dL/da to opacity and power only where it does not clamp.
//
// Depth.  s_rgb[k].w carries the record's depth z, D += (T a) z beside the colour sums, and a tenth value per used
// pair.  With g_D the pixel's gradient to D, D_i the prefix that includes pair i and D_final the pixel's sum:
//   dL/dz_i = w g_D
//   dL/da_i = T (g_rgb . rgb_i + g_D z_i) - (g_rgb . (C_final - C_i) + g_D (D_final - D_i) + tail) / (1 - a)
// D_final - D_i is a difference of two long f32 sums of w z, and at camera depths far above the depth range of a tile's
// list it cancels most of their digits.  So both walks sum w (z - z0) instead, z0 the depth of the tile's first (nearest)
// entry: D = D' + z0 (1 - T_final), which is the same loss with z - z0 for z and g_alpha + g_D z0 for g_alpha:
//   dL/da_i = T (g_rgb . rgb_i + g_D (z_i - z0)) - (g_rgb . (C_final - C_i) + g_D (D'_final - D'_i) + tail') / (1 - a)
//   tail'   = T_final (g_rgb . bg - g_alpha - g_D z0)
// dL/dz_i is unchanged.  The tenth sum goes to an array of its own, so the n x 9 layout stays.
//
// The colour instance stages 0 in s_rgb[k].w, reads no depth, no z0 and no grad_depth, and reads grad_image without a
// null check; every depth term is added after the colour terms of its sum, so each instance rounds as its formula reads.
template <bool kDepth>
__device__ __forceinline__ void blend_backward_body(const BlendBackwardParams &p, const float *grad_depth,
                                                    float *depth_grad) {
  constexpr uint32_t kGrads = kDepth ? kRecGrads + 1 : kRecGrads;  // and the record's depth z
  __shared__ float2 s_xy[kBlendThreads];
  __shared__ float4 s_co[kBlendThreads];   // conic A, B, C, opacity
  __shared__ float4 s_rgb[kBlendThreads];  // rgb, z - z0 (0 without the depth)
  __shared__ float s_grad[kGrads][kBlendThreads];
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
  if (begin >= end) return;  // workgroup-uniform: nothing blends here
  const float fu = (float)u, fv = (float)v;
  float z0 = 0.0f;
  if constexpr (kDepth) z0 = p.rec[p.sorted_gid[begin]].depth;  // workgroup-uniform: the list is in depth order
  // the forward blend, for the pixel's final colour sum, depth sum (of z - z0) and T
  float T = 1.0f, c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, D = 0.0f;
  bool done = !inside;
  for (uint32_t base = begin; base < end; base += kBlendThreads) {
    // also the barrier between the previous batch's reads and this batch's writes
    if (__syncthreads_count(done ? 1 : 0) == (int)kBlendThreads) break;
    const uint32_t j = base + t;
    if (j < end) {
      const spz_amd_render_record &q = p.rec[p.sorted_gid[j]];
      s_xy[t] = make_float2(q.mean[0], q.mean[1]);
      s_co[t] = make_float4(q.conic[0], q.conic[1], q.conic[2], q.opacity);
      s_rgb[t] = make_float4(q.rgb[0], q.rgb[1], q.rgb[2], kDepth ? q.depth - z0 : 0.0f);
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
      const float4 rgbz = s_rgb[k];
      const float w = T * a;
      c0 = c0 + w * rgbz.x;
      c1 = c1 + w * rgbz.y;
      c2 = c2 + w * rgbz.z;
      if constexpr (kDepth) D = D + w * rgbz.w;
      T = Tn;
    }
  }
  const float f0 = c0, f1 = c1, f2 = c2, fD = D;
  float g0 = 0.0f, g1 = 0.0f, g2 = 0.0f, g3 = 0.0f, gD = 0.0f;
  if (inside) {
    const unsigned long long at = (unsigned long long)v * p.width + u;
    if (!kDepth || p.grad_image) {  // only the depth kernel's may be null
      const float *g = p.grad_image + at * 4u;
      g0 = g[0];
      g1 = g[1];
      g2 = g[2];
      g3 = g[3];
    }
    if constexpr (kDepth) gD = grad_depth[at];
  }
  // the background and the alpha channel, and with the depth z0 (1 - T_final)
  float tail = (g0 * p.bg[0] + g1 * p.bg[1] + g2 * p.bg[2]) - g3;
  if constexpr (kDepth) tail = tail - gD * z0;
  tail = T * tail;
  // the same walk again, in step across the wave (a stopped lane takes no more pairs)
  T = 1.0f;
  c0 = 0.0f;
  c1 = 0.0f;
  c2 = 0.0f;
  D = 0.0f;
  done = !inside;
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
      s_rgb[t] = make_float4(q.rgb[0], q.rgb[1], q.rgb[2], kDepth ? q.depth - z0 : 0.0f);
    }
#pragma unroll
    for (uint32_t e = 0; e < kGrads; ++e) s_grad[e][t] = 0.0f;
    __syncthreads();
    const uint32_t cnt = (end - base) < kBlendThreads ? end - base : kBlendThreads;
    for (uint32_t k = 0; k < cnt; ++k) {
      if (__ballot(!done) == 0ull) break;  // wave-uniform: every lane of the wave has stopped
      const float2 xy = s_xy[k];
      const float4 co = s_co[k];
      const float dx = fu - xy.x, dy = fv - xy.y;
      const float power = -0.5f * (co.x * dx * dx + co.z * dy * dy) - co.y * dx * dy;
      const float ex = expf(power);
      const float raw = co.w * ex;
      const float a = fminf(0.99f, raw);
      const float Tn = T * (1.0f - a);
      bool use = !done && !(power > 0.0f) && !(a < 1.0f / 255.0f);
      if (use && Tn < 1e-4f) {
        done = true;
        use = false;
      }
      if (__ballot(use) == 0ull) continue;  // wave-uniform
      float d[kGrads] = {};
      if (use) {
        const float4 rgbz = s_rgb[k];
        const float w = T * a;
        c0 = c0 + w * rgbz.x;
        c1 = c1 + w * rgbz.y;
        c2 = c2 + w * rgbz.z;
        float front = g0 * rgbz.x + g1 * rgbz.y + g2 * rgbz.z;
        float behind = g0 * (f0 - c0) + g1 * (f1 - c1) + g2 * (f2 - c2);
        if constexpr (kDepth) {
          D = D + w * rgbz.w;
          front = front + gD * rgbz.w;
          behind = behind + gD * (fD - D);
          d[kRecGrads] = w * gD;
        }
        behind = behind + tail;
        const float da = T * front - behind / (1.0f - a);
        d[6] = w * g0;
        d[7] = w * g1;
        d[8] = w * g2;
        if (!(raw > 0.99f)) {  // a is opacity e^power
          const float dp = da * raw;
          d[0] = dp * (co.x * dx + co.y * dy);
          d[1] = dp * (co.z * dy + co.y * dx);
          d[2] = dp * (-0.5f * dx * dx);
          d[3] = dp * (-(dx * dy));
          d[4] = dp * (-0.5f * dy * dy);
          d[5] = da * ex;
        }
        T = Tn;
      }
#pragma unroll
      for (uint32_t e = 0; e < kGrads; ++e) d[e] = wave_sum_f32(d[e]);
      if ((t & 63u) == 0u) {
#pragma unroll
        for (uint32_t e = 0; e < kGrads; ++e) atomicAdd(&s_grad[e][k], d[e]);
      }
    }
    __syncthreads();
    if (j < end) {
      float *o = p.rec_grad + (unsigned long long)gid * kRecGrads;
#pragma unroll
      for (uint32_t e = 0; e < kRecGrads; ++e) {
        const float s = s_grad[e][t];
        if (s != 0.0f) atomicAdd(o + e, s);
      }
      if constexpr (kDepth) {
        const float s = s_grad[kRecGrads][t];
        if (s != 0.0f) atomicAdd(depth_grad + gid, s);
      }
    }
  }
}

// The two entries keep their names and parameter blocks (the tools and the recorded profiles find them by name).
__global__ __launch_bounds__(kBlendThreads) void spz_render_blend_backward_kernel(const BlendBackwardParams p) {
  blend_backward_body<false>(p, nullptr, nullptr);
}

__global__ __launch_bounds__(kBlendThreads) void spz_render_depth_blend_backward_kernel(const DepthBlendBackwardParams pp) {
  blend_backward_body<true>(pp.b, pp.grad_depth, pp.depth_grad);
}

struct PreprocessBackwardParams {
  FloatSrc src;
  RenderCam cam;
  const spz_amd_render_record *rec;
  const float *rec_grad;  // n x 9
  const unsigned long long *total;
  unsigned long long max_entries;
  float *positions, *scales, *rotations, *alphas, *colors, *sh;  // the six gradients
  float *rec_grad_out;  // may be null: n x 9
  uint32_t *status;
  uint32_t n;
  const float *depth_grad;  // may be null: n, the gradients to the records' depth z ("render depth backward")
  float *depth_grad_out;    // may be null: n
};

// The forward's symbols (spz_render_preprocess_kernel): p_c = (x, y, z), R_q, s = exp(log scale), M = R_q diag(s),
// S = M M^T, J (with the clamped quotients qx, qy), T = J R, cov = T S T^T = (a0, b, c0), a = a0 + 0.3, c = c0 + 0.3,
// det, conic = (c, -b, a) / det, opacity = sigmoid(alpha) [sqrt(max(0, det0) / det)], rgb = max(0, sh(n) + 0.5).
// One Gaussian's chain (host and device: the arithmetic has no device-only part, so a CPU build can check it).
__host__ __device__ inline void preprocess_backward_one(const PreprocessBackwardParams &p, uint32_t i) {
  const unsigned long long i3 = (unsigned long long)i * 3u, i4 = (unsigned long long)i * 4u;
  const unsigned long long ish = (unsigned long long)i * p.src.sh_dim * 3u;
  const RenderCam &cam = p.cam;
  float rg[kRecGrads];
#pragma unroll
  for (uint32_t e = 0; e < kRecGrads; ++e) rg[e] = p.rec_grad[(unsigned long long)i * kRecGrads + e];
  if (p.rec_grad_out) {
#pragma unroll
    for (uint32_t e = 0; e < kRecGrads; ++e) p.rec_grad_out[(unsigned long long)i * kRecGrads + e] = rg[e];
  }
  if (p.depth_grad_out) p.depth_grad_out[i] = p.depth_grad ? p.depth_grad[i] : 0.0f;
  const spz_amd_render_record q = p.rec[i];
  if (!(q.depth < __builtin_huge_valf())) {  // invisible: the forward's own decision
#pragma unroll
    for (uint32_t a = 0; a < 3; ++a) {
      p.positions[i3 + a] = 0.0f;
      p.scales[i3 + a] = 0.0f;
      p.colors[i3 + a] = 0.0f;
    }
#pragma unroll
    for (uint32_t a = 0; a < 4; ++a) p.rotations[i4 + a] = 0.0f;
    p.alphas[i] = 0.0f;
    for (uint32_t e = 0; e < p.src.sh_dim * 3u; ++e) p.sh[ish + e] = 0.0f;
    return;
  }
  Gauss g;
#pragma unroll
  for (uint32_t a = 0; a < 3; ++a) {
    g.p[a] = p.src.positions[i3 + a];
    g.s[a] = p.src.scales[i3 + a];
  }
#pragma unroll
  for (uint32_t a = 0; a < 4; ++a) g.q[a] = p.src.rotations[i4 + a];
  g.alpha = p.src.alphas[i];
  // ---- the forward again
  const double px = g.p[0], py = g.p[1], pz = g.p[2];
  const double *R = cam.R;
  const double x = R[0] * px + R[1] * py + R[2] * pz + cam.t[0];
  const double y = R[3] * px + R[4] * py + R[5] * pz + cam.t[1];
  const double z = R[6] * px + R[7] * py + R[8] * pz + cam.t[2];
  const double qn = sqrt((double)g.q[0] * g.q[0] + (double)g.q[1] * g.q[1] + (double)g.q[2] * g.q[2] +
                         (double)g.q[3] * g.q[3]);
  const double qx = g.q[0] / qn, qy = g.q[1] / qn, qz = g.q[2] / qn, qw = g.q[3] / qn;
  const double Rq[9] = {1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy),
                        2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx),
                        2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)};
  const double s[3] = {exp((double)g.s[0]), exp((double)g.s[1]), exp((double)g.s[2])};
  double M[9];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) M[r * 3 + c] = Rq[r * 3 + c] * s[c];
  }
  double S[9];  // Sigma = M M^T
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) S[r * 3 + c] = M[r * 3 + 0] * M[c * 3 + 0] + M[r * 3 + 1] * M[c * 3 + 1] + M[r * 3 + 2] * M[c * 3 + 2];
  }
  const double rx = x / z, ry = y / z;
  const double cqx = rx < -cam.lim_x_neg ? -cam.lim_x_neg : (rx > cam.lim_x_pos ? cam.lim_x_pos : rx);
  const double cqy = ry < -cam.lim_y_neg ? -cam.lim_y_neg : (ry > cam.lim_y_pos ? cam.lim_y_pos : ry);
  const double free_x = cqx == rx ? 1.0 : 0.0, free_y = cqy == ry ? 1.0 : 0.0;  // 0: the quotient is clamped
  const double tx = z * cqx, ty = z * cqy;
  const double J00 = cam.fx / z, J02 = -(cam.fx * tx) / (z * z);
  const double J11 = cam.fy / z, J12 = -(cam.fy * ty) / (z * z);
  double T[6];  // J R
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
  const double a0 = TS[0] * T[0] + TS[1] * T[1] + TS[2] * T[2];
  const double b = TS[0] * T[3] + TS[1] * T[4] + TS[2] * T[5];
  const double c0 = TS[3] * T[3] + TS[4] * T[4] + TS[5] * T[5];
  const double det0 = a0 * c0 - b * b;
  const double a = a0 + 0.3, c = c0 + 0.3;
  const double det = a * c - b * b;
  const double sig = 1.0 / (1.0 + exp(-(double)g.alpha));
  const bool aa = cam.antialiased && det0 > 0.0;
  const double h = cam.antialiased ? sqrt((det0 > 0.0 ? det0 : 0.0) / det) : 1.0;
  // ---- conic and opacity -> cov
  const double g_ca = rg[2], g_cb = rg[3], g_cc = rg[4], g_op = rg[5];
  const double inv = 1.0 / det;
  double g_det = (g_cb * b - g_ca * c - g_cc * a) * inv * inv;
  double g_a = g_cc * inv, g_c = g_ca * inv, g_b = -g_cb * inv;
  if (aa) {
    const double g_h = g_op * sig;
    const double g_det0 = g_h * h / (2.0 * det0);
    g_det = g_det - g_h * h / (2.0 * det);
    g_a = g_a + g_det0 * c0;
    g_c = g_c + g_det0 * a0;
    g_b = g_b - 2.0 * b * g_det0;
  }
  g_a = g_a + g_det * c;
  g_c = g_c + g_det * a;
  g_b = g_b - 2.0 * b * g_det;
  const double g_alpha = g_op * h * sig * (1.0 - sig);
  // ---- cov -> T and Sigma
  double gT[6];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    gT[k] = 2.0 * g_a * TS[k] + g_b * TS[3 + k];
    gT[3 + k] = g_b * TS[k] + 2.0 * g_c * TS[3 + k];
  }
  double gS[9];  // to the nine entries of Sigma taken as independent
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int k = 0; k < 3; ++k) gS[r * 3 + k] = g_a * T[r] * T[k] + g_b * T[r] * T[3 + k] + g_c * T[3 + r] * T[3 + k];
  }
  double gM[9];  // (gS + gS^T) M
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      gM[r * 3 + k] = (gS[r * 3 + 0] + gS[0 * 3 + r]) * M[0 * 3 + k] + (gS[r * 3 + 1] + gS[1 * 3 + r]) * M[1 * 3 + k] +
                      (gS[r * 3 + 2] + gS[2 * 3 + r]) * M[2 * 3 + k];
    }
  }
  double D[9];  // to R_q
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int k = 0; k < 3; ++k) D[r * 3 + k] = gM[r * 3 + k] * s[k];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double g_s = gM[k] * Rq[k] + gM[3 + k] * Rq[3 + k] + gM[6 + k] * Rq[6 + k];
    p.scales[i3 + k] = (float)(g_s * s[k]);
  }
  // ---- R_q -> the normalised quaternion -> the raw one
  const double gu[4] = {
      2.0 * (qy * (D[1] + D[3]) + qz * (D[2] + D[6]) - 2.0 * qx * (D[4] + D[8]) + qw * (D[7] - D[5])),
      2.0 * (qx * (D[1] + D[3]) + qz * (D[5] + D[7]) - 2.0 * qy * (D[0] + D[8]) + qw * (D[2] - D[6])),
      2.0 * (qx * (D[2] + D[6]) + qy * (D[5] + D[7]) - 2.0 * qz * (D[0] + D[4]) + qw * (D[3] - D[1])),
      2.0 * (qz * (D[3] - D[1]) + qy * (D[2] - D[6]) + qx * (D[7] - D[5]))};
  const double un[4] = {qx, qy, qz, qw};
  const double udot = un[0] * gu[0] + un[1] * gu[1] + un[2] * gu[2] + un[3] * gu[3];
#pragma unroll
  for (int k = 0; k < 4; ++k) p.rotations[i4 + k] = (float)((gu[k] - un[k] * udot) / qn);
  p.alphas[i] = (float)g_alpha;
  // ---- T and the mean -> the camera-space position
  const double g_J00 = gT[0] * R[0] + gT[1] * R[1] + gT[2] * R[2];
  const double g_J02 = gT[0] * R[6] + gT[1] * R[7] + gT[2] * R[8];
  const double g_J11 = gT[3] * R[3] + gT[4] * R[4] + gT[5] * R[5];
  const double g_J12 = gT[3] * R[6] + gT[4] * R[7] + gT[5] * R[8];
  const double g_mx = rg[0], g_my = rg[1];
  const double z2 = z * z, z3 = z2 * z;
  // J02 = -fx qx / z with qx = x / z where it is free and a constant where it is clamped
  const double g_x = g_mx * cam.fx / z - g_J02 * free_x * cam.fx / z2;
  const double g_y = g_my * cam.fy / z - g_J12 * free_y * cam.fy / z2;
  const double g_z = -(g_mx * cam.fx * x) / z2 - (g_my * cam.fy * y) / z2 - (g_J00 * cam.fx) / z2 - (g_J11 * cam.fy) / z2 +
                     g_J02 * (cam.fx * cqx / z2 + free_x * cam.fx * x / z3) +
                     g_J12 * (cam.fy * cqy / z2 + free_y * cam.fy * y / z3);
  double gp[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) gp[k] = R[k] * g_x + R[3 + k] * g_y + R[6 + k] * g_z;
  if (p.depth_grad) {  // the record's depth is z itself, rounded to f32 (straight through)
    const double g_depth = p.depth_grad[i];
#pragma unroll
    for (int k = 0; k < 3; ++k) gp[k] = gp[k] + R[6 + k] * g_depth;
  }
  // ---- rgb -> colour, sh and the view direction
  double gr[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    gr[ch] = q.rgb[ch] > 0.0f ? (double)rg[6 + ch] : 0.0;  // max(0, .) passes nothing where it clamps
    p.colors[i3 + ch] = (float)(kC0 * gr[ch]);
  }
  const uint32_t nk = cam.sh_coeffs;
  if (nk != 0u) {
    double dx = px - cam.campos[0], dy = py - cam.campos[1], dz = pz - cam.campos[2];
    const double dn = sqrt(dx * dx + dy * dy + dz * dz);
    dx /= dn;
    dy /= dn;
    dz /= dn;
    double gn[3] = {0.0, 0.0, 0.0};
    // coefficient k with basis value bv and its derivatives to the unit direction
    auto band = [&](uint32_t k, double bv, double bx, double by, double bz) {
      const unsigned long long at = ish + k * 3u;
      double ck = 0.0;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        ck = ck + gr[ch] * (double)p.src.sh[at + ch];
        p.sh[at + ch] = (float)(gr[ch] * bv);
      }
      gn[0] = gn[0] + ck * bx;
      gn[1] = gn[1] + ck * by;
      gn[2] = gn[2] + ck * bz;
    };
    band(0, -kC1 * dy, 0.0, -kC1, 0.0);
    band(1, kC1 * dz, 0.0, 0.0, kC1);
    band(2, -kC1 * dx, -kC1, 0.0, 0.0);
    if (nk >= 8u) {
      const double xx = dx * dx, yy = dy * dy, zz = dz * dz, xy = dx * dy, yz = dy * dz, xz = dx * dz;
      band(3, kC2[0] * xy, kC2[0] * dy, kC2[0] * dx, 0.0);
      band(4, kC2[1] * yz, 0.0, kC2[1] * dz, kC2[1] * dy);
      band(5, kC2[2] * (2.0 * zz - xx - yy), kC2[2] * (-2.0 * dx), kC2[2] * (-2.0 * dy), kC2[2] * (4.0 * dz));
      band(6, kC2[3] * xz, kC2[3] * dz, 0.0, kC2[3] * dx);
      band(7, kC2[4] * (xx - yy), kC2[4] * (2.0 * dx), kC2[4] * (-2.0 * dy), 0.0);
      if (nk >= 15u) {
        band(8, kC3[0] * dy * (3.0 * xx - yy), kC3[0] * (6.0 * xy), kC3[0] * (3.0 * xx - 3.0 * yy), 0.0);
        band(9, kC3[1] * xy * dz, kC3[1] * yz, kC3[1] * xz, kC3[1] * xy);
        band(10, kC3[2] * dy * (4.0 * zz - xx - yy), kC3[2] * (-2.0 * xy), kC3[2] * (4.0 * zz - xx - 3.0 * yy),
             kC3[2] * (8.0 * yz));
        band(11, kC3[3] * dz * (2.0 * zz - 3.0 * xx - 3.0 * yy), kC3[3] * (-6.0 * xz), kC3[3] * (-6.0 * yz),
             kC3[3] * (6.0 * zz - 3.0 * xx - 3.0 * yy));
        band(12, kC3[4] * dx * (4.0 * zz - xx - yy), kC3[4] * (4.0 * zz - 3.0 * xx - yy), kC3[4] * (-2.0 * xy),
             kC3[4] * (8.0 * xz));
        band(13, kC3[5] * dz * (xx - yy), kC3[5] * (2.0 * xz), kC3[5] * (-2.0 * yz), kC3[5] * (xx - yy));
        band(14, kC3[6] * dx * (xx - 3.0 * yy), kC3[6] * (3.0 * xx - 3.0 * yy), kC3[6] * (-6.0 * xy), 0.0);
      }
    }
    // through the normalisation of the direction
    const double ndot = dx * gn[0] + dy * gn[1] + dz * gn[2];
    gp[0] = gp[0] + (gn[0] - dx * ndot) / dn;
    gp[1] = gp[1] + (gn[1] - dy * ndot) / dn;
    gp[2] = gp[2] + (gn[2] - dz * ndot) / dn;
  }
  for (uint32_t e = nk * 3u; e < p.src.sh_dim * 3u; ++e) p.sh[ish + e] = 0.0f;  // above the used degree
#pragma unroll
  for (int k = 0; k < 3; ++k) p.positions[i3 + k] = (float)gp[k];
}

__global__ __launch_bounds__(kPreBlock) void spz_render_preprocess_backward_kernel(const PreprocessBackwardParams p) {
  const uint32_t i = blockIdx.x * kPreBlock + threadIdx.x;
  if (*p.total > p.max_entries) {
    if (i == 0u) *p.status = 1u;
    return;
  }
  if (i < p.n) preprocess_backward_one(p, i);
}

}  // namespace spz_amd_detail

using namespace spz_amd_detail;

namespace {

// render_backward_device (d_grad_depth null: the colour blend backward, d_grad_image required) and
// render_depth_backward_device (d_grad_depth given: the depth blend backward, d_grad_image may be null) are one
// sequence: clear the record gradients, the blend backward, the per-Gaussian chain.
int backward_impl(const spz_amd_cloud_in *d_cloud, uint64_t num_points, int sh_degree, int antialiased,
                  const spz_amd_render_params *params, uint64_t max_entries, const float *d_grad_image,
                  const float *d_grad_depth, bool depth, const spz_amd_cloud_grads *d_grads, float *d_record_grads,
                  float *d_depth_grads, uint32_t *d_status, const void *d_render_workspace, void *d_backward_workspace,
                  void *hip_stream) {
  int rc = check_params(params);
  if (rc != SPZ_AMD_OK) return rc;
  FloatSrc src;
  rc = cloud_source(d_cloud, num_points, sh_degree, &src);
  if (rc != SPZ_AMD_OK) return rc;
  if (max_entries > kMaxEntries) return SPZ_AMD_ERR_INVALID_ARG;
  if ((depth ? d_grad_depth : d_grad_image) == nullptr || d_grads == nullptr || d_status == nullptr ||
      d_render_workspace == nullptr || d_backward_workspace == nullptr) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  if (num_points && (!d_grads->positions || !d_grads->scales || !d_grads->rotations || !d_grads->alphas ||
                     !d_grads->colors || (src.sh_dim > 0 && !d_grads->sh))) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  const hipStream_t st = static_cast<hipStream_t>(hip_stream);
  SPZ_HIP_TRY(hipMemsetAsync(d_status, 0, sizeof(uint32_t), st));
  if (num_points == 0) return SPZ_AMD_OK;  // the total is 0 and there is nothing to write
  const RenderLayout wl = render_layout(num_points, max_entries);
  const uint8_t *base = align_ws(const_cast<void *>(d_render_workspace));
  uint8_t *bws = align_ws(d_backward_workspace);
  float *rec_grad = reinterpret_cast<float *>(bws);
  // the n depth gradients follow the n x 9 record gradients
  float *depth_grad = depth ? reinterpret_cast<float *>(bws + al(num_points * kRecGrads * sizeof(float))) : nullptr;
  SPZ_HIP_TRY(hipMemsetAsync(rec_grad, 0, num_points * kRecGrads * sizeof(float), st));
  if (depth) SPZ_HIP_TRY(hipMemsetAsync(depth_grad, 0, num_points * sizeof(float), st));
  BlendBackwardParams b = {};
  const dim3 grid = fill_blend_params(b, wl, base, base + wl.prefix, params, max_entries);
  b.grad_image = d_grad_image;
  b.rec_grad = rec_grad;
  if (depth) {
    DepthBlendBackwardParams db = {};
    db.b = b;
    db.grad_depth = d_grad_depth;
    db.depth_grad = depth_grad;
    hipLaunchKernelGGL(spz_render_depth_blend_backward_kernel, grid, dim3(kBlendThreads), 0, st, db);
  } else {
    hipLaunchKernelGGL(spz_render_blend_backward_kernel, grid, dim3(kBlendThreads), 0, st, b);
  }
  SPZ_HIP_TRY(hipGetLastError());
  PreprocessBackwardParams q = {};
  q.src = src;
  q.cam = make_cam(params, sh_degree, antialiased);
  q.rec = b.rec;
  q.rec_grad = rec_grad;
  q.total = b.total;
  q.max_entries = max_entries;
  q.positions = d_grads->positions;
  q.scales = d_grads->scales;
  q.rotations = d_grads->rotations;
  q.alphas = d_grads->alphas;
  q.colors = d_grads->colors;
  q.sh = d_grads->sh;
  q.rec_grad_out = d_record_grads;
  q.status = d_status;
  q.n = (uint32_t)num_points;
  q.depth_grad = depth_grad;
  q.depth_grad_out = depth ? d_depth_grads : nullptr;
  hipLaunchKernelGGL(spz_render_preprocess_backward_kernel, dim3((unsigned)((num_points + kPreBlock - 1) / kPreBlock)),
                     dim3(kPreBlock), 0, st, q);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

}  // namespace

extern "C" {

uint64_t spz_amd_render_backward_workspace_bytes(uint64_t num_points) {
  return al(num_points * kRecGrads * sizeof(float)) + 256u;  // room to align a caller's pointer up to 256
}

int spz_amd_render_backward_device(const spz_amd_cloud_in *d_cloud, uint64_t num_points, int sh_degree, int antialiased,
                                   const spz_amd_render_params *params, uint64_t max_entries, const float *d_image,
                                   const float *d_grad_image, const spz_amd_cloud_grads *d_grads, float *d_record_grads,
                                   uint32_t *d_status, const void *d_render_workspace, void *d_backward_workspace,
                                   void *hip_stream) {
  (void)d_image;  // the blend runs again instead: see the contract
  return backward_impl(d_cloud, num_points, sh_degree, antialiased, params, max_entries, d_grad_image, nullptr, false,
                       d_grads, d_record_grads, nullptr, d_status, d_render_workspace, d_backward_workspace, hip_stream);
}

uint64_t spz_amd_render_depth_backward_workspace_bytes(uint64_t num_points) {
  // the n x 9 record gradients, the n depth gradients, and room to align a caller's pointer up to 256
  return al(num_points * kRecGrads * sizeof(float)) + al(num_points * sizeof(float)) + 256u;
}

int spz_amd_render_depth_backward_device(const spz_amd_cloud_in *d_cloud, uint64_t num_points, int sh_degree,
                                         int antialiased, const spz_amd_render_params *params, uint64_t max_entries,
                                         const float *d_grad_image, const float *d_grad_depth,
                                         const spz_amd_cloud_grads *d_grads, float *d_record_grads, float *d_depth_grads,
                                         uint32_t *d_status, const void *d_render_workspace, void *d_backward_workspace,
                                         void *hip_stream) {
  return backward_impl(d_cloud, num_points, sh_degree, antialiased, params, max_entries, d_grad_image, d_grad_depth, true,
                       d_grads, d_record_grads, d_depth_grads, d_status, d_render_workspace, d_backward_workspace,
                       hip_stream);
}

}  // extern "C"

// ---- the blend half on its own ("render view backward": the pose fit needs no gradients to the cloud)
namespace spz_amd_detail {

// Zeroes the caller's n x 9 record gradients for the blend backward to add into; with the total above max_entries it
// sets the status instead and writes nothing, as the blend backward then adds nothing.
__global__ __launch_bounds__(kPreBlock) void spz_render_records_clear_kernel(float *__restrict__ rec_grad,
                                                                             unsigned long long count,
                                                                             const unsigned long long *total,
                                                                             unsigned long long max_entries,
                                                                             uint32_t *status) {
  const unsigned long long j = (unsigned long long)blockIdx.x * kPreBlock + threadIdx.x;
  if (*total > max_entries) {
    if (j == 0ull) *status = 1u;
    return;
  }
  if (j < count) rec_grad[j] = 0.0f;
}

}  // namespace spz_amd_detail

extern "C" {

int spz_amd_render_records_backward_device(uint64_t num_points, const spz_amd_render_params *params,
                                           uint64_t max_entries, const float *d_grad_image, float *d_record_grads,
                                           uint32_t *d_status, const void *d_render_workspace, void *hip_stream) {
  int rc = check_params(params);
  if (rc != SPZ_AMD_OK) return rc;
  if (num_points > kMaxEntries) return SPZ_AMD_ERR_TOO_MANY_POINTS;
  if (max_entries > kMaxEntries) return SPZ_AMD_ERR_INVALID_ARG;
  if (d_grad_image == nullptr || d_status == nullptr || d_render_workspace == nullptr ||
      (num_points && d_record_grads == nullptr)) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  const hipStream_t st = static_cast<hipStream_t>(hip_stream);
  SPZ_HIP_TRY(hipMemsetAsync(d_status, 0, sizeof(uint32_t), st));
  if (num_points == 0) return SPZ_AMD_OK;  // the total is 0 and there is nothing to write
  const RenderLayout wl = render_layout(num_points, max_entries);
  const uint8_t *base = align_ws(const_cast<void *>(d_render_workspace));
  BlendBackwardParams b = {};
  const dim3 grid = fill_blend_params(b, wl, base, base + wl.prefix, params, max_entries);
  b.grad_image = d_grad_image;
  b.rec_grad = d_record_grads;
  const unsigned long long count = (unsigned long long)num_points * kRecGrads;
  hipLaunchKernelGGL(spz_render_records_clear_kernel, dim3((unsigned)((count + kPreBlock - 1) / kPreBlock)),
                     dim3(kPreBlock), 0, st, d_record_grads, count, b.total, max_entries, d_status);
  SPZ_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(spz_render_blend_backward_kernel, grid, dim3(kBlendThreads), 0, st, b);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

}  // extern "C"
