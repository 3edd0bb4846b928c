// spz_preprocess_backward_core.hpp — one Gaussian's chain from the nine record gradients to the cloud's six arrays
// (DESIGN §8 "Render backward"; the contract is in include/spz_amd.h "render backward"): the lane's work of
// spz_render_preprocess_backward_kernel (spz_render_backward.hip).  Host and device: the arithmetic has no device-only
// part, so a CPU build can check it (tests/cpp/render_chain_host.cpp), as spz_view_backward_core.hpp's.
#pragma once

#include <cmath>
#include <cstdint>

#include "spz_amd.h"
#include "spz_render_internal.hpp"

#pragma clang fp contract(off)

namespace spz_amd_detail {

constexpr uint32_t kRecGrads = 9;  // mean 2, conic 3, opacity 1, rgb 3: the record's first nine floats

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

}  // namespace spz_amd_detail
