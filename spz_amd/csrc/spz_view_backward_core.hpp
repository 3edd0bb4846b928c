// spz_view_backward_core.hpp — one Gaussian's part of the gradient of a view to its camera (DESIGN §8 "Locate"; the
// contract is in include/spz_amd.h "render view backward").  Host and device: the arithmetic has no device-only part,
// so a CPU build can check it (tools/view_grad_check.cpp).
#pragma once

#include <cmath>
#include <cstdint>

#include "spz_amd.h"
#include "spz_render_internal.hpp"

#pragma clang fp contract(off)

namespace spz_amd_detail {

constexpr uint32_t kViewGrads = 12;  // [R | t], row-major 3 x 4

struct ViewBackwardParams {
  FloatSrc src;
  RenderCam cam;
  const spz_amd_render_record *rec;
  const float *rec_grad;  // n x 9
  const unsigned long long *total;
  unsigned long long max_entries;
  double *partials;  // one row of 12 per workgroup
  uint32_t *status;
  uint32_t n;
};

// The forward's symbols are those of preprocess_backward_one (spz_render_backward.hip): p_c = R p + t = (x, y, z),
// S = Sigma, J with the clamped quotients, T = J R, cov = T S T^T, conic, opacity, rgb.  The camera enters three times:
//   p_c = R p + t        dL/dR += g_pc p^T,  dL/dt += g_pc      (g_pc: through the mean and through J)
//   T = J R              dL/dR += J^T gT                        (gT: the gradient to the 2 x 3 T)
//   c = -R^T t           dL/dR += t g_d^T,   dL/dt += R g_d     (g_d = -dL/dc: the gradient the position gets through
//                                                                the view direction normalize(p - c))
// out: the 12 contributions of Gaussian i, zero when it is invisible.
__host__ __device__ inline void view_backward_one(const ViewBackwardParams &p, uint32_t i, double out[kViewGrads]) {
  const unsigned long long i3 = (unsigned long long)i * 3u, i4 = (unsigned long long)i * 4u;
  const unsigned long long ish = (unsigned long long)i * p.src.sh_dim * 3u;
  const RenderCam &cam = p.cam;
#pragma unroll
  for (uint32_t e = 0; e < kViewGrads; ++e) out[e] = 0.0;
  const spz_amd_render_record q = p.rec[i];
  if (!(q.depth < __builtin_huge_valf())) return;  // invisible: the forward's own decision
  float rg[9];
#pragma unroll
  for (uint32_t e = 0; e < 9; ++e) rg[e] = p.rec_grad[(unsigned long long)i * 9u + e];
  // ---- the forward again
  const double px = p.src.positions[i3], py = p.src.positions[i3 + 1], pz = p.src.positions[i3 + 2];
  const float q0 = p.src.rotations[i4], q1 = p.src.rotations[i4 + 1], q2 = p.src.rotations[i4 + 2],
              q3 = p.src.rotations[i4 + 3];
  const double *R = cam.R;
  const double x = R[0] * px + R[1] * py + R[2] * pz + cam.t[0];
  const double y = R[3] * px + R[4] * py + R[5] * pz + cam.t[1];
  const double z = R[6] * px + R[7] * py + R[8] * pz + cam.t[2];
  const double qn = sqrt((double)q0 * q0 + (double)q1 * q1 + (double)q2 * q2 + (double)q3 * q3);
  const double qx = q0 / qn, qy = q1 / qn, qz = q2 / qn, qw = q3 / qn;
  const double Rq[9] = {1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy),
                        2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx),
                        2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)};
  const double s[3] = {exp((double)p.src.scales[i3]), exp((double)p.src.scales[i3 + 1]),
                       exp((double)p.src.scales[i3 + 2])};
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
  const double sig = 1.0 / (1.0 + exp(-(double)p.src.alphas[i]));
  const bool aa = cam.antialiased && det0 > 0.0;
  const double h = cam.antialiased ? sqrt((det0 > 0.0 ? det0 : 0.0) / det) : 1.0;
  // ---- conic and opacity -> cov -> T
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
  double gT[6];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    gT[k] = 2.0 * g_a * TS[k] + g_b * TS[3 + k];
    gT[3 + k] = g_b * TS[k] + 2.0 * g_c * TS[3 + k];
  }
  // ---- T and the mean -> the camera-space position
  const double g_J00 = gT[0] * R[0] + gT[1] * R[1] + gT[2] * R[2];
  const double g_J02 = gT[0] * R[6] + gT[1] * R[7] + gT[2] * R[8];
  const double g_J11 = gT[3] * R[3] + gT[4] * R[4] + gT[5] * R[5];
  const double g_J12 = gT[3] * R[6] + gT[4] * R[7] + gT[5] * R[8];
  const double g_mx = rg[0], g_my = rg[1];
  const double z2 = z * z, z3 = z2 * z;
  double gpc[3];
  gpc[0] = g_mx * cam.fx / z - g_J02 * free_x * cam.fx / z2;
  gpc[1] = g_my * cam.fy / z - g_J12 * free_y * cam.fy / z2;
  gpc[2] = -(g_mx * cam.fx * x) / z2 - (g_my * cam.fy * y) / z2 - (g_J00 * cam.fx) / z2 - (g_J11 * cam.fy) / z2 +
           g_J02 * (cam.fx * cqx / z2 + free_x * cam.fx * x / z3) + g_J12 * (cam.fy * cqy / z2 + free_y * cam.fy * y / z3);
  // ---- rgb -> the view direction
  double gd[3] = {0.0, 0.0, 0.0};
  const uint32_t nk = cam.sh_coeffs;
  if (nk != 0u) {
    double gr[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) gr[ch] = q.rgb[ch] > 0.0f ? (double)rg[6 + ch] : 0.0;  // max(0, .) passes nothing where it clamps
    double dx = px - cam.campos[0], dy = py - cam.campos[1], dz = pz - cam.campos[2];
    const double dn = sqrt(dx * dx + dy * dy + dz * dz);
    dx /= dn;
    dy /= dn;
    dz /= dn;
    double gn[3] = {0.0, 0.0, 0.0};
    // coefficient k with its basis value's derivatives to the unit direction
    auto band = [&](uint32_t k, double bx, double by, double bz) {
      const unsigned long long at = ish + k * 3u;
      double ck = 0.0;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) ck = ck + gr[ch] * (double)p.src.sh[at + ch];
      gn[0] = gn[0] + ck * bx;
      gn[1] = gn[1] + ck * by;
      gn[2] = gn[2] + ck * bz;
    };
    band(0, 0.0, -kC1, 0.0);
    band(1, 0.0, 0.0, kC1);
    band(2, -kC1, 0.0, 0.0);
    if (nk >= 8u) {
      const double xx = dx * dx, yy = dy * dy, zz = dz * dz, xy = dx * dy, yz = dy * dz, xz = dx * dz;
      band(3, kC2[0] * dy, kC2[0] * dx, 0.0);
      band(4, 0.0, kC2[1] * dz, kC2[1] * dy);
      band(5, kC2[2] * (-2.0 * dx), kC2[2] * (-2.0 * dy), kC2[2] * (4.0 * dz));
      band(6, kC2[3] * dz, 0.0, kC2[3] * dx);
      band(7, kC2[4] * (2.0 * dx), kC2[4] * (-2.0 * dy), 0.0);
      if (nk >= 15u) {
        band(8, kC3[0] * (6.0 * xy), kC3[0] * (3.0 * xx - 3.0 * yy), 0.0);
        band(9, kC3[1] * yz, kC3[1] * xz, kC3[1] * xy);
        band(10, kC3[2] * (-2.0 * xy), kC3[2] * (4.0 * zz - xx - 3.0 * yy), kC3[2] * (8.0 * yz));
        band(11, kC3[3] * (-6.0 * xz), kC3[3] * (-6.0 * yz), kC3[3] * (6.0 * zz - 3.0 * xx - 3.0 * yy));
        band(12, kC3[4] * (4.0 * zz - 3.0 * xx - yy), kC3[4] * (-2.0 * xy), kC3[4] * (8.0 * xz));
        band(13, kC3[5] * (2.0 * xz), kC3[5] * (-2.0 * yz), kC3[5] * (xx - yy));
        band(14, kC3[6] * (3.0 * xx - 3.0 * yy), kC3[6] * (-6.0 * xy), 0.0);
      }
    }
    // through the normalisation of the direction
    const double ndot = dx * gn[0] + dy * gn[1] + dz * gn[2];
    gd[0] = (gn[0] - dx * ndot) / dn;
    gd[1] = (gn[1] - dy * ndot) / dn;
    gd[2] = (gn[2] - dz * ndot) / dn;
  }
  // ---- the three paths into [R | t]
  const double pw[3] = {px, py, pz};
  const double Jc0[3] = {J00, 0.0, J02}, Jc1[3] = {0.0, J11, J12};  // J's two rows
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      out[r * 4 + k] = (gpc[r] * pw[k] + (Jc0[r] * gT[k] + Jc1[r] * gT[3 + k])) + cam.t[r] * gd[k];
    }
    out[r * 4 + 3] = gpc[r] + (R[r * 3] * gd[0] + R[r * 3 + 1] * gd[1] + R[r * 3 + 2] * gd[2]);
  }
}

}  // namespace spz_amd_detail
