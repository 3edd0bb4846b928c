// spz_decimate.hip — a coarser version of a packed stream (DESIGN §8 "Decimate"): one point per occupied octree cell of
// edge 2^L quanta, in ascending Morton order of the cells.  The input is put in Morton order first (spz_sort.hip's
// spz_amd_morton_order_device, then the filter's spz_amd_subset_device), so the points of every cell at every level are
// contiguous and each level is a segmented reduction over the sorted stream.
//
//   spz_dec_hist_kernel      per tile of kDecTile sorted points, the histogram of the level at which each point leaves
//                            its predecessor's cell: max_a msb(u_a ^ u'_a) (= msb of the Morton XOR / 3), bin 24: equal.
//   spz_dec_levels_kernel    one workgroup: the tiles' histograms summed, then cells(L) = 1 + #{bin in L..23}.
//   spz_dec_flags_kernel     per tile, the number of cell starts at level L and of non-zero alpha bytes (one u64).
//   spz_dec_scan_kernel      one workgroup: exclusive scan of those pairs; the cell count m, the output header.
//   spz_dec_apply_kernel     per tile: every point's cell (output index), each cell's first point and its alpha count
//                            prefix, parents through the order.
//   spz_dec_reduce_kernel<D> one wave per 64 points: the moments of every point, a segmented inclusive scan over the
//                            wave (shuffles, fixed order).  A cell that starts and ends in the wave is finished by its
//                            last lane (one point: its bytes copied); the partials of cells that cross the wave's edges
//                            go to the workspace.
//   spz_dec_combine_kernel<D> one workgroup per wave tile whose last cell runs on: that cell's partials summed in tile
//                            order (fixed assignment to threads, then a fixed tree), finished by thread 0.
// No float atomics and no inter-workgroup waits: every sum is taken in an order fixed by n alone, so a run repeats its
// bytes.
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
#include "spz_xf.hpp"

#pragma clang fp contract(off)

namespace spz_amd_detail {
namespace {

constexpr uint32_t kDecBlock = kOpsBlock;  // 256
constexpr uint32_t kDecItems = 8;                          // contiguous points per thread of the integer passes
constexpr uint32_t kDecTile = kDecBlock * kDecItems;       // 2048 points per tile
constexpr uint32_t kDecLevels = 25;                        // L = 0..24
constexpr uint32_t kWaveTile = 64;                         // points per wave of the moment reduction
constexpr uint32_t kMagic = 0x5053474eu;                   // load-spz.cc:132

// The moments of a set of points (see decimate in spz_amd.h): W, sum w p (quanta from the cell origin), sum w (p p^T +
// Sigma_i) (quanta^2; xx, xy, xz, yy, yz, zz) in f64; sum w c and sum w sh in f32.  The workspace form holds degree 3.
struct MomentSlot {
  double w, p[3], q[6];
  float c[3], h[45];
};

template <int D3>
struct Moments {
  double w, p[3], q[6];
  float c[3], h[D3 > 0 ? D3 : 1];
};

struct DecPlan {
  uint32_t m;         // output points
  uint32_t ok;        // the output fits the caller's capacity
};

// Sections of the sorted (input-version) stream and of the v3 output.
struct DecIo {
  const uint8_t *pos, *alpha, *color, *scale, *rot, *sh;   // sorted stream
  uint32_t version, n, level, fb;
  uint8_t *out;                                            // output stream base
};

__device__ __forceinline__ void load_u(const uint8_t *pos, unsigned long long i, uint32_t u[3]) {
  const uint8_t *b = pos + i * 9ull;
#pragma unroll
  for (uint32_t a = 0; a < 3; ++a) {
    u[a] = ((uint32_t)b[3 * a] | ((uint32_t)b[3 * a + 1] << 8) | ((uint32_t)b[3 * a + 2] << 16)) ^ 0x800000u;
  }
}

// The level at which point i leaves point i - 1's cell: max over axes of msb(u_a ^ u'_a); 24 when they are equal.
__device__ __forceinline__ uint32_t leave_bin(const uint8_t *pos, unsigned long long i) {
  uint32_t u[3], v[3];
  load_u(pos, i, u);
  load_u(pos, i - 1ull, v);
  const uint32_t x = (u[0] ^ v[0]) | (u[1] ^ v[1]) | (u[2] ^ v[2]);
  return x ? 31u - (uint32_t)__clz(x) : 24u;
}

__device__ __forceinline__ bool cell_start(const uint8_t *pos, unsigned long long i, uint32_t level) {
  if (i == 0) return true;
  const uint32_t b = leave_bin(pos, i);
  return b < 24u && b >= level;
}

// Offsets of the v3 output of m points at dim sh coefficients.
struct OutLayout {
  unsigned long long pos, alpha, color, scale, rot, sh, total;
};
__device__ __host__ __forceinline__ OutLayout out_layout(unsigned long long m, uint32_t dim) {
  OutLayout o;
  o.pos = 16;
  o.alpha = o.pos + 9ull * m;
  o.color = o.alpha + m;
  o.scale = o.color + 3ull * m;
  o.rot = o.scale + 3ull * m;
  o.sh = o.rot + 4ull * m;
  o.total = o.sh + 3ull * dim * m;
  return o;
}

// ---- the per-point moments ---------------------------------------------------------------------------------------
template <int D3>
__device__ __forceinline__ void zero(Moments<D3> &a) {
  a.w = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) a.p[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) a.q[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) a.c[k] = 0.0f;
#pragma unroll
  for (int k = 0; k < (D3 > 0 ? D3 : 1); ++k) a.h[k] = 0.0f;
}

template <int D3>
__device__ __forceinline__ void add(Moments<D3> &a, const Moments<D3> &b) {
  a.w += b.w;
#pragma unroll
  for (int k = 0; k < 3; ++k) a.p[k] += b.p[k];
#pragma unroll
  for (int k = 0; k < 6; ++k) a.q[k] += b.q[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) a.c[k] += b.c[k];
#pragma unroll
  for (int k = 0; k < D3; ++k) a.h[k] += b.h[k];
}

template <int D3>
__device__ __forceinline__ void to_slot(const Moments<D3> &a, MomentSlot *s) {
  s->w = a.w;
#pragma unroll
  for (int k = 0; k < 3; ++k) s->p[k] = a.p[k];
#pragma unroll
  for (int k = 0; k < 6; ++k) s->q[k] = a.q[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) s->c[k] = a.c[k];
#pragma unroll
  for (int k = 0; k < D3; ++k) s->h[k] = a.h[k];
}

template <int D3>
__device__ __forceinline__ void from_slot(const MomentSlot *s, Moments<D3> &a) {
  a.w = s->w;
#pragma unroll
  for (int k = 0; k < 3; ++k) a.p[k] = s->p[k];
#pragma unroll
  for (int k = 0; k < 6; ++k) a.q[k] = s->q[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) a.c[k] = s->c[k];
#pragma unroll
  for (int k = 0; k < D3; ++k) a.h[k] = s->h[k];
}

// Point i of the sorted stream, decoded with the decoder's arithmetic: w = alpha_byte / 255 * exp(ls_x + ls_y + ls_z)
// (unit_weight: 1), p = u - origin in quanta, Sigma_i = R diag(exp(2 ls)) R^T (R of the normalised decoded quaternion)
// in quanta^2.
template <int D3>
__device__ __forceinline__ void point_moments(const DecIo &io, unsigned long long i, const uint32_t u[3],
                                              const uint32_t origin[3], bool unit_weight, Moments<D3> &a) {
  float ls[3];
#pragma unroll
  for (uint32_t k = 0; k < 3; ++k) ls[k] = scale_from_byte(io.scale[i * 3ull + k]);
  const double w = unit_weight ? 1.0 : ((double)io.alpha[i] / 255.0) * exp((double)(ls[0] + ls[1] + ls[2]));
  F32x4 r;
  if (io.version >= 3u) {
    r = unpack_quat_smallest_three(*reinterpret_cast<const u32_a1 *>(io.rot + i * 4ull), 0u);
  } else {
    const uint8_t *b = io.rot + i * 3ull;
    r = unpack_quat_first_three((uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16), 0u);
  }
  double x = r.x, y = r.y, z = r.z, qw = r.w;
  const double nq = sqrt(x * x + y * y + z * z + qw * qw);
  if (nq > 0.0) {
    x /= nq;
    y /= nq;
    z /= nq;
    qw /= nq;
  }
  const double R[3][3] = {{1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - qw * z), 2.0 * (x * z + qw * y)},
                          {2.0 * (x * y + qw * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - qw * x)},
                          {2.0 * (x * z - qw * y), 2.0 * (y * z + qw * x), 1.0 - 2.0 * (x * x + y * y)}};
  const double q2 = ldexp(1.0, 2 * (int)io.fb);  // world^2 -> quanta^2
  double s2[3];
#pragma unroll
  for (uint32_t k = 0; k < 3; ++k) s2[k] = exp(2.0 * (double)ls[k]) * q2;
  double p[3];
#pragma unroll
  for (uint32_t k = 0; k < 3; ++k) p[k] = (double)(u[k] - origin[k]);
  constexpr int QA[6] = {0, 0, 0, 1, 1, 2}, QB[6] = {0, 1, 2, 1, 2, 2};
  a.w = w;
#pragma unroll
  for (uint32_t k = 0; k < 3; ++k) a.p[k] = w * p[k];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int ra = QA[k], rb = QB[k];
    const double sig = R[ra][0] * R[rb][0] * s2[0] + R[ra][1] * R[rb][1] * s2[1] + R[ra][2] * R[rb][2] * s2[2];
    a.q[k] = w * (p[ra] * p[rb] + sig);
  }
  const float wf = (float)w;
#pragma unroll
  for (uint32_t k = 0; k < 3; ++k) {
    const float c = ((float)io.color[i * 3ull + k] / 255.0f - 0.5f) / 0.15f;  // load-spz.cc:522
    a.c[k] = wf * c;
  }
#pragma unroll
  for (int k = 0; k < D3; ++k) a.h[k] = wf * sh_from_byte(io.sh[i * (unsigned long long)D3 + k]);
}

// ---- one output point --------------------------------------------------------------------------------------------
__device__ __forceinline__ void put_position(const DecIo &io, const OutLayout &o, uint32_t s, const uint32_t u[3]) {
  uint8_t *d = io.out + o.pos + 9ull * s;
#pragma unroll
  for (uint32_t a = 0; a < 3; ++a) {
    const uint32_t f = (u[a] ^ 0x800000u) & 0xffffffu;
    d[3 * a] = (uint8_t)f;
    d[3 * a + 1] = (uint8_t)(f >> 8);
    d[3 * a + 2] = (uint8_t)(f >> 16);
  }
}

// A cell of one point: its bytes, the rotation re-encoded from a v2 input (as mergeSpz copies a point).
template <int D3>
__device__ __forceinline__ void copy_point(const DecIo &io, const OutLayout &o, uint32_t s, unsigned long long i) {
  const uint8_t *ps = io.pos + i * 9ull;
  uint8_t *pd = io.out + o.pos + 9ull * s;
#pragma unroll
  for (uint32_t k = 0; k < 9; ++k) pd[k] = ps[k];
  io.out[o.alpha + s] = io.alpha[i];
#pragma unroll
  for (uint32_t k = 0; k < 3; ++k) {
    io.out[o.color + 3ull * s + k] = io.color[i * 3ull + k];
    io.out[o.scale + 3ull * s + k] = io.scale[i * 3ull + k];
  }
  uint32_t r;
  if (io.version >= 3u) {
    const uint8_t *b = io.rot + i * 4ull;
    r = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
  } else {
    r = xf_rotation_point(io.rot, i, io.version, nullptr);
  }
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) io.out[o.rot + 4ull * s + k] = (uint8_t)(r >> (8u * k));
#pragma unroll
  for (int k = 0; k < D3; ++k) io.out[o.sh + (unsigned long long)D3 * s + k] = io.sh[i * (unsigned long long)D3 + k];
}

// Symmetric 3x3 eigen-decomposition by cyclic Jacobi (fixed sweeps): A is destroyed, V gets the eigenvectors as columns.
__device__ __forceinline__ void jacobi3(double A[3][3], double V[3][3]) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) V[r][c] = r == c ? 1.0 : 0.0;
  }
  constexpr int P[3] = {0, 0, 1}, Q[3] = {1, 2, 2};
  for (int sweep = 0; sweep < 12; ++sweep) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int p = P[k], q = Q[k];
      const double apq = A[p][q];
      if (apq == 0.0) continue;
      const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
      const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
      const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
      for (int j = 0; j < 3; ++j) {  // A <- J^T A J, J the rotation in the (p, q) plane
        const double ajp = A[j][p], ajq = A[j][q];
        A[j][p] = c * ajp - s * ajq;
        A[j][q] = s * ajp + c * ajq;
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double apj = A[p][j], aqj = A[q][j];
        A[p][j] = c * apj - s * aqj;
        A[q][j] = s * apj + c * aqj;
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double vjp = V[j][p], vjq = V[j][q];
        V[j][p] = c * vjp - s * vjq;
        V[j][q] = s * vjp + c * vjq;
      }
    }
  }
}

// A cell of several points from its moments: position, covariance -> scales + rotation, mass-conserving alpha,
// w-weighted colour and sh, each through the encoder's arithmetic.
template <int D3>
__device__ void finish_cell(const DecIo &io, const OutLayout &o, uint32_t s, const Moments<D3> &a,
                            const uint32_t origin[3], bool unit_weight) {
  const double W = a.w;
  double mu[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) mu[k] = a.p[k] / W;
  const double q2 = ldexp(1.0, -2 * (int)io.fb);  // quanta^2 -> world^2
  double A[3][3];
  constexpr int QA[6] = {0, 0, 0, 1, 1, 2}, QB[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const double v = (a.q[k] / W - mu[QA[k]] * mu[QB[k]]) * q2;
    A[QA[k]][QB[k]] = v;
    A[QB[k]][QA[k]] = v;
  }
  double V[3][3];
  jacobi3(A, V);
  double lam[3] = {A[0][0], A[1][1], A[2][2]};
  int idx[3] = {0, 1, 2};
  // descending, ties in index order
  if (lam[idx[1]] > lam[idx[0]]) { const int t = idx[0]; idx[0] = idx[1]; idx[1] = t; }
  if (lam[idx[2]] > lam[idx[1]]) { const int t = idx[1]; idx[1] = idx[2]; idx[2] = t; }
  if (lam[idx[1]] > lam[idx[0]]) { const int t = idx[0]; idx[0] = idx[1]; idx[1] = t; }
  double M[3][3], ls[3];
  const double floor_l = exp(-20.0);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double l = lam[idx[c]];
    ls[c] = 0.5 * log(l > floor_l ? l : floor_l);
#pragma unroll
    for (int r = 0; r < 3; ++r) M[r][c] = V[r][idx[c]];
  }
  const double det = M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
                     M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
  if (det < 0.0) {
#pragma unroll
    for (int r = 0; r < 3; ++r) M[r][2] = -M[r][2];
  }
  // rotation matrix -> quaternion (x, y, z, w)
  double qx, qy, qz, qw;
  const double tr = M[0][0] + M[1][1] + M[2][2];
  if (tr > 0.0) {
    const double t = sqrt(tr + 1.0) * 2.0;
    qw = 0.25 * t;
    qx = (M[2][1] - M[1][2]) / t;
    qy = (M[0][2] - M[2][0]) / t;
    qz = (M[1][0] - M[0][1]) / t;
  } else if (M[0][0] > M[1][1] && M[0][0] > M[2][2]) {
    const double t = sqrt(1.0 + M[0][0] - M[1][1] - M[2][2]) * 2.0;
    qw = (M[2][1] - M[1][2]) / t;
    qx = 0.25 * t;
    qy = (M[0][1] + M[1][0]) / t;
    qz = (M[0][2] + M[2][0]) / t;
  } else if (M[1][1] > M[2][2]) {
    const double t = sqrt(1.0 + M[1][1] - M[0][0] - M[2][2]) * 2.0;
    qw = (M[0][2] - M[2][0]) / t;
    qx = (M[0][1] + M[1][0]) / t;
    qy = 0.25 * t;
    qz = (M[1][2] + M[2][1]) / t;
  } else {
    const double t = sqrt(1.0 + M[2][2] - M[0][0] - M[1][1]) * 2.0;
    qw = (M[1][0] - M[0][1]) / t;
    qx = (M[0][2] + M[2][0]) / t;
    qy = (M[1][2] + M[2][1]) / t;
    qz = 0.25 * t;
  }
  F32x4 qf;
  qf.x = (float)qx;
  qf.y = (float)qy;
  qf.z = (float)qz;
  qf.w = (float)qw;
  const uint32_t rot = pack_quat_smallest_three(qf, 0u);
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) io.out[o.rot + 4ull * s + k] = (uint8_t)(rot >> (8u * k));
#pragma unroll
  for (int k = 0; k < 3; ++k) io.out[o.scale + 3ull * s + k] = (uint8_t)scale_to_byte_f((float)ls[k]);
  // alpha: the mass of the cell over the output's volume, before the scale encoder's clamp
  const double alpha = unit_weight ? 0.0 : fmin(1.0, W / exp(ls[0] + ls[1] + ls[2]));
  const double ab = round(255.0 * alpha);  // half away from zero
  io.out[o.alpha + s] = (uint8_t)(ab < 0.0 ? 0.0 : (ab > 255.0 ? 255.0 : ab));
  constexpr float kc = 0.15f * 255.0f, hc = 0.5f * 255.0f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float c = (float)((double)a.c[k] / W);
    io.out[o.color + 3ull * s + k] = (uint8_t)to_uint8_f(fmul_sep(c, kc) + hc);  // load-spz.cc:306
  }
#pragma unroll
  for (int k = 0; k < D3; ++k) {
    const float v = (float)((double)a.h[k] / W);
    io.out[o.sh + (unsigned long long)D3 * s + k] = (uint8_t)quantize_sh_f(v, k < 9);  // coefficients 0..2: degree 1
  }
  // position: origin + the rounded mean, inside the cell
  const long long edge = 1ll << io.level;
  uint32_t u[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    long long r = (long long)round(mu[k]);
    r = r < 0 ? 0 : (r > edge - 1 ? edge - 1 : r);
    u[k] = origin[k] + (uint32_t)r;
  }
  put_position(io, o, s, u);
}

__device__ __forceinline__ void cell_origin(const uint8_t *pos, unsigned long long i, uint32_t level, uint32_t o[3]) {
  load_u(pos, i, o);
#pragma unroll
  for (int k = 0; k < 3; ++k) o[k] = level >= 24u ? 0u : (o[k] >> level) << level;
}

// shfl_up of every field
template <int D3>
__device__ __forceinline__ void shfl_up_add(Moments<D3> &a, uint32_t d, bool take) {
  Moments<D3> b;
  b.w = __shfl_up(a.w, d);
#pragma unroll
  for (int k = 0; k < 3; ++k) b.p[k] = __shfl_up(a.p[k], d);
#pragma unroll
  for (int k = 0; k < 6; ++k) b.q[k] = __shfl_up(a.q[k], d);
#pragma unroll
  for (int k = 0; k < 3; ++k) b.c[k] = __shfl_up(a.c[k], d);
#pragma unroll
  for (int k = 0; k < D3; ++k) b.h[k] = __shfl_up(a.h[k], d);
  if (take) add(a, b);
}

template <int D3>
__device__ __forceinline__ void shfl_xor_add(Moments<D3> &a, int m) {
  Moments<D3> b;
  b.w = __shfl_xor(a.w, m);
#pragma unroll
  for (int k = 0; k < 3; ++k) b.p[k] = __shfl_xor(a.p[k], m);
#pragma unroll
  for (int k = 0; k < 6; ++k) b.q[k] = __shfl_xor(a.q[k], m);
#pragma unroll
  for (int k = 0; k < 3; ++k) b.c[k] = __shfl_xor(a.c[k], m);
#pragma unroll
  for (int k = 0; k < D3; ++k) b.h[k] = __shfl_xor(a.h[k], m);
  // the lower lane's value first on both sides: the same sum in every lane
  if (((int)threadIdx.x & m) == 0) {
    add(a, b);
  } else {
    add(b, a);
    a = b;
  }
}

struct ReduceParams {
  DecIo io;
  const uint32_t *seg;        // [n] output index of every sorted point
  const uint32_t *start;      // [m + 1] first sorted point of every cell, start[m] = n
  const uint32_t *nz_start;   // [m + 1] non-zero alpha bytes before the cell's first point
  const DecPlan *plan;
  MomentSlot *head;           // [wave tiles] the wave's first cell, begun in an earlier wave
  MomentSlot *tail;           // [wave tiles] the wave's last cell, begun in it and running on
  uint32_t *tail_cell;        // [wave tiles] that cell, or 0xffffffff
  uint32_t sh_dim, tiles;
};

}  // namespace

__global__ __launch_bounds__(kDecBlock) void spz_dec_hist_kernel(const uint8_t *pos, uint32_t n, uint32_t *hist) {
  __shared__ uint32_t h[32];
  if (threadIdx.x < 32) h[threadIdx.x] = 0;
  __syncthreads();
  const unsigned long long first = (unsigned long long)blockIdx.x * kDecTile;
#pragma unroll
  for (uint32_t r = 0; r < kDecItems; ++r) {
    const unsigned long long i = first + r * kDecBlock + threadIdx.x;
    if (i >= 1 && i < n) atomicAdd(&h[leave_bin(pos, i)], 1u);  // integer counts: the order cannot show
  }
  __syncthreads();
  if (threadIdx.x < kDecLevels) hist[(unsigned long long)blockIdx.x * kDecLevels + threadIdx.x] = h[threadIdx.x];
}

__global__ __launch_bounds__(kDecBlock) void spz_dec_levels_kernel(const uint32_t *hist, uint32_t tiles, uint32_t n,
                                                                   unsigned long long *counts) {
  __shared__ unsigned long long s[kDecLevels];
  const uint32_t b = threadIdx.x;
  if (b < kDecLevels) {
    unsigned long long sum = 0;
    for (uint32_t t = 0; t < tiles; ++t) sum += hist[(unsigned long long)t * kDecLevels + b];
    s[b] = sum;
  }
  __syncthreads();
  if (b < kDecLevels) {
    unsigned long long c = n ? 1ull : 0ull;
    for (uint32_t k = b; k < 24u; ++k) c += s[k];
    counts[b] = c;
  }
}

__global__ __launch_bounds__(kDecBlock) void spz_dec_flags_kernel(const uint8_t *pos, const uint8_t *alpha, uint32_t n,
                                                                  uint32_t level, unsigned long long *tile_sums) {
  __shared__ unsigned long long s[kDecBlock];
  const unsigned long long first = (unsigned long long)blockIdx.x * kDecTile + (unsigned long long)threadIdx.x * kDecItems;
  unsigned long long v = 0;
  for (uint32_t r = 0; r < kDecItems; ++r) {
    const unsigned long long i = first + r;
    if (i >= n) break;
    v += (cell_start(pos, i, level) ? 1ull : 0ull) + (alpha[i] ? (1ull << 32) : 0ull);
  }
  const unsigned long long e = block_exclusive_scan(v, s);
  if (threadIdx.x == kDecBlock - 1u) tile_sums[blockIdx.x] = e + v;
}

// Exclusive scan of the tiles' (starts, non-zero alphas) in place; the plan and the output header.
__global__ __launch_bounds__(kDecBlock) void spz_dec_scan_kernel(unsigned long long *tile_sums, uint32_t tiles,
                                                                 DecPlan *plan, uint8_t *out, unsigned long long capacity,
                                                                 uint32_t sh_degree, uint32_t sh_dim, uint32_t fb,
                                                                 uint32_t flags) {
  __shared__ unsigned long long s[kDecBlock];
  const unsigned long long sum = block_scan_owned_runs(
      tiles, s, [&](uint32_t k) { return tile_sums[k]; },
      [&](uint32_t k, unsigned long long before) { tile_sums[k] = before; });
  if (threadIdx.x == 0) {
    const uint32_t m = (uint32_t)sum;
    const bool ok = out_layout(m, sh_dim).total <= capacity;
    plan->m = m;
    plan->ok = ok ? 1u : 0u;
    if (ok) {
      const uint32_t words[4] = {kMagic, 3u, m, sh_degree | (fb << 8) | ((flags & 1u) << 16)};
#pragma unroll
      for (int k = 0; k < 16; ++k) out[k] = (uint8_t)(words[k / 4] >> (8 * (k % 4)));
    }
  }
}

__global__ __launch_bounds__(kDecBlock) void spz_dec_apply_kernel(const uint8_t *pos, const uint8_t *alpha, uint32_t n,
                                                                  uint32_t level, const unsigned long long *tile_sums,
                                                                  const uint32_t *order, uint32_t *seg, uint32_t *start,
                                                                  uint32_t *nz_start, uint32_t *parents) {
  __shared__ unsigned long long s[kDecBlock];
  const unsigned long long first = (unsigned long long)blockIdx.x * kDecTile + (unsigned long long)threadIdx.x * kDecItems;
  uint32_t bits = 0;  // bit r: a cell start; bit 8 + r: a non-zero alpha
  unsigned long long v = 0;
  for (uint32_t r = 0; r < kDecItems; ++r) {
    const unsigned long long i = first + r;
    if (i >= n) break;
    const bool f = cell_start(pos, i, level), z = alpha[i] != 0;
    bits |= (f ? 1u : 0u) << r;
    bits |= (z ? 1u : 0u) << (8 + r);
    v += (f ? 1ull : 0ull) + (z ? (1ull << 32) : 0ull);
  }
  unsigned long long run = tile_sums[blockIdx.x] + block_exclusive_scan(v, s);
  for (uint32_t r = 0; r < kDecItems; ++r) {
    const unsigned long long i = first + r;
    if (i >= n) break;
    const bool f = (bits >> r) & 1u;
    const uint32_t starts = (uint32_t)run + (f ? 1u : 0u);   // inclusive
    const uint32_t c = starts - 1u;                          // point 0 is a start: starts >= 1
    const uint32_t nz = (uint32_t)(run >> 32);
    seg[i] = c;
    if (f) {
      start[c] = (uint32_t)i;
      nz_start[c] = nz;
    }
    if (parents != nullptr) parents[order[i]] = c;
    run += (f ? 1ull : 0ull) + (((bits >> (8 + r)) & 1u) ? (1ull << 32) : 0ull);
    if (i == n - 1ull) {
      start[c + 1u] = n;
      nz_start[c + 1u] = (uint32_t)(run >> 32);
    }
  }
}

template <int D3>
__global__ __launch_bounds__(kDecBlock) void spz_dec_reduce_kernel(const ReduceParams p) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t t = blockIdx.x * (kDecBlock / 64u) + (threadIdx.x >> 6);
  if (t >= p.tiles) return;  // a whole wave: no block-level synchronisation below
  if (!p.plan->ok) return;
  const OutLayout o = out_layout(p.plan->m, (uint32_t)D3 / 3u);
  const DecIo &io = p.io;
  const uint32_t n = io.n;
  const unsigned long long i = (unsigned long long)t * kWaveTile + lane;
  const bool valid = i < n;
  const uint32_t s = valid ? p.seg[i] : 0xffffffffu;
  const uint32_t s_prev = __shfl_up(s, 1u);
  // lanes past n start cells of their own, so that no valid cell runs into them
  const bool flag = !valid || i == 0 || (lane == 0 ? p.seg[i - 1ull] != s : s_prev != s);
  const unsigned long long F = __ballot(flag);
  const unsigned long long upto = F & ((2ull << lane) - 1ull);  // flags of lanes 0..lane (lane 63: all)
  const bool started_in = upto != 0ull;
  const int first = started_in ? 63 - (int)__clzll(upto) : -1;   // this cell's first lane, -1: an earlier wave
  Moments<D3> a;
  uint32_t u[3] = {0, 0, 0}, origin[3] = {0, 0, 0};
  bool unit = false;
  if (valid) {
    load_u(io.pos, i, u);
#pragma unroll
    for (int k = 0; k < 3; ++k) origin[k] = io.level >= 24u ? 0u : (u[k] >> io.level) << io.level;
    unit = p.nz_start[s + 1u] == p.nz_start[s];
    point_moments<D3>(io, i, u, origin, unit, a);
  } else {
    zero(a);
  }
  // segmented inclusive scan: after it, the last lane of each cell in the wave holds the cell's sum over the wave
#pragma unroll
  for (uint32_t d = 1; d < 64u; d <<= 1) shfl_up_add(a, d, lane >= d && (int)(lane - d) >= first);
  if (!valid) return;
  const bool next_flag = lane == 63u ? true : ((F >> (lane + 1u)) & 1ull) != 0ull;
  if (!next_flag) return;  // not the last lane of its cell in this wave
  const bool continues = lane == 63u && i + 1ull < n && p.seg[i + 1ull] == s;
  const bool last_lane = lane == 63u || i + 1ull == n;
  if (last_lane) p.tail_cell[t] = (started_in && continues) ? s : 0xffffffffu;
  if (!started_in) {
    to_slot(a, p.head + t);
  } else if (continues) {
    to_slot(a, p.tail + t);
  } else if (first == (int)lane) {
    copy_point<D3>(io, o, s, i);
  } else {
    finish_cell<D3>(io, o, s, a, origin, unit);
  }
}

template <int D3>
__global__ __launch_bounds__(kDecBlock) void spz_dec_combine_kernel(const ReduceParams p) {
  __shared__ MomentSlot s_w[kDecBlock / 64u];
  const uint32_t t = blockIdx.x;
  const uint32_t c = p.tail_cell[t];
  if (c == 0xffffffffu || !p.plan->ok) return;  // uniform over the block
  const OutLayout o = out_layout(p.plan->m, (uint32_t)D3 / 3u);
  const uint32_t end = p.start[c + 1u];
  const uint32_t t1 = (end - 1u) / kWaveTile;
  const uint32_t slots = t1 - t + 1u;  // slot 0: tail[t]; slot k >= 1: head[t + k]
  Moments<D3> a;
  zero(a);
  for (uint32_t k = threadIdx.x; k < slots; k += kDecBlock) {
    Moments<D3> b;
    from_slot(k == 0 ? p.tail + t : p.head + t + k, b);
    add(a, b);
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) shfl_xor_add(a, m);
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0) to_slot(a, &s_w[wave]);
  __syncthreads();
  if (threadIdx.x != 0) return;
  from_slot(&s_w[0], a);
  for (uint32_t w = 1; w < kDecBlock / 64u; ++w) {
    Moments<D3> b;
    from_slot(&s_w[w], b);
    add(a, b);
  }
  uint32_t origin[3];
  cell_origin(p.io.pos, p.start[c], p.io.level, origin);
  const bool unit = p.nz_start[c + 1u] == p.nz_start[c];
  finish_cell<D3>(p.io, o, c, a, origin, unit);
}

}  // namespace spz_amd_detail

namespace {

using namespace spz_amd_detail;

struct DecLayout {
  uint64_t tiles, wave_tiles;
  uint64_t sort_ws, order, sorted, seg, start, nz_start, tile_sums, hist, counts, plan, head, tail, tail_cell, bytes;
};

DecLayout dec_layout(uint64_t n, int sh_degree) {
  DecLayout w;
  w.tiles = (n + kDecTile - 1) / kDecTile;
  w.wave_tiles = (n + kWaveTile - 1) / kWaveTile;
  spz_amd_layout sl;
  if (spz_amd_stream_layout(n, sh_degree, 3, &sl) != SPZ_AMD_OK) sl.total_bytes = 16 + 64 * n;
  WorkspaceOffsets o;
  o.put(&w.sort_ws, spz_amd_sort_workspace_bytes(n));
  o.put(&w.order, n * 4u);
  o.put(&w.sorted, sl.total_bytes);
  o.put(&w.seg, n * 4u);
  o.put(&w.start, (n + 1) * 4u);
  o.put(&w.nz_start, (n + 1) * 4u);
  o.put(&w.tile_sums, w.tiles * 8u);
  o.put(&w.hist, w.tiles * kDecLevels * 4u);
  o.put(&w.counts, kDecLevels * 8u);
  o.put(&w.plan, sizeof(DecPlan));
  o.put(&w.head, w.wave_tiles * sizeof(MomentSlot));
  o.put(&w.tail, w.wave_tiles * sizeof(MomentSlot));
  o.put(&w.tail_cell, w.wave_tiles * 4u);
  w.bytes = o.bytes();
  return w;
}

int check_input(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, spz_amd_layout *lay) {
  const int rc = check_packed_stream(d_stream, size, hdr, lay);
  if (rc != SPZ_AMD_OK) return rc;
  if (hdr->version == 1) return SPZ_AMD_ERR_UNSUPPORTED;  // float16 positions: no integer cell
  if (hdr->num_points > 0x7fffffffu) return SPZ_AMD_ERR_INVALID_ARG;
  return SPZ_AMD_OK;
}

// The sorted stream (Morton order of the stored positions) in the workspace.
int dec_sort(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, uint8_t *ws, const DecLayout &wl,
             const spz_amd_layout &lay, hipStream_t st) {
  uint32_t *order = reinterpret_cast<uint32_t *>(ws + wl.order);
  int rc = spz_amd_morton_order_device(d_stream, size, hdr, 0, order, ws + wl.sort_ws, st);
  if (rc != SPZ_AMD_OK) return rc;
  return spz_amd_subset_device(d_stream, size, hdr, order, hdr->num_points, -1, ws + wl.sorted, lay.total_bytes, st);
}

int dec_levels(const spz_amd_header *hdr, uint8_t *ws, const DecLayout &wl, const spz_amd_layout &lay,
               unsigned long long *d_counts, hipStream_t st) {
  const uint32_t n = hdr->num_points;
  uint32_t *hist = reinterpret_cast<uint32_t *>(ws + wl.hist);
  if (wl.tiles) {
    hipLaunchKernelGGL(spz_dec_hist_kernel, dim3((unsigned)wl.tiles), dim3(kDecBlock), 0, st,
                       ws + wl.sorted + lay.offset[SPZ_AMD_SEC_POSITIONS], n, hist);
    SPZ_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(spz_dec_levels_kernel, dim3(1), dim3(kDecBlock), 0, st, hist, (uint32_t)wl.tiles, n, d_counts);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

template <int D3>
int dec_reduce_launch(const ReduceParams &p, hipStream_t st) {
  const uint32_t blocks = (uint32_t)((p.tiles + kDecBlock / 64u - 1) / (kDecBlock / 64u));
  hipLaunchKernelGGL(spz_dec_reduce_kernel<D3>, dim3(blocks), dim3(kDecBlock), 0, st, p);
  SPZ_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(spz_dec_combine_kernel<D3>, dim3(p.tiles), dim3(kDecBlock), 0, st, p);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

// Cells at `level`, the moment reduction and the output, over the sorted stream already in the workspace.
int dec_run(const spz_amd_header *hdr, int level, uint8_t *ws, const DecLayout &wl, const spz_amd_layout &lay,
            uint8_t *d_out, size_t capacity, uint32_t *d_parents, hipStream_t st) {
  const uint32_t n = hdr->num_points;
  const uint8_t *sorted = ws + wl.sorted;
  const uint8_t *pos = sorted + lay.offset[SPZ_AMD_SEC_POSITIONS];
  const uint8_t *alpha = sorted + lay.offset[SPZ_AMD_SEC_ALPHAS];
  auto *tile_sums = reinterpret_cast<unsigned long long *>(ws + wl.tile_sums);
  auto *plan = reinterpret_cast<DecPlan *>(ws + wl.plan);
  const uint32_t dim = (uint32_t)sh_dim_for_degree(hdr->sh_degree);
  if (wl.tiles) {
    hipLaunchKernelGGL(spz_dec_flags_kernel, dim3((unsigned)wl.tiles), dim3(kDecBlock), 0, st, pos, alpha, n,
                       (uint32_t)level, tile_sums);
    SPZ_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(spz_dec_scan_kernel, dim3(1), dim3(kDecBlock), 0, st, tile_sums, (uint32_t)wl.tiles, plan, d_out,
                     (unsigned long long)capacity, (uint32_t)hdr->sh_degree, dim, (uint32_t)hdr->fractional_bits,
                     (uint32_t)hdr->flags);
  SPZ_HIP_TRY(hipGetLastError());
  if (n == 0) return SPZ_AMD_OK;
  ReduceParams p = {};
  p.seg = reinterpret_cast<uint32_t *>(ws + wl.seg);
  uint32_t *start = reinterpret_cast<uint32_t *>(ws + wl.start);
  uint32_t *nz_start = reinterpret_cast<uint32_t *>(ws + wl.nz_start);
  hipLaunchKernelGGL(spz_dec_apply_kernel, dim3((unsigned)wl.tiles), dim3(kDecBlock), 0, st, pos, alpha, n,
                     (uint32_t)level, tile_sums, reinterpret_cast<const uint32_t *>(ws + wl.order),
                     const_cast<uint32_t *>(p.seg), start, nz_start, d_parents);
  SPZ_HIP_TRY(hipGetLastError());
  p.io.pos = pos;
  p.io.alpha = alpha;
  p.io.color = sorted + lay.offset[SPZ_AMD_SEC_COLORS];
  p.io.scale = sorted + lay.offset[SPZ_AMD_SEC_SCALES];
  p.io.rot = sorted + lay.offset[SPZ_AMD_SEC_ROTATIONS];
  p.io.sh = sorted + lay.offset[SPZ_AMD_SEC_SH];
  p.io.version = hdr->version;
  p.io.n = n;
  p.io.level = (uint32_t)level;
  p.io.fb = hdr->fractional_bits;
  p.io.out = d_out;
  p.start = start;
  p.nz_start = nz_start;
  p.plan = plan;
  p.head = reinterpret_cast<MomentSlot *>(ws + wl.head);
  p.tail = reinterpret_cast<MomentSlot *>(ws + wl.tail);
  p.tail_cell = reinterpret_cast<uint32_t *>(ws + wl.tail_cell);
  p.sh_dim = dim;
  p.tiles = (uint32_t)wl.wave_tiles;
  switch (dim) {
    case 0: return dec_reduce_launch<0>(p, st);
    case 3: return dec_reduce_launch<9>(p, st);
    case 8: return dec_reduce_launch<24>(p, st);
    default: return dec_reduce_launch<45>(p, st);
  }
}

}  // namespace

extern "C" {

uint64_t spz_amd_decimate_workspace_bytes(uint64_t n, int sh_degree) {
  return dec_layout(n, sh_degree < 0 || sh_degree > 3 ? 3 : sh_degree).bytes;
}

int spz_amd_decimate_level_counts_device(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr,
                                         uint64_t *d_counts, void *d_workspace, void *hip_stream) {
  spz_amd_layout lay;
  int rc = check_input(d_stream, size, hdr, &lay);
  if (rc != SPZ_AMD_OK) return rc;
  if (d_counts == nullptr || d_workspace == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const DecLayout wl = dec_layout(hdr->num_points, hdr->sh_degree);
  uint8_t *ws = align_ws(d_workspace);
  if (hdr->num_points) {
    rc = dec_sort(d_stream, size, hdr, ws, wl, lay, st);
    if (rc != SPZ_AMD_OK) return rc;
  }
  return dec_levels(hdr, ws, wl, lay, reinterpret_cast<unsigned long long *>(d_counts), st);
}

int spz_amd_decimate_device(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, int level, uint8_t *d_out,
                            size_t capacity, uint32_t *d_parents, void *d_workspace, void *hip_stream) {
  spz_amd_layout lay;
  int rc = check_input(d_stream, size, hdr, &lay);
  if (rc != SPZ_AMD_OK) return rc;
  if (level < 0 || level > 24 || d_out == nullptr || d_workspace == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  if (capacity < 16) return SPZ_AMD_ERR_CAPACITY;
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const DecLayout wl = dec_layout(hdr->num_points, hdr->sh_degree);
  uint8_t *ws = align_ws(d_workspace);
  if (hdr->num_points) {
    rc = dec_sort(d_stream, size, hdr, ws, wl, lay, st);
    if (rc != SPZ_AMD_OK) return rc;
  }
  return dec_run(hdr, level, ws, wl, lay, d_out, capacity, d_parents, st);
}

int spz_amd_decimate_open(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, int level,
                          uint64_t target_points, int device, void **ctx, uint64_t *h_out_bytes, int *h_level,
                          spz_amd_header *h_out_hdr, uint32_t *h_parents, float *h_ms) {
  if (ctx == nullptr || h_out_bytes == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  *ctx = nullptr;
  *h_out_bytes = 0;
  spz_amd_layout lay;
  int rc = check_input(d_stream, size, hdr, &lay);
  if (rc != SPZ_AMD_OK) return rc;
  const bool by_level = level >= 0;
  if (by_level == (target_points != 0)) return SPZ_AMD_ERR_INVALID_ARG;  // exactly one of the two
  if (by_level && level > 24) return SPZ_AMD_ERR_INVALID_ARG;
  if (!by_level && level != -1) return SPZ_AMD_ERR_INVALID_ARG;
  const uint64_t n = hdr->num_points;
  if (n > SPZ_AMD_REFERENCE_MAX_POINTS) return SPZ_AMD_ERR_TOO_MANY_POINTS;
  DeviceGuard guard;
  rc = guard.enter(device);
  if (rc != SPZ_AMD_OK) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  PackedResultPtr c;
  rc = packed_result_open(device, &c);
  if (rc != SPZ_AMD_OK) return rc;
  const DecLayout wl = dec_layout(n, hdr->sh_degree);
  SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&c->block), wl.bytes));
  uint8_t *ws = align_ws(c->block);
  if (n) {
    rc = dec_sort(d_stream, size, hdr, ws, wl, lay, c->st);
    if (rc != SPZ_AMD_OK) return rc;
  }
  SPZ_HIP_TRY(hipStreamSynchronize(c->st));
  const double sort_ms = ms_since(t0);
  auto *d_counts = reinterpret_cast<unsigned long long *>(ws + wl.counts);
  rc = dec_levels(hdr, ws, wl, lay, d_counts, c->st);
  if (rc != SPZ_AMD_OK) return rc;
  unsigned long long counts[kDecLevels];
  SPZ_HIP_TRY(hipMemcpyAsync(counts, d_counts, sizeof(counts), hipMemcpyDeviceToHost, c->st));
  SPZ_HIP_TRY(hipStreamSynchronize(c->st));
  const double levels_ms = ms_since(t0) - sort_ms;
  int L = level;
  if (!by_level) {
    L = 24;  // one cell (or none): every target >= 1 is reachable
    for (int k = 0; k < (int)kDecLevels; ++k) {
      if (counts[k] <= target_points) {
        L = k;
        break;
      }
    }
  }
  const uint64_t m = counts[L];
  const uint32_t dim = (uint32_t)sh_dim_for_degree(hdr->sh_degree);
  c->out_bytes = out_layout(m, dim).total;
  SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&c->out_block), c->out_bytes));
  c->out = c->out_block;
  uint32_t *d_parents = h_parents && n ? reinterpret_cast<uint32_t *>(ws + wl.sort_ws) : nullptr;  // the sort is done
  rc = dec_run(hdr, L, ws, wl, lay, c->out, c->out_bytes, d_parents, c->st);
  if (rc != SPZ_AMD_OK) return rc;
  if (d_parents) SPZ_HIP_TRY(hipMemcpyAsync(h_parents, d_parents, n * 4u, hipMemcpyDeviceToHost, c->st));
  SPZ_HIP_TRY(hipStreamSynchronize(c->st));
  if (h_ms) {
    h_ms[0] = (float)sort_ms;
    h_ms[1] = (float)levels_ms;
    h_ms[2] = (float)(ms_since(t0) - sort_ms - levels_ms);
  }
  if (h_level) *h_level = L;
  if (h_out_hdr) {
    h_out_hdr->version = 3;
    h_out_hdr->num_points = (uint32_t)m;
    h_out_hdr->sh_degree = hdr->sh_degree;
    h_out_hdr->fractional_bits = hdr->fractional_bits;
    h_out_hdr->flags = hdr->flags & 1u;
    h_out_hdr->reserved = 0;
  }
  *h_out_bytes = c->out_bytes;
  *ctx = c.release();
  return SPZ_AMD_OK;
}

int spz_amd_decimate_fetch(void *ctx, uint8_t *h_out) { return packed_result_fetch(ctx, h_out); }

const uint8_t *spz_amd_decimate_device_data(void *ctx) { return packed_result_device_data(ctx); }

void spz_amd_decimate_close(void *ctx) { packed_result_close(ctx); }

}  // extern "C"
