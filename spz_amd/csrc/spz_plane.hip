// spz_plane.hip — the dominant planes of a packed stream (DESIGN §8 "Level"; the contract is in include/spz_amd.h): MSAC
// over seeded hypotheses, an exact least-squares refinement, and the placement that levels the scene.  Everything after
// the hypotheses' normals is integer arithmetic on the stored 24-bit positions.
//
//   spz_plane_mask_kernel     mask[i] = i % stride == 0 && labels[i] == 0; the filter's selection (select_device) turns
//                             it into the taking-part indices in input order and their count m.
//   spz_plane_fill_kernel     the prepared points: int32 (X, Y, Z, input index) and the same X, Y, Z as f64 for the score.
//   spz_plane_gather_kernel   the 3 H sampled points of a round, for one copy to the host.
//   spz_plane_score_kernel    the hot one: one lane per hypothesis, one wave per (64 planes, chunk of points).  A lane
//                             keeps its plane and its K and S in registers; the points are wave-uniform (scalar loads of
//                             the f64 copies), so there is no cross-lane step.  d = a X + b Y + c Z - e in three f64
//                             fused multiply-adds: every operand and partial sum is an integer below 2^46, so each is
//                             exact and d is the integer of the definition.  S is summed in f64 over at most 2^16 points
//                             (2^16 2^36 = 2^52: exact), then added to a uint64.  The grid is (plane groups) x (chunks),
//                             few and long chunks: at most 4096 waves, a slab of at most 4 MiB.
//   spz_plane_reduce_kernel   one lane per plane: the chunks' K and S summed, the cost, the invalid planes.
//   spz_plane_moment_kernel / one lane per point; per tile of 2048 points int64 sums (2048 2^46 < 2^63: exact), then one
//   spz_plane_join_kernel     workgroup joins the tiles into 128-bit integers.  No float anywhere.
//   spz_plane_mark_kernel     labels[index] = value for the inliers.
// The hypotheses (f64) and the solve (128-bit integers, then a 3x3 cyclic Jacobi in f64) run on the host.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "spz_amd.h"
#include "spz_block_ops.hpp"
#include "spz_common.hpp"

#pragma clang fp contract(off)

namespace spz_amd_detail {
namespace {

constexpr uint32_t kPlBlock = 256;
static_assert(kPlBlock == kOpsBlock, "block_sum is over 256 threads");
constexpr uint32_t kPlItems = 8;                       // points per thread of the moment sums
constexpr uint32_t kPlTile = kPlBlock * kPlItems;      // 2048
constexpr uint32_t kPlSums = 13;                       // K, S, above, below, sum P (3), sum P P^T (6)
constexpr uint32_t kPlWave = 64;                       // planes per wave of the score
constexpr uint32_t kPlMaxWaves = 4096;                 // of one score launch
constexpr uint32_t kPlMinChunk = 2048;                 // points: a chunk is not shorter unless it is the only one
constexpr uint32_t kPlExact = 65536;                   // points whose |d| sum stays below 2^53 in f64
constexpr int32_t kPlMaxNormal = 65536;
constexpr long long kPlMaxOffset = 1ll << 42;
constexpr uint64_t kPlMaxThreshold = 1ull << 36;
constexpr uint32_t kPlMaxHypotheses = 65536;

struct ScoreParams {
  const double4 *pd;            // m prepared points as f64 (w unused)
  const spz_amd_plane *planes;  // H
  unsigned long long *slab;     // chunks x groups x 64 x (K, S)
  uint32_t m, H, chunk_len;
  double T;
};

__device__ __forceinline__ bool pl_valid(const spz_amd_plane &q) {
  const bool range = q.a >= -kPlMaxNormal && q.a <= kPlMaxNormal && q.b >= -kPlMaxNormal && q.b <= kPlMaxNormal &&
                     q.c >= -kPlMaxNormal && q.c <= kPlMaxNormal && q.e >= -kPlMaxOffset && q.e <= kPlMaxOffset;
  return range && (q.a != 0 || q.b != 0 || q.c != 0);
}

// d of prepared point i for the moments and the mark, in 64-bit integers.
__device__ __forceinline__ long long pl_distance(const spz_amd_plane &q, const int4 &pt) {
  return (long long)q.a * pt.x + (long long)q.b * pt.y + (long long)q.c * pt.z - q.e;
}

}  // namespace

__global__ __launch_bounds__(kPlBlock) void spz_plane_mask_kernel(const uint8_t *labels, uint32_t n, uint32_t stride,
                                                                  uint8_t *mask) {
  const uint32_t i = blockIdx.x * kPlBlock + threadIdx.x;
  if (i >= n) return;
  mask[i] = (i % stride == 0u && (labels == nullptr || labels[i] == 0u)) ? 1u : 0u;
}

__global__ __launch_bounds__(kPlBlock) void spz_plane_fill_kernel(const uint8_t *positions, const uint32_t *indices,
                                                                  uint32_t m, int4 *pts, double4 *pd) {
  const uint32_t k = blockIdx.x * kPlBlock + threadIdx.x;
  if (k >= m) return;
  const uint32_t i = indices[k];
  const uint8_t *b = positions + (unsigned long long)i * 9u;
  int32_t v[3];
#pragma unroll
  for (uint32_t a = 0; a < 3; ++a) {
    const uint32_t u = (uint32_t)b[3 * a] | ((uint32_t)b[3 * a + 1] << 8) | ((uint32_t)b[3 * a + 2] << 16);
    v[a] = (int32_t)(u << 8) >> 8;
  }
  pts[k] = make_int4(v[0], v[1], v[2], (int32_t)i);
  pd[k] = make_double4((double)v[0], (double)v[1], (double)v[2], 0.0);
}

__global__ __launch_bounds__(kPlBlock) void spz_plane_gather_kernel(const int4 *pts, uint32_t m, const uint32_t *indices,
                                                                    uint32_t count, int32_t *out) {
  const uint32_t k = blockIdx.x * kPlBlock + threadIdx.x;
  if (k >= count) return;
  const uint32_t i = indices[k] < m ? indices[k] : m - 1u;
  const int4 pt = pts[i];
  out[3 * k] = pt.x;
  out[3 * k + 1] = pt.y;
  out[3 * k + 2] = pt.z;
}

// One wave: 64 planes (blockIdx.x) over one chunk of the prepared points (blockIdx.y).  See the file comment.
__global__ __launch_bounds__(kPlWave) void spz_plane_score_kernel(const ScoreParams p) {
  const uint32_t h = blockIdx.x * kPlWave + threadIdx.x;
  double a = 0.0, b = 0.0, c = 0.0, ne = 0.0;
  if (h < p.H) {
    const spz_amd_plane q = p.planes[h];
    if (pl_valid(q)) {
      a = (double)q.a;
      b = (double)q.b;
      c = (double)q.c;
      ne = -(double)q.e;
    }
  }
  const double T = p.T;
  const double4 *__restrict__ pd = p.pd;
  const uint32_t begin = blockIdx.y * p.chunk_len;  // chunks * chunk_len < m + chunk_len <= 2^24 + 2^24
  const uint32_t end = min(begin + p.chunk_len, p.m);
  unsigned long long S = 0;
  uint32_t K = 0;
  for (uint32_t i0 = begin; i0 < end; i0 += kPlExact) {
    const uint32_t i1 = min(i0 + kPlExact, end);
    double s = 0.0;
#pragma unroll 8
    for (uint32_t i = i0; i < i1; ++i) {
      const double4 pt = pd[i];  // wave-uniform
      const double d = __builtin_fma(a, pt.x, __builtin_fma(b, pt.y, __builtin_fma(c, pt.z, ne)));
      const double ad = __builtin_fabs(d);
      const bool in = ad <= T;
      K += in ? 1u : 0u;
      s += in ? ad : 0.0;
    }
    S += (unsigned long long)s;
  }
  unsigned long long *out = p.slab + ((unsigned long long)blockIdx.y * gridDim.x * kPlWave + h) * 2ull;
  out[0] = K;
  out[1] = S;
}

__global__ __launch_bounds__(kPlBlock) void spz_plane_reduce_kernel(const unsigned long long *slab,
                                                                    const spz_amd_plane *planes, uint32_t H,
                                                                    uint32_t groups, uint32_t chunks, uint32_t m,
                                                                    unsigned long long T, unsigned long long *scores) {
  const uint32_t h = blockIdx.x * kPlBlock + threadIdx.x;
  if (h >= H) return;
  unsigned long long K = 0, S = 0, cost = ~0ull;
  if (pl_valid(planes[h])) {
    for (uint32_t k = 0; k < chunks; ++k) {
      const unsigned long long *at = slab + ((unsigned long long)k * groups * kPlWave + h) * 2ull;
      K += at[0];
      S += at[1];
    }
    cost = S + T * ((unsigned long long)m - K);
  }
  scores[3ull * h] = K;
  scores[3ull * h + 1] = S;
  scores[3ull * h + 2] = cost;
}

// The int64 sums of one tile of 2048 prepared points into partials[tile][13] (two's complement words).
__global__ __launch_bounds__(kPlBlock) void spz_plane_moment_kernel(const int4 *pts, uint32_t m, const spz_amd_plane q,
                                                                    long long T, unsigned long long *partials) {
  __shared__ unsigned long long s[kPlBlock];
  unsigned long long v[kPlSums];
#pragma unroll
  for (uint32_t k = 0; k < kPlSums; ++k) v[k] = 0;
  const unsigned long long first = (unsigned long long)blockIdx.x * kPlTile + threadIdx.x;
#pragma unroll
  for (uint32_t r = 0; r < kPlItems; ++r) {
    const unsigned long long i = first + (unsigned long long)r * kPlBlock;
    if (i >= m) break;
    const int4 pt = pts[i];
    const long long d = pl_distance(q, pt);
    const long long ad = d < 0 ? -d : d;
    if (ad <= T) {
      const long long x = pt.x, y = pt.y, z = pt.z;
      v[0] += 1ull;
      v[1] += (unsigned long long)ad;
      v[4] += (unsigned long long)x;
      v[5] += (unsigned long long)y;
      v[6] += (unsigned long long)z;
      v[7] += (unsigned long long)(x * x);
      v[8] += (unsigned long long)(x * y);
      v[9] += (unsigned long long)(x * z);
      v[10] += (unsigned long long)(y * y);
      v[11] += (unsigned long long)(y * z);
      v[12] += (unsigned long long)(z * z);
    } else if (d > 0) {
      v[2] += 1ull;
    } else {
      v[3] += 1ull;
    }
  }
  unsigned long long *out = partials + (unsigned long long)blockIdx.x * kPlSums;
#pragma unroll
  for (uint32_t k = 0; k < kPlSums; ++k) {
    const unsigned long long t = block_sum(v[k], s);
    if (threadIdx.x == 0) out[k] = t;
  }
}

// One workgroup over the tiles.  A tile's int64 is split into its low 32 bits (unsigned) and its high 32 (signed); each
// half is summed in 64 bits (at most 2^13 tiles of 2^32), and the two sums are joined into a 128-bit integer.
__global__ __launch_bounds__(kPlBlock) void spz_plane_join_kernel(const unsigned long long *partials, uint32_t tiles,
                                                                  uint32_t m, spz_amd_plane_moments *out) {
  __shared__ unsigned long long s[kPlBlock];
  unsigned long long lo[kPlSums];
  long long hi[kPlSums];
  for (uint32_t k = 0; k < kPlSums; ++k) {
    unsigned long long l = 0, h = 0;
    for (uint32_t t = threadIdx.x; t < tiles; t += kPlBlock) {
      const unsigned long long w = partials[(unsigned long long)t * kPlSums + k];
      l += w & 0xffffffffull;
      h += (unsigned long long)((long long)w >> 32);
    }
    const unsigned long long ls = block_sum(l, s);
    const unsigned long long hs = block_sum(h, s);
    // hs 2^32 + ls as (hi, lo)
    const unsigned long long shifted = hs << 32;
    lo[k] = shifted + ls;
    hi[k] = ((long long)hs >> 32) + (lo[k] < shifted ? 1ll : 0ll);
  }
  if (threadIdx.x != 0) return;
  out->count = lo[0];
  out->sum_abs = lo[1];
  out->above = lo[2];
  out->below = lo[3];
  out->points = m;
  for (uint32_t k = 0; k < 3; ++k) out->sum_p[k] = (long long)lo[4 + k];
  for (uint32_t k = 0; k < 6; ++k) {
    out->sum_pp_lo[k] = lo[7 + k];
    out->sum_pp_hi[k] = hi[7 + k];
  }
}

__global__ __launch_bounds__(kPlBlock) void spz_plane_mark_kernel(const int4 *pts, uint32_t m, const spz_amd_plane q,
                                                                  long long T, uint8_t value, uint32_t n,
                                                                  uint8_t *labels) {
  const uint32_t i = blockIdx.x * kPlBlock + threadIdx.x;
  if (i >= m) return;
  const int4 pt = pts[i];
  const long long d = pl_distance(q, pt);
  const long long ad = d < 0 ? -d : d;
  if (ad <= T && (uint32_t)pt.w < n) labels[(uint32_t)pt.w] = value;
}

// side[i] = 0 (|d| <= T), 1 (d > T) or 2 (d < -T) of every point of the stream.
__global__ __launch_bounds__(kPlBlock) void spz_plane_side_kernel(const uint8_t *positions, uint32_t n,
                                                                  const spz_amd_plane q, long long T, uint8_t *side) {
  const uint32_t i = blockIdx.x * kPlBlock + threadIdx.x;
  if (i >= n) return;
  const uint8_t *b = positions + (unsigned long long)i * 9u;
  int32_t v[3];
#pragma unroll
  for (uint32_t a = 0; a < 3; ++a) {
    const uint32_t u = (uint32_t)b[3 * a] | ((uint32_t)b[3 * a + 1] << 8) | ((uint32_t)b[3 * a + 2] << 16);
    v[a] = (int32_t)(u << 8) >> 8;
  }
  const long long d = pl_distance(q, make_int4(v[0], v[1], v[2], 0));
  side[i] = d > T ? 1u : (d < -T ? 2u : 0u);
}

}  // namespace spz_amd_detail

namespace {

using namespace spz_amd_detail;

struct PlLayout {
  uint64_t tiles;
  uint64_t mask, idx, fws, pts, pd, slab, partials, bytes;
};

PlLayout pl_layout(uint64_t n) {
  PlLayout w;
  w.tiles = (n + kPlTile - 1) / kPlTile;
  WorkspaceOffsets o;
  o.put(&w.mask, n);
  o.put(&w.idx, n * 4u);
  o.put(&w.fws, spz_amd_filter_workspace_bytes(n));
  o.put(&w.pts, n * 16u);
  o.put(&w.pd, n * 32u);
  o.put(&w.slab, (uint64_t)kPlMaxWaves * kPlWave * 16u);
  o.put(&w.partials, (w.tiles + 1) * kPlSums * 8u);
  w.bytes = o.bytes();
  return w;
}

int pl_check_stream(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, spz_amd_layout *lay) {
  const int rc = check_packed_stream(d_stream, size, hdr, lay);
  if (rc != SPZ_AMD_OK) return rc;
  if (hdr->version == 1) return SPZ_AMD_ERR_UNSUPPORTED;  // float16 positions: no integer distances
  if (hdr->num_points > SPZ_AMD_REFERENCE_MAX_POINTS) return SPZ_AMD_ERR_TOO_MANY_POINTS;
  if (hdr->fractional_bits > 24) return SPZ_AMD_ERR_INVALID_ARG;
  return SPZ_AMD_OK;
}

// What the device forms on a prepared workspace refuse.
bool pl_bad_prepared(const void *d_workspace, uint64_t n, uint64_t m) {
  return d_workspace == nullptr || n > SPZ_AMD_REFERENCE_MAX_POINTS || m > n;
}

bool pl_plane_ok(const spz_amd_plane *q) {
  if (q == nullptr) return false;
  for (int32_t v : {q->a, q->b, q->c}) {
    if (v < -kPlMaxNormal || v > kPlMaxNormal) return false;
  }
  if (q->e < -kPlMaxOffset || q->e > kPlMaxOffset) return false;
  return q->a != 0 || q->b != 0 || q->c != 0;
}

int pl_prepare(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, const spz_amd_layout &lay,
               uint32_t stride, const uint8_t *d_labels, uint8_t *ws, const PlLayout &wl, uint64_t *h_count,
               hipStream_t st) {
  *h_count = 0;
  const uint32_t n = hdr->num_points;
  if (n == 0) return SPZ_AMD_OK;
  const unsigned blocks = (n + kPlBlock - 1) / kPlBlock;
  hipLaunchKernelGGL(spz_plane_mask_kernel, dim3(blocks), dim3(kPlBlock), 0, st, d_labels, n, stride, ws + wl.mask);
  SPZ_HIP_TRY(hipGetLastError());
  uint32_t *d_idx = reinterpret_cast<uint32_t *>(ws + wl.idx);
  uint64_t m = 0;
  const int rc = spz_amd_select_device(d_stream, size, hdr, nullptr, ws + wl.mask, d_idx, ws + wl.fws, &m, st);
  if (rc != SPZ_AMD_OK) return rc;
  if (m) {
    hipLaunchKernelGGL(spz_plane_fill_kernel, dim3((unsigned)((m + kPlBlock - 1) / kPlBlock)), dim3(kPlBlock), 0, st,
                       d_stream + lay.offset[SPZ_AMD_SEC_POSITIONS], d_idx, (uint32_t)m,
                       reinterpret_cast<int4 *>(ws + wl.pts), reinterpret_cast<double4 *>(ws + wl.pd));
    SPZ_HIP_TRY(hipGetLastError());
  }
  *h_count = m;
  return SPZ_AMD_OK;
}

int pl_score(uint8_t *ws, const PlLayout &wl, uint32_t m, const spz_amd_plane *d_planes, uint32_t H, uint64_t T,
             uint64_t *d_scores, hipStream_t st) {
  const uint32_t groups = (H + kPlWave - 1) / kPlWave;
  uint32_t chunks = kPlMaxWaves / groups;                      // groups <= 1024: at least 4
  const uint32_t most = (m + kPlMinChunk - 1) / kPlMinChunk;   // chunks of at least 2048 points
  if (chunks > most) chunks = most;
  if (chunks < 1u) chunks = 1u;
  ScoreParams p = {};
  p.pd = reinterpret_cast<const double4 *>(ws + wl.pd);
  p.planes = d_planes;
  p.slab = reinterpret_cast<unsigned long long *>(ws + wl.slab);
  p.m = m;
  p.H = H;
  p.chunk_len = m ? (m + chunks - 1) / chunks : 0u;
  p.T = (double)T;
  hipLaunchKernelGGL(spz_plane_score_kernel, dim3(groups, chunks), dim3(kPlWave), 0, st, p);
  SPZ_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(spz_plane_reduce_kernel, dim3((H + kPlBlock - 1) / kPlBlock), dim3(kPlBlock), 0, st, p.slab,
                     d_planes, H, groups, chunks, m, (unsigned long long)T,
                     reinterpret_cast<unsigned long long *>(d_scores));
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

int pl_moments(uint8_t *ws, const PlLayout &wl, uint32_t m, const spz_amd_plane &q, uint64_t T,
               spz_amd_plane_moments *d_out, hipStream_t st) {
  const uint32_t tiles = (m + kPlTile - 1) / kPlTile;
  unsigned long long *partials = reinterpret_cast<unsigned long long *>(ws + wl.partials);
  if (tiles) {
    hipLaunchKernelGGL(spz_plane_moment_kernel, dim3(tiles), dim3(kPlBlock), 0, st,
                       reinterpret_cast<const int4 *>(ws + wl.pts), m, q, (long long)T, partials);
    SPZ_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(spz_plane_join_kernel, dim3(1), dim3(kPlBlock), 0, st, partials, tiles, m, d_out);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

int pl_mark(const uint8_t *ws, const PlLayout &wl, uint32_t n, uint32_t m, const spz_amd_plane &q, uint64_t T,
            uint8_t value, uint8_t *d_labels, hipStream_t st) {
  if (m == 0) return SPZ_AMD_OK;
  hipLaunchKernelGGL(spz_plane_mark_kernel, dim3((m + kPlBlock - 1) / kPlBlock), dim3(kPlBlock), 0, st,
                     reinterpret_cast<const int4 *>(ws + wl.pts), m, q, (long long)T, value, n, d_labels);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

// ---- the host side ----------------------------------------------------------------------------------------------
uint64_t mix64(uint64_t z) {  // splitmix64's finaliser
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

bool pl_bad_vector(const double *v) {
  double n2 = 0.0;
  for (int k = 0; k < 3; ++k) {
    if (!std::isfinite(v[k])) return true;
    n2 += v[k] * v[k];
  }
  const double norm = std::sqrt(n2);
  return !(norm > 0.0) || !std::isfinite(norm);
}

// The axis flips between `coord` and the stored RUB frame, and their determinant (spz_amd_transform_params' conjugation).
void pl_flips(int coord, double f[3], double *det) {
  const uint32_t fp = flip_masks(coord, SPZ_AMD_RUB).p;
  for (int a = 0; a < 3; ++a) f[a] = ((fp >> a) & 1u) ? -1.0 : 1.0;
  *det = f[0] * f[1] * f[2];
}

// Eigenvalues (the diagonal of A on return) and eigenvectors (the columns of V) of the symmetric A by cyclic Jacobi.
void jacobi3(double A[3][3], double V[3][3]) {
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  }
  for (int sweep = 0; sweep < 64; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < 2; ++p) {
      for (int q = p + 1; q < 3; ++q) {
        const double apq = A[p][q];
        if (apq == 0.0 || std::fabs(apq) <= 1e-17 * std::sqrt(std::fabs(A[p][p])) * std::sqrt(std::fabs(A[q][q]))) continue;
        rotated = true;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(1.0 + theta * theta));
        const double c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
        for (int k = 0; k < 3; ++k) {
          const double x = A[k][p], y = A[k][q];
          A[k][p] = c * x - s * y;
          A[k][q] = s * x + c * y;
        }
        for (int k = 0; k < 3; ++k) {
          const double x = A[p][k], y = A[q][k];
          A[p][k] = c * x - s * y;
          A[q][k] = s * x + c * y;
        }
        for (int k = 0; k < 3; ++k) {
          const double x = V[k][p], y = V[k][q];
          V[k][p] = c * x - s * y;
          V[k][q] = s * x + c * y;
        }
      }
    }
    if (!rotated) break;
  }
}

__int128 pl_wide(uint64_t lo, int64_t hi) { return (__int128)(((unsigned __int128)(uint64_t)hi << 64) | lo); }

// num / den to the nearest integer, ties to even; den > 0.
__int128 pl_div_round(__int128 num, __int128 den) {
  __int128 q = num / den, r = num % den;  // truncated
  if (r < 0) {
    q -= 1;
    r += den;
  }
  const __int128 twice = 2 * r;
  if (twice > den || (twice == den && (q & 1))) q += 1;
  return q;
}

void pl_negate(spz_amd_plane *q) {
  q->a = -q->a;
  q->b = -q->b;
  q->c = -q->c;
  q->e = -q->e;
}

}  // namespace

extern "C" {

int spz_amd_plane_default_options(spz_amd_plane_options *o) {
  if (o == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  std::memset(o, 0, sizeof(*o));
  o->threshold = std::nan("");
  o->hypotheses = 4096;
  o->refine = 3;
  o->max_planes = 1;
  o->stride = 1;
  o->max_tilt = 90.0;
  o->coord = SPZ_AMD_UNSPECIFIED;
  return SPZ_AMD_OK;
}

int spz_amd_plane_check(const spz_amd_plane_options *o) {
  if (o == nullptr || !valid_coord(o->coord)) return SPZ_AMD_ERR_INVALID_ARG;
  if (o->hypotheses < 1u || o->hypotheses > kPlMaxHypotheses || o->refine > 16u) return SPZ_AMD_ERR_INVALID_ARG;
  if (o->max_planes < 1u || o->max_planes > 255u || o->stride < 1u) return SPZ_AMD_ERR_INVALID_ARG;
  if (!std::isfinite(o->threshold) || !(o->threshold >= 0.0)) return SPZ_AMD_ERR_INVALID_ARG;
  if (o->has_axis && pl_bad_vector(o->axis)) return SPZ_AMD_ERR_INVALID_ARG;
  if (o->has_up_hint && pl_bad_vector(o->up_hint)) return SPZ_AMD_ERR_INVALID_ARG;
  if (!(o->max_tilt >= 0.0) || !(o->max_tilt <= 90.0)) return SPZ_AMD_ERR_INVALID_ARG;
  return SPZ_AMD_OK;
}

int spz_amd_plane_threshold(double tau, int fractional_bits, uint64_t *threshold) {
  if (threshold == nullptr || fractional_bits < 0 || fractional_bits > 24) return SPZ_AMD_ERR_INVALID_ARG;
  if (!std::isfinite(tau) || !(tau >= 0.0)) return SPZ_AMD_ERR_INVALID_ARG;
  const double t = std::floor(std::ldexp(tau, fractional_bits + 16));  // the scaling is exact
  if (!(t <= (double)kPlMaxThreshold)) return SPZ_AMD_ERR_INVALID_ARG;
  *threshold = (uint64_t)t;
  return SPZ_AMD_OK;
}

uint64_t spz_amd_plane_workspace_bytes(uint64_t num_points) { return pl_layout(num_points).bytes; }

int spz_amd_plane_prepare_device(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, uint32_t stride,
                                 const uint8_t *d_labels, void *d_workspace, uint64_t *h_count, void *hip_stream) {
  if (h_count == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  *h_count = 0;
  spz_amd_layout lay;
  int rc = pl_check_stream(d_stream, size, hdr, &lay);
  if (rc != SPZ_AMD_OK) return rc;
  if (stride < 1u || d_workspace == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  return pl_prepare(d_stream, size, hdr, lay, stride, d_labels, align_ws(d_workspace), pl_layout(hdr->num_points), h_count,
                    static_cast<hipStream_t>(hip_stream));
}

int spz_amd_plane_gather_device(const void *d_workspace, uint64_t num_points, uint64_t m, const uint32_t *d_indices,
                                uint64_t count, int32_t *d_out, void *hip_stream) {
  if (pl_bad_prepared(d_workspace, num_points, m) || count > 3ull * kPlMaxHypotheses) return SPZ_AMD_ERR_INVALID_ARG;
  if (count == 0) return SPZ_AMD_OK;
  if (m == 0 || d_indices == nullptr || d_out == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  int device = 0;
  const int rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  const PlLayout wl = pl_layout(num_points);
  const uint8_t *ws = align_ws(const_cast<void *>(d_workspace));
  hipLaunchKernelGGL(spz_plane_gather_kernel, dim3((unsigned)((count + kPlBlock - 1) / kPlBlock)), dim3(kPlBlock), 0,
                     static_cast<hipStream_t>(hip_stream), reinterpret_cast<const int4 *>(ws + wl.pts), (uint32_t)m,
                     d_indices, (uint32_t)count, d_out);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

int spz_amd_plane_hypotheses(uint64_t seed, uint32_t round, uint32_t hypotheses, uint64_t m, const int32_t *h_points,
                             const double *axis, double max_tilt, uint32_t *h_indices, spz_amd_plane *h_planes) {
  if (hypotheses < 1u || hypotheses > kPlMaxHypotheses || m < 1u || m > SPZ_AMD_REFERENCE_MAX_POINTS) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  if (h_points != nullptr && h_planes == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  double u[3] = {0.0, 0.0, 0.0}, limit = 0.0;
  if (axis != nullptr) {
    if (pl_bad_vector(axis) || !(max_tilt >= 0.0) || !(max_tilt <= 90.0)) return SPZ_AMD_ERR_INVALID_ARG;
    const double norm = std::sqrt((axis[0] * axis[0] + axis[1] * axis[1]) + axis[2] * axis[2]);
    for (int k = 0; k < 3; ++k) u[k] = axis[k] / norm;
    limit = 65536.0 * std::cos(max_tilt * (3.14159265358979323846 / 180.0));
  }
  for (uint32_t h = 0; h < hypotheses; ++h) {
    uint32_t idx[3];
    for (uint32_t k = 0; k < 3; ++k) {
      idx[k] = (uint32_t)(mix64(seed + ((uint64_t)round << 48) + 3ull * h + k) % m);
      if (h_indices) h_indices[3 * h + k] = idx[k];
    }
    if (h_points == nullptr) continue;
    spz_amd_plane q = {};
    const int32_t *P = h_points + 9ull * h;
    if (idx[0] != idx[1] && idx[0] != idx[2] && idx[1] != idx[2]) {
      int64_t u1[3], u2[3];
      for (int k = 0; k < 3; ++k) {
        u1[k] = (int64_t)P[3 + k] - P[k];
        u2[k] = (int64_t)P[6 + k] - P[k];
      }
      const int64_t N[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
      if (N[0] != 0 || N[1] != 0 || N[2] != 0) {
        const double nx = (double)N[0], ny = (double)N[1], nz = (double)N[2];
        const double L = std::sqrt((nx * nx + ny * ny) + nz * nz);
        q.a = (int32_t)std::rint(65536.0 * nx / L);
        q.b = (int32_t)std::rint(65536.0 * ny / L);
        q.c = (int32_t)std::rint(65536.0 * nz / L);
        q.e = (int64_t)q.a * P[0] + (int64_t)q.b * P[1] + (int64_t)q.c * P[2];
        if (axis != nullptr &&
            std::fabs(((double)q.a * u[0] + (double)q.b * u[1]) + (double)q.c * u[2]) < limit) {
          q = spz_amd_plane{};
        }
      }
    }
    h_planes[h] = q;
  }
  return SPZ_AMD_OK;
}

int spz_amd_plane_score_device(void *d_workspace, uint64_t num_points, uint64_t m, const spz_amd_plane *d_planes,
                               uint32_t hypotheses, uint64_t threshold, uint64_t *d_scores, void *hip_stream) {
  if (pl_bad_prepared(d_workspace, num_points, m) || d_planes == nullptr || d_scores == nullptr) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  if (hypotheses < 1u || hypotheses > kPlMaxHypotheses || threshold > kPlMaxThreshold) return SPZ_AMD_ERR_INVALID_ARG;
  int device = 0;
  const int rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  return pl_score(align_ws(d_workspace), pl_layout(num_points), (uint32_t)m, d_planes, hypotheses, threshold, d_scores,
                  static_cast<hipStream_t>(hip_stream));
}

int spz_amd_plane_moments_device(void *d_workspace, uint64_t num_points, uint64_t m, const spz_amd_plane *plane,
                                 uint64_t threshold, spz_amd_plane_moments *d_moments, void *hip_stream) {
  if (pl_bad_prepared(d_workspace, num_points, m) || !pl_plane_ok(plane) || d_moments == nullptr ||
      threshold > kPlMaxThreshold) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  int device = 0;
  const int rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  return pl_moments(align_ws(d_workspace), pl_layout(num_points), (uint32_t)m, *plane, threshold, d_moments,
                    static_cast<hipStream_t>(hip_stream));
}

int spz_amd_plane_solve(const spz_amd_plane_moments *mo, spz_amd_plane *out, double *normal, double *eigenvalues,
                        int *degenerate) {
  if (mo == nullptr || out == nullptr || degenerate == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  *degenerate = 1;
  if (mo->count < 3 || mo->count > SPZ_AMD_REFERENCE_MAX_POINTS) return SPZ_AMD_OK;
  const __int128 K = (__int128)mo->count;
  const int pair[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
  double A[3][3], V[3][3];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) {
      const int k = pair[i][j];
      const __int128 v = K * pl_wide(mo->sum_pp_lo[k], mo->sum_pp_hi[k]) - (__int128)mo->sum_p[i] * mo->sum_p[j];
      A[i][j] = (double)v;  // rounded once
    }
  }
  jacobi3(A, V);
  int order[3] = {0, 1, 2};  // descending eigenvalues, ties in index order
  for (int a = 0; a < 2; ++a) {
    for (int b = a + 1; b < 3; ++b) {
      if (A[order[b]][order[b]] > A[order[a]][order[a]]) std::swap(order[a], order[b]);
    }
  }
  const double l0 = A[order[0]][order[0]], l1 = A[order[1]][order[1]];
  if (!(l0 > 0.0) || !std::isfinite(l0) || !(l1 > 1e-12 * l0)) return SPZ_AMD_OK;
  const int s = order[2];
  const double nv[3] = {V[0][s], V[1][s], V[2][s]};
  spz_amd_plane q = {};
  q.a = (int32_t)std::rint(65536.0 * nv[0]);
  q.b = (int32_t)std::rint(65536.0 * nv[1]);
  q.c = (int32_t)std::rint(65536.0 * nv[2]);
  const __int128 num = (__int128)q.a * mo->sum_p[0] + (__int128)q.b * mo->sum_p[1] + (__int128)q.c * mo->sum_p[2];
  q.e = (int64_t)pl_div_round(num, K);
  if (!pl_plane_ok(&q)) return SPZ_AMD_OK;
  *out = q;
  for (int k = 0; k < 3; ++k) {
    if (normal) normal[k] = nv[k];
    if (eigenvalues) eigenvalues[k] = A[order[k]][order[k]];
  }
  *degenerate = 0;
  return SPZ_AMD_OK;
}

int spz_amd_plane_mark_device(const void *d_workspace, uint64_t num_points, uint64_t m, const spz_amd_plane *plane,
                              uint64_t threshold, uint8_t value, uint8_t *d_labels, void *hip_stream) {
  if (pl_bad_prepared(d_workspace, num_points, m) || !pl_plane_ok(plane) || d_labels == nullptr ||
      threshold > kPlMaxThreshold) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  int device = 0;
  const int rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  return pl_mark(align_ws(const_cast<void *>(d_workspace)), pl_layout(num_points), (uint32_t)num_points, (uint32_t)m,
                 *plane, threshold, value, d_labels, static_cast<hipStream_t>(hip_stream));
}

int spz_amd_plane_placement(const spz_amd_plane *plane, int fractional_bits, int coord, int no_translate,
                            spz_amd_plane_result *out) {
  if (!pl_plane_ok(plane) || out == nullptr || !valid_coord(coord) || fractional_bits < 0 || fractional_bits > 24) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  double flip[3], det;
  pl_flips(coord, flip, &det);
  out->plane = *plane;
  const double a = plane->a, b = plane->b, c = plane->c;
  const double L = std::sqrt((a * a + b * b) + c * c);
  const double nr[3] = {a / L, b / L, c / L};
  const double d = std::ldexp((double)plane->e / L, -fractional_bits);
  for (int k = 0; k < 3; ++k) out->normal[k] = flip[k] * nr[k];
  out->offset = d;
  // the shortest arc n -> stored +Y: q = (n x up, 1 + n . up); below the horizon 1 + n_y = (n_x^2 + n_z^2) / (1 - n_y)
  // has no cancellation
  const double w = nr[1] < 0.0 ? (nr[0] * nr[0] + nr[2] * nr[2]) / (1.0 - nr[1]) : 1.0 + nr[1];
  double q[4] = {-nr[2], 0.0, nr[0], w};
  if (q[3] < 1e-12) {
    q[0] = 1.0;  // a half turn about stored X
    q[1] = q[2] = q[3] = 0.0;
  }
  const double qn = std::sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  for (int k = 0; k < 3; ++k) out->rotation[k] = det * flip[k] * q[k] / qn;
  out->rotation[3] = q[3] / qn;
  out->translation[0] = out->translation[2] = 0.0;
  out->translation[1] = no_translate ? 0.0 : flip[1] * -d;
  out->scale = 1.0;
  return SPZ_AMD_OK;
}

int spz_amd_plane_sides_host(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, const spz_amd_plane *plane,
                             uint64_t threshold, int device, uint8_t *h_side) {
  spz_amd_layout lay;
  int rc = pl_check_stream(d_stream, size, hdr, &lay);
  if (rc != SPZ_AMD_OK) return rc;
  if (!pl_plane_ok(plane) || threshold > kPlMaxThreshold) return SPZ_AMD_ERR_INVALID_ARG;
  const uint32_t n = hdr->num_points;
  if (n == 0) return SPZ_AMD_OK;
  if (h_side == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  DeviceGuard guard;
  rc = guard.enter(device);
  if (rc != SPZ_AMD_OK) return rc;
  PackedResultPtr c;
  rc = packed_result_open(device, &c);
  if (rc != SPZ_AMD_OK) return rc;
  SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&c->block), n));
  hipLaunchKernelGGL(spz_plane_side_kernel, dim3((n + kPlBlock - 1) / kPlBlock), dim3(kPlBlock), 0, c->st,
                     d_stream + lay.offset[SPZ_AMD_SEC_POSITIONS], n, *plane, (long long)threshold, c->block);
  SPZ_HIP_TRY(hipGetLastError());
  SPZ_HIP_TRY(hipMemcpyAsync(h_side, c->block, n, hipMemcpyDeviceToHost, c->st));
  SPZ_HIP_TRY(hipStreamSynchronize(c->st));
  return SPZ_AMD_OK;
}

int spz_amd_plane_host(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr,
                       const spz_amd_plane_options *options, int device, spz_amd_plane_result *results,
                       uint32_t capacity, uint32_t *h_found, uint8_t *h_labels, float *h_ms) {
  if (h_found == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  *h_found = 0;
  int rc = spz_amd_plane_check(options);
  if (rc != SPZ_AMD_OK) return rc;
  const spz_amd_plane_options &o = *options;
  if (results == nullptr || capacity < o.max_planes) return SPZ_AMD_ERR_INVALID_ARG;
  spz_amd_layout lay;
  rc = pl_check_stream(d_stream, size, hdr, &lay);
  if (rc != SPZ_AMD_OK) return rc;
  const int f = (int)hdr->fractional_bits;
  uint64_t T = 0;
  rc = spz_amd_plane_threshold(o.threshold, f, &T);
  if (rc != SPZ_AMD_OK) return rc;
  // the constraint and the hint in the stored frame
  double flip[3], det;
  pl_flips(o.coord, flip, &det);
  double axis[3], hint[3];
  for (int k = 0; k < 3; ++k) {
    axis[k] = flip[k] * o.axis[k];
    hint[k] = flip[k] * o.up_hint[k];
  }
  DeviceGuard guard;
  rc = guard.enter(device);
  if (rc != SPZ_AMD_OK) return rc;
  const uint32_t n = hdr->num_points, H = o.hypotheses;
  PackedResultPtr c;  // the workspace; there is no output stream
  rc = packed_result_open(device, &c);
  if (rc != SPZ_AMD_OK) return rc;
  const PlLayout wl = pl_layout(n);
  WorkspaceOffsets ex;
  ex.off = Workspace::aligned(wl.bytes);
  const uint64_t labels_off = ex.put(n), idx_off = ex.put(3ull * H * 4u), pts_off = ex.put(9ull * H * 4u),
                 planes_off = ex.put((uint64_t)(H + 1u) * sizeof(spz_amd_plane)), scores_off = ex.put(3ull * (H + 1u) * 8u),
                 mom_off = ex.put(sizeof(spz_amd_plane_moments));
  SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&c->block), ex.bytes()));
  uint8_t *ws = align_ws(c->block);
  uint8_t *d_labels = ws + labels_off;
  uint32_t *d_sample = reinterpret_cast<uint32_t *>(ws + idx_off);
  int32_t *d_sampled = reinterpret_cast<int32_t *>(ws + pts_off);
  spz_amd_plane *d_planes = reinterpret_cast<spz_amd_plane *>(ws + planes_off);  // [H]: the refinement's one plane
  uint64_t *d_scores = reinterpret_cast<uint64_t *>(ws + scores_off);
  auto *d_mom = reinterpret_cast<spz_amd_plane_moments *>(ws + mom_off);
  if (n) SPZ_HIP_TRY(hipMemsetAsync(d_labels, 0, n, c->st));
  std::vector<uint32_t> sample(3ull * H);
  std::vector<int32_t> sampled(9ull * H);
  std::vector<spz_amd_plane> planes(H);
  std::vector<uint64_t> scores(3ull * H);
  double ms[3] = {0.0, 0.0, 0.0};
  for (uint32_t r = 0; r < o.max_planes; ++r) {
    auto t0 = std::chrono::steady_clock::now();
    uint64_t m64 = 0;
    rc = pl_prepare(d_stream, size, hdr, lay, o.stride, d_labels, ws, wl, &m64, c->st);
    if (rc != SPZ_AMD_OK) return rc;
    const uint32_t m = (uint32_t)m64;
    if (m < 3u) {
      ms[0] += ms_since(t0);
      break;
    }
    rc = spz_amd_plane_hypotheses(o.seed, r, H, m, nullptr, nullptr, 0.0, sample.data(), nullptr);
    if (rc != SPZ_AMD_OK) return rc;
    SPZ_HIP_TRY(hipMemcpyAsync(d_sample, sample.data(), sample.size() * 4u, hipMemcpyHostToDevice, c->st));
    hipLaunchKernelGGL(spz_plane_gather_kernel, dim3((3u * H + kPlBlock - 1) / kPlBlock), dim3(kPlBlock), 0, c->st,
                       reinterpret_cast<const int4 *>(ws + wl.pts), m, d_sample, 3u * H, d_sampled);
    SPZ_HIP_TRY(hipGetLastError());
    SPZ_HIP_TRY(hipMemcpyAsync(sampled.data(), d_sampled, sampled.size() * 4u, hipMemcpyDeviceToHost, c->st));
    SPZ_HIP_TRY(hipStreamSynchronize(c->st));
    rc = spz_amd_plane_hypotheses(o.seed, r, H, m, sampled.data(), o.has_axis ? axis : nullptr, o.max_tilt, nullptr,
                                  planes.data());
    if (rc != SPZ_AMD_OK) return rc;
    ms[0] += ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    SPZ_HIP_TRY(hipMemcpyAsync(d_planes, planes.data(), planes.size() * sizeof(spz_amd_plane), hipMemcpyHostToDevice, c->st));
    rc = pl_score(ws, wl, m, d_planes, H, T, d_scores, c->st);
    if (rc != SPZ_AMD_OK) return rc;
    SPZ_HIP_TRY(hipMemcpyAsync(scores.data(), d_scores, scores.size() * 8u, hipMemcpyDeviceToHost, c->st));
    SPZ_HIP_TRY(hipStreamSynchronize(c->st));
    ms[1] += ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    uint32_t best = 0;
    for (uint32_t h = 1; h < H; ++h) {
      if (scores[3ull * h + 2] < scores[3ull * best + 2]) best = h;
    }
    uint64_t cost = scores[3ull * best + 2];
    if (cost == UINT64_MAX) break;  // no valid plane
    spz_amd_plane cur = planes[best];
    spz_amd_plane_moments mom;
    uint32_t accepted = 0;
    for (uint32_t it = 0; it < o.refine; ++it) {
      rc = pl_moments(ws, wl, m, cur, T, d_mom, c->st);
      if (rc != SPZ_AMD_OK) return rc;
      SPZ_HIP_TRY(hipMemcpyAsync(&mom, d_mom, sizeof(mom), hipMemcpyDeviceToHost, c->st));
      SPZ_HIP_TRY(hipStreamSynchronize(c->st));
      spz_amd_plane next;
      int degenerate = 0;
      rc = spz_amd_plane_solve(&mom, &next, nullptr, nullptr, &degenerate);
      if (rc != SPZ_AMD_OK) return rc;
      if (degenerate) break;
      uint64_t sc[3];
      SPZ_HIP_TRY(hipMemcpyAsync(d_planes + H, &next, sizeof(next), hipMemcpyHostToDevice, c->st));
      rc = pl_score(ws, wl, m, d_planes + H, 1u, T, d_scores + 3ull * H, c->st);
      if (rc != SPZ_AMD_OK) return rc;
      SPZ_HIP_TRY(hipMemcpyAsync(sc, d_scores + 3ull * H, sizeof(sc), hipMemcpyDeviceToHost, c->st));
      SPZ_HIP_TRY(hipStreamSynchronize(c->st));
      if (!(sc[2] < cost)) break;
      cost = sc[2];
      cur = next;
      accepted += 1u;
    }
    rc = pl_moments(ws, wl, m, cur, T, d_mom, c->st);  // of the final plane: K, S and the sides
    if (rc != SPZ_AMD_OK) return rc;
    SPZ_HIP_TRY(hipMemcpyAsync(&mom, d_mom, sizeof(mom), hipMemcpyDeviceToHost, c->st));
    SPZ_HIP_TRY(hipStreamSynchronize(c->st));
    if (mom.count < o.min_inliers) {
      ms[2] += ms_since(t0);
      break;
    }
    bool negate;
    if (o.has_up_hint) {
      negate = ((double)cur.a * hint[0] + (double)cur.b * hint[1]) + (double)cur.c * hint[2] < 0.0;
    } else if (mom.above != mom.below) {
      negate = mom.below > mom.above;
    } else {
      negate = cur.b < 0;
    }
    if (negate) {
      pl_negate(&cur);
      std::swap(mom.above, mom.below);
    }
    rc = pl_mark(ws, wl, n, m, cur, T, (uint8_t)(r + 1u), d_labels, c->st);
    if (rc != SPZ_AMD_OK) return rc;
    SPZ_HIP_TRY(hipStreamSynchronize(c->st));
    ms[2] += ms_since(t0);
    spz_amd_plane_result &out = results[r];
    std::memset(&out, 0, sizeof(out));
    out.plane = cur;
    out.inliers = mom.count;
    out.sum_abs = mom.sum_abs;
    out.points = m;
    out.above = mom.above;
    out.below = mom.below;
    out.best_hypothesis = best;
    out.refinements = accepted;
    out.fitness = (double)mom.count / (double)m;
    out.mean_distance = mom.count ? std::ldexp((double)mom.sum_abs / (double)mom.count, -(f + 16)) : 0.0;
    rc = spz_amd_plane_placement(&cur, f, o.coord, o.no_translate, &out);
    if (rc != SPZ_AMD_OK) return rc;
    *h_found = r + 1u;
  }
  if (h_labels && n) {
    SPZ_HIP_TRY(hipMemcpyAsync(h_labels, d_labels, n, hipMemcpyDeviceToHost, c->st));
    SPZ_HIP_TRY(hipStreamSynchronize(c->st));
  }
  if (h_ms) {
    for (int k = 0; k < 3; ++k) h_ms[k] = (float)ms[k];
  }
  return SPZ_AMD_OK;
}

}  // extern "C"
