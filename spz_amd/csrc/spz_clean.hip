// spz_clean.hip — floater removal on a packed stream (DESIGN §8 "Clean"): the exact k nearest neighbours of every point
// (statistical outlier removal) and the count of neighbours within a radius, on the stored 24-bit integers, then the
// filter's subset of the kept points.  The input is put in Morton order first (spz_sort.hip's morton_sorted_points:
// sorted (u_x, u_y, u_z, input index), 16 B per point), and both searches are the walk of spz_morton_walk.hpp, which
// describes the traversal; this file holds what the two searches do with a candidate.
//
//   spz_clean_level_kernel       per sorted point, the start level of the k-NN search: the smallest L at which its
//                                own cell holds at least k_eff + 1 points (sliding max / min over the level at which
//                                consecutive points part, in LDS).
//   spz_clean_search_kernel<K>   one wave per 64 consecutive sorted points; every lane keeps a sorted top-K of d2 in
//                                registers (fully unrolled, no runtime index).  A chunk whose common Morton cell is no
//                                nearer than every group lane's k-th distance is skipped.  A point whose k-th d2 is
//                                above its gap to the block's faces retries one level up.
//   spz_clean_radius_kernel      the same walk at one level (4^L >= R2), counting d2 <= R2 up to min_neighbors.
//   spz_clean_sum_kernel /       the threshold: per tile of 2048 scores a sum in a fixed tree, then one workgroup
//   spz_clean_stats_kernel       over the tiles; two passes (mean, then the squared deviations).
//   spz_clean_mask_kernel        keep[i] from the scores, the threshold and the counts.
// Distances are exact: |du| < 2^24, so d2 < 3 * 2^48 is an integer held exactly in f64.  No float atomics: every sum
// runs in an order fixed by n alone, so a run repeats itself.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "spz_amd.h"
#include "spz_block_ops.hpp"
#include "spz_common.hpp"
#include "spz_morton_walk.hpp"
#include "spz_sort_internal.hpp"

#pragma clang fp contract(off)

namespace spz_amd_detail {
namespace {

constexpr uint32_t kClBlock = 256;
constexpr uint32_t kClWaves = kClBlock / 64u;
static_assert(kClBlock == kOpsBlock, "block_sum is over 256 threads");
constexpr uint32_t kClItems = 8;                        // scores per thread of the threshold sums
constexpr uint32_t kClTile = kClBlock * kClItems;       // 2048
constexpr uint32_t kClMaxK = 64;
constexpr uint32_t kClMaxMinNeighbors = 256;
constexpr double kClR2Cap = 1125899906842624.0;         // 2^50 > every d2 (< 3 * 2^48)

struct CleanStats {
  double sum, mean, sq, std, thr;
};

// The smallest distance from u to a point of the closed box [lo, hi], squared, in f64 (exact).
__device__ __forceinline__ double box_d2(const uint32_t u[3], const uint32_t lo[3], const uint32_t hi[3]) {
  double s = 0.0;
#pragma unroll
  for (uint32_t a = 0; a < 3; ++a) {
    const uint32_t d = u[a] < lo[a] ? lo[a] - u[a] : (u[a] > hi[a] ? u[a] - hi[a] : 0u);
    const double f = (double)d;
    s = s + f * f;
  }
  return s;
}

__device__ __forceinline__ double pair_d2(const uint32_t u[3], uint32_t x, uint32_t y, uint32_t z) {
  const double dx = (double)((int32_t)u[0] - (int32_t)x);
  const double dy = (double)((int32_t)u[1] - (int32_t)y);
  const double dz = (double)((int32_t)u[2] - (int32_t)z);
  return dx * dx + dy * dy + dz * dz;  // every term and partial sum is an integer < 2^50: exact
}

// Sorted ascending list t[0..K), insertion of d with the last entry dropped; compile-time indices only.
template <int K>
__device__ __forceinline__ void topk_insert(double (&t)[K], double d) {
#pragma unroll
  for (int j = K - 1; j >= 1; --j) t[j] = fmax(fmin(t[j], d), t[j - 1]);
  t[0] = fmin(t[0], d);
}

struct SearchParams {
  const uint4 *pts;
  const uint8_t *lvl;
  uint32_t n, keff, min_neighbors, radius_level;
  double r2, scale;
  double *scores;
  unsigned long long *kth;
  uint32_t *counts;
};

}  // namespace

// b_t (t >= 1): the level at which sorted points t - 1 and t part, max_a msb(u_a ^ u'_a), -1 when equal.  Window j
// (points j .. j + keff) lies in one cell at level L iff M_j = max(b_j+1 .. b_j+keff) < L; point i's start level is
// 1 + min of M_j over the windows that hold it.
__global__ __launch_bounds__(kClBlock) void spz_clean_level_kernel(const uint4 *pts, uint32_t n, uint32_t keff,
                                                                   uint8_t *lvl) {
  constexpr int H = (int)kClMaxK;
  __shared__ int8_t b[kClBlock + 2 * H];    // b_t for t = i0 - H + 1 .. i0 + 255 + H
  __shared__ int8_t M[kClBlock + H];        // M_j for j = i0 - H .. i0 + 255
  const long long i0 = (long long)blockIdx.x * kClBlock;
  const int K = (int)keff;
  for (int x = threadIdx.x; x < (int)kClBlock + 2 * H; x += kClBlock) {
    const long long t = i0 - H + 1 + x;
    int8_t v = 24;  // outside the points: never joins a window (such windows are not used)
    if (t >= 1 && t < (long long)n) {
      const uint4 p = pts[t], q = pts[t - 1];
      const uint32_t d = (p.x ^ q.x) | (p.y ^ q.y) | (p.z ^ q.z);
      v = d ? (int8_t)(31 - __clz(d)) : (int8_t)-1;
    }
    b[x] = v;
  }
  __syncthreads();
  for (int x = threadIdx.x; x < (int)kClBlock + H; x += kClBlock) {
    const long long j = i0 - H + x;            // b index of b_{j+1} is j + 1 - (i0 - H + 1) = x
    int m = -1;
    for (int r = 0; r < K; ++r) m = max(m, (int)b[x + r]);
    M[x] = (int8_t)m;
    (void)j;
  }
  __syncthreads();
  const long long i = i0 + threadIdx.x;
  if (i >= (long long)n) return;
  const long long jlo = i - K > 0 ? i - K : 0;
  const long long jhi = i < (long long)n - 1 - K ? i : (long long)n - 1 - K;
  int best = 24;
  for (long long j = jlo; j <= jhi; ++j) best = min(best, (int)M[j - (i0 - H)]);
  lvl[i] = (uint8_t)min(best + 1, 24);
}

namespace {

// The k-NN search's side of the walk: a sorted top-K of d2 in registers (fully unrolled, no runtime index).
template <int K>
struct KnnPolicy {
  static constexpr bool kSaturates = true;
  const SearchParams &p;
  uint32_t u[3], self, orig;
  double t[K];

  __device__ __forceinline__ void start() {
#pragma unroll
    for (int j = 0; j < K; ++j) t[j] = (j < K - (int)p.keff) ? -__builtin_inf() : __builtin_inf();
  }
  __device__ __forceinline__ bool more() const { return t[K - 1] > 0.0; }  // else k zero distances: final
  __device__ __forceinline__ bool near(const uint32_t lo[3], const uint32_t hi[3]) const {
    return box_d2(u, lo, hi) < t[K - 1];
  }
  __device__ __forceinline__ void visit(bool mine, uint32_t x, uint32_t y, uint32_t z, uint32_t, uint32_t at) {
    const double d2 = pair_d2(u, x, y, z);
    if (mine && d2 < t[K - 1] && at != self) topk_insert<K>(t, d2);
  }
  // settled when no point outside the block can be nearer than the k-th: its gap to the block's faces
  __device__ __forceinline__ bool settle(uint32_t Lg) {
    const int32_t q[3] = {(int32_t)u[0], (int32_t)u[1], (int32_t)u[2]};
    const long long g = face_gap(q, u, Lg);
    const bool done = Lg >= 24u || g < 0 || t[K - 1] <= (double)g * (double)g;  // g < 2^25: exact in f64
    if (done) {
      double sum = 0.0;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        if (j >= K - (int)p.keff) sum = sum + __builtin_sqrt(t[j]);  // ascending
      }
      p.scores[orig] = sum / (double)p.keff * p.scale;
      if (p.kth) p.kth[orig] = (unsigned long long)t[K - 1];
    }
    return done;
  }
};

// The radius counts' side: other points with d2 <= r2, up to min_neighbors; one level settles every query.
struct RadiusPolicy {
  static constexpr bool kSaturates = true;
  const SearchParams &p;
  uint32_t u[3], self, orig, count;

  __device__ __forceinline__ void start() {}
  __device__ __forceinline__ bool more() const { return count < p.min_neighbors; }
  __device__ __forceinline__ bool near(const uint32_t lo[3], const uint32_t hi[3]) const {
    return more() && box_d2(u, lo, hi) <= p.r2;
  }
  __device__ __forceinline__ void visit(bool mine, uint32_t x, uint32_t y, uint32_t z, uint32_t, uint32_t at) {
    count += (mine && pair_d2(u, x, y, z) <= p.r2 && at != self) ? 1u : 0u;
  }
  __device__ __forceinline__ bool settle(uint32_t) {
    p.counts[orig] = min(count, p.min_neighbors);
    return true;
  }
};

// This lane's sorted point of the wave's 64 into the policy; false for the lanes past the end.  *whole_wave: the wave
// has no point at all.
template <class Policy>
__device__ __forceinline__ bool load_query(const SearchParams &p, Policy &pol, bool *whole_wave) {
  const unsigned long long base_i = ((unsigned long long)blockIdx.x * kClWaves + (threadIdx.x >> 6)) * 64ull;
  *whole_wave = base_i >= p.n;
  pol.self = (uint32_t)base_i + (threadIdx.x & 63u);
  pol.u[0] = pol.u[1] = pol.u[2] = pol.orig = 0;
  if (pol.self >= p.n) return false;
  const uint4 me = p.pts[pol.self];
  pol.u[0] = me.x;
  pol.u[1] = me.y;
  pol.u[2] = me.z;
  pol.orig = me.w;
  return true;
}

}  // namespace

// One wave per 64 sorted points, each from its start level.  See the file comment.
template <int K>
__global__ __launch_bounds__(kClBlock) void spz_clean_search_kernel(const SearchParams p) {
  KnnPolicy<K> pol = {p};
  bool none;
  const bool valid = load_query(p, pol, &none);
  if (none) return;
  morton_walk(p.pts, p.n, threadIdx.x & 63u, valid, pol.u, valid ? (uint32_t)p.lvl[pol.self] : 0u, pol);
}

// The radius counts: every point at radius_level, counting other points with d2 <= r2 up to min_neighbors.
__global__ __launch_bounds__(kClBlock) void spz_clean_radius_kernel(const SearchParams p) {
  RadiusPolicy pol = {p};
  bool none;
  const bool valid = load_query(p, pol, &none);
  if (none) return;
  pol.count = 0;
  morton_walk(p.pts, p.n, threadIdx.x & 63u, valid, pol.u, p.radius_level, pol);
}

// pass 0: the sum of the scores of each tile; pass 1: of their squared deviations from the mean.
__global__ __launch_bounds__(kClBlock) void spz_clean_sum_kernel(const double *scores, uint32_t n, uint32_t pass,
                                                                 const CleanStats *stats, double *partials) {
  __shared__ double s[kClBlock];
  const unsigned long long first = (unsigned long long)blockIdx.x * kClTile + (unsigned long long)threadIdx.x * kClItems;
  const double mean = pass ? stats->mean : 0.0;
  double v = 0.0;
  for (uint32_t r = 0; r < kClItems; ++r) {
    const unsigned long long i = first + r;
    if (i >= n) break;
    const double x = scores[i];
    if (pass) {
      const double d = x - mean;
      v = v + d * d;
    } else {
      v = v + x;
    }
  }
  const double t = block_sum(v, s);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

__global__ __launch_bounds__(kClBlock) void spz_clean_stats_kernel(const double *partials, uint32_t tiles, uint32_t n,
                                                                   uint32_t pass, double std_ratio, CleanStats *stats) {
  __shared__ double s[kClBlock];
  double v = 0.0;
  for (uint32_t t = threadIdx.x; t < tiles; t += kClBlock) v = v + partials[t];
  const double total = block_sum(v, s);
  if (threadIdx.x != 0) return;
  if (pass == 0) {
    stats->sum = total;
    stats->mean = n ? total / (double)n : 0.0;
  } else {
    stats->sq = total;
    stats->std = n > 1 ? __builtin_sqrt(total / (double)(n - 1u)) : 0.0;
    stats->thr = stats->mean + std_ratio * stats->std;
  }
}

// keep[i]: score <= thr (when scores) and count >= min_neighbors (when counts); n <= 1 keeps everything.
__global__ __launch_bounds__(kClBlock) void spz_clean_mask_kernel(const double *scores, const CleanStats *stats,
                                                                  const uint32_t *counts, uint32_t min_neighbors,
                                                                  uint32_t n, uint8_t *keep) {
  const unsigned long long i = (unsigned long long)blockIdx.x * kClBlock + threadIdx.x;
  if (i >= n) return;
  bool k = true;
  if (n > 1) {
    if (scores) k = scores[i] <= stats->thr;
    if (counts) k = k && counts[i] >= min_neighbors;
  }
  keep[i] = k ? 1u : 0u;
}

}  // namespace spz_amd_detail

namespace {

using namespace spz_amd_detail;

struct ClLayout {
  uint64_t tiles;
  uint64_t sort_ws, order, pts, lvl, partials, stats, bytes;
};

ClLayout cl_layout(uint64_t n) {
  ClLayout w;
  w.tiles = (n + kClTile - 1) / kClTile;
  WorkspaceOffsets o;
  o.put(&w.sort_ws, spz_amd_sort_workspace_bytes(n));
  o.put(&w.order, n * 4u);
  o.put(&w.pts, n * 16u);
  o.put(&w.lvl, n);
  o.put(&w.partials, (w.tiles ? w.tiles : 1) * 8u);
  o.put(&w.stats, sizeof(CleanStats));
  w.bytes = o.bytes();
  return w;
}

int check_input(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, spz_amd_layout *lay) {
  const int rc = check_packed_stream(d_stream, size, hdr, lay);
  if (rc != SPZ_AMD_OK) return rc;
  if (hdr->version == 1) return SPZ_AMD_ERR_UNSUPPORTED;  // float16 positions: no integer distances
  if (hdr->num_points > SPZ_AMD_REFERENCE_MAX_POINTS) return SPZ_AMD_ERR_TOO_MANY_POINTS;
  return SPZ_AMD_OK;
}

bool bad_k(int k) { return k < 1 || k > (int)kClMaxK; }
bool bad_min_neighbors(uint32_t m) { return m < 1 || m > kClMaxMinNeighbors; }

// Morton order, then the sorted positions with their input index.
int cl_prepare(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, const spz_amd_layout &lay, uint8_t *ws,
               const ClLayout &wl, hipStream_t st) {
  return morton_sorted_points(d_stream, size, hdr, lay, reinterpret_cast<uint32_t *>(ws + wl.order),
                              reinterpret_cast<uint4 *>(ws + wl.pts), ws + wl.sort_ws, st);
}

uint32_t search_blocks(uint32_t n) { return (n + kClBlock - 1) / kClBlock; }

template <int K>
int launch_search(const SearchParams &p, hipStream_t st) {
  hipLaunchKernelGGL(spz_clean_search_kernel<K>, dim3(search_blocks(p.n)), dim3(kClBlock), 0, st, p);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

// Scores (and k-th d2) of the prepared workspace.  n == 1: score 0, k-th 0.
int cl_scores(const spz_amd_header *hdr, int k, uint8_t *ws, const ClLayout &wl, double *d_scores,
              uint64_t *d_kth, hipStream_t st) {
  const uint32_t n = hdr->num_points;
  if (n == 0) return SPZ_AMD_OK;
  if (n == 1) {
    SPZ_HIP_TRY(hipMemsetAsync(d_scores, 0, 8, st));
    if (d_kth) SPZ_HIP_TRY(hipMemsetAsync(d_kth, 0, 8, st));
    return SPZ_AMD_OK;
  }
  const uint32_t keff = (uint32_t)k < n - 1u ? (uint32_t)k : n - 1u;
  const uint4 *pts = reinterpret_cast<const uint4 *>(ws + wl.pts);
  uint8_t *lvl = ws + wl.lvl;
  hipLaunchKernelGGL(spz_clean_level_kernel, dim3(search_blocks(n)), dim3(kClBlock), 0, st, pts, n, keff, lvl);
  SPZ_HIP_TRY(hipGetLastError());
  SearchParams p = {};
  p.pts = pts;
  p.lvl = lvl;
  p.n = n;
  p.keff = keff;
  p.scale = std::ldexp(1.0, -(int)hdr->fractional_bits);
  p.scores = d_scores;
  p.kth = reinterpret_cast<unsigned long long *>(d_kth);
  if (keff <= 8) return launch_search<8>(p, st);
  if (keff <= 16) return launch_search<16>(p, st);
  if (keff <= 32) return launch_search<32>(p, st);
  return launch_search<64>(p, st);
}

int cl_counts(const spz_amd_header *hdr, uint64_t r2, uint32_t min_neighbors, uint8_t *ws, const ClLayout &wl,
              uint32_t *d_counts, hipStream_t st) {
  const uint32_t n = hdr->num_points;
  if (n == 0) return SPZ_AMD_OK;
  SearchParams p = {};
  p.pts = reinterpret_cast<const uint4 *>(ws + wl.pts);
  p.n = n;
  p.min_neighbors = min_neighbors;
  const double r2d = r2 >= (uint64_t)kClR2Cap ? kClR2Cap : (double)r2;  // exact below 2^50
  p.r2 = r2d;
  uint32_t L = 0;
  while (L < 24u && (double)(1ull << (2u * L)) < r2d) ++L;  // 4^L >= R2: a point outside the block is beyond r
  p.radius_level = L;
  p.counts = d_counts;
  hipLaunchKernelGGL(spz_clean_radius_kernel, dim3(search_blocks(n)), dim3(kClBlock), 0, st, p);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

// The threshold into ws.stats (nothing for n == 0).
int cl_threshold(uint32_t n, double std_ratio, const double *d_scores, uint8_t *ws, const ClLayout &wl,
                 hipStream_t st) {
  if (n == 0) return SPZ_AMD_OK;
  double *partials = reinterpret_cast<double *>(ws + wl.partials);
  CleanStats *stats = reinterpret_cast<CleanStats *>(ws + wl.stats);
  for (uint32_t pass = 0; pass < 2; ++pass) {
    hipLaunchKernelGGL(spz_clean_sum_kernel, dim3((unsigned)wl.tiles), dim3(kClBlock), 0, st, d_scores, n, pass, stats,
                       partials);
    SPZ_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(spz_clean_stats_kernel, dim3(1), dim3(kClBlock), 0, st, partials, (uint32_t)wl.tiles, n, pass,
                       std_ratio, stats);
    SPZ_HIP_TRY(hipGetLastError());
  }
  return SPZ_AMD_OK;
}

}  // namespace

extern "C" {

uint64_t spz_amd_clean_workspace_bytes(uint64_t n) { return cl_layout(n).bytes; }

int spz_amd_clean_radius_r2(double radius, int fractional_bits, uint64_t *r2) {
  if (r2 == nullptr || !std::isfinite(radius) || !(radius > 0.0) || fractional_bits < 0 || fractional_bits > 24) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  const double q = radius * std::ldexp(1.0, fractional_bits);
  const double s = std::floor(q * q);
  *r2 = s >= 18446744073709551616.0 ? UINT64_MAX : (uint64_t)s;
  return SPZ_AMD_OK;
}

int spz_amd_knn_scores_device(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, int k,
                              double *d_scores, uint64_t *d_kth_d2, void *d_workspace, void *hip_stream) {
  spz_amd_layout lay;
  int rc = check_input(d_stream, size, hdr, &lay);
  if (rc != SPZ_AMD_OK) return rc;
  if (bad_k(k) || d_scores == nullptr || d_workspace == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const ClLayout wl = cl_layout(hdr->num_points);
  uint8_t *ws = align_ws(d_workspace);
  rc = cl_prepare(d_stream, size, hdr, lay, ws, wl, st);
  if (rc != SPZ_AMD_OK) return rc;
  return cl_scores(hdr, k, ws, wl, d_scores, d_kth_d2, st);
}

int spz_amd_radius_counts_device(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, uint64_t r2,
                                 uint32_t min_neighbors, uint32_t *d_counts, void *d_workspace, void *hip_stream) {
  spz_amd_layout lay;
  int rc = check_input(d_stream, size, hdr, &lay);
  if (rc != SPZ_AMD_OK) return rc;
  if (bad_min_neighbors(min_neighbors) || d_counts == nullptr || d_workspace == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const ClLayout wl = cl_layout(hdr->num_points);
  uint8_t *ws = align_ws(d_workspace);
  rc = cl_prepare(d_stream, size, hdr, lay, ws, wl, st);
  if (rc != SPZ_AMD_OK) return rc;
  return cl_counts(hdr, r2, min_neighbors, ws, wl, d_counts, st);
}

int spz_amd_clean_open(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, int k, double std_ratio,
                       double radius, uint32_t min_neighbors, int device, void **ctx, uint64_t *h_out_bytes,
                       uint64_t *h_kept, double *h_threshold, uint8_t *h_mask, double *h_scores, float *h_ms) {
  if (ctx == nullptr || h_out_bytes == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  *ctx = nullptr;
  *h_out_bytes = 0;
  spz_amd_layout lay;
  int rc = check_input(d_stream, size, hdr, &lay);
  if (rc != SPZ_AMD_OK) return rc;
  const bool stat = k != 0, rad = min_neighbors != 0;
  if (!stat && !rad) return SPZ_AMD_ERR_INVALID_ARG;  // at least one rule
  if (stat && (bad_k(k) || !std::isfinite(std_ratio))) return SPZ_AMD_ERR_INVALID_ARG;
  uint64_t r2 = 0;
  if (rad && (bad_min_neighbors(min_neighbors) ||
              spz_amd_clean_radius_r2(radius, hdr->fractional_bits, &r2) != SPZ_AMD_OK)) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  if (h_scores && !stat) return SPZ_AMD_ERR_INVALID_ARG;
  const uint64_t n = hdr->num_points;
  DeviceGuard guard;
  rc = guard.enter(device);
  if (rc != SPZ_AMD_OK) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  PackedResultPtr c;
  rc = packed_result_open(device, &c);
  if (rc != SPZ_AMD_OK) return rc;
  const ClLayout wl = cl_layout(n);
  WorkspaceOffsets o = {wl.bytes};
  const uint64_t o_scores = o.put(n * 8u), o_counts = o.put(n * 4u), o_mask = o.put(n), o_idx = o.put(n * 4u),
                 o_fws = o.put(spz_amd_filter_workspace_bytes(n));
  SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&c->block), o.off));
  uint8_t *ws = align_ws(c->block);
  uint8_t *raw = c->block;  // the extra sections are placed from the unaligned base (each is 256-aligned by hipMalloc)
  double *d_scores = stat ? reinterpret_cast<double *>(raw + o_scores) : nullptr;
  uint32_t *d_counts = rad ? reinterpret_cast<uint32_t *>(raw + o_counts) : nullptr;
  uint8_t *d_mask = raw + o_mask;
  uint32_t *d_idx = reinterpret_cast<uint32_t *>(raw + o_idx);
  rc = cl_prepare(d_stream, size, hdr, lay, ws, wl, c->st);
  if (rc != SPZ_AMD_OK) return rc;
  SPZ_HIP_TRY(hipStreamSynchronize(c->st));
  const double sort_ms = ms_since(t0);
  if (stat) {
    rc = cl_scores(hdr, k, ws, wl, d_scores, nullptr, c->st);
    if (rc != SPZ_AMD_OK) return rc;
  }
  if (rad) {
    rc = cl_counts(hdr, r2, min_neighbors, ws, wl, d_counts, c->st);
    if (rc != SPZ_AMD_OK) return rc;
  }
  SPZ_HIP_TRY(hipStreamSynchronize(c->st));
  const double search_ms = ms_since(t0) - sort_ms;
  CleanStats stats = {};
  if (n) {
    if (stat) {
      rc = cl_threshold((uint32_t)n, std_ratio, d_scores, ws, wl, c->st);
      if (rc != SPZ_AMD_OK) return rc;
    }
    hipLaunchKernelGGL(spz_clean_mask_kernel, dim3((unsigned)((n + kClBlock - 1) / kClBlock)), dim3(kClBlock), 0,
                       c->st, d_scores, reinterpret_cast<const CleanStats *>(ws + wl.stats), d_counts, min_neighbors,
                       (uint32_t)n, d_mask);
    SPZ_HIP_TRY(hipGetLastError());
    if (stat) {
      SPZ_HIP_TRY(hipMemcpyAsync(&stats, ws + wl.stats, sizeof(stats), hipMemcpyDeviceToHost, c->st));
    }
  }
  uint64_t kept = 0;
  rc = select_subset_masked(d_stream, size, hdr, d_mask, d_idx, raw + o_fws, c.get(), &kept);
  if (rc != SPZ_AMD_OK) return rc;
  if (h_mask && n) SPZ_HIP_TRY(hipMemcpyAsync(h_mask, d_mask, n, hipMemcpyDeviceToHost, c->st));
  if (h_scores && n) SPZ_HIP_TRY(hipMemcpyAsync(h_scores, d_scores, n * 8u, hipMemcpyDeviceToHost, c->st));
  SPZ_HIP_TRY(hipStreamSynchronize(c->st));
  if (h_ms) {
    h_ms[0] = (float)sort_ms;
    h_ms[1] = (float)search_ms;
    h_ms[2] = (float)(ms_since(t0) - sort_ms - search_ms);
  }
  if (h_kept) *h_kept = kept;
  if (h_threshold) *h_threshold = stat ? stats.thr : __builtin_nan("");
  *h_out_bytes = c->out_bytes;
  *ctx = c.release();
  return SPZ_AMD_OK;
}

int spz_amd_clean_fetch(void *ctx, uint8_t *h_out) { return packed_result_fetch(ctx, h_out); }

const uint8_t *spz_amd_clean_device_data(void *ctx) { return packed_result_device_data(ctx); }

void spz_amd_clean_close(void *ctx) { packed_result_close(ctx); }

}  // extern "C"
