// spz_align.hip — registration of two packed streams (DESIGN §8 "Align"; the contract is in include/spz_amd.h): a
// point-to-point, trimmed ICP with an optional scale, on the stored 24-bit integers of both clouds.
//
//   spz_align_query_kernel       one wave per 64 consecutive source points of the source's own Morton order (both clouds
//                                are sorted once per run: spz_sort.hip's morton_sorted_points).  Every lane maps its
//                                point (f64, no fused multiply-add), rounds it to the target's grid and saturates it;
//                                its start level comes from the target's occupancy at the query's cell (one binary
//                                search for the query's place in the sorted target: the two points beside that place
//                                share the longest Morton prefix with it).  Then the walk of spz_morton_walk.hpp, which
//                                describes the traversal; a query whose best d2 is not below its gap to the block's
//                                faces retries one level up.  A query outside the target's cube is located by its
//                                projection onto the cube (no target point is nearer to the query than to that
//                                projection); its distances are its own.  k = 1 with (d2, target input index) as the
//                                key; distances are uint64 (< 2^56, beyond f64's exact range).  With a distance limit
//                                the level whose cell side covers it is final.
//   spz_align_key_kernel /       trimming: d2 as two u32 key planes for the stable radix sort (spz_sort_internal.hpp),
//   spz_align_select_kernel      ties in input order; the first K = min(c, ceil(overlap c)) ranks are the inliers.
//   spz_align_moment_kernel /    the moments of the inliers: per tile of 2048 source points a pairwise sum in a fixed
//   spz_align_reduce_kernel      tree, then one workgroup over the tiles.  No float atomics: the order depends on n_s
//                                alone, so a run repeats its bits.  Counts and the sum of d2 are integers.
// The solve (means, covariance, a 3x3 one-sided Jacobi SVD, Umeyama's scale) runs on the host in f64.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstddef>
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

constexpr uint32_t kAlBlock = 256;
constexpr uint32_t kAlWaves = kAlBlock / 64u;
static_assert(kAlBlock == kOpsBlock, "block_sum is over 256 threads");
constexpr uint32_t kAlItems = 8;                      // source points per thread of the moment sums
constexpr uint32_t kAlTile = kAlBlock * kAlItems;     // 2048
constexpr uint32_t kAlSums = 17;                      // f64 sums: a (3), b (3), a b^T (9), |a|^2, |b|^2
constexpr uint32_t kAlPartial = kAlSums + 3;          // + count, sum d2 low and high halves (u64)
constexpr uint32_t kAlReduceItems = 32;               // tiles per thread of the reduce: 8192 tiles >= 10 M / 2048
constexpr uint32_t kAlNone = 0xffffffffu;
constexpr int32_t kAlBias = 0x800000;
constexpr uint64_t kAlNoLimit = UINT64_MAX;

struct QueryParams {
  const uint4 *tpts;
  const uint4 *spts;
  uint32_t nt, ns, stride, limit_level;
  double m[12];
  double src_scale, tgt_scale;   // 2^-f_s, 2^f_t
  unsigned long long limit;      // candidates have d2 <= limit
  uint32_t *index;
  unsigned long long *d2;
  uint32_t *counter;             // += the number of queries with a neighbour
};

struct MomentParams {
  const uint8_t *spos, *tpos;    // the position sections
  uint32_t ns, stride, self;     // self: every taking-part point is its own neighbour (a centroid)
  const uint32_t *index;
  const unsigned long long *d2;
  const uint8_t *inlier;
  double src_scale, tgt_scale;   // 2^-f_s, 2^-f_t
  unsigned long long *partials;  // tiles x kAlPartial words
};

__device__ __forceinline__ unsigned long long al_sq(int32_t d) {
  const uint32_t a = (uint32_t)(d < 0 ? -d : d);  // |d| < 2^27
  return (unsigned long long)a * a;
}

// The smallest squared distance from the query q (biased, may lie outside the cube) to the closed box [lo, hi].
__device__ __forceinline__ unsigned long long al_box_d2(const int32_t q[3], const uint32_t lo[3], const uint32_t hi[3]) {
  unsigned long long s = 0;
#pragma unroll
  for (uint32_t a = 0; a < 3; ++a) {
    const int32_t l = (int32_t)lo[a], h = (int32_t)hi[a];
    const int32_t d = q[a] < l ? l - q[a] : (q[a] > h ? q[a] - h : 0);
    s += al_sq(d);
  }
  return s;
}

__device__ __forceinline__ unsigned long long al_pair_d2(const int32_t q[3], uint32_t x, uint32_t y, uint32_t z) {
  return al_sq(q[0] - (int32_t)x) + al_sq(q[1] - (int32_t)y) + al_sq(q[2] - (int32_t)z);  // < 3 * 2^54
}

// The nearest-neighbour side of the walk: the minimum of (d2, target input index) within the limit.
struct NearestPolicy {
  static constexpr bool kSaturates = false;
  const QueryParams &p;
  int32_t q[3];        // the query, biased; may lie outside the cube
  uint32_t c[3], orig; // q clamped to the cube
  unsigned long long best;
  uint32_t bidx;

  __device__ __forceinline__ void start() {}
  __device__ __forceinline__ bool more() const { return true; }
  // <=: a point at the best distance with a smaller input index replaces the best
  __device__ __forceinline__ bool near(const uint32_t lo[3], const uint32_t hi[3]) const {
    return al_box_d2(q, lo, hi) <= (best < p.limit ? best : p.limit);
  }
  __device__ __forceinline__ void visit(bool mine, uint32_t x, uint32_t y, uint32_t z, uint32_t w, uint32_t) {
    const unsigned long long d2 = al_pair_d2(q, x, y, z);
    if (mine && d2 <= p.limit && (d2 < best || (d2 == best && w < bidx))) {
      best = d2;
      bidx = w;
    }
  }
  // settled when every point outside the block is farther than the best: the gap to the block's faces, strictly (a
  // point at the same distance outside the block could have the smaller index)
  __device__ __forceinline__ bool settle(uint32_t Lg) {
    const long long g = face_gap(q, c, Lg);
    if (Lg < 24u && Lg < p.limit_level && g >= 0 && !(best < (unsigned long long)g * (unsigned long long)g)) return false;
    p.index[orig] = bidx;
    p.d2[orig] = bidx == kAlNone ? kAlNoLimit : best;
    return true;
  }
};

}  // namespace

// One wave per 64 sorted source points.  See the file comment.
__global__ __launch_bounds__(kAlBlock) void spz_align_query_kernel(const QueryParams p) {
  const uint32_t lane = threadIdx.x & 63u;
  const unsigned long long base_i = ((unsigned long long)blockIdx.x * kAlWaves + (threadIdx.x >> 6)) * 64ull;
  if (base_i >= p.ns) return;  // the whole wave
  const uint32_t i = (uint32_t)base_i + lane;
  const bool in_range = i < p.ns;
  NearestPolicy pol = {p, {0, 0, 0}, {0, 0, 0}, 0, kAlNoLimit, kAlNone};
  uint32_t L = 0;
  bool valid = false;
  if (in_range) {
    const uint4 me = p.spts[i];
    pol.orig = me.w;
    if (pol.orig % p.stride == 0u) {
      const double x = (double)((int32_t)me.x - kAlBias) * p.src_scale;
      const double y = (double)((int32_t)me.y - kAlBias) * p.src_scale;
      const double z = (double)((int32_t)me.z - kAlBias) * p.src_scale;
      valid = true;
#pragma unroll
      for (uint32_t a = 0; a < 3; ++a) {
        const double v = ((p.m[3 * a] * x + p.m[3 * a + 1] * y) + p.m[3 * a + 2] * z) + p.m[9 + a];
        valid = valid && __builtin_isfinite(v);
        const double r = fmax(-67108864.0, fmin(67108864.0, __builtin_rint(v * p.tgt_scale)));  // +-2^26
        pol.q[a] = (valid ? (int32_t)r : 0) + kAlBias;
        pol.c[a] = (uint32_t)min(max(pol.q[a], 0), 0xffffff);
      }
    }
  }
  if (valid) L = min(occupied_level(p.tpts, p.nt, pol.c), p.limit_level);
  morton_walk(p.tpts, p.nt, lane, valid, pol.c, L, pol);
  if (in_range && !valid) {
    p.index[pol.orig] = kAlNone;
    p.d2[pol.orig] = kAlNoLimit;
  }
  const unsigned long long found = __ballot(valid && pol.bidx != kAlNone);
  if (lane == 0 && found) atomicAdd(p.counter, (uint32_t)__popcll(found));
}

// d2 as radix keys: the stable ascending sort ranks by (d2, input index); points without a neighbour come last.
__global__ __launch_bounds__(kAlBlock) void spz_align_key_kernel(const unsigned long long *d2, uint32_t n, uint32_t *k0,
                                                                 uint32_t *k1) {
  const uint32_t i = blockIdx.x * kAlBlock + threadIdx.x;
  if (i >= n) return;
  const unsigned long long k = d2[i];
  k0[i] = (uint32_t)k;
  k1[i] = (uint32_t)(k >> 32);
}

// order != NULL: inlier[order[r]] = r < K, K = min(c, ceil(overlap c)) in f64 over the c candidates (*counter).
// order == NULL (overlap 1): every candidate is an inlier.
__global__ __launch_bounds__(kAlBlock) void spz_align_select_kernel(const uint32_t *order, const uint32_t *index,
                                                                    uint32_t n, const uint32_t *counter, double overlap,
                                                                    uint8_t *inlier) {
  const uint32_t r = blockIdx.x * kAlBlock + threadIdx.x;
  if (r >= n) return;
  if (order == nullptr) {
    inlier[r] = index[r] != kAlNone ? 1u : 0u;
    return;
  }
  const uint32_t c = *counter;
  const double k = __builtin_ceil(overlap * (double)c);
  const uint32_t K = k >= (double)c ? c : (uint32_t)k;
  inlier[order[r]] = r < K ? 1u : 0u;
}

// The moments of one tile of 2048 source points (input order).  A thread's eight terms are added pairwise, then the
// workgroup's 256 sums in a binary tree: depth 11 for the tile.
__global__ __launch_bounds__(kAlBlock) void spz_align_moment_kernel(const MomentParams p) {
  __shared__ unsigned long long s[kAlBlock];
  const unsigned long long first = (unsigned long long)blockIdx.x * kAlTile + (unsigned long long)threadIdx.x * kAlItems;
  double l0[kAlSums], l1[kAlSums], l2[kAlSums];
  unsigned long long count = 0, dlo = 0, dhi = 0;
#pragma unroll
  for (uint32_t r = 0; r < kAlItems; ++r) {
    const unsigned long long i = first + r;
    double t[kAlSums];
#pragma unroll
    for (uint32_t k = 0; k < kAlSums; ++k) t[k] = 0.0;
    const bool in = i < p.ns && (p.self ? (i % p.stride == 0u) : p.inlier[i] != 0u);
    if (in) {
      double a[3], b[3];
#pragma unroll
      for (uint32_t k = 0; k < 3; ++k) a[k] = (double)((int32_t)load_u(p.spos, i, k) - kAlBias) * p.src_scale;
      if (p.self) {
#pragma unroll
        for (uint32_t k = 0; k < 3; ++k) b[k] = a[k];
      } else {
        const uint32_t j = p.index[i];
#pragma unroll
        for (uint32_t k = 0; k < 3; ++k) b[k] = (double)((int32_t)load_u(p.tpos, j, k) - kAlBias) * p.tgt_scale;
        const unsigned long long d = p.d2[i];
        dlo += d & 0xffffffffull;
        dhi += d >> 32;
      }
      count += 1;
#pragma unroll
      for (uint32_t k = 0; k < 3; ++k) {
        t[k] = a[k];
        t[3 + k] = b[k];
#pragma unroll
        for (uint32_t m = 0; m < 3; ++m) t[6 + 3 * k + m] = a[k] * b[m];
      }
      t[15] = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
      t[16] = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2];
    }
#pragma unroll
    for (uint32_t k = 0; k < kAlSums; ++k) {  // a binary counter: pairs, fours, eight
      if ((r & 1u) == 0u) {
        l0[k] = t[k];
      } else {
        l0[k] = l0[k] + t[k];
        if ((r & 2u) == 0u) {
          l1[k] = l0[k];
        } else {
          l1[k] = l1[k] + l0[k];
          if ((r & 4u) == 0u) {
            l2[k] = l1[k];
          } else {
            l2[k] = l2[k] + l1[k];
          }
        }
      }
    }
  }
  unsigned long long *out = p.partials + (unsigned long long)blockIdx.x * kAlPartial;
#pragma unroll
  for (uint32_t k = 0; k < kAlSums; ++k) {
    const double v = block_sum(l2[k], reinterpret_cast<double *>(s));
    if (threadIdx.x == 0) out[k] = (unsigned long long)__double_as_longlong(v);
  }
  const unsigned long long c = block_sum(count, s), lo = block_sum(dlo, s), hi = block_sum(dhi, s);
  if (threadIdx.x == 0) {
    out[kAlSums] = c;
    out[kAlSums + 1] = lo;
    out[kAlSums + 2] = hi;
  }
}

// One workgroup over the tiles: a thread adds its (at most 32) tiles pairwise, then the binary tree.
__global__ __launch_bounds__(kAlBlock) void spz_align_reduce_kernel(const unsigned long long *partials, uint32_t tiles,
                                                                    const uint32_t *counter, uint64_t taking_part,
                                                                    spz_amd_align_moments *out) {
  __shared__ unsigned long long s[kAlBlock];
  // sum_a, sum_b, sum_ab, sum_aa, sum_bb are 17 consecutive doubles of the result, in the partials' order
  double *sums = out->sum_a;
  static_assert(offsetof(spz_amd_align_moments, sum_bb) - offsetof(spz_amd_align_moments, sum_a) == (kAlSums - 1) * 8,
                "the f64 sums are contiguous");
  for (uint32_t k = 0; k < kAlSums; ++k) {
    double v[kAlReduceItems];
#pragma unroll
    for (uint32_t r = 0; r < kAlReduceItems; ++r) {
      const uint32_t t = threadIdx.x + r * kAlBlock;
      v[r] = t < tiles ? __longlong_as_double((long long)partials[(unsigned long long)t * kAlPartial + k]) : 0.0;
    }
#pragma unroll
    for (uint32_t w = 1; w < kAlReduceItems; w <<= 1) {
#pragma unroll
      for (uint32_t r = 0; r < kAlReduceItems; r += 2u * w) v[r] = v[r] + v[r + w];
    }
    const double total = block_sum(v[0], reinterpret_cast<double *>(s));
    if (threadIdx.x == 0) sums[k] = total;
  }
  unsigned long long ints[3];
#pragma unroll
  for (uint32_t k = 0; k < 3; ++k) {
    unsigned long long v = 0;
    for (uint32_t t = threadIdx.x; t < tiles; t += kAlBlock) v += partials[(unsigned long long)t * kAlPartial + kAlSums + k];
    ints[k] = block_sum(v, s);
  }
  if (threadIdx.x != 0) return;
  out->count = ints[0];
  out->taking_part = taking_part;
  out->candidates = counter ? (uint64_t)*counter : ints[0];
  // sum d2 = high * 2^32 + low, carried into two words
  const unsigned long long carry = ints[1] >> 32;
  out->sum_d2_lo = ((ints[2] + carry) << 32) | (ints[1] & 0xffffffffull);
  out->sum_d2_hi = (ints[2] + carry) >> 32;
}

}  // namespace spz_amd_detail

namespace {

using namespace spz_amd_detail;

struct AlLayout {
  uint64_t tiles;
  uint64_t sort_ws, order, tpts, spts, index, d2, inlier, partials, counter, bytes;
};

AlLayout al_layout(uint64_t ns, uint64_t nt) {
  AlLayout w;
  w.tiles = (ns + kAlTile - 1) / kAlTile;
  const uint64_t nmax = ns > nt ? ns : nt;
  WorkspaceOffsets o;
  o.put(&w.sort_ws, spz_amd_sort_workspace_bytes(nmax));
  o.put(&w.order, nmax * 4u);
  o.put(&w.tpts, nt * 16u);
  o.put(&w.spts, ns * 16u);
  o.put(&w.index, ns * 4u);
  o.put(&w.d2, ns * 8u);
  o.put(&w.inlier, ns);
  o.put(&w.partials, ((nmax + kAlTile - 1) / kAlTile + 1) * kAlPartial * 8u);  // the target's centroid uses it too
  o.put(&w.counter, 256u);
  w.bytes = o.bytes();
  return w;
}

int al_check_cloud(const spz_amd_align_cloud *c, spz_amd_layout *lay) {
  if (c == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  const spz_amd_header *hdr = &c->hdr;
  const int rc = check_packed_stream(c->d_stream, c->size, hdr, lay);
  if (rc != SPZ_AMD_OK) return rc;
  if (hdr->version == 1) return SPZ_AMD_ERR_UNSUPPORTED;  // float16 positions: no integer distances
  if (hdr->num_points > SPZ_AMD_REFERENCE_MAX_POINTS) return SPZ_AMD_ERR_TOO_MANY_POINTS;
  if (hdr->fractional_bits > 24) return SPZ_AMD_ERR_INVALID_ARG;
  return SPZ_AMD_OK;
}

// Both clouds: the source may be empty, the target may not.
int al_check_pair(const spz_amd_align_cloud *source, const spz_amd_align_cloud *target, spz_amd_layout *sl,
                  spz_amd_layout *tl) {
  int rc = al_check_cloud(source, sl);
  if (rc != SPZ_AMD_OK) return rc;
  rc = al_check_cloud(target, tl);
  if (rc != SPZ_AMD_OK) return rc;
  if (target->hdr.num_points == 0) return SPZ_AMD_ERR_INVALID_ARG;
  return SPZ_AMD_OK;
}

bool al_bad_map(const double *map) {
  if (map == nullptr) return true;
  for (int k = 0; k < 12; ++k) {
    if (!std::isfinite(map[k])) return true;
  }
  return false;
}

bool al_bad_overlap(double f) { return !(f > 0.0) || !(f <= 1.0); }

int al_sort_one(const spz_amd_align_cloud *c, const spz_amd_layout &lay, uint8_t *ws, const AlLayout &wl, uint64_t pts_off,
                hipStream_t st) {
  return morton_sorted_points(c->d_stream, c->size, &c->hdr, lay, reinterpret_cast<uint32_t *>(ws + wl.order),
                              reinterpret_cast<uint4 *>(ws + pts_off), ws + wl.sort_ws, st);
}

int al_prepare(const spz_amd_align_cloud *source, const spz_amd_layout &sl, const spz_amd_align_cloud *target,
               const spz_amd_layout &tl, uint8_t *ws, const AlLayout &wl, hipStream_t st) {
  int rc = al_sort_one(target, tl, ws, wl, wl.tpts, st);
  if (rc != SPZ_AMD_OK) return rc;
  return al_sort_one(source, sl, ws, wl, wl.spts, st);
}

// Steps 1-3 into (d_index, d_d2); the candidate count into the workspace's counter.
int al_query(const spz_amd_align_cloud *source, const spz_amd_align_cloud *target, uint32_t stride, const double *map,
             uint64_t r2, uint32_t *d_index, uint64_t *d_d2, uint8_t *ws, const AlLayout &wl, hipStream_t st) {
  const uint32_t ns = source->hdr.num_points;
  uint32_t *counter = reinterpret_cast<uint32_t *>(ws + wl.counter);
  SPZ_HIP_TRY(hipMemsetAsync(counter, 0, 4, st));
  if (ns == 0) return SPZ_AMD_OK;
  QueryParams p = {};
  p.tpts = reinterpret_cast<const uint4 *>(ws + wl.tpts);
  p.spts = reinterpret_cast<const uint4 *>(ws + wl.spts);
  p.nt = target->hdr.num_points;
  p.ns = ns;
  p.stride = stride;
  std::memcpy(p.m, map, sizeof(p.m));
  p.src_scale = std::ldexp(1.0, -(int)source->hdr.fractional_bits);
  p.tgt_scale = std::ldexp(1.0, (int)target->hdr.fractional_bits);
  p.limit = r2;
  uint32_t L = 24u;
  if (r2 != kAlNoLimit) {
    L = 0;
    while (L < 24u && (1ull << (2u * L)) < r2) ++L;  // 4^L >= R2: a point outside the block is beyond the limit
  }
  p.limit_level = L;
  p.index = d_index;
  p.d2 = reinterpret_cast<unsigned long long *>(d_d2);
  p.counter = counter;
  hipLaunchKernelGGL(spz_align_query_kernel, dim3((ns + kAlBlock - 1) / kAlBlock), dim3(kAlBlock), 0, st, p);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

// Step 4 into d_inlier.
int al_select(uint32_t ns, double overlap, const uint32_t *d_index, const uint64_t *d_d2, uint8_t *d_inlier, uint8_t *ws,
              const AlLayout &wl, hipStream_t st) {
  if (ns == 0) return SPZ_AMD_OK;
  const unsigned blocks = (ns + kAlBlock - 1) / kAlBlock;
  const uint32_t *counter = reinterpret_cast<const uint32_t *>(ws + wl.counter);
  const uint32_t *order = nullptr;
  if (overlap < 1.0) {
    const SortLayout sl = sort_layout(ns);
    uint8_t *sws = ws + wl.sort_ws;  // 256-aligned: ws is
    hipLaunchKernelGGL(spz_align_key_kernel, dim3(blocks), dim3(kAlBlock), 0, st,
                       reinterpret_cast<const unsigned long long *>(d_d2), ns,
                       reinterpret_cast<uint32_t *>(sws + sl.planes_off[0][0]),
                       reinterpret_cast<uint32_t *>(sws + sl.planes_off[0][1]));
    SPZ_HIP_TRY(hipGetLastError());
    uint32_t *d_order = reinterpret_cast<uint32_t *>(ws + wl.order);
    const int rc = radix_passes(ns, 8u, d_order, sws, sl, st);
    if (rc != SPZ_AMD_OK) return rc;
    order = d_order;
  }
  hipLaunchKernelGGL(spz_align_select_kernel, dim3(blocks), dim3(kAlBlock), 0, st, order, d_index, ns, counter, overlap,
                     d_inlier);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

// Step 5 into *d_out.  self: the centroid sums of `source` alone (every taking-part point, b = a).
int al_moments(const spz_amd_align_cloud *source, const spz_amd_layout &sl, const spz_amd_align_cloud *target,
               const spz_amd_layout *tl, uint32_t stride, bool self, const uint32_t *d_index, const uint64_t *d_d2,
               const uint8_t *d_inlier, spz_amd_align_moments *d_out, uint8_t *ws, const AlLayout &wl, hipStream_t st) {
  const uint32_t ns = source->hdr.num_points;
  const uint64_t tiles = ((uint64_t)ns + kAlTile - 1) / kAlTile;
  const uint64_t taking_part = ((uint64_t)ns + stride - 1) / stride;
  unsigned long long *partials = reinterpret_cast<unsigned long long *>(ws + wl.partials);
  if (ns) {
    MomentParams p = {};
    p.spos = source->d_stream + sl.offset[SPZ_AMD_SEC_POSITIONS];
    p.tpos = self ? nullptr : target->d_stream + tl->offset[SPZ_AMD_SEC_POSITIONS];
    p.ns = ns;
    p.stride = stride;
    p.self = self ? 1u : 0u;
    p.index = d_index;
    p.d2 = reinterpret_cast<const unsigned long long *>(d_d2);
    p.inlier = d_inlier;
    p.src_scale = std::ldexp(1.0, -(int)source->hdr.fractional_bits);
    p.tgt_scale = self ? p.src_scale : std::ldexp(1.0, -(int)target->hdr.fractional_bits);
    p.partials = partials;
    hipLaunchKernelGGL(spz_align_moment_kernel, dim3((unsigned)tiles), dim3(kAlBlock), 0, st, p);
    SPZ_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(spz_align_reduce_kernel, dim3(1), dim3(kAlBlock), 0, st, partials, (uint32_t)tiles,
                     self ? nullptr : reinterpret_cast<const uint32_t *>(ws + wl.counter), taking_part, d_out);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

// ---- the host side of the solve ----------------------------------------------------------------------------------
double det3(const double m[3][3]) {
  return m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
         m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
}

// H = U diag(D) V^T by one-sided Jacobi (Hestenes): the columns of A = H V are made orthogonal; D descending.  The third
// column of U is +-(u0 x u1), so U is orthonormal whatever D[2] is.  false when D[1] <= 1e-12 D[0] (U is not set).
bool svd3(const double H[3][3], double U[3][3], double D[3], double V[3][3]) {
  double A[3][3];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) {
      A[i][j] = H[i][j];
      V[i][j] = i == j ? 1.0 : 0.0;
    }
  }
  for (int sweep = 0; sweep < 64; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < 2; ++p) {
      for (int q = p + 1; q < 3; ++q) {
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
        for (int k = 0; k < 3; ++k) {
          alpha += A[k][p] * A[k][p];
          beta += A[k][q] * A[k][q];
          gamma += A[k][p] * A[k][q];
        }
        if (gamma == 0.0 || std::fabs(gamma) <= 1e-17 * std::sqrt(alpha) * std::sqrt(beta)) continue;
        rotated = true;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
        for (int k = 0; k < 3; ++k) {
          const double a = A[k][p], b = A[k][q];
          A[k][p] = c * a - s * b;
          A[k][q] = s * a + c * b;
          const double va = V[k][p], vb = V[k][q];
          V[k][p] = c * va - s * vb;
          V[k][q] = s * va + c * vb;
        }
      }
    }
    if (!rotated) break;
  }
  for (int j = 0; j < 3; ++j) D[j] = std::sqrt(A[0][j] * A[0][j] + A[1][j] * A[1][j] + A[2][j] * A[2][j]);
  for (int a = 0; a < 2; ++a) {  // descending
    for (int b = a + 1; b < 3; ++b) {
      if (D[b] > D[a]) {
        std::swap(D[a], D[b]);
        for (int k = 0; k < 3; ++k) {
          std::swap(A[k][a], A[k][b]);
          std::swap(V[k][a], V[k][b]);
        }
      }
    }
  }
  if (!(D[0] > 0.0) || !std::isfinite(D[0]) || !(D[1] > 1e-12 * D[0])) return false;
  for (int k = 0; k < 3; ++k) {
    U[k][0] = A[k][0] / D[0];
    U[k][1] = A[k][1] / D[1];
  }
  double x[3] = {U[1][0] * U[2][1] - U[2][0] * U[1][1], U[2][0] * U[0][1] - U[0][0] * U[2][1],
                 U[0][0] * U[1][1] - U[1][0] * U[0][1]};
  const double dot = x[0] * A[0][2] + x[1] * A[1][2] + x[2] * A[2][2];
  const double sign = dot < 0.0 ? -1.0 : 1.0;
  for (int k = 0; k < 3; ++k) U[k][2] = sign * x[k];
  return true;
}

// The rotation (row-major) and translation of a placement stated in `coord`, in the stored RUB frame, and back
// (spz_amd_transform_params' conjugation: R = F R_c F, t = F t_c, the quaternion's vector part det(F) F v).
void al_flips(int coord, double f[3], double *det) {
  const uint32_t fp = flip_masks(coord, SPZ_AMD_RUB).p;
  for (int a = 0; a < 3; ++a) f[a] = ((fp >> a) & 1u) ? -1.0 : 1.0;
  *det = f[0] * f[1] * f[2];
}

void al_quat_to_rub(const double q[4], int coord, double R[3][3]) {
  double f[3], det;
  al_flips(coord, f, &det);
  const double norm = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double x = det * f[0] * q[0] / norm, y = det * f[1] * q[1] / norm, z = det * f[2] * q[2] / norm, w = q[3] / norm;
  const double r[3][3] = {{1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w)},
                          {2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w)},
                          {2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)}};
  std::memcpy(R, r, sizeof(r));
}

// The unit quaternion (x, y, z, w), w >= 0, of a rotation in RUB, stated in `coord`.
void al_rub_to_quat(const double R[3][3], int coord, double q[4]) {
  double f[3], det;
  al_flips(coord, f, &det);
  double x, y, z, w;
  const double tr = R[0][0] + R[1][1] + R[2][2];
  if (tr > 0.0) {
    const double s = std::sqrt(tr + 1.0) * 2.0;
    w = 0.25 * s;
    x = (R[2][1] - R[1][2]) / s;
    y = (R[0][2] - R[2][0]) / s;
    z = (R[1][0] - R[0][1]) / s;
  } else if (R[0][0] > R[1][1] && R[0][0] > R[2][2]) {
    const double s = std::sqrt(1.0 + R[0][0] - R[1][1] - R[2][2]) * 2.0;
    w = (R[2][1] - R[1][2]) / s;
    x = 0.25 * s;
    y = (R[0][1] + R[1][0]) / s;
    z = (R[0][2] + R[2][0]) / s;
  } else if (R[1][1] > R[2][2]) {
    const double s = std::sqrt(1.0 + R[1][1] - R[0][0] - R[2][2]) * 2.0;
    w = (R[0][2] - R[2][0]) / s;
    x = (R[0][1] + R[1][0]) / s;
    y = 0.25 * s;
    z = (R[1][2] + R[2][1]) / s;
  } else {
    const double s = std::sqrt(1.0 + R[2][2] - R[0][0] - R[1][1]) * 2.0;
    w = (R[1][0] - R[0][1]) / s;
    x = (R[0][2] + R[2][0]) / s;
    y = (R[1][2] + R[2][1]) / s;
    z = 0.25 * s;
  }
  const double n = std::sqrt(x * x + y * y + z * z + w * w);
  const double sg = w < 0.0 ? -1.0 : 1.0;
  q[0] = sg * det * f[0] * x / n;
  q[1] = sg * det * f[1] * y / n;
  q[2] = sg * det * f[2] * z / n;
  q[3] = sg * w / n;
}

double al_sum_d2(const spz_amd_align_moments *m) {
  const unsigned __int128 v = ((unsigned __int128)m->sum_d2_hi << 64) | m->sum_d2_lo;
  return (double)v;  // rounded once
}

}  // namespace

extern "C" {

int spz_amd_align_default_options(spz_amd_align_options *o) {
  if (o == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  std::memset(o, 0, sizeof(*o));
  o->rotation[3] = 1.0;
  o->scale = 1.0;
  o->coord = SPZ_AMD_UNSPECIFIED;
  o->overlap = 1.0;
  o->stride = 1;
  o->max_iterations = 30;
  o->relative_fitness = 1e-6;
  o->relative_rmse = 1e-6;
  return SPZ_AMD_OK;
}

int spz_amd_align_check(const spz_amd_align_options *o) {
  if (o == nullptr || !valid_coord(o->coord)) return SPZ_AMD_ERR_INVALID_ARG;
  if (o->stride < 1u || al_bad_overlap(o->overlap)) return SPZ_AMD_ERR_INVALID_ARG;
  if (o->has_max_distance && (!std::isfinite(o->max_distance) || !(o->max_distance > 0.0))) return SPZ_AMD_ERR_INVALID_ARG;
  if (o->max_iterations < 1u || o->max_iterations > 1000u) return SPZ_AMD_ERR_INVALID_ARG;
  if (!std::isfinite(o->relative_fitness) || !(o->relative_fitness >= 0.0)) return SPZ_AMD_ERR_INVALID_ARG;
  if (!std::isfinite(o->relative_rmse) || !(o->relative_rmse >= 0.0)) return SPZ_AMD_ERR_INVALID_ARG;
  double n2 = 0.0;
  for (double v : o->rotation) {
    if (!std::isfinite(v)) return SPZ_AMD_ERR_INVALID_ARG;
    n2 += v * v;
  }
  const double norm = std::sqrt(n2);
  if (!(norm > 0.0) || !std::isfinite(norm)) return SPZ_AMD_ERR_INVALID_ARG;
  for (double v : o->translation) {
    if (!std::isfinite(v)) return SPZ_AMD_ERR_INVALID_ARG;
  }
  if (!std::isfinite(o->scale) || !(o->scale > 0.0)) return SPZ_AMD_ERR_INVALID_ARG;
  return SPZ_AMD_OK;
}

uint64_t spz_amd_align_workspace_bytes(uint64_t num_source, uint64_t num_target) {
  return al_layout(num_source, num_target).bytes;
}

int spz_amd_align_prepare_device(const spz_amd_align_cloud *source, const spz_amd_align_cloud *target, void *d_workspace,
                                 void *hip_stream) {
  spz_amd_layout sl, tl;
  int rc = al_check_pair(source, target, &sl, &tl);
  if (rc != SPZ_AMD_OK) return rc;
  if (d_workspace == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  const AlLayout wl = al_layout(source->hdr.num_points, target->hdr.num_points);
  return al_prepare(source, sl, target, tl, align_ws(d_workspace), wl, static_cast<hipStream_t>(hip_stream));
}

int spz_amd_nearest_device(const spz_amd_align_cloud *source, const spz_amd_align_cloud *target, uint32_t stride,
                           const double map[12], uint64_t r2, uint32_t *d_index, uint64_t *d_d2, void *d_workspace,
                           void *hip_stream) {
  spz_amd_layout sl, tl;
  int rc = al_check_pair(source, target, &sl, &tl);
  if (rc != SPZ_AMD_OK) return rc;
  if (stride < 1u || al_bad_map(map) || d_workspace == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  if (source->hdr.num_points && (d_index == nullptr || d_d2 == nullptr)) return SPZ_AMD_ERR_INVALID_ARG;
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  const AlLayout wl = al_layout(source->hdr.num_points, target->hdr.num_points);
  return al_query(source, target, stride, map, r2, d_index, d_d2, align_ws(d_workspace), wl,
                  static_cast<hipStream_t>(hip_stream));
}

int spz_amd_align_step_device(const spz_amd_align_cloud *source, const spz_amd_align_cloud *target, uint32_t stride,
                              const double map[12], uint64_t r2, double overlap, uint32_t *d_index, uint64_t *d_d2,
                              uint8_t *d_inlier, spz_amd_align_moments *d_out, void *d_workspace, void *hip_stream) {
  spz_amd_layout sl, tl;
  int rc = al_check_pair(source, target, &sl, &tl);
  if (rc != SPZ_AMD_OK) return rc;
  if (stride < 1u || al_bad_map(map) || al_bad_overlap(overlap) || d_out == nullptr || d_workspace == nullptr) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const AlLayout wl = al_layout(source->hdr.num_points, target->hdr.num_points);
  uint8_t *ws = align_ws(d_workspace);
  if (d_index == nullptr) d_index = reinterpret_cast<uint32_t *>(ws + wl.index);
  if (d_d2 == nullptr) d_d2 = reinterpret_cast<uint64_t *>(ws + wl.d2);
  if (d_inlier == nullptr) d_inlier = ws + wl.inlier;
  rc = al_query(source, target, stride, map, r2, d_index, d_d2, ws, wl, st);
  if (rc != SPZ_AMD_OK) return rc;
  rc = al_select(source->hdr.num_points, overlap, d_index, d_d2, d_inlier, ws, wl, st);
  if (rc != SPZ_AMD_OK) return rc;
  return al_moments(source, sl, target, &tl, stride, false, d_index, d_d2, d_inlier, d_out, ws, wl, st);
}

int spz_amd_align_solve(const spz_amd_align_moments *m, int estimate_scale, double scale_in, double map_out[12],
                        double *scale_out, int *degenerate) {
  if (m == nullptr || map_out == nullptr || degenerate == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  if (!std::isfinite(scale_in) || !(scale_in > 0.0)) return SPZ_AMD_ERR_INVALID_ARG;
  *degenerate = 1;
  if (m->count < 3) return SPZ_AMD_OK;
  const double K = (double)m->count;
  double ma[3], mb[3];
  for (int k = 0; k < 3; ++k) {
    ma[k] = m->sum_a[k] / K;
    mb[k] = m->sum_b[k] / K;
  }
  const double var_a = m->sum_aa / K - ((ma[0] * ma[0] + ma[1] * ma[1]) + ma[2] * ma[2]);
  if (!(var_a > 0.0) || !std::isfinite(var_a)) return SPZ_AMD_OK;
  double H[3][3], U[3][3], V[3][3], D[3];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) {
      H[i][j] = m->sum_ab[3 * j + i] / K - mb[i] * ma[j];
      if (!std::isfinite(H[i][j])) return SPZ_AMD_OK;
    }
  }
  if (!svd3(H, U, D, V)) return SPZ_AMD_OK;
  const double sgn = det3(U) * det3(V) < 0.0 ? -1.0 : 1.0;
  double R[3][3];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) R[i][j] = (U[i][0] * V[j][0] + U[i][1] * V[j][1]) + sgn * U[i][2] * V[j][2];
  }
  const double s = estimate_scale ? ((D[0] + D[1]) + sgn * D[2]) / var_a : scale_in;
  if (!std::isfinite(s) || !(s > 0.0)) return SPZ_AMD_OK;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) map_out[3 * i + j] = s * R[i][j];
    map_out[9 + i] = mb[i] - s * ((R[i][0] * ma[0] + R[i][1] * ma[1]) + R[i][2] * ma[2]);
  }
  if (scale_out) *scale_out = s;
  *degenerate = 0;
  return SPZ_AMD_OK;
}

int spz_amd_align_host(const spz_amd_align_cloud *source, const spz_amd_align_cloud *target,
                       const spz_amd_align_options *options, int device, spz_amd_align_result *result,
                       spz_amd_align_history *history, uint32_t capacity, float *h_ms) {
  if (result == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  std::memset(result, 0, sizeof(*result));
  int rc = spz_amd_align_check(options);
  if (rc != SPZ_AMD_OK) return rc;
  spz_amd_layout sl, tl;
  rc = al_check_pair(source, target, &sl, &tl);
  if (rc != SPZ_AMD_OK) return rc;
  const spz_amd_align_options &o = *options;
  uint64_t r2 = kAlNoLimit;
  if (o.has_max_distance) {
    rc = spz_amd_clean_radius_r2(o.max_distance, (int)target->hdr.fractional_bits, &r2);
    if (rc != SPZ_AMD_OK) return rc;
  }
  DeviceGuard guard;
  rc = guard.enter(device);
  if (rc != SPZ_AMD_OK) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  PackedResultPtr c;  // the stream and the workspace; there is no output stream
  rc = packed_result_open(device, &c);
  if (rc != SPZ_AMD_OK) return rc;
  const AlLayout wl = al_layout(source->hdr.num_points, target->hdr.num_points);
  SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&c->block), wl.bytes + 256));
  uint8_t *ws = align_ws(c->block);
  auto *d_mom = reinterpret_cast<spz_amd_align_moments *>(c->block + wl.bytes);
  static_assert(sizeof(spz_amd_align_moments) <= 256, "the moments follow the workspace");
  rc = al_prepare(source, sl, target, tl, ws, wl, c->st);
  if (rc != SPZ_AMD_OK) return rc;
  SPZ_HIP_TRY(hipStreamSynchronize(c->st));
  const double prepare_ms = ms_since(t0);
  double query_ms = 0.0;
  // the initial map in the stored frame
  double R[3][3], f[3], det;
  al_quat_to_rub(o.rotation, o.coord, R);
  al_flips(o.coord, f, &det);
  double scale = o.scale, map[12];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) map[3 * i + j] = scale * R[i][j];
    map[9 + i] = f[i] * o.translation[i];
  }
  spz_amd_align_moments mom;
  if (o.init_centroids) {
    double cs[3], ct[3];
    for (int pass = 0; pass < 2; ++pass) {
      rc = al_moments(pass ? target : source, pass ? tl : sl, nullptr, nullptr, pass ? 1u : o.stride, true, nullptr,
                      nullptr, nullptr, d_mom, ws, wl, c->st);
      if (rc != SPZ_AMD_OK) return rc;
      SPZ_HIP_TRY(hipMemcpyAsync(&mom, d_mom, sizeof(mom), hipMemcpyDeviceToHost, c->st));
      SPZ_HIP_TRY(hipStreamSynchronize(c->st));
      for (int k = 0; k < 3; ++k) (pass ? ct : cs)[k] = mom.count ? mom.sum_a[k] / (double)mom.count : 0.0;
    }
    for (int i = 0; i < 3; ++i) map[9 + i] = ct[i] - ((map[3 * i] * cs[0] + map[3 * i + 1] * cs[1]) + map[3 * i + 2] * cs[2]);
  }
  uint32_t *d_index = reinterpret_cast<uint32_t *>(ws + wl.index);
  uint64_t *d_d2 = reinterpret_cast<uint64_t *>(ws + wl.d2);
  uint8_t *d_inlier = ws + wl.inlier;
  const double quantum = std::ldexp(1.0, -(int)target->hdr.fractional_bits);
  double prev_fitness = 0.0, prev_rmse = 0.0;
  for (uint32_t it = 0; it < o.max_iterations; ++it) {
    const auto tq = std::chrono::steady_clock::now();
    rc = al_query(source, target, o.stride, map, r2, d_index, d_d2, ws, wl, c->st);
    if (rc != SPZ_AMD_OK) return rc;
    SPZ_HIP_TRY(hipStreamSynchronize(c->st));
    query_ms += ms_since(tq);
    rc = al_select(source->hdr.num_points, o.overlap, d_index, d_d2, d_inlier, ws, wl, c->st);
    if (rc != SPZ_AMD_OK) return rc;
    rc = al_moments(source, sl, target, &tl, o.stride, false, d_index, d_d2, d_inlier, d_mom, ws, wl, c->st);
    if (rc != SPZ_AMD_OK) return rc;
    SPZ_HIP_TRY(hipMemcpyAsync(&mom, d_mom, sizeof(mom), hipMemcpyDeviceToHost, c->st));
    SPZ_HIP_TRY(hipStreamSynchronize(c->st));
    const double fitness = mom.taking_part ? (double)mom.count / (double)mom.taking_part : 0.0;
    const double rmse = mom.count ? std::sqrt(al_sum_d2(&mom) / (double)mom.count) * quantum : 0.0;
    if (history && it < capacity) {
      history[it].fitness = fitness;
      history[it].inlier_rmse = rmse;
      history[it].inliers = mom.count;
    }
    std::memcpy(result->map, map, sizeof(map));
    result->scale = scale;
    result->fitness = fitness;
    result->inlier_rmse = rmse;
    result->inliers = mom.count;
    result->iterations = it + 1u;
    if (it > 0 && std::fabs(fitness - prev_fitness) <= o.relative_fitness * std::fmax(fitness, prev_fitness) &&
        std::fabs(rmse - prev_rmse) <= o.relative_rmse * std::fmax(rmse, prev_rmse)) {
      result->converged = 1;
      break;
    }
    prev_fitness = fitness;
    prev_rmse = rmse;
    if (it + 1u == o.max_iterations) break;
    double next[12], next_scale = scale;
    int degenerate = 0;
    rc = spz_amd_align_solve(&mom, o.estimate_scale, scale, next, &next_scale, &degenerate);
    if (rc != SPZ_AMD_OK) return rc;
    if (degenerate) {
      result->degenerate = 1;
      break;
    }
    std::memcpy(map, next, sizeof(map));
    scale = next_scale;
  }
  // the reported map, stated in the caller's frame
  double Rr[3][3];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) Rr[i][j] = result->map[3 * i + j] / result->scale;
    result->translation[i] = f[i] * result->map[9 + i];
  }
  al_rub_to_quat(Rr, o.coord, result->rotation);
  if (h_ms) {
    h_ms[0] = (float)prepare_ms;
    h_ms[1] = (float)query_ms;
    h_ms[2] = (float)(ms_since(t0) - prepare_ms - query_ms);
  }
  return SPZ_AMD_OK;
}

}  // extern "C"
