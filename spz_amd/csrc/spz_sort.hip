// spz_sort.hip — point order for a packed stream (DESIGN §8 "sort"): a stable device argsort, the Morton key of the
// stored positions, and the per-chunk bounds a renderer reads from a sorted file.  The stream stays in HBM; the reorder
// itself is spz_subset_kernel (spz_filter.hip), so nothing is requantised.
//
//   spz_morton_key_kernel     one pass over the 9-byte position records: u_a = field ^ 0x800000 per axis, key bit
//                             3b + a = bit b of u_a (72 bits), written as three u32 planes (bits 0..31, 32..63, 64..71).
//   spz_float_key_kernel      f32 -> an order-preserving u32 (-0 = +0, every NaN 0xffffffff: last in both directions).
//   spz_radix_hist_kernel     per tile of kSortTile points, the histogram of one 8-bit digit, written digit-major.
//   spz_radix_scan_kernel     one workgroup per digit: exclusive scan of that digit's tile counts, and the row total.
//   spz_radix_scatter_kernel  stable in-tile rank (wave64 __ballot match masks + a prefix over (round, wave) in LDS),
//                             the tile staged in LDS in digit order, then each digit's run written contiguously at
//                             digit base + tile offset.  Reduce-then-scan: no inter-workgroup flags, no global atomics.
//   spz_morton_gather_kernel  the positions in an order: sorted (u_x, u_y, u_z, input index), 16 B per point, for the
//                             neighbour searches (spz_morton_walk.hpp).
//   spz_chunk_bounds_kernel   one wave per run of `chunk` points: min / max of the sign-extended stored integers.
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

namespace spz_amd_detail {
namespace {

constexpr uint32_t kSortBlock = kOpsBlock;                // 256
constexpr uint32_t kSortWaves = kSortBlock / 64u;
constexpr uint32_t kSortItems = 8;                        // points per thread and tile
constexpr uint32_t kSortTile = kSortBlock * kSortItems;   // 2048 points per tile
constexpr uint32_t kRadix = 256;                          // 8-bit digits
constexpr uint32_t kMortonDigits = 9;                     // 72-bit Morton key
constexpr uint32_t kFloatDigits = 4;
constexpr uint32_t kBoundsBlock = 256;                    // 4 chunks (one per wave) per workgroup

struct PassParams {
  const uint32_t *key_in[3];
  uint32_t *key_out[3];
  const uint32_t *idx_in;       // nullptr: the identity (first pass)
  uint32_t *idx_out;
  const uint32_t *counts;       // [kRadix][tiles], each row scanned (exclusive)
  const uint32_t *totals;       // [kRadix] row totals
  uint32_t n, tiles;
  uint32_t plane, shift;        // digit = (key_in[plane][i] >> shift) & 255
  uint32_t carry;               // bit w: plane w moves with the point (a later pass reads it)
};

// Lanes of this wave whose (valid) digit equals this lane's: eight ballots, one per digit bit.
__device__ __forceinline__ unsigned long long match_digit(uint32_t d, bool valid) {
  unsigned long long m = __ballot(valid);
#pragma unroll
  for (uint32_t b = 0; b < 8; ++b) {
    const bool bit = (d >> b) & 1u;
    const unsigned long long t = __ballot(bit);
    m &= bit ? t : ~t;
  }
  return m;
}

// bits 0..20 of x -> bits 0, 3, 6, ..., 60
__device__ __forceinline__ unsigned long long spread3_21(unsigned long long x) {
  x &= 0x1fffffull;
  x = (x | x << 32) & 0x1f00000000ffffull;
  x = (x | x << 16) & 0x1f0000ff0000ffull;
  x = (x | x << 8) & 0x100f00f00f00f00full;
  x = (x | x << 4) & 0x10c30c30c30c30c3ull;
  x = (x | x << 2) & 0x1249249249249249ull;
  return x;
}

}  // namespace

__global__ __launch_bounds__(kSortBlock) void spz_morton_key_kernel(const uint8_t *positions, uint32_t n,
                                                                    uint32_t complement, uint32_t *k0, uint32_t *k1,
                                                                    uint32_t *k2) {
  const uint32_t i = blockIdx.x * kSortBlock + threadIdx.x;
  if (i >= n) return;
  const uint8_t *b = positions + (unsigned long long)i * 9u;
  uint32_t u[3];
#pragma unroll
  for (uint32_t a = 0; a < 3; ++a) {
    u[a] = ((uint32_t)b[3 * a] | ((uint32_t)b[3 * a + 1] << 8) | ((uint32_t)b[3 * a + 2] << 16)) ^ 0x800000u;
  }
  // bits 0..20 of every axis -> key bits 0..62; bits 21..23 -> key bits 63..71
  unsigned long long lo = spread3_21(u[0]) | (spread3_21(u[1]) << 1) | (spread3_21(u[2]) << 2);
  uint32_t h = 0;
#pragma unroll
  for (uint32_t a = 0; a < 3; ++a) {
    const uint32_t t = u[a] >> 21;
    h |= ((t & 1u) | ((t & 2u) << 2) | ((t & 4u) << 4)) << a;
  }
  lo |= (unsigned long long)(h & 1u) << 63;
  uint32_t w0 = (uint32_t)lo, w1 = (uint32_t)(lo >> 32), w2 = h >> 1;
  if (complement) {
    w0 = ~w0;
    w1 = ~w1;
    w2 = ~w2 & 0xffu;
  }
  k0[i] = w0;
  k1[i] = w1;
  k2[i] = w2;
}

__global__ __launch_bounds__(kSortBlock) void spz_morton_gather_kernel(const uint8_t *pos, const uint32_t *order,
                                                                       uint32_t n, uint4 *pts) {
  const unsigned long long i = (unsigned long long)blockIdx.x * kSortBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t s = order[i];
  pts[i] = make_uint4(load_u(pos, s, 0), load_u(pos, s, 1), load_u(pos, s, 2), s);
}

__global__ __launch_bounds__(kSortBlock) void spz_float_key_kernel(const float *keys, uint32_t n, uint32_t descending,
                                                                   uint32_t *k0) {
  const uint32_t i = blockIdx.x * kSortBlock + threadIdx.x;
  if (i >= n) return;
  uint32_t v = __float_as_uint(keys[i]);
  uint32_t code;
  if ((v & 0x7fffffffu) > 0x7f800000u) {
    code = 0xffffffffu;  // NaN: after every number, ascending or descending
  } else {
    if (v == 0x80000000u) v = 0u;  // -0 == +0
    code = (v & 0x80000000u) ? ~v : (v | 0x80000000u);
    if (descending) code = ~code;  // the largest code of a number stays below the NaNs'
  }
  k0[i] = code;
}

__global__ __launch_bounds__(kSortBlock) void spz_radix_hist_kernel(const uint32_t *keys, uint32_t n, uint32_t shift,
                                                                    uint32_t tiles, uint32_t *counts) {
  __shared__ uint32_t h[kRadix];
  const uint32_t tile = blockIdx.x, lane = threadIdx.x & 63u;
  h[threadIdx.x] = 0;
  __syncthreads();
  uint32_t d[kSortItems];
  bool valid[kSortItems];
#pragma unroll
  for (uint32_t r = 0; r < kSortItems; ++r) {
    const uint32_t i = tile * kSortTile + r * kSortBlock + threadIdx.x;
    valid[r] = i < n;
    d[r] = valid[r] ? (keys[i] >> shift) & 0xffu : 0u;
  }
#pragma unroll
  for (uint32_t r = 0; r < kSortItems; ++r) {
    const unsigned long long m = match_digit(d[r], valid[r]);
    // one LDS add per distinct digit of the wave, by its lowest lane (the counts commute: no order reaches the output)
    if (valid[r] && (m & ((1ull << lane) - 1ull)) == 0ull) atomicAdd(&h[d[r]], (uint32_t)__popcll(m));
  }
  __syncthreads();
  counts[(unsigned long long)threadIdx.x * tiles + tile] = h[threadIdx.x];
}

// Row blockIdx.x of counts ([kRadix][tiles]) -> exclusive prefix sums in place; totals[row] = the row's sum.  Thread t
// owns a contiguous run of ceil(tiles / 256) counts.
__global__ __launch_bounds__(kSortBlock) void spz_radix_scan_kernel(uint32_t *counts, uint32_t tiles, uint32_t *totals) {
  __shared__ uint32_t s[kSortBlock];
  uint32_t *row = counts + (unsigned long long)blockIdx.x * tiles;
  const uint32_t sum = block_scan_owned_runs(
      tiles, s, [&](uint32_t k) { return row[k]; }, [&](uint32_t k, uint32_t before) { row[k] = before; });
  if (threadIdx.x == 0) totals[blockIdx.x] = sum;
}

__global__ __launch_bounds__(kSortBlock) void spz_radix_scatter_kernel(const PassParams p) {
  // The per-(round, wave, digit) counts and, once the ranks are in registers, the tile staged in sorted order
  // (slot 0: index, 1 + w: key plane w) share these 32 KiB.
  __shared__ uint32_t s_mem[kSortItems * kSortWaves * kRadix];
  __shared__ uint8_t s_digit[kSortTile];
  __shared__ uint32_t s_start[kRadix], s_gbase[kRadix];
  static_assert(kSortItems * kSortWaves * kRadix == 4 * kSortTile, "the staging aliases the counts exactly");
  uint32_t(*s_cnt)[kSortWaves][kRadix] = reinterpret_cast<uint32_t(*)[kSortWaves][kRadix]>(s_mem);
  uint32_t(*s_stage)[kSortTile] = reinterpret_cast<uint32_t(*)[kSortTile]>(s_mem);

  const uint32_t tile = blockIdx.x, t = threadIdx.x;
  const uint32_t lane = t & 63u, wave = t >> 6;
  const uint32_t first = tile * kSortTile;
  const uint32_t tile_n = (p.n - first) < kSortTile ? p.n - first : kSortTile;

  // this tile's global start of every digit: the digit's base (scan of the row totals) + the tile's row offset
  const uint32_t base = block_exclusive_scan(p.totals[t], s_gbase);
  s_gbase[t] = base + p.counts[(unsigned long long)t * p.tiles + tile];
#pragma unroll
  for (uint32_t k = 0; k < kSortItems * kSortWaves; ++k) s_mem[k * kSortBlock + t] = 0u;

  uint32_t v[4][kSortItems];  // slot 0: index, 1 + w: key plane w (when carried)
  uint32_t d[kSortItems];
  bool valid[kSortItems];
#pragma unroll
  for (uint32_t r = 0; r < kSortItems; ++r) {
    const uint32_t i = first + r * kSortBlock + t;
    valid[r] = i < p.n;
    const uint32_t j = valid[r] ? i : first;
    d[r] = (p.key_in[p.plane][j] >> p.shift) & 0xffu;
    v[0][r] = p.idx_in ? p.idx_in[j] : j;
#pragma unroll
    for (uint32_t w = 0; w < 3; ++w) v[1 + w][r] = ((p.carry >> w) & 1u) ? p.key_in[w][j] : 0u;
  }
  __syncthreads();  // s_cnt zeroed

  uint32_t rank[kSortItems];
#pragma unroll
  for (uint32_t r = 0; r < kSortItems; ++r) {
    const unsigned long long m = match_digit(d[r], valid[r]);
    rank[r] = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (valid[r] && rank[r] == 0u) s_cnt[r][wave][d[r]] = (uint32_t)__popcll(m);
  }
  __syncthreads();
  // thread t = digit t: (round, wave) counts -> exclusive prefixes in point order; the digit's tile total
  uint32_t run = 0;
#pragma unroll
  for (uint32_t r = 0; r < kSortItems; ++r) {
#pragma unroll
    for (uint32_t w = 0; w < kSortWaves; ++w) {
      const uint32_t c = s_cnt[r][w][t];
      s_cnt[r][w][t] = run;
      run += c;
    }
  }
  const uint32_t start = block_exclusive_scan(run, s_start);  // also orders the writes above before the reads below
  s_start[t] = start;
  s_gbase[t] -= start;  // global position = s_gbase[digit] + position in the staged tile
#pragma unroll
  for (uint32_t r = 0; r < kSortItems; ++r) rank[r] += s_cnt[r][wave][d[r]];
  __syncthreads();  // every rank read before the staging overwrites the counts
#pragma unroll
  for (uint32_t r = 0; r < kSortItems; ++r) {
    if (!valid[r]) continue;
    const uint32_t pos = s_start[d[r]] + rank[r];
    if (pos >= kSortTile) continue;  // cannot happen with consistent counts
    s_digit[pos] = (uint8_t)d[r];
    s_stage[0][pos] = v[0][r];
#pragma unroll
    for (uint32_t w = 0; w < 3; ++w) {
      if ((p.carry >> w) & 1u) s_stage[1 + w][pos] = v[1 + w][r];
    }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t r = 0; r < kSortItems; ++r) {
    const uint32_t j = r * kSortBlock + t;
    if (j >= tile_n) break;
    const uint32_t g = s_gbase[s_digit[j]] + j;
    if (g >= p.n) continue;  // cannot happen with consistent counts; never write past the buffers
    p.idx_out[g] = s_stage[0][j];
#pragma unroll
    for (uint32_t w = 0; w < 3; ++w) {
      if ((p.carry >> w) & 1u) p.key_out[w][g] = s_stage[1 + w][j];
    }
  }
}

__global__ __launch_bounds__(kBoundsBlock) void spz_chunk_bounds_kernel(const uint8_t *positions, uint32_t n,
                                                                       uint32_t chunk, uint32_t chunks, float scale,
                                                                       float *bounds) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t c = blockIdx.x * (kBoundsBlock / 64u) + (threadIdx.x >> 6);
  if (c >= chunks) return;  // a whole wave: no block-level synchronisation below
  const unsigned long long begin = (unsigned long long)c * chunk;
  const unsigned long long end = (n - begin) < chunk ? (unsigned long long)n : begin + chunk;
  int32_t lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
  for (unsigned long long i = begin + lane; i < end; i += 64u) {
    const uint8_t *b = positions + i * 9u;
#pragma unroll
    for (uint32_t a = 0; a < 3; ++a) {
      const uint32_t u = (uint32_t)b[3 * a] | ((uint32_t)b[3 * a + 1] << 8) | ((uint32_t)b[3 * a + 2] << 16);
      const int32_t s = (int32_t)(u << 8) >> 8;
      lo[a] = s < lo[a] ? s : lo[a];
      hi[a] = s > hi[a] ? s : hi[a];
    }
  }
#pragma unroll
  for (uint32_t off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (uint32_t a = 0; a < 3; ++a) {
      const int32_t l = __shfl_xor(lo[a], (int)off), h = __shfl_xor(hi[a], (int)off);
      lo[a] = l < lo[a] ? l : lo[a];
      hi[a] = h > hi[a] ? h : hi[a];
    }
  }
  if (lane < 3) {
    bounds[(unsigned long long)c * 6u + lane] = (float)lo[lane] * scale;
    bounds[(unsigned long long)c * 6u + 3u + lane] = (float)hi[lane] * scale;
  }
}

// The workspace of one sort of n keys, and the digit passes over it (spz_sort_internal.hpp).
SortLayout sort_layout(uint64_t n) {
  SortLayout w;
  w.tiles = (n + kSortTile - 1) / kSortTile;
  const uint64_t plane = Workspace::aligned(n * 4u);
  uint64_t off = 0;
  w.idx_off = off;
  off += plane;
  for (int s = 0; s < 2; ++s) {
    for (int k = 0; k < 3; ++k) {
      w.planes_off[s][k] = off;
      off += plane;
    }
  }
  w.counts_off = off;
  off += Workspace::aligned(w.tiles * kRadix * 4u);
  w.totals_off = off;
  off += Workspace::aligned(kRadix * 4u);
  w.bytes = off + 256;  // room to align a caller's pointer up to 256
  return w;
}

int radix_passes(uint32_t n, uint32_t digits, uint32_t *d_order, uint8_t *ws, const SortLayout &wl, hipStream_t st) {
  uint32_t *planes[2][3];
  for (int s = 0; s < 2; ++s) {
    for (int k = 0; k < 3; ++k) planes[s][k] = reinterpret_cast<uint32_t *>(ws + wl.planes_off[s][k]);
  }
  // pass p writes idx[(p + 1) & 1]: the last one (p = digits - 1) writes the caller's buffer
  uint32_t *idx[2];
  idx[digits & 1u] = d_order;
  idx[(digits + 1u) & 1u] = reinterpret_cast<uint32_t *>(ws + wl.idx_off);
  uint32_t *counts = reinterpret_cast<uint32_t *>(ws + wl.counts_off);
  uint32_t *totals = reinterpret_cast<uint32_t *>(ws + wl.totals_off);
  const uint32_t tiles = (uint32_t)wl.tiles;
  for (uint32_t q = 0; q < digits; ++q) {
    PassParams p = {};
    for (int k = 0; k < 3; ++k) {
      p.key_in[k] = planes[q & 1u][k];
      p.key_out[k] = planes[(q + 1u) & 1u][k];
    }
    p.idx_in = q == 0 ? nullptr : idx[q & 1u];
    p.idx_out = idx[(q + 1u) & 1u];
    p.counts = counts;
    p.totals = totals;
    p.n = n;
    p.tiles = tiles;
    p.plane = q / 4u;
    p.shift = 8u * (q % 4u);
    for (uint32_t w = 0; w < 3; ++w) {
      const uint32_t last_digit_of_w = w * 4u + 3u < digits - 1u ? w * 4u + 3u : digits - 1u;
      if (w * 4u < digits && q < last_digit_of_w) p.carry |= 1u << w;
    }
    hipLaunchKernelGGL(spz_radix_hist_kernel, dim3(tiles), dim3(kSortBlock), 0, st, p.key_in[p.plane], n, p.shift,
                       tiles, counts);
    SPZ_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(spz_radix_scan_kernel, dim3(kRadix), dim3(kSortBlock), 0, st, counts, tiles, totals);
    SPZ_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(spz_radix_scatter_kernel, dim3(tiles), dim3(kSortBlock), 0, st, p);
    SPZ_HIP_TRY(hipGetLastError());
  }
  return SPZ_AMD_OK;
}

}  // namespace spz_amd_detail

namespace {

using namespace spz_amd_detail;

int morton_impl(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, int descending, uint32_t *d_order,
                void *d_workspace, hipStream_t st) {
  spz_amd_layout lay;
  int rc = check_packed_stream(d_stream, size, hdr, &lay);
  if (rc != SPZ_AMD_OK) return rc;
  if (hdr->version == 1) return SPZ_AMD_ERR_UNSUPPORTED;  // float16 positions: no stored integers
  const uint64_t n = hdr->num_points;
  if (n == 0) return SPZ_AMD_OK;
  if (n > 0x7fffffffull || d_order == nullptr || d_workspace == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  const SortLayout wl = sort_layout(n);
  uint8_t *ws = align_ws(d_workspace);
  uint32_t *k[3];
  for (int j = 0; j < 3; ++j) k[j] = reinterpret_cast<uint32_t *>(ws + wl.planes_off[0][j]);
  const uint32_t blocks = (uint32_t)((n + kSortBlock - 1) / kSortBlock);
  hipLaunchKernelGGL(spz_morton_key_kernel, dim3(blocks), dim3(kSortBlock), 0, st,
                     d_stream + lay.offset[SPZ_AMD_SEC_POSITIONS], (uint32_t)n, descending ? 1u : 0u, k[0], k[1], k[2]);
  SPZ_HIP_TRY(hipGetLastError());
  return radix_passes((uint32_t)n, kMortonDigits, d_order, ws, wl, st);
}

int argsort_impl(const float *d_keys, uint64_t n, int descending, uint32_t *d_order, void *d_workspace,
                 hipStream_t st) {
  if (n > 0x7fffffffull) return SPZ_AMD_ERR_INVALID_ARG;
  if (n == 0) return SPZ_AMD_OK;
  if (d_keys == nullptr || d_order == nullptr || d_workspace == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  int device = 0;
  int rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  const SortLayout wl = sort_layout(n);
  uint8_t *ws = align_ws(d_workspace);
  const uint32_t blocks = (uint32_t)((n + kSortBlock - 1) / kSortBlock);
  hipLaunchKernelGGL(spz_float_key_kernel, dim3(blocks), dim3(kSortBlock), 0, st, d_keys, (uint32_t)n,
                     descending ? 1u : 0u, reinterpret_cast<uint32_t *>(ws + wl.planes_off[0][0]));
  SPZ_HIP_TRY(hipGetLastError());
  return radix_passes((uint32_t)n, kFloatDigits, d_order, ws, wl, st);
}

}  // namespace

namespace spz_amd_detail {

int morton_sorted_points(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, const spz_amd_layout &lay,
                         uint32_t *d_order, uint4 *d_pts, void *d_sort_ws, hipStream_t st) {
  const uint32_t n = hdr->num_points;
  if (n == 0) return SPZ_AMD_OK;
  const int rc = morton_impl(d_stream, size, hdr, 0, d_order, d_sort_ws, st);
  if (rc != SPZ_AMD_OK) return rc;
  hipLaunchKernelGGL(spz_morton_gather_kernel, dim3((n + kSortBlock - 1) / kSortBlock), dim3(kSortBlock), 0, st,
                     d_stream + lay.offset[SPZ_AMD_SEC_POSITIONS], d_order, n, d_pts);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

}  // namespace spz_amd_detail

extern "C" {

uint64_t spz_amd_sort_workspace_bytes(uint64_t n) { return sort_layout(n).bytes; }

int spz_amd_morton_order_device(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, int descending,
                                uint32_t *d_order, void *d_workspace, void *hip_stream) {
  return morton_impl(d_stream, size, hdr, descending, d_order, d_workspace, static_cast<hipStream_t>(hip_stream));
}

int spz_amd_argsort_f32_device(const float *d_keys, uint64_t n, int descending, uint32_t *d_order, void *d_workspace,
                               void *hip_stream) {
  return argsort_impl(d_keys, n, descending, d_order, d_workspace, static_cast<hipStream_t>(hip_stream));
}

int spz_amd_chunk_bounds_device(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, uint32_t chunk,
                                float *d_bounds, void *hip_stream) {
  spz_amd_layout lay;
  int rc = check_packed_stream(d_stream, size, hdr, &lay);
  if (rc != SPZ_AMD_OK) return rc;
  if (hdr->version == 1) return SPZ_AMD_ERR_UNSUPPORTED;
  if (chunk == 0) return SPZ_AMD_ERR_INVALID_ARG;
  const uint64_t n = hdr->num_points;
  if (n == 0) return SPZ_AMD_OK;
  if (d_bounds == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  const uint64_t chunks = (n + chunk - 1) / chunk;
  const uint64_t blocks = (chunks + kBoundsBlock / 64u - 1) / (kBoundsBlock / 64u);
  // int * 2^-fractionalBits: exact in f32 for the 24-bit integers
  const float scale = (float)std::ldexp(1.0, -(int)hdr->fractional_bits);
  hipLaunchKernelGGL(spz_chunk_bounds_kernel, dim3((unsigned)blocks), dim3(kBoundsBlock), 0,
                     static_cast<hipStream_t>(hip_stream), d_stream + lay.offset[SPZ_AMD_SEC_POSITIONS], (uint32_t)n,
                     chunk, (uint32_t)chunks, scale, d_bounds);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

int spz_amd_sort_open(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, const float *h_keys,
                      int descending, int device, void **ctx, uint64_t *h_out_bytes, uint32_t *h_order, float *h_ms) {
  if (ctx == nullptr || h_out_bytes == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  *ctx = nullptr;
  *h_out_bytes = 0;
  spz_amd_layout in;
  int rc = check_packed_stream(d_stream, size, hdr, &in);
  if (rc != SPZ_AMD_OK) return rc;
  if (h_keys == nullptr && hdr->version == 1) return SPZ_AMD_ERR_UNSUPPORTED;
  const uint64_t n = hdr->num_points;
  if (n > SPZ_AMD_REFERENCE_MAX_POINTS) return SPZ_AMD_ERR_TOO_MANY_POINTS;
  DeviceGuard guard;
  rc = guard.enter(device);
  if (rc != SPZ_AMD_OK) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  PackedResultPtr c;
  rc = packed_result_open(device, &c);
  if (rc != SPZ_AMD_OK) return rc;
  const uint64_t key_bytes = h_keys ? Workspace::aligned(n * 4u) : 0;
  const uint64_t ws_bytes = Workspace::aligned(sort_layout(n).bytes);
  const size_t total = key_bytes + Workspace::aligned(n * 4u) + ws_bytes + Workspace::aligned(in.total_bytes);
  SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&c->block), total));
  uint8_t *q = c->block;
  float *d_keys = reinterpret_cast<float *>(q);
  q += key_bytes;
  uint32_t *d_order = reinterpret_cast<uint32_t *>(q);
  q += Workspace::aligned(n * 4u);
  void *d_ws = q;
  q += ws_bytes;
  c->out = q;
  if (h_keys) {
    if (n) SPZ_HIP_TRY(hipMemcpyAsync(d_keys, h_keys, n * 4u, hipMemcpyHostToDevice, c->st));
    rc = argsort_impl(d_keys, n, descending, d_order, d_ws, c->st);
  } else {
    rc = morton_impl(d_stream, size, hdr, descending, d_order, d_ws, c->st);
  }
  if (rc != SPZ_AMD_OK) return rc;
  SPZ_HIP_TRY(hipStreamSynchronize(c->st));
  const double order_ms = ms_since(t0);
  rc = spz_amd_subset_device(d_stream, size, hdr, d_order, n, -1, c->out, in.total_bytes, c->st);
  if (rc != SPZ_AMD_OK) return rc;
  if (h_order != nullptr && n) SPZ_HIP_TRY(hipMemcpyAsync(h_order, d_order, n * 4u, hipMemcpyDeviceToHost, c->st));
  SPZ_HIP_TRY(hipStreamSynchronize(c->st));
  if (h_ms) {
    h_ms[0] = (float)order_ms;
    h_ms[1] = (float)(ms_since(t0) - order_ms);
  }
  c->out_bytes = in.total_bytes;
  *h_out_bytes = in.total_bytes;
  *ctx = c.release();
  return SPZ_AMD_OK;
}

int spz_amd_sort_fetch(void *ctx, uint8_t *h_out) { return packed_result_fetch(ctx, h_out); }

const uint8_t *spz_amd_sort_device_data(void *ctx) { return packed_result_device_data(ctx); }

void spz_amd_sort_close(void *ctx) { packed_result_close(ctx); }

}  // extern "C"
