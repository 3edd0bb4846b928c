// spz_tile.hip — an octree of LOD tiles over a packed stream (DESIGN §8 "Tile"; the contract is in spz_amd.h, "tile").
// The input is put in Morton order (spz_amd_morton_order_device + spz_amd_subset_device, as the decimate does), so every
// octree cell at every level is a contiguous range of the sorted points and the whole tree is a function of one byte per
// point: dd[i] = the smallest level at which points i - 1 and i share a cell (0: the same position; dd[0] = 0).
//
//   spz_tile_dd_kernel          dd from the sorted positions.
//   spz_tile_pyramid_kernel     maxima of dd over runs of 64, 64^2, ...: "the next / previous i with dd[i] > L" in
//                               O(64 log_64 n) byte reads, which is all the tree build asks of the data.
//   spz_tile_enum_kernel        per sorted point s: the levels of the tiles that start at s, as a bit mask.  The nodes
//                               that start at s are (L, s) for L < dd[s]; the topmost is reached iff its parent cell holds
//                               more than cap points, and the descent stops at the first leaf, so most points cost two
//                               searches and the rest cost one per emitted tile.
//   spz_tile_scan_*             exclusive scan of the masks' bit counts: the pre-order id of every tile.
//   spz_tile_write_kernel       the table rows: level, cell, range, parent (the nearest emitted ancestor), first child.
//   spz_tile_hist_kernel /      per run of 1024 points the histogram of dd, and its prefix over the runs: the number of
//   spz_tile_hist_prefix_kernel occupied level-l cells of any range from two rows and two partial runs.
//   spz_tile_level_kernel       one workgroup per tile: cells_l(node) for all l, content_level, the index range of the
//                               content in its source, child counts (integer atomics).
//   spz_tile_offsets_kernel     one workgroup: every tile's byte offset in the arena.
//   spz_tile_worklist_kernel    one workgroup: the (tile, chunk of 1024 points) work items of one source stream.
//   spz_tile_bounds_kernel      per work item: min / max of the stored integers and the largest scale byte (integer
//                               atomics); spz_tile_bounds_finish_kernel turns them into floats.
//   spz_tile_emit_kernel        per work item: header + the six sections' byte ranges copied into the arena, 16 bytes
//                               per thread and step with byte heads and tails.  One launch per source stream.
// No float atomics and no inter-workgroup waits: a run repeats its table and bytes.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "spz_amd.h"
#include "spz_block_ops.hpp"
#include "spz_common.hpp"

namespace spz_amd_detail {
namespace {

constexpr uint32_t kBlock = kOpsBlock;  // 256
constexpr uint32_t kScanItems = 8;
constexpr uint32_t kScanTile = kBlock * kScanItems;   // positions per workgroup of the id scan
constexpr uint32_t kHistRun = 1024;                   // positions per row of the dd histogram
constexpr uint32_t kLevels = 25;                      // L = 0..24
constexpr uint32_t kChunk = 1024;                     // content points per work item of the bounds and the emit
constexpr uint32_t kPyrMax = 6;                       // 64^6 > 2^31
constexpr uint32_t kMagic = 0x5053474eu;              // load-spz.cc:132
constexpr uint32_t kNanBits = 0x7fc00000u;

struct Pyramid {
  const uint8_t *a[kPyrMax];   // a[0] = dd
  uint32_t size[kPyrMax];
  uint32_t levels;
};

struct __attribute__((packed, aligned(1))) U4a1 { uint32_t x, y, z, w; };

__device__ __forceinline__ void load_u(const uint8_t *pos, unsigned long long i, uint32_t u[3]) {
  const uint8_t *b = pos + i * 9ull;
#pragma unroll
  for (uint32_t a = 0; a < 3; ++a) {
    u[a] = ((uint32_t)b[3 * a] | ((uint32_t)b[3 * a + 1] << 8) | ((uint32_t)b[3 * a + 2] << 16)) ^ 0x800000u;
  }
}

// The smallest j > s with dd[j] > L, or n.
__device__ uint32_t next_greater(const Pyramid &p, uint32_t n, uint32_t s, uint32_t L) {
  uint32_t j = s + 1u, lvl = 0;
  for (;;) {
    const uint32_t size = p.size[lvl];
    if (j >= size) return n;
    uint32_t end = ((j >> 6) + 1u) << 6;
    if (end > size) end = size;
    const uint8_t *a = p.a[lvl];
    bool found = false;
    for (; j < end; ++j) {
      if (a[j] > L) {
        found = true;
        break;
      }
    }
    if (found) break;
    if (j >= size || lvl + 1u >= p.levels) return n;
    j >>= 6;  // j is a multiple of 64: the next run one level up
    ++lvl;
  }
  while (lvl > 0) {
    --lvl;
    j <<= 6;
    const uint8_t *a = p.a[lvl];
    while (a[j] <= L) ++j;  // the run's maximum is > L: ends inside the run
  }
  return j;
}

// The largest j < s with dd[j] > L, or 0 (dd[0] = 0 is never greater: position 0 bounds every level).
__device__ uint32_t prev_greater(const Pyramid &p, uint32_t s, uint32_t L) {
  if (s == 0) return 0;
  int64_t j = (int64_t)s - 1;
  uint32_t lvl = 0;
  for (;;) {
    const int64_t begin = (j >> 6) << 6;
    const uint8_t *a = p.a[lvl];
    bool found = false;
    for (; j >= begin; --j) {
      if (a[j] > L) {
        found = true;
        break;
      }
    }
    if (found) break;
    if (j < 0 || lvl + 1u >= p.levels) return 0;
    j >>= 6;  // j = begin - 1: the previous run one level up
    ++lvl;
  }
  while (lvl > 0) {
    --lvl;
    j = (j << 6) + 63;
    const uint8_t *a = p.a[lvl];
    if (j >= (int64_t)p.size[lvl]) j = (int64_t)p.size[lvl] - 1;
    while (a[j] <= L) --j;
  }
  return (uint32_t)j;
}

// The root's level: the largest dd (the top of the pyramid has at most 64 entries).
__device__ __forceinline__ uint32_t root_level(const Pyramid &p) {
  const uint32_t t = p.levels - 1u;
  uint32_t m = 0;
  for (uint32_t k = 0; k < p.size[t]; ++k) m = p.a[t][k] > m ? p.a[t][k] : m;
  return m;
}

// Per-point bytes of the six sections of a stream of `version` with dim sh coefficients per channel.
__device__ __host__ __forceinline__ void section_bytes(uint32_t version, uint32_t dim, uint32_t bpp[6]) {
  bpp[0] = 9;
  bpp[1] = 1;
  bpp[2] = 3;
  bpp[3] = 3;
  bpp[4] = version >= 3u ? 4u : 3u;
  bpp[5] = 3u * dim;
}

__device__ __host__ __forceinline__ uint32_t point_bytes(uint32_t version, uint32_t dim) {
  return 16u + (version >= 3u ? 4u : 3u) + 3u * dim;
}

__device__ __host__ __forceinline__ uint32_t dim_of_degree(uint32_t d) { return d == 0 ? 0u : d == 1 ? 3u : d == 2 ? 8u : 15u; }

// The rows a kernel may touch: `count`, or with a summary (the count still on the device) its tile count, 0 when the
// tree did not fit.
__device__ __forceinline__ uint32_t rows_of(const spz_amd_tile_summary *summary, uint32_t count) {
  if (summary == nullptr) return count;
  return summary->ok ? (uint32_t)summary->num_tiles : 0u;
}

struct RadiusTable {
  float r[256];   // 3 exp(scale of byte b), from the host's libm
};

}  // namespace

__global__ __launch_bounds__(kBlock) void spz_tile_dd_kernel(const uint8_t *pos, uint32_t n, uint8_t *dd) {
  const unsigned long long i = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  uint32_t v = 0;
  if (i > 0) {
    uint32_t u[3], w[3];
    load_u(pos, i, u);
    load_u(pos, i - 1ull, w);
    const uint32_t x = (u[0] ^ w[0]) | (u[1] ^ w[1]) | (u[2] ^ w[2]);
    v = x ? 32u - (uint32_t)__clz(x) : 0u;   // msb + 1: the first level that joins the two
  }
  dd[i] = (uint8_t)v;
}

__global__ __launch_bounds__(kBlock) void spz_tile_pyramid_kernel(const uint8_t *src, uint32_t nsrc, uint8_t *dst,
                                                                  uint32_t ndst) {
  const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= ndst) return;
  const uint32_t b = k << 6;
  uint32_t e = b + 64u;
  if (e > nsrc) e = nsrc;
  uint32_t m = 0;
  for (uint32_t j = b; j < e; ++j) m = src[j] > m ? src[j] : m;
  dst[k] = (uint8_t)m;
}

// Bit L of mask[s]: a tile (L, s) is emitted.
__global__ __launch_bounds__(kBlock) void spz_tile_enum_kernel(const Pyramid p, uint32_t n, uint32_t cap, uint32_t *mask) {
  const unsigned long long s64 = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
  if (s64 >= n) return;
  const uint32_t s = (uint32_t)s64;
  const uint32_t lroot = root_level(p);
  const uint32_t v = s == 0 ? lroot + 1u : p.a[0][s];
  uint32_t m = 0;
  if (v > 0) {
    uint32_t L = v - 1u;
    bool reached = L == lroot;
    if (!reached) {  // the parent cell (L + 1) holds more than cap points
      const uint32_t ps = prev_greater(p, s, L + 1u), pe = next_greater(p, n, s, L + 1u);
      reached = pe - ps > cap;
    }
    if (reached) {
      uint32_t e = next_greater(p, n, s, L);
      for (;;) {
        if (e - s <= cap || L == 0) {  // a leaf
          m |= 1u << L;
          break;
        }
        const uint32_t e1 = next_greater(p, n, s, L - 1u);
        if (e1 < e) m |= 1u << L;     // two or more children: an interior tile (else the child takes its place)
        e = e1;
        --L;
      }
    }
  }
  mask[s] = m;
}

__global__ __launch_bounds__(kBlock) void spz_tile_scan_reduce_kernel(const uint32_t *mask, uint32_t n, uint32_t *sums) {
  __shared__ uint32_t sh[kBlock];
  const unsigned long long first = (unsigned long long)blockIdx.x * kScanTile + (unsigned long long)threadIdx.x * kScanItems;
  uint32_t v = 0;
  for (uint32_t r = 0; r < kScanItems; ++r) {
    if (first + r < n) v += (uint32_t)__popc(mask[first + r]);
  }
  const uint32_t e = block_exclusive_scan(v, sh);
  if (threadIdx.x == kBlock - 1u) sums[blockIdx.x] = e + v;
}

// Exclusive scan of the workgroups' sums in place; the tile count and whether it fits.
__global__ __launch_bounds__(kBlock) void spz_tile_scan_sums_kernel(uint32_t *sums, uint32_t count, uint32_t max_tiles,
                                                                    const Pyramid p, spz_amd_tile_summary *summary) {
  __shared__ unsigned long long sh[kBlock];
  const unsigned long long num_tiles = block_scan_owned_runs(
      count, sh, [&](uint32_t k) { return (unsigned long long)sums[k]; },
      [&](uint32_t k, unsigned long long before) { sums[k] = (uint32_t)before; });
  if (threadIdx.x == 0) {
    summary->num_tiles = num_tiles;
    summary->arena_bytes = 0;
    summary->ok = num_tiles <= max_tiles ? 1u : 0u;
    summary->root_level = root_level(p);
  }
}

__global__ __launch_bounds__(kBlock) void spz_tile_scan_apply_kernel(const uint32_t *mask, uint32_t n, const uint32_t *sums,
                                                                     uint32_t *toff) {
  __shared__ uint32_t sh[kBlock];
  const unsigned long long first = (unsigned long long)blockIdx.x * kScanTile + (unsigned long long)threadIdx.x * kScanItems;
  uint32_t v = 0;
  for (uint32_t r = 0; r < kScanItems; ++r) {
    if (first + r < n) v += (uint32_t)__popc(mask[first + r]);
  }
  uint32_t run = sums[blockIdx.x] + block_exclusive_scan(v, sh);
  for (uint32_t r = 0; r < kScanItems; ++r) {
    if (first + r >= n) break;
    toff[first + r] = run;
    run += (uint32_t)__popc(mask[first + r]);
  }
}

__global__ __launch_bounds__(kBlock) void spz_tile_write_kernel(const Pyramid p, const uint8_t *pos, uint32_t n, uint32_t cap,
                                                                const uint32_t *mask, const uint32_t *toff,
                                                                const spz_amd_tile_summary *summary,
                                                                spz_amd_tile_info *table) {
  const unsigned long long s64 = (unsigned long long)blockIdx.x * kBlock + threadIdx.x;
  if (s64 >= n || !summary->ok) return;
  const uint32_t s = (uint32_t)s64;
  uint32_t m = mask[s];
  if (m == 0) return;
  const uint32_t lroot = summary->root_level;
  uint32_t u[3];
  load_u(pos, s, u);
  uint32_t id = toff[s];
  while (m) {
    const uint32_t L = 31u - (uint32_t)__clz(m);   // the larger level first
    m &= ~(1u << L);
    const uint32_t e = next_greater(p, n, s, L);
    // the nearest emitted ancestor
    int32_t parent = -1;
    uint32_t q = s;
    for (uint32_t up = L + 1u; up <= lroot; ++up) {
      const uint32_t dq = q == 0 ? kLevels : p.a[0][q];
      if (dq <= up) q = prev_greater(p, q, up);   // the start of the level-`up` cell around q
      const uint32_t mq = mask[q];
      if ((mq >> up) & 1u) {
        parent = (int32_t)(toff[q] + (uint32_t)__popc(up >= 31u ? 0u : mq >> (up + 1u)));
        break;
      }
    }
    const bool leaf = e - s <= cap || L == 0;
    spz_amd_tile_info r;
    r.id = id;
    r.parent = parent;
    r.first_child = leaf ? -1 : (int32_t)(id + 1u);
    r.child_count = 0;
    r.level = (int32_t)L;
#pragma unroll
    for (int a = 0; a < 3; ++a) r.cell[a] = L >= 24u ? 0u : u[a] >> L;
    r.range_begin = s;
    r.range_end = e;
    r.content_level = -1;
    r.num_points = leaf ? e - s : 0u;
    r.content_begin = leaf ? s : 0u;
    r.reserved = 0;
    r.offset = 0;
    r.bytes = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      r.box_min[a] = __uint_as_float(kNanBits);
      r.box_max[a] = __uint_as_float(kNanBits);
    }
    r.max_radius = 0.0f;
    r.geometric_error = 0.0f;
    table[id] = r;
    ++id;
  }
}

__global__ __launch_bounds__(kBlock) void spz_tile_hist_kernel(const uint8_t *dd, uint32_t n, uint32_t *rows) {
  __shared__ uint32_t h[32];
  if (threadIdx.x < 32) h[threadIdx.x] = 0;
  __syncthreads();
  const unsigned long long first = (unsigned long long)blockIdx.x * kHistRun;
  for (uint32_t r = threadIdx.x; r < kHistRun; r += kBlock) {
    if (first + r < n) atomicAdd(&h[dd[first + r]], 1u);   // integer counts: the order cannot show
  }
  __syncthreads();
  if (threadIdx.x < kLevels) rows[(unsigned long long)blockIdx.x * kLevels + threadIdx.x] = h[threadIdx.x];
}

// rows[b] <- the counts of all runs before b (runs + 1 rows: the last one is the total); cells(L) into the summary.
__global__ __launch_bounds__(kBlock) void spz_tile_hist_prefix_kernel(uint32_t *rows, uint32_t runs, uint32_t n,
                                                                      spz_amd_tile_summary *summary) {
  __shared__ uint32_t part[8][kLevels];
  __shared__ unsigned long long tot[kLevels];
  const uint32_t v = threadIdx.x % 32u, g = threadIdx.x / 32u;   // 8 groups of rows, one column per lane
  const uint32_t per = (runs + 7u) / 8u;
  const uint32_t b = g * per < runs ? g * per : runs;
  const uint32_t e = runs - b < per ? runs : b + per;
  uint32_t sum = 0;
  if (v < kLevels) {
    for (uint32_t k = b; k < e; ++k) sum += rows[(unsigned long long)k * kLevels + v];
    part[g][v] = sum;
  }
  __syncthreads();
  if (v < kLevels) {
    uint32_t run = 0;
    for (uint32_t k = 0; k < g; ++k) run += part[k][v];
    for (uint32_t k = b; k < e; ++k) {
      const uint32_t c = rows[(unsigned long long)k * kLevels + v];
      rows[(unsigned long long)k * kLevels + v] = run;
      run += c;
    }
    if (g == 7u) {
      rows[(unsigned long long)runs * kLevels + v] = run;
      tot[v] = run;
    }
  }
  __syncthreads();
  if (threadIdx.x < kLevels) {
    unsigned long long c = n ? 1ull : 0ull;
    for (uint32_t k = threadIdx.x + 1u; k < kLevels; ++k) c += tot[k];
    summary->cells[threadIdx.x] = c;
  }
}

// One workgroup per tile: child counts; for an interior tile cells_l, content_level and the content's index range.
__global__ __launch_bounds__(kBlock) void spz_tile_level_kernel(const uint8_t *dd, const uint32_t *rows, uint32_t cap,
                                                                uint32_t fb, const spz_amd_tile_summary *summary,
                                                                spz_amd_tile_info *table) {
  __shared__ uint32_t h[2][32];
  if (!summary->ok || blockIdx.x >= summary->num_tiles) return;   // uniform over the block
  spz_amd_tile_info *t = table + blockIdx.x;
  if (threadIdx.x == 0 && t->parent >= 0) atomicAdd(&table[t->parent].child_count, 1u);
  if (t->first_child < 0) return;
  if (threadIdx.x < 64) h[threadIdx.x / 32u][threadIdx.x % 32u] = 0;
  __syncthreads();
  const uint32_t x[2] = {t->range_begin + 1u, t->range_end};
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const uint32_t base = (x[k] / kHistRun) * kHistRun;
    for (uint32_t j = base + threadIdx.x; j < x[k]; j += kBlock) atomicAdd(&h[k][dd[j]], 1u);
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const uint32_t *ra = rows + (unsigned long long)(x[0] / kHistRun) * kLevels;
  const uint32_t *rb = rows + (unsigned long long)(x[1] / kHistRun) * kLevels;
  // G_l(x) = #{j < x : dd[j] > l}; cells_l = 1 + G_l(e) - G_l(s + 1), not increasing in l
  uint32_t ga = 0, gb = 0, best_l = (uint32_t)t->level, best_cells = 1, best_begin = 0;
  for (int l = 24; l >= 0; --l) {
    const uint32_t cells = 1u + gb - ga;
    if ((uint32_t)l <= (uint32_t)t->level && cells <= cap) {
      best_l = (uint32_t)l;
      best_cells = cells;
      best_begin = ga;
    }
    ga += ra[l] + h[0][l];
    gb += rb[l] + h[1][l];
  }
  t->content_level = (int32_t)best_l;
  t->num_points = best_cells;
  t->content_begin = best_begin;
  t->geometric_error = ldexpf(1.0f, (int)best_l - (int)fb);
}

// One workgroup: the tiles' streams laid out in id order, each at a multiple of 16 bytes.
__global__ __launch_bounds__(kBlock) void spz_tile_offsets_kernel(uint32_t version, uint32_t dim,
                                                                  spz_amd_tile_summary *summary, spz_amd_tile_info *table) {
  __shared__ unsigned long long sh[kBlock];
  if (!summary->ok) return;
  auto bytes_of = [&](uint32_t k) {
    return 16ull + (unsigned long long)table[k].num_points * point_bytes(table[k].content_level < 0 ? version : 3u, dim);
  };
  const unsigned long long arena_bytes = block_scan_owned_runs(
      (uint32_t)summary->num_tiles, sh, [&](uint32_t k) { return (bytes_of(k) + 15ull) & ~15ull; },
      [&](uint32_t k, unsigned long long before) {
        table[k].bytes = bytes_of(k);
        table[k].offset = before;
      });
  if (threadIdx.x == 0) summary->arena_bytes = arena_bytes;
}

// The n == 0 tree: one empty leaf.
__global__ void spz_tile_empty_kernel(uint32_t max_tiles, spz_amd_tile_summary *summary, spz_amd_tile_info *table) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  summary->num_tiles = 1;
  summary->arena_bytes = 16;
  summary->ok = max_tiles >= 1u ? 1u : 0u;
  summary->root_level = 0;
  for (uint32_t k = 0; k < kLevels; ++k) summary->cells[k] = 0;
  if (max_tiles < 1u) return;
  spz_amd_tile_info r;
  memset(&r, 0, sizeof(r));
  r.parent = -1;
  r.first_child = -1;
  r.content_level = -1;
  r.bytes = 16;
  for (int a = 0; a < 3; ++a) {
    r.box_min[a] = __uint_as_float(kNanBits);
    r.box_max[a] = __uint_as_float(kNanBits);
  }
  table[0] = r;
}

// prefix[t] = work items of the tiles before t whose content_level is `level` (each such tile: at least one item);
// prefix[num_tiles] = their total.  Their boxes are reset to the integer extremes for the atomics.
__global__ __launch_bounds__(kBlock) void spz_tile_worklist_kernel(spz_amd_tile_info *table,
                                                                   const spz_amd_tile_summary *summary, uint32_t count,
                                                                   int level, uint32_t *prefix) {
  __shared__ uint32_t sh[kBlock];
  count = rows_of(summary, count);
  const uint32_t items = block_scan_owned_runs(
      count, sh,
      [&](uint32_t k) {
        if (table[k].content_level != level) return 0u;
        const uint32_t c = (table[k].num_points + kChunk - 1u) / kChunk;
        return c ? c : 1u;
      },
      [&](uint32_t k, uint32_t before) {
        prefix[k] = before;
        if (table[k].content_level != level) return;
        int32_t *lo = reinterpret_cast<int32_t *>(table[k].box_min), *hi = reinterpret_cast<int32_t *>(table[k].box_max);
        for (int a = 0; a < 3; ++a) {
          lo[a] = 0x7fffffff;
          hi[a] = (int32_t)0x80000000;
        }
        *reinterpret_cast<uint32_t *>(&table[k].max_radius) = 0u;
      });
  if (threadIdx.x == 0) prefix[count] = items;
}

namespace {

// The source stream's header as the kernels trust it: a v2 / v3 stream that lies inside `size` bytes.
struct Source {
  uint32_t version, n, degree, dim, word3;
  unsigned long long off[6];
  uint32_t bpp[6];
  bool ok;
};

__device__ __forceinline__ Source read_source(const uint8_t *src, unsigned long long size) {
  Source s;
  s.ok = false;
  if (size < 16ull) return s;
  const uint32_t *w = reinterpret_cast<const uint32_t *>(src);   // streams are at least 4-aligned (allocations)
  s.version = w[1];
  s.n = w[2];
  s.word3 = w[3];
  s.degree = w[3] & 0xffu;
  if (w[0] != kMagic || s.version < 2u || s.version > 3u || s.degree > 3u) return s;
  s.dim = dim_of_degree(s.degree);
  section_bytes(s.version, s.dim, s.bpp);
  unsigned long long o = 16;
  for (int k = 0; k < 6; ++k) {
    s.off[k] = o;
    o += (unsigned long long)s.n * s.bpp[k];
  }
  s.ok = o <= size;
  return s;
}

// The work item of this workgroup: the tile (the last t with prefix[t] <= item among those with items) and the chunk.
__device__ __forceinline__ bool find_item(const uint32_t *prefix, uint32_t count, uint32_t item, uint32_t *tile,
                                          uint32_t *chunk) {
  if (item >= prefix[count]) return false;
  uint32_t lo = 0, hi = count;   // the first t with prefix[t] > item is in (lo, hi]
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (prefix[mid] <= item) lo = mid; else hi = mid;
  }
  *tile = lo;
  *chunk = item - prefix[lo];
  return true;
}

// A tile's content lies inside the source and its stream inside the arena.
__device__ __forceinline__ bool tile_fits(const spz_amd_tile_info &t, const Source &s, unsigned long long arena_bytes,
                                          bool with_arena) {
  if ((unsigned long long)t.content_begin + t.num_points > s.n) return false;
  if (!with_arena) return true;
  const unsigned long long bytes = 16ull + (unsigned long long)t.num_points * point_bytes(s.version, s.dim);
  return t.bytes == bytes && t.offset <= arena_bytes && bytes <= arena_bytes - t.offset;
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = min(v, __shfl_xor(v, m));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = max(v, __shfl_xor(v, m));
  return v;
}

// dst[0 .. nbytes) = src[0 .. nbytes) by the whole workgroup: a byte head up to dst's 16-byte grid, 16-byte steps, a
// byte tail.  src has whatever alignment the section offsets give it.
__device__ __forceinline__ void copy_bytes(uint8_t *dst, const uint8_t *src, unsigned long long nbytes) {
  const uint32_t t = threadIdx.x;
  unsigned long long head = (16u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u;
  if (head > nbytes) head = nbytes;
  if (t < head) dst[t] = src[t];
  const unsigned long long body = (nbytes - head) / 16ull;
  const U4a1 *s4 = reinterpret_cast<const U4a1 *>(src + head);
  uint4 *d4 = reinterpret_cast<uint4 *>(dst + head);
  for (unsigned long long i = t; i < body; i += kBlock) {
    const U4a1 v = s4[i];
    d4[i] = make_uint4(v.x, v.y, v.z, v.w);
  }
  const unsigned long long done = head + body * 16ull;
  if (done + t < nbytes) dst[done + t] = src[done + t];
}

}  // namespace

__global__ __launch_bounds__(kBlock) void spz_tile_bounds_kernel(spz_amd_tile_info *table,
                                                                 const spz_amd_tile_summary *summary, uint32_t count,
                                                                 int level, const uint32_t *prefix, const uint8_t *src,
                                                                 unsigned long long src_size) {
  uint32_t tile, chunk;
  count = rows_of(summary, count);
  if (!find_item(prefix, count, blockIdx.x, &tile, &chunk)) return;
  const Source s = read_source(src, src_size);
  spz_amd_tile_info *t = table + tile;
  if (!s.ok || t->content_level != level || !tile_fits(*t, s, 0, false)) return;
  const uint32_t p0 = chunk * kChunk;
  const uint32_t p1 = t->num_points - p0 < kChunk ? t->num_points : p0 + kChunk;
  if (p0 >= p1) return;   // an empty tile
  int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000};
  int sc = 0;
  for (uint32_t q = p0 + threadIdx.x; q < p1; q += kBlock) {
    const unsigned long long i = (unsigned long long)t->content_begin + q;
    const uint8_t *b = src + s.off[0] + i * 9ull;
    const uint8_t *c = src + s.off[3] + i * 3ull;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const uint32_t f = (uint32_t)b[3 * a] | ((uint32_t)b[3 * a + 1] << 8) | ((uint32_t)b[3 * a + 2] << 16);
      const int v = (int)(f << 8) >> 8;
      lo[a] = min(lo[a], v);
      hi[a] = max(hi[a], v);
      sc = max(sc, (int)c[a]);
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = wave_min(lo[a]);
    hi[a] = wave_max(hi[a]);
  }
  sc = wave_max(sc);
  if ((threadIdx.x & 63u) == 0 && lo[0] <= hi[0]) {   // integer extremes: the order of the atomics cannot show
    int *tlo = reinterpret_cast<int *>(t->box_min), *thi = reinterpret_cast<int *>(t->box_max);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      atomicMin(&tlo[a], lo[a]);
      atomicMax(&thi[a], hi[a]);
    }
    atomicMax(reinterpret_cast<uint32_t *>(&t->max_radius), (uint32_t)sc);
  }
}

__global__ __launch_bounds__(kBlock) void spz_tile_bounds_finish_kernel(spz_amd_tile_info *table,
                                                                        const spz_amd_tile_summary *summary,
                                                                        uint32_t count, int level, const uint8_t *src,
                                                                        unsigned long long src_size,
                                                                        const RadiusTable radius) {
  const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
  count = rows_of(summary, count);
  if (k >= count) return;
  spz_amd_tile_info *t = table + k;
  if (t->content_level != level) return;
  const Source s = read_source(src, src_size);
  const uint32_t fb = s.ok ? (s.word3 >> 8) & 0xffu : 0u;
  const int *lo = reinterpret_cast<const int *>(t->box_min), *hi = reinterpret_cast<const int *>(t->box_max);
  const bool any = s.ok && lo[0] <= hi[0];
  const uint32_t sc = *reinterpret_cast<const uint32_t *>(&t->max_radius);
  float fl[3], fh[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    fl[a] = any ? ldexpf((float)lo[a], -(int)fb) : __uint_as_float(kNanBits);   // |v| < 2^23: exact
    fh[a] = any ? ldexpf((float)hi[a], -(int)fb) : __uint_as_float(kNanBits);
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    t->box_min[a] = fl[a];
    t->box_max[a] = fh[a];
  }
  t->max_radius = any ? radius.r[sc & 255u] : 0.0f;
}

__global__ __launch_bounds__(kBlock) void spz_tile_emit_kernel(const spz_amd_tile_info *table,
                                                               const spz_amd_tile_summary *summary, uint32_t count,
                                                               int level, const uint32_t *prefix, const uint8_t *src,
                                                               unsigned long long src_size, uint8_t *arena,
                                                               unsigned long long arena_bytes) {
  uint32_t tile, chunk;
  count = rows_of(summary, count);
  if (!find_item(prefix, count, blockIdx.x, &tile, &chunk)) return;
  const Source s = read_source(src, src_size);
  const spz_amd_tile_info *t = table + tile;
  if (!s.ok || t->content_level != level || !tile_fits(*t, s, arena_bytes, true)) return;
  const uint32_t np = t->num_points;
  uint8_t *dst = arena + t->offset;
  if (chunk == 0 && threadIdx.x < 16u) {
    const uint32_t words[4] = {kMagic, s.version, np, s.word3 & 0x0001ffffu};
    dst[threadIdx.x] = (uint8_t)(words[threadIdx.x / 4u] >> (8u * (threadIdx.x % 4u)));
  }
  const uint32_t p0 = chunk * kChunk;
  const uint32_t p1 = np - p0 < kChunk ? np : p0 + kChunk;
  if (p0 >= p1) return;
  unsigned long long doff = 16;
  for (int k = 0; k < 6; ++k) {
    const unsigned long long bpp = s.bpp[k];
    copy_bytes(dst + doff + p0 * bpp, src + s.off[k] + ((unsigned long long)t->content_begin + p0) * bpp, (p1 - p0) * bpp);
    doff += np * bpp;
  }
}

}  // namespace spz_amd_detail

namespace {

using namespace spz_amd_detail;

struct TileLayout {
  uint64_t scan_tiles, hist_runs, table_rows;
  uint32_t pyr_levels, pyr_size[kPyrMax];
  uint64_t sort_ws, order, sorted, dd[kPyrMax], mask, toff, sums, rows, prefix, bytes;
};

uint64_t table_rows_for(uint64_t n, uint64_t max_tiles) {
  const uint64_t most = n ? 2 * n - 1 : 1;   // every interior tile has two or more children
  return max_tiles < most ? max_tiles : most;
}

TileLayout tile_layout(uint64_t n, int sh_degree, uint64_t max_tiles) {
  TileLayout w = {};
  w.scan_tiles = (n + kScanTile - 1) / kScanTile;
  w.hist_runs = (n + kHistRun - 1) / kHistRun;
  w.table_rows = table_rows_for(n, max_tiles);
  spz_amd_layout sl;
  if (spz_amd_stream_layout(n, sh_degree, 3, &sl) != SPZ_AMD_OK) sl.total_bytes = 16 + 64 * n;
  WorkspaceOffsets o;
  o.put(&w.sort_ws, spz_amd_sort_workspace_bytes(n));
  o.put(&w.order, n * 4u);
  o.put(&w.sorted, sl.total_bytes);
  uint64_t size = n ? n : 1;
  w.pyr_levels = 0;
  for (;;) {
    w.pyr_size[w.pyr_levels] = (uint32_t)size;
    o.put(&w.dd[w.pyr_levels], size);
    ++w.pyr_levels;
    if (size <= 64 || w.pyr_levels == kPyrMax) break;
    size = (size + 63) / 64;
  }
  o.put(&w.mask, n * 4u);
  o.put(&w.toff, n * 4u);
  o.put(&w.sums, (w.scan_tiles + 1) * 4u);
  o.put(&w.rows, (w.hist_runs + 1) * kLevels * 4u);
  o.put(&w.prefix, (w.table_rows + 1) * 4u);
  w.bytes = o.bytes();
  return w;
}

int check_input(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, spz_amd_layout *lay) {
  const int rc = check_packed_stream(d_stream, size, hdr, lay);
  if (rc != SPZ_AMD_OK) return rc;
  if (hdr->version == 1) return SPZ_AMD_ERR_UNSUPPORTED;  // float16 positions: no integer cell
  if (hdr->num_points > SPZ_AMD_REFERENCE_MAX_POINTS) return SPZ_AMD_ERR_TOO_MANY_POINTS;
  return SPZ_AMD_OK;
}

int check_caps(uint32_t max_points, uint32_t max_tiles) {
  if (max_points < 1u || max_points > SPZ_AMD_REFERENCE_MAX_POINTS) return SPZ_AMD_ERR_INVALID_ARG;
  if (max_tiles < 1u || max_tiles > 0x7fffffffu) return SPZ_AMD_ERR_INVALID_ARG;
  return SPZ_AMD_OK;
}

RadiusTable radius_table() {
  RadiusTable r;
  for (int b = 0; b < 256; ++b) r.r[b] = 3.0f * (float)std::exp((double)((float)b / 16.0f - 10.0f));
  return r;
}

// Work items, bounds and (d_arena != NULL) the emit of the tiles whose content_level is `level`, from one source.
// max_items: an upper bound of the items (content points / kChunk + tiles).  With d_summary the tile count is read on the
// device and num_tiles is the table's capacity.
int content_run(spz_amd_tile_info *d_table, const spz_amd_tile_summary *d_summary, uint32_t num_tiles, int level,
                const uint8_t *d_source, size_t source_size,
                uint8_t *d_arena, uint64_t arena_bytes, uint32_t *d_prefix, uint64_t max_items, hipStream_t st) {
  if (max_items > 0x7fffffffu) return SPZ_AMD_ERR_INVALID_ARG;
  const uint32_t grid = max_items ? (uint32_t)max_items : 1u;
  hipLaunchKernelGGL(spz_tile_worklist_kernel, dim3(1), dim3(kBlock), 0, st, d_table, d_summary, num_tiles, level, d_prefix);
  SPZ_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(spz_tile_bounds_kernel, dim3(grid), dim3(kBlock), 0, st, d_table, d_summary, num_tiles, level,
                     d_prefix, d_source, (unsigned long long)source_size);
  SPZ_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(spz_tile_bounds_finish_kernel, dim3((num_tiles + kBlock - 1u) / kBlock), dim3(kBlock), 0, st, d_table,
                     d_summary, num_tiles, level, d_source, (unsigned long long)source_size, radius_table());
  SPZ_HIP_TRY(hipGetLastError());
  if (d_arena != nullptr) {
    hipLaunchKernelGGL(spz_tile_emit_kernel, dim3(grid), dim3(kBlock), 0, st, d_table, d_summary, num_tiles, level,
                       d_prefix, d_source, (unsigned long long)source_size, d_arena, (unsigned long long)arena_bytes);
    SPZ_HIP_TRY(hipGetLastError());
  }
  return SPZ_AMD_OK;
}

// The sort, the tree, the level choice, the arena layout and the leaves' bounds.  The sorted stream stays at
// ws + wl.sorted (n == 0: the input is its own sorted stream).
int tree_run(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, const spz_amd_layout &lay, uint32_t cap,
             uint32_t max_tiles, spz_amd_tile_info *d_table, spz_amd_tile_summary *d_summary, uint8_t *ws,
             const TileLayout &wl, hipStream_t st, double *sort_ms) {
  const uint32_t n = hdr->num_points;
  const uint32_t rows = (uint32_t)wl.table_rows;
  uint32_t *prefix = reinterpret_cast<uint32_t *>(ws + wl.prefix);
  const auto t0 = std::chrono::steady_clock::now();
  if (n == 0) {
    hipLaunchKernelGGL(spz_tile_empty_kernel, dim3(1), dim3(64), 0, st, max_tiles, d_summary, d_table);
    SPZ_HIP_TRY(hipGetLastError());
    if (sort_ms) *sort_ms = 0.0;
    return SPZ_AMD_OK;
  }
  uint32_t *order = reinterpret_cast<uint32_t *>(ws + wl.order);
  int rc = spz_amd_morton_order_device(d_stream, size, hdr, 0, order, ws + wl.sort_ws, st);
  if (rc != SPZ_AMD_OK) return rc;
  rc = spz_amd_subset_device(d_stream, size, hdr, order, n, -1, ws + wl.sorted, lay.total_bytes, st);
  if (rc != SPZ_AMD_OK) return rc;
  if (sort_ms) {  // the host form's lap
    SPZ_HIP_TRY(hipStreamSynchronize(st));
    *sort_ms = ms_since(t0);
  }
  const uint8_t *pos = ws + wl.sorted + lay.offset[SPZ_AMD_SEC_POSITIONS];
  Pyramid p = {};
  p.levels = wl.pyr_levels;
  for (uint32_t k = 0; k < wl.pyr_levels; ++k) {
    p.a[k] = ws + wl.dd[k];
    p.size[k] = wl.pyr_size[k];
  }
  const uint32_t point_blocks = (n + kBlock - 1u) / kBlock;
  hipLaunchKernelGGL(spz_tile_dd_kernel, dim3(point_blocks), dim3(kBlock), 0, st, pos, n, ws + wl.dd[0]);
  SPZ_HIP_TRY(hipGetLastError());
  for (uint32_t k = 1; k < wl.pyr_levels; ++k) {
    hipLaunchKernelGGL(spz_tile_pyramid_kernel, dim3((wl.pyr_size[k] + kBlock - 1u) / kBlock), dim3(kBlock), 0, st,
                       ws + wl.dd[k - 1], wl.pyr_size[k - 1], ws + wl.dd[k], wl.pyr_size[k]);
    SPZ_HIP_TRY(hipGetLastError());
  }
  uint32_t *mask = reinterpret_cast<uint32_t *>(ws + wl.mask), *toff = reinterpret_cast<uint32_t *>(ws + wl.toff);
  uint32_t *sums = reinterpret_cast<uint32_t *>(ws + wl.sums), *hist = reinterpret_cast<uint32_t *>(ws + wl.rows);
  hipLaunchKernelGGL(spz_tile_enum_kernel, dim3(point_blocks), dim3(kBlock), 0, st, p, n, cap, mask);
  SPZ_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(spz_tile_scan_reduce_kernel, dim3((unsigned)wl.scan_tiles), dim3(kBlock), 0, st, mask, n, sums);
  SPZ_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(spz_tile_scan_sums_kernel, dim3(1), dim3(kBlock), 0, st, sums, (uint32_t)wl.scan_tiles, rows, p,
                     d_summary);
  SPZ_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(spz_tile_scan_apply_kernel, dim3((unsigned)wl.scan_tiles), dim3(kBlock), 0, st, mask, n, sums, toff);
  SPZ_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(spz_tile_write_kernel, dim3(point_blocks), dim3(kBlock), 0, st, p, pos, n, cap, mask,
                     toff, d_summary, d_table);
  SPZ_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(spz_tile_hist_kernel, dim3((unsigned)wl.hist_runs), dim3(kBlock), 0, st, ws + wl.dd[0], n, hist);
  SPZ_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(spz_tile_hist_prefix_kernel, dim3(1), dim3(kBlock), 0, st, hist, (uint32_t)wl.hist_runs, n, d_summary);
  SPZ_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(spz_tile_level_kernel, dim3(rows), dim3(kBlock), 0, st, ws + wl.dd[0], hist, cap,
                     (uint32_t)hdr->fractional_bits, d_summary, d_table);
  SPZ_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(spz_tile_offsets_kernel, dim3(1), dim3(kBlock), 0, st, (uint32_t)hdr->version,
                     (uint32_t)sh_dim_for_degree(hdr->sh_degree), d_summary, d_table);
  SPZ_HIP_TRY(hipGetLastError());
  // the leaves' bounds, from the sorted stream
  return content_run(d_table, d_summary, rows, -1, ws + wl.sorted, lay.total_bytes, nullptr, 0, prefix,
                     (uint64_t)(n + kChunk - 1u) / kChunk + rows, st);
}

// An open tileset: the device memory in a PackedResult (block: workspace + table + summary; scratch: the decimate's
// workspace; extra: one decimate output; out_block: the arena) and the host copy of the finished table.
struct TileResult {
  PackedResultPtr r;
  std::vector<spz_amd_tile_info> table;
};

}  // namespace

extern "C" {

uint64_t spz_amd_tile_workspace_bytes(uint64_t num_points, int sh_degree, uint64_t max_tiles) {
  return tile_layout(num_points, sh_degree < 0 || sh_degree > 3 ? 3 : sh_degree, max_tiles ? max_tiles : 1).bytes;
}

uint64_t spz_amd_tile_content_workspace_bytes(uint64_t num_tiles) { return (num_tiles + 1) * 4u + 256u; }

int spz_amd_tile_content_device(spz_amd_tile_info *d_table, uint32_t num_tiles, int content_level,
                                const uint8_t *d_source, size_t source_size, uint8_t *d_arena, uint64_t arena_bytes,
                                void *d_workspace, void *hip_stream) {
  if (d_table == nullptr || d_source == nullptr || d_workspace == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  if (num_tiles < 1u || num_tiles > 0x7fffffffu || content_level < -1 || content_level > 24) return SPZ_AMD_ERR_INVALID_ARG;
  if (source_size < 16) return SPZ_AMD_ERR_SHORT_STREAM;
  int device = 0;
  int rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  // a point takes at least 19 bytes, and every tile at least one item
  const uint64_t max_items = ((source_size - 16) / 19u + kChunk - 1) / kChunk + num_tiles;
  return content_run(d_table, nullptr, num_tiles, content_level, d_source, source_size, d_arena, arena_bytes,
                     reinterpret_cast<uint32_t *>(align_ws(d_workspace)), max_items, static_cast<hipStream_t>(hip_stream));
}

int spz_amd_tile_tree_device(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, uint32_t max_points,
                             uint32_t max_tiles, spz_amd_tile_info *d_table, spz_amd_tile_summary *d_summary,
                             void *d_workspace, void *hip_stream) {
  spz_amd_layout lay;
  int rc = check_input(d_stream, size, hdr, &lay);
  if (rc != SPZ_AMD_OK) return rc;
  rc = check_caps(max_points, max_tiles);
  if (rc != SPZ_AMD_OK) return rc;
  if (d_table == nullptr || d_summary == nullptr || d_workspace == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const uint64_t n = hdr->num_points;
  const TileLayout wl = tile_layout(n, hdr->sh_degree, max_tiles);
  uint8_t *ws = align_ws(d_workspace);
  return tree_run(d_stream, size, hdr, lay, max_points, max_tiles, d_table, d_summary, ws, wl, st, nullptr);
}

int spz_amd_tile_open(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, uint32_t max_points,
                      uint32_t max_tiles, int device, void **ctx, uint64_t *h_num_tiles, uint64_t *h_arena_bytes,
                      float *h_ms) {
  if (ctx == nullptr || h_num_tiles == nullptr || h_arena_bytes == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  *ctx = nullptr;
  *h_num_tiles = 0;
  *h_arena_bytes = 0;
  spz_amd_layout lay;
  int rc = check_input(d_stream, size, hdr, &lay);
  if (rc != SPZ_AMD_OK) return rc;
  rc = check_caps(max_points, max_tiles);
  if (rc != SPZ_AMD_OK) return rc;
  const uint64_t n = hdr->num_points;
  DeviceGuard guard;
  rc = guard.enter(device);
  if (rc != SPZ_AMD_OK) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  std::unique_ptr<TileResult> res(new TileResult);
  rc = packed_result_open(device, &res->r);
  if (rc != SPZ_AMD_OK) return rc;
  PackedResult *c = res->r.get();
  const TileLayout wl = tile_layout(n, hdr->sh_degree, max_tiles);
  const uint64_t table_bytes = Workspace::aligned(wl.table_rows * sizeof(spz_amd_tile_info));
  SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&c->block), wl.bytes + table_bytes + 256));
  uint8_t *ws = align_ws(c->block);
  auto *d_table = reinterpret_cast<spz_amd_tile_info *>(ws + wl.bytes - 256);
  auto *d_summary = reinterpret_cast<spz_amd_tile_summary *>(ws + wl.bytes - 256 + table_bytes);
  uint32_t *prefix = reinterpret_cast<uint32_t *>(ws + wl.prefix);
  double sort_ms = 0.0;
  rc = tree_run(d_stream, size, hdr, lay, max_points, max_tiles, d_table, d_summary, ws, wl, c->st, &sort_ms);
  if (rc != SPZ_AMD_OK) return rc;
  spz_amd_tile_summary sum;
  SPZ_HIP_TRY(hipMemcpyAsync(&sum, d_summary, sizeof(sum), hipMemcpyDeviceToHost, c->st));
  SPZ_HIP_TRY(hipStreamSynchronize(c->st));
  if (!sum.ok) return SPZ_AMD_ERR_CAPACITY;   // before any content is produced
  const uint32_t tiles = (uint32_t)sum.num_tiles;
  res->table.resize(tiles);
  SPZ_HIP_TRY(hipMemcpyAsync(res->table.data(), d_table, tiles * sizeof(spz_amd_tile_info), hipMemcpyDeviceToHost, c->st));
  SPZ_HIP_TRY(hipStreamSynchronize(c->st));
  const double tree_ms = ms_since(t0) - sort_ms;
  // the work of each distinct content level
  uint64_t level_points[kLevels] = {}, level_tiles[kLevels] = {}, leaf_points = 0, leaf_tiles = 0;
  for (const spz_amd_tile_info &t : res->table) {
    if (t.content_level < 0) {
      leaf_points += t.num_points;
      ++leaf_tiles;
    } else {
      level_points[t.content_level] += t.num_points;
      ++level_tiles[t.content_level];
    }
  }
  c->out_bytes = sum.arena_bytes;
  SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&c->out_block), c->out_bytes));
  c->out = c->out_block;
  SPZ_HIP_TRY(hipMemsetAsync(c->out, 0, c->out_bytes, c->st));   // the padding between the streams
  const uint32_t dim = (uint32_t)sh_dim_for_degree(hdr->sh_degree);
  uint64_t dec_bytes = 0;
  for (uint32_t l = 0; l < kLevels; ++l) {
    if (level_tiles[l] == 0) continue;
    const uint64_t b = 16 + sum.cells[l] * point_bytes(3u, dim);
    dec_bytes = b > dec_bytes ? b : dec_bytes;
  }
  if (dec_bytes) {
    SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&c->extra), dec_bytes));
    SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&c->scratch), spz_amd_decimate_workspace_bytes(n, hdr->sh_degree)));
  }
  double dec_ms = 0.0;
  for (uint32_t l = 0; l < kLevels; ++l) {   // one decimate at a time into the reused buffer; no readbacks
    if (level_tiles[l] == 0) continue;
    const auto t1 = std::chrono::steady_clock::now();
    const uint64_t b = 16 + sum.cells[l] * point_bytes(3u, dim);
    rc = spz_amd_decimate_device(d_stream, size, hdr, (int)l, c->extra, b, nullptr, c->scratch, c->st);
    if (rc != SPZ_AMD_OK) return rc;
    if (h_ms) {
      SPZ_HIP_TRY(hipStreamSynchronize(c->st));
      dec_ms += ms_since(t1);
    }
    rc = content_run(d_table, nullptr, tiles, (int)l, c->extra, b, c->out, c->out_bytes, prefix,
                     (level_points[l] + kChunk - 1) / kChunk + level_tiles[l], c->st);
    if (rc != SPZ_AMD_OK) return rc;
  }
  const uint8_t *sorted = n ? ws + wl.sorted : d_stream;
  rc = content_run(d_table, nullptr, tiles, -1, sorted, lay.total_bytes, c->out, c->out_bytes, prefix,
                   (leaf_points + kChunk - 1) / kChunk + leaf_tiles, c->st);
  if (rc != SPZ_AMD_OK) return rc;
  SPZ_HIP_TRY(hipMemcpyAsync(res->table.data(), d_table, tiles * sizeof(spz_amd_tile_info), hipMemcpyDeviceToHost, c->st));
  SPZ_HIP_TRY(hipStreamSynchronize(c->st));
  if (h_ms) {
    h_ms[0] = (float)sort_ms;
    h_ms[1] = (float)tree_ms;
    h_ms[2] = (float)dec_ms;
    h_ms[3] = (float)(ms_since(t0) - sort_ms - tree_ms - dec_ms);
  }
  *h_num_tiles = tiles;
  *h_arena_bytes = c->out_bytes;
  *ctx = res.release();
  return SPZ_AMD_OK;
}

int spz_amd_tile_table(void *ctx, spz_amd_tile_info *h_table) {
  TileResult *r = static_cast<TileResult *>(ctx);
  if (r == nullptr || h_table == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  std::memcpy(h_table, r->table.data(), r->table.size() * sizeof(spz_amd_tile_info));
  return SPZ_AMD_OK;
}

int spz_amd_tile_fetch(void *ctx, uint32_t id, uint8_t *h_out) {
  TileResult *r = static_cast<TileResult *>(ctx);
  if (r == nullptr || h_out == nullptr || id >= r->table.size()) return SPZ_AMD_ERR_INVALID_ARG;
  PackedResult *c = r->r.get();
  DeviceGuard guard;
  int rc = guard.enter(c->device);
  if (rc != SPZ_AMD_OK) return rc;
  SPZ_HIP_TRY(hipMemcpyAsync(h_out, c->out + r->table[id].offset, r->table[id].bytes, hipMemcpyDeviceToHost, c->st));
  SPZ_HIP_TRY(hipStreamSynchronize(c->st));
  return SPZ_AMD_OK;
}

int spz_amd_tile_fetch_arena(void *ctx, uint8_t *h_out) {
  TileResult *r = static_cast<TileResult *>(ctx);
  return r == nullptr ? SPZ_AMD_ERR_INVALID_ARG : packed_result_fetch(r->r.get(), h_out);
}

const uint8_t *spz_amd_tile_device_data(void *ctx, uint32_t id) {
  TileResult *r = static_cast<TileResult *>(ctx);
  if (r == nullptr || id >= r->table.size()) return nullptr;
  return r->r->out + r->table[id].offset;
}

void spz_amd_tile_close(void *ctx) { delete static_cast<TileResult *>(ctx); }

}  // extern "C"
