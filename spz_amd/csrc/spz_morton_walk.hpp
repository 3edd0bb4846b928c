// spz_morton_walk.hpp — the exact nearest-neighbour walk over Morton-sorted integer positions, for the kernels of
// libspz_amd.so that search neighbours (spz_clean.hip: k-NN and radius counts; spz_align.hip: the nearest target point).
//
// The points are (u_x, u_y, u_z, input index), u = the stored 24-bit field XOR 0x800000, in Morton order
// (spz_sort.hip's morton_sorted_points), so every octree cell at every level is a contiguous range, found by binary
// search.  One wave serves 64 queries.  Lanes that share a level and a cell form a group; 54 lanes find the ranges of
// the group's 3x3x3 block of cells; the wave streams the block's points in chunks of 64 (one coalesced load, each
// candidate broadcast with readlane) and every lane of the group scores every candidate.  A chunk whose common Morton
// cell cannot matter to any lane of the group is skipped.  A query that the block does not settle (its gap to the
// block's faces, face_gap) retries one level up; level 24 covers all of space.
//
// What differs between the searches is a policy object, passed by reference and inlined (no function pointers):
//
//   static constexpr bool kSaturates   whether more() is ever false
//   void start()                       a group begins a block (any lane)
//   bool more() const                  this lane can still use a candidate; when no lane of the group can, the block ends
//   bool near(lo, hi) const            a point of the closed box [lo, hi] could change this lane's result
//   void visit(mine, x, y, z, w, at)   one candidate (u, input index w, sorted index `at`), on every lane; `mine`: this
//                                      lane is of the group (the others leave their state alone)
//   bool settle(Lg)                    lanes of the group only, after the block at level Lg: true when this lane's result
//                                      is final (the policy stores it), false to retry at Lg + 1
//
// The distance type and its tie rule belong to the policy: f64 and `<` in spz_clean.hip, u64 and `<=` in spz_align.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#pragma clang fp contract(off)

namespace spz_amd_detail {

// Axis a of point i of a position section, as the walk's unsigned coordinate.
__device__ __forceinline__ uint32_t load_u(const uint8_t *pos, unsigned long long i, uint32_t a) {
  const uint8_t *b = pos + i * 9ull + 3u * a;
  return ((uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16)) ^ 0x800000u;
}

// msb(p) < msb(q) (msb(0) = -1)
__device__ __forceinline__ bool msb_less(uint32_t p, uint32_t q) { return p < q && p < (p ^ q); }

// Morton order of two cells at one level: the axis of the highest differing bit decides; at equal bits z outranks y
// outranks x (key bit 3b + a).
__device__ __forceinline__ int cell_cmp(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t b0, uint32_t b1, uint32_t b2) {
  uint32_t best = a2 ^ b2, x = a2, y = b2;
  if (msb_less(best, a1 ^ b1)) {
    best = a1 ^ b1;
    x = a1;
    y = b1;
  }
  if (msb_less(best, a0 ^ b0)) {
    best = a0 ^ b0;
    x = a0;
    y = b0;
  }
  if (best == 0) return 0;
  return x < y ? -1 : 1;
}

// The first sorted point whose cell at level L is >= c (upper: > c) in Morton order.
static __device__ uint32_t cell_bound(const uint4 *pts, uint32_t n, uint32_t L, uint32_t c0, uint32_t c1, uint32_t c2,
                                      bool upper) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    const uint4 p = pts[mid];
    const int r = cell_cmp(p.x >> L, p.y >> L, p.z >> L, c0, c1, c2);
    if (r < 0 || (upper && r == 0)) {
      lo = mid + 1;
    } else {
      hi = mid;
    }
  }
  return lo;
}

// Cell q of the 3x3x3 block in scan order: q = 0 is the centre, then the other 26.
__device__ __forceinline__ void block_offset(uint32_t q, int *o) {
  const uint32_t t = q == 0 ? 13u : (q == 13 ? 0u : q);
  o[0] = (int)(t % 3u) - 1;
  o[1] = (int)((t / 3u) % 3u) - 1;
  o[2] = (int)(t / 9u) - 1;
}

// The smallest Morton cell holding sorted points f and l (and so every point between them): [lo, hi] per axis.
__device__ __forceinline__ void common_cell(uint32_t f0, uint32_t f1, uint32_t f2, uint32_t l0, uint32_t l1, uint32_t l2,
                                            uint32_t lo[3], uint32_t hi[3]) {
  const uint32_t x = (f0 ^ l0) | (f1 ^ l1) | (f2 ^ l2);
  const uint32_t lv = x ? 32u - (uint32_t)__clz(x) : 0u;  // the level of the common cell
  const uint32_t mask = lv >= 32u ? 0xffffffffu : ((1u << lv) - 1u);
  lo[0] = f0 & ~mask;
  lo[1] = f1 & ~mask;
  lo[2] = f2 & ~mask;
  hi[0] = lo[0] | mask;
  hi[1] = lo[1] | mask;
  hi[2] = lo[2] | mask;
}

__device__ __forceinline__ uint32_t rl(uint32_t v, uint32_t lane) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)lane);
}

// The smallest level at which c and p lie in one cell.
__device__ __forceinline__ uint32_t join_level(const uint32_t c[3], const uint4 p) {
  const uint32_t d = (c[0] ^ p.x) | (c[1] ^ p.y) | (c[2] ^ p.z);
  return d ? 32u - (uint32_t)__clz(d) : 0u;
}

// The smallest level, 24 at the most, at which the cell of c holds a sorted point: the two points beside c's place in
// the Morton order share the longest prefix with it.
__device__ __forceinline__ uint32_t occupied_level(const uint4 *pts, uint32_t n, const uint32_t c[3]) {
  const uint32_t at = cell_bound(pts, n, 0u, c[0], c[1], c[2], false);
  uint32_t l = 24u;
  if (at < n) l = min(l, join_level(c, pts[at]));
  if (at > 0u) l = min(l, join_level(c, pts[at - 1u]));
  return l;
}

// The distance from q (c: q clamped to the cube) to the nearest face of the 3x3x3 block around c's cell at level Lg
// that has space beyond it, as the smallest whole step that leaves the block; -1 when the block has no such face.
// Every point outside the block is at least this far from q.
__device__ __forceinline__ long long face_gap(const int32_t q[3], const uint32_t c[3], uint32_t Lg) {
  const uint32_t last = (1u << (24u - Lg)) - 1u;
  long long g = -1;
#pragma unroll
  for (uint32_t a = 0; a < 3; ++a) {
    const uint32_t cc = c[a] >> Lg;
    if (cc > 1u) {
      const long long v = (long long)q[a] - (long long)((unsigned long long)(cc - 1u) << Lg) + 1;
      g = g < 0 || v < g ? v : g;
    }
    if (cc + 1u < last) {
      const long long v = (long long)((unsigned long long)(cc + 2u) << Lg) - (long long)q[a];
      g = g < 0 || v < g ? v : g;
    }
  }
  return g;
}

// The ranges of the 3x3x3 block around cell (c0, c1, c2) at level Lg: lane q < 27 returns the first sorted point of cell
// q (block_offset's order), lane 27 + q its end; a cell outside the cube is empty (0, 0).
__device__ __forceinline__ uint32_t walk_bounds(const uint4 *pts, uint32_t n, uint32_t lane, uint32_t Lg, uint32_t c0,
                                                uint32_t c1, uint32_t c2) {
  uint32_t bound = 0;
  if (lane < 54u) {
    int o[3];
    block_offset(lane % 27u, o);
    const long long cells = 1ll << (24 - Lg);
    const long long x = (long long)c0 + o[0], y = (long long)c1 + o[1], z = (long long)c2 + o[2];
    if (x >= 0 && y >= 0 && z >= 0 && x < cells && y < cells && z < cells) {
      bound = cell_bound(pts, n, Lg, (uint32_t)x, (uint32_t)y, (uint32_t)z, lane >= 27u);
    }
  }
  return bound;
}

// The block's points, cell by cell in chunks of 64, through the lanes of the group.
template <class Policy>
__device__ __forceinline__ void walk_block(const uint4 *pts, uint32_t lane, uint32_t bound, bool in_g, Policy &pol) {
  bool stop = false;  // a flag and a break: a return out of both loops costs the k-NN kernels half their occupancy
  for (uint32_t q = 0; q < 27u && !stop; ++q) {
    const uint32_t s = rl(bound, q), e = rl(bound, q + 27u);
    for (uint32_t b0 = s; b0 < e; b0 += 64u) {
      if constexpr (Policy::kSaturates) {
        if (!__ballot(in_g && pol.more())) {
          stop = true;
          break;
        }
      }
      const uint32_t cnt = min(64u, e - b0);
      uint4 cand = make_uint4(0, 0, 0, 0);
      if (lane < cnt) cand = pts[b0 + lane];
      uint32_t lo[3], hi[3];
      common_cell(rl(cand.x, 0), rl(cand.y, 0), rl(cand.z, 0), rl(cand.x, cnt - 1), rl(cand.y, cnt - 1),
                  rl(cand.z, cnt - 1), lo, hi);
      if (!__ballot(in_g && pol.near(lo, hi))) continue;
      for (uint32_t k = 0; k < cnt; ++k) {
        const uint32_t x = rl(cand.x, k), y = rl(cand.y, k), z = rl(cand.z, k), w = rl(cand.w, k);
        pol.visit(in_g, x, y, z, w, b0 + k);
      }
    }
  }
}

// The walk of one wave: lane `lane` holds one query (`valid`), located at c (inside the cube) and starting at level L.
// Returns when every query is settled.
template <class Policy>
__device__ __forceinline__ void morton_walk(const uint4 *pts, uint32_t n, uint32_t lane, bool valid, const uint32_t c[3],
                                            uint32_t L, Policy &pol) {
  unsigned long long pending = __ballot(valid);
  while (pending) {
    const uint32_t leader = (uint32_t)__builtin_ctzll(pending);
    const uint32_t Lg = rl(L, leader);
    const uint32_t c0 = rl(c[0] >> Lg, leader), c1 = rl(c[1] >> Lg, leader), c2 = rl(c[2] >> Lg, leader);
    const bool in_g = ((pending >> lane) & 1ull) && L == Lg && (c[0] >> Lg) == c0 && (c[1] >> Lg) == c1 &&
                      (c[2] >> Lg) == c2;
    const uint32_t bound = walk_bounds(pts, n, lane, Lg, c0, c1, c2);
    pol.start();
    walk_block(pts, lane, bound, in_g, pol);
    const bool done = in_g && pol.settle(Lg);
    if (in_g && !done) L = Lg + 1u;
    pending &= ~__ballot(done);
  }
}

}  // namespace spz_amd_detail
