// spz_mesh.hip — a triangle mesh of a scene (DESIGN §8 "Mesh"; the contract is in include/spz_amd.h "mesh"): depth maps
// fused into a truncated signed distance volume, and the zero level set of that volume by marching tetrahedra.
//
//   spz_tsdf_integrate_kernel   one lane per lattice point, x on the fastest thread index (a wave covers 64 consecutive
//                               x of one row): the projection in f64, every skip test before a plane is touched, then the
//                               five planes read, added to and written, coalesced.  No atomics: one lane owns one point.
//   spz_mesh_bounds_kernel      the box of a stream's finite decoded positions: wave minima and maxima, then integer
//                               atomic min / max on order-preserving keys (the result does not depend on the order).
//   spz_mesh_classify_kernel    one lane per cube: valid?, the 8-bit inside mask, the triangle count from the table, and
//                               a 1 in the dense edge map (7 u32 per lattice point) for every edge a triangle uses.
//   spz_mesh_scan_*             exclusive scans of the triangle counts and of the edge map (2048 values per block: block
//                               sums, one block over the sums, the prefix applied in place).
//   spz_mesh_vertices_kernel    one lane per edge of the map: position and colour where the edge is used.
//   spz_mesh_triangles_kernel   one lane per cube: its triangles, the vertex numbers looked up in the edge map.
//
// The (tet, mask) -> triangles table is built on the host from the rule of the contract (tet_table()), at first use,
// and uploaded to the front of the extraction's workspace.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>

#include "spz_amd.h"
#include "spz_block_ops.hpp"
#include "spz_common.hpp"
#include "spz_view_pass.hpp"

#pragma clang fp contract(off)

namespace spz_amd_detail {
namespace {

constexpr uint32_t kMeshBlock = 256;
constexpr uint32_t kScanPer = 8;                         // values per lane of a scan block
constexpr uint32_t kScanTile = kMeshBlock * kScanPer;    // 2048 values per block
constexpr uint32_t kNoVertex = 0xffffffffu;
constexpr uint64_t kMaxLattice = 1ull << 28;

// The six Kuhn tetrahedra of a cube and, per (tet, inside mask), the triangles as tet edge numbers.  Corners are
// numbered x + 2 y + 4 z; tet edges by vertex pairs (0,1), (0,2), (0,3), (1,2), (1,3), (2,3).
struct TetTable {
  uint8_t corner[6][4];
  uint8_t ntri[6][16];
  uint8_t edge[6][16][6];
};

__host__ __device__ inline uint32_t tet_edge_lo(uint32_t q) { return q < 3u ? 0u : (q < 5u ? 1u : 2u); }
__host__ __device__ inline uint32_t tet_edge_hi(uint32_t q) { return q < 3u ? q + 1u : (q < 5u ? q - 1u : 3u); }

int tet_edge_of(int a, int b) {
  for (int q = 0; q < 6; ++q) {
    if ((int)tet_edge_lo((uint32_t)q) == a && (int)tet_edge_hi((uint32_t)q) == b) return q;
  }
  return -1;
}

TetTable build_tet_table() {
  TetTable t;
  std::memset(&t, 0, sizeof(t));
  static const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
  for (int k = 0; k < 6; ++k) {
    t.corner[k][0] = 0;
    t.corner[k][1] = (uint8_t)(1 << perm[k][0]);
    t.corner[k][2] = (uint8_t)(t.corner[k][1] | (1 << perm[k][1]));
    t.corner[k][3] = 7;
    for (int m = 1; m < 15; ++m) {
      int in[4], nin = 0, out[4], nout = 0;
      for (int v = 0; v < 4; ++v) {
        if ((m >> v) & 1) in[nin++] = v; else out[nout++] = v;
      }
      int tri[2][3], ntri = 0;
      if (nin == 1 || nin == 3) {
        const int lone = nin == 1 ? in[0] : out[0];
        int e = 0;
        for (int q = 0; q < 6; ++q) {  // the three edges at `lone`, ascending edge number
          if ((int)tet_edge_lo((uint32_t)q) == lone || (int)tet_edge_hi((uint32_t)q) == lone) tri[0][e++] = q;
        }
        ntri = 1;
      } else {
        const int *with0 = in[0] == 0 ? in : out, *other = in[0] == 0 ? out : in;
        const int j = with0[1], kk = other[0], l = other[1];
        const int q[4] = {tet_edge_of(0, kk), tet_edge_of(0, l), tet_edge_of(j < l ? j : l, j < l ? l : j),
                          tet_edge_of(j < kk ? j : kk, j < kk ? kk : j)};
        tri[0][0] = q[0]; tri[0][1] = q[1]; tri[0][2] = q[2];
        tri[1][0] = q[0]; tri[1][1] = q[2]; tri[1][2] = q[3];
        ntri = 2;
      }
      // orientation, with edge midpoints as positions (twice the midpoint: integers): the normal points from the
      // centroid of the inside vertices to the centroid of the outside vertices
      int sin3[3] = {0, 0, 0}, sout3[3] = {0, 0, 0};
      for (int v = 0; v < 4; ++v) {
        for (int a = 0; a < 3; ++a) {
          const int c = (t.corner[k][v] >> a) & 1;
          if ((m >> v) & 1) sin3[a] += c; else sout3[a] += c;
        }
      }
      int dir[3];
      for (int a = 0; a < 3; ++a) dir[a] = nin * sout3[a] - nout * sin3[a];
      for (int r = 0; r < ntri; ++r) {
        int p[3][3];
        for (int e = 0; e < 3; ++e) {
          const int ca = t.corner[k][tet_edge_lo((uint32_t)tri[r][e])], cb = t.corner[k][tet_edge_hi((uint32_t)tri[r][e])];
          for (int a = 0; a < 3; ++a) p[e][a] = ((ca >> a) & 1) + ((cb >> a) & 1);
        }
        int u[3], w[3];
        for (int a = 0; a < 3; ++a) {
          u[a] = p[1][a] - p[0][a];
          w[a] = p[2][a] - p[0][a];
        }
        const int nrm[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
        if (nrm[0] * dir[0] + nrm[1] * dir[1] + nrm[2] * dir[2] < 0) {
          const int s = tri[r][1];
          tri[r][1] = tri[r][2];
          tri[r][2] = s;
        }
        for (int e = 0; e < 3; ++e) t.edge[k][m][3 * r + e] = (uint8_t)tri[r][e];
      }
      t.ntri[k][m] = (uint8_t)ntri;
    }
  }
  return t;
}

const TetTable &tet_table() {
  static const TetTable t = build_tet_table();
  return t;
}

struct Lattice {
  uint32_t nx, ny, nz;
  uint32_t count;  // nx ny nz <= 2^28
};

__device__ __forceinline__ uint32_t corner_offset(const Lattice &l, uint32_t c) {
  return (c & 1u) + ((c >> 1) & 1u) * l.nx + ((c >> 2) & 1u) * l.nx * l.ny;
}

// ---- fuse ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMeshBlock) void spz_tsdf_integrate_kernel(spz_amd_tsdf_volume vol, spz_amd_render_params rp,
                                                                        const float *__restrict__ depth,
                                                                        const float *__restrict__ image, int expected,
                                                                        float min_alpha, float *grid) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x, j = blockIdx.y * 4u + threadIdx.y, k = blockIdx.z;
  if (i >= vol.dims[0] || j >= vol.dims[1]) return;
  const double s = (double)vol.voxel_size;
  const double px = (double)vol.lo[0] + (double)i * s, py = (double)vol.lo[1] + (double)j * s,
               pz = (double)vol.lo[2] + (double)k * s;
  const float *M = rp.world_to_camera;
  const double z = (((double)M[8] * px + (double)M[9] * py) + (double)M[10] * pz) + (double)M[11];
  if (!(z > (double)rp.near_plane)) return;
  const double x = (((double)M[0] * px + (double)M[1] * py) + (double)M[2] * pz) + (double)M[3];
  const double y = (((double)M[4] * px + (double)M[5] * py) + (double)M[6] * pz) + (double)M[7];
  const double uf = floor((double)rp.fx * (x / z) + (double)rp.cx), vf = floor((double)rp.fy * (y / z) + (double)rp.cy);
  if (!(uf >= 0.0 && uf < (double)rp.width && vf >= 0.0 && vf < (double)rp.height)) return;
  const size_t pix = (size_t)(uint32_t)vf * rp.width + (uint32_t)uf;
  float D;
  if (expected) {
    const float a = image[pix * 4u + 3u];
    if (!(a >= min_alpha)) return;
    D = depth[pix * 2u] / a;
  } else {
    D = depth[pix * 2u + 1u];
  }
  if (!(D > 0.0f) || !(D < INFINITY)) return;
  const double sdf = (double)D - z;
  if (sdf < -(double)vol.truncation) return;
  const double q = sdf / (double)vol.truncation;
  const float d = (float)(q < 1.0 ? q : 1.0);
  const size_t plane = (size_t)vol.dims[0] * vol.dims[1] * vol.dims[2];
  const size_t lin = ((size_t)k * vol.dims[1] + j) * vol.dims[0] + i;
  grid[lin] = grid[lin] + 1.0f;
  grid[plane + lin] = grid[plane + lin] + d;
  grid[2u * plane + lin] = grid[2u * plane + lin] + image[pix * 4u];
  grid[3u * plane + lin] = grid[3u * plane + lin] + image[pix * 4u + 1u];
  grid[4u * plane + lin] = grid[4u * plane + lin] + image[pix * 4u + 2u];
}

// ---- the box of a stream's positions ----------------------------------------------------------------------------
__device__ __forceinline__ uint32_t order_key(float v) {
  const uint32_t b = __float_as_uint(v);
  return (b >> 31) ? ~b : (b | 0x80000000u);
}

inline float order_key_value(uint32_t k) {
  const uint32_t b = (k >> 31) ? (k & 0x7fffffffu) : ~k;
  float v;
  std::memcpy(&v, &b, 4);
  return v;
}

__global__ __launch_bounds__(kMeshBlock) void spz_mesh_bounds_kernel(const uint8_t *positions, uint32_t n, uint32_t float16,
                                                                     float pos_scale, uint32_t flip_p, uint32_t *keys) {
  uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
  for (unsigned long long i = (unsigned long long)blockIdx.x * kMeshBlock + threadIdx.x; i < n;
       i += (unsigned long long)gridDim.x * kMeshBlock) {
    float v[3];
#pragma unroll
    for (uint32_t a = 0; a < 3; ++a) v[a] = decode_position_axis(positions, i, a, float16 != 0u, pos_scale, flip_p);
    if (!(fabsf(v[0]) < INFINITY && fabsf(v[1]) < INFINITY && fabsf(v[2]) < INFINITY)) continue;
#pragma unroll
    for (uint32_t a = 0; a < 3; ++a) {
      const uint32_t key = order_key(v[a]);
      lo[a] = key < lo[a] ? key : lo[a];
      hi[a] = key > hi[a] ? key : hi[a];
    }
  }
#pragma unroll
  for (uint32_t off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (uint32_t a = 0; a < 3; ++a) {
      const uint32_t l = (uint32_t)__shfl_xor((int)lo[a], (int)off), h = (uint32_t)__shfl_xor((int)hi[a], (int)off);
      lo[a] = l < lo[a] ? l : lo[a];
      hi[a] = h > hi[a] ? h : hi[a];
    }
  }
  if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
    for (uint32_t a = 0; a < 3; ++a) {
      atomicMin(&keys[a], lo[a]);
      atomicMax(&keys[3u + a], hi[a]);
    }
  }
}

// ---- extract ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMeshBlock) void spz_mesh_classify_kernel(Lattice l, const float *__restrict__ grid,
                                                                       float min_weight, const TetTable *__restrict__ table,
                                                                       uint8_t *cube_mask, uint32_t *tri_count,
                                                                       uint32_t *edge_map) {
  __shared__ TetTable s_table;
  for (uint32_t b = threadIdx.x; b < sizeof(TetTable); b += kMeshBlock) {
    reinterpret_cast<uint8_t *>(&s_table)[b] = reinterpret_cast<const uint8_t *>(table)[b];
  }
  __syncthreads();
  const uint32_t lin = blockIdx.x * kMeshBlock + threadIdx.x;
  if (lin >= l.count) return;
  const uint32_t i = lin % l.nx, j = (lin / l.nx) % l.ny, k = lin / (l.nx * l.ny);
  uint32_t cm = 0u;
  bool valid = i + 1u < l.nx && j + 1u < l.ny && k + 1u < l.nz;
  if (valid) {
#pragma unroll
    for (uint32_t c = 0; c < 8; ++c) {
      const uint32_t at = lin + corner_offset(l, c);
      const float w = grid[at];
      valid = valid && (w >= min_weight);
      const float f = grid[(size_t)l.count + at] / w;
      cm |= (f < 0.0f ? 1u : 0u) << c;
    }
  }
  if (!valid || cm == 0xffu) cm = 0u;
  uint32_t count = 0u;
  if (cm != 0u) {
    for (uint32_t t = 0; t < 6; ++t) {
      uint32_t m = 0u;
#pragma unroll
      for (uint32_t v = 0; v < 4; ++v) m |= ((cm >> s_table.corner[t][v]) & 1u) << v;
      const uint32_t nt = s_table.ntri[t][m];
      count += nt;
      for (uint32_t e = 0; e < 3u * nt; ++e) {
        const uint32_t q = s_table.edge[t][m][e];
        const uint32_t ca = s_table.corner[t][tet_edge_lo(q)], cb = s_table.corner[t][tet_edge_hi(q)];
        edge_map[7u * (lin + corner_offset(l, ca)) + (cb - ca) - 1u] = 1u;  // every writer writes the same 1
      }
    }
  }
  cube_mask[lin] = (uint8_t)cm;
  tri_count[lin] = count;
}

__global__ __launch_bounds__(kMeshBlock) void spz_mesh_scan_reduce_kernel(const uint32_t *__restrict__ a, uint32_t n,
                                                                          uint32_t *block_sum_out) {
  __shared__ unsigned long long s[kMeshBlock];
  const uint32_t base = blockIdx.x * kScanTile + threadIdx.x * kScanPer;
  unsigned long long v = 0ull;
#pragma unroll
  for (uint32_t e = 0; e < kScanPer; ++e) v += base + e < n ? a[base + e] : 0u;
  const unsigned long long total = block_sum(v, s);
  if (threadIdx.x == 0u) block_sum_out[blockIdx.x] = (uint32_t)total;  // <= 2048 * 12
}

// One block: the exclusive prefixes of the block sums (u64) and the total.
__global__ __launch_bounds__(kMeshBlock) void spz_mesh_scan_sums_kernel(const uint32_t *__restrict__ sums, uint32_t blocks,
                                                                        unsigned long long *offsets,
                                                                        unsigned long long *total) {
  __shared__ unsigned long long s[kMeshBlock];
  unsigned long long carry = 0ull;
  for (uint32_t base = 0; base < blocks; base += kMeshBlock) {
    const uint32_t at = base + threadIdx.x;
    const unsigned long long v = at < blocks ? sums[at] : 0ull;
    const unsigned long long pre = block_exclusive_scan(v, s);
    if (at < blocks) offsets[at] = carry + pre;
    carry += block_sum(v, s);
  }
  if (threadIdx.x == 0u) *total = carry;
}

// In place.  to_vertex == 0: a[c] = the prefix inside its block (the triangle kernel adds the block's offset).
// to_vertex != 0: a[e] = the global prefix where a[e] != 0 (the vertex number), kNoVertex elsewhere.
__global__ __launch_bounds__(kMeshBlock) void spz_mesh_scan_apply_kernel(uint32_t *a, uint32_t n,
                                                                         const unsigned long long *__restrict__ offsets,
                                                                         uint32_t to_vertex) {
  __shared__ unsigned long long s[kMeshBlock];
  const uint32_t base = blockIdx.x * kScanTile + threadIdx.x * kScanPer;
  uint32_t v[kScanPer];
  unsigned long long sum = 0ull;
#pragma unroll
  for (uint32_t e = 0; e < kScanPer; ++e) {
    v[e] = base + e < n ? a[base + e] : 0u;
    sum += v[e];
  }
  unsigned long long pre = block_exclusive_scan(sum, s);
  if (to_vertex) pre += offsets[blockIdx.x];
#pragma unroll
  for (uint32_t e = 0; e < kScanPer; ++e) {
    if (base + e < n) a[base + e] = to_vertex ? (v[e] ? (uint32_t)pre : kNoVertex) : (uint32_t)pre;
    pre += v[e];
  }
}

__global__ __launch_bounds__(kMeshBlock) void spz_mesh_vertices_kernel(spz_amd_tsdf_volume vol, Lattice l,
                                                                       const float *__restrict__ grid,
                                                                       const uint32_t *__restrict__ edge_map,
                                                                       unsigned long long num_vertices, float *positions,
                                                                       float *colors) {
  const uint32_t e = blockIdx.x * kMeshBlock + threadIdx.x;
  if (e >= 7u * l.count) return;
  const uint32_t vi = edge_map[e];
  if (vi == kNoVertex || vi >= num_vertices) return;  // the second: never write past the caller's buffers
  const uint32_t a = e / 7u, code = e % 7u + 1u, b = a + corner_offset(l, code);
  const size_t n = l.count;
  const float wa = grid[a], wb = grid[b];
  const float fa = grid[n + a] / wa, fb = grid[n + b] / wb;
  const double t = (double)fa / ((double)fa - (double)fb);
  const uint32_t idx[3] = {a % l.nx, (a / l.nx) % l.ny, a / (l.nx * l.ny)};
  const double s = (double)vol.voxel_size;
#pragma unroll
  for (uint32_t ax = 0; ax < 3; ++ax) {
    const double d = (double)((code >> ax) & 1u);
    positions[(size_t)vi * 3u + ax] = (float)((double)vol.lo[ax] + ((double)idx[ax] + t * d) * s);
    const float ca = grid[(2u + ax) * n + a] / wa, cb = grid[(2u + ax) * n + b] / wb;
    colors[(size_t)vi * 3u + ax] = (float)((double)ca + t * ((double)cb - (double)ca));
  }
}

__global__ __launch_bounds__(kMeshBlock) void spz_mesh_triangles_kernel(Lattice l, const TetTable *__restrict__ table,
                                                                        const uint8_t *__restrict__ cube_mask,
                                                                        const uint32_t *__restrict__ tri_prefix,
                                                                        const unsigned long long *__restrict__ offsets,
                                                                        const uint32_t *__restrict__ edge_map,
                                                                        unsigned long long num_triangles,
                                                                        uint32_t *triangles) {
  __shared__ TetTable s_table;
  for (uint32_t b = threadIdx.x; b < sizeof(TetTable); b += kMeshBlock) {
    reinterpret_cast<uint8_t *>(&s_table)[b] = reinterpret_cast<const uint8_t *>(table)[b];
  }
  __syncthreads();
  const uint32_t lin = blockIdx.x * kMeshBlock + threadIdx.x;
  if (lin >= l.count) return;
  const uint32_t cm = cube_mask[lin];
  if (cm == 0u) return;
  unsigned long long at = offsets[lin / kScanTile] + tri_prefix[lin];
  for (uint32_t t = 0; t < 6; ++t) {
    uint32_t m = 0u;
#pragma unroll
    for (uint32_t v = 0; v < 4; ++v) m |= ((cm >> s_table.corner[t][v]) & 1u) << v;
    const uint32_t nt = s_table.ntri[t][m];
    for (uint32_t r = 0; r < nt; ++r, ++at) {
      if (at >= num_triangles) return;  // cannot happen with the counts of this workspace; never write past the buffer
      for (uint32_t e = 0; e < 3; ++e) {
        const uint32_t q = s_table.edge[t][m][3u * r + e];
        const uint32_t ca = s_table.corner[t][tet_edge_lo(q)], cb = s_table.corner[t][tet_edge_hi(q)];
        triangles[at * 3u + e] = edge_map[7u * (lin + corner_offset(l, ca)) + (cb - ca) - 1u];
      }
    }
  }
}

// The sections of the extraction's workspace.
struct MeshLayout {
  uint64_t table, mask, tri, edge, tri_sums, tri_offsets, edge_sums, edge_offsets, bytes;
  uint32_t tri_blocks, edge_blocks;
};

MeshLayout mesh_layout(uint64_t count) {
  MeshLayout m;
  WorkspaceOffsets o;
  m.tri_blocks = (uint32_t)((count + kScanTile - 1) / kScanTile);
  m.edge_blocks = (uint32_t)((7u * count + kScanTile - 1) / kScanTile);
  m.table = o.put(sizeof(TetTable));
  m.mask = o.put(count);
  m.tri = o.put(count * 4u);
  m.edge = o.put(count * 28u);
  m.tri_sums = o.put((uint64_t)m.tri_blocks * 4u);
  m.tri_offsets = o.put((uint64_t)m.tri_blocks * 8u);
  m.edge_sums = o.put((uint64_t)m.edge_blocks * 4u);
  m.edge_offsets = o.put((uint64_t)m.edge_blocks * 8u);
  m.bytes = o.bytes();
  return m;
}

Lattice lattice_of(const spz_amd_tsdf_volume *v) {
  return Lattice{v->dims[0], v->dims[1], v->dims[2], v->dims[0] * v->dims[1] * v->dims[2]};
}

// What the host form keeps until its close: the three output arrays in one allocation.
struct MeshResult {
  int device = 0;
  hipStream_t st = nullptr;
  uint8_t *out = nullptr;  // positions, colours, triangles
  uint8_t *grid = nullptr, *maps = nullptr, *scratch = nullptr, *ws = nullptr;  // freed before open returns
  uint64_t nv = 0, nt = 0, o_col = 0, o_tri = 0;
};

void mesh_result_free(MeshResult *r) {
  if (r == nullptr) return;
  int prev = -1;
  (void)hipGetDevice(&prev);
  (void)hipSetDevice(r->device);
  if (r->st) {
    (void)hipStreamSynchronize(r->st);
    (void)hipStreamDestroy(r->st);
  }
  for (uint8_t *p : {r->out, r->grid, r->maps, r->scratch, r->ws}) {
    if (p) (void)hipFree(p);
  }
  if (prev >= 0) (void)hipSetDevice(prev);
  delete r;
}

struct MeshResultFree {
  void operator()(MeshResult *r) const { mesh_result_free(r); }
};

}  // namespace
}  // namespace spz_amd_detail

using namespace spz_amd_detail;

extern "C" {

int spz_amd_tsdf_check(const spz_amd_tsdf_volume *v) {
  if (v == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  uint64_t count = 1;
  for (int a = 0; a < 3; ++a) {
    if (v->dims[a] < 2u || v->dims[a] > 2048u || !std::isfinite(v->lo[a])) return SPZ_AMD_ERR_INVALID_ARG;
    count *= v->dims[a];
  }
  if (count > kMaxLattice) return SPZ_AMD_ERR_INVALID_ARG;
  if (!(v->voxel_size > 0.0f) || !std::isfinite(v->voxel_size)) return SPZ_AMD_ERR_INVALID_ARG;
  if (!(v->truncation > 0.0f) || !std::isfinite(v->truncation)) return SPZ_AMD_ERR_INVALID_ARG;
  return SPZ_AMD_OK;
}

uint64_t spz_amd_tsdf_bytes(const spz_amd_tsdf_volume *v) {
  if (spz_amd_tsdf_check(v) != SPZ_AMD_OK) return 0;
  return 20ull * v->dims[0] * v->dims[1] * v->dims[2];
}

int spz_amd_tsdf_volume_from_box(const double lo[3], const double hi[3], double voxel_size, double truncation,
                                 spz_amd_tsdf_volume *out) {
  if (lo == nullptr || hi == nullptr || out == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  if (!(voxel_size > 0.0) || !std::isfinite(voxel_size) || !(truncation > 0.0) || !std::isfinite(truncation)) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  spz_amd_tsdf_volume v;
  std::memset(&v, 0, sizeof(v));
  for (int a = 0; a < 3; ++a) {
    if (!std::isfinite(lo[a]) || !std::isfinite(hi[a]) || !(hi[a] >= lo[a])) return SPZ_AMD_ERR_INVALID_ARG;
    const double d = std::floor((hi[a] - lo[a]) / voxel_size) + 2.0;
    if (!(d <= 2048.0)) return SPZ_AMD_ERR_INVALID_ARG;
    v.dims[a] = (uint32_t)d;
    v.lo[a] = (float)lo[a];
  }
  v.voxel_size = (float)voxel_size;
  v.truncation = (float)truncation;
  const int rc = spz_amd_tsdf_check(&v);
  if (rc != SPZ_AMD_OK) return rc;
  *out = v;
  return SPZ_AMD_OK;
}

int spz_amd_tsdf_integrate_device(const spz_amd_tsdf_volume *volume, float *d_grid, const spz_amd_render_params *params,
                                  const float *d_depth, const float *d_image, int depth_kind, float min_alpha,
                                  void *hip_stream) {
  int rc = spz_amd_tsdf_check(volume);
  if (rc != SPZ_AMD_OK) return rc;
  rc = spz_amd_render_check_params(params);
  if (rc != SPZ_AMD_OK) return rc;
  if (d_grid == nullptr || d_depth == nullptr || d_image == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  if (depth_kind != SPZ_AMD_MESH_DEPTH_MEDIAN && depth_kind != SPZ_AMD_MESH_DEPTH_EXPECTED) return SPZ_AMD_ERR_INVALID_ARG;
  if (!(min_alpha >= 0.0f) || !(min_alpha <= 1.0f)) return SPZ_AMD_ERR_INVALID_ARG;
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  const dim3 blocks((volume->dims[0] + 63u) / 64u, (volume->dims[1] + 3u) / 4u, volume->dims[2]);
  hipLaunchKernelGGL(spz_tsdf_integrate_kernel, blocks, dim3(64, 4, 1), 0, static_cast<hipStream_t>(hip_stream), *volume,
                     *params, d_depth, d_image, depth_kind == SPZ_AMD_MESH_DEPTH_EXPECTED ? 1 : 0, min_alpha, d_grid);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

int spz_amd_mesh_tet_table(uint8_t corners[24], uint8_t num_triangles[96], uint8_t edges[576]) {
  if (corners == nullptr || num_triangles == nullptr || edges == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  const TetTable &t = tet_table();
  std::memcpy(corners, t.corner, 24);
  std::memcpy(num_triangles, t.ntri, 96);
  std::memcpy(edges, t.edge, 576);
  return SPZ_AMD_OK;
}

uint64_t spz_amd_mesh_workspace_bytes(const spz_amd_tsdf_volume *volume) {
  if (spz_amd_tsdf_check(volume) != SPZ_AMD_OK) return 0;
  return mesh_layout((uint64_t)volume->dims[0] * volume->dims[1] * volume->dims[2]).bytes;
}

int spz_amd_mesh_count_device(const spz_amd_tsdf_volume *volume, const float *d_grid, float min_weight,
                              uint64_t *d_counts, void *d_workspace, void *hip_stream) {
  int rc = spz_amd_tsdf_check(volume);
  if (rc != SPZ_AMD_OK) return rc;
  if (d_grid == nullptr || d_counts == nullptr || d_workspace == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  if (!(min_weight > 0.0f) || !std::isfinite(min_weight)) return SPZ_AMD_ERR_INVALID_ARG;
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const Lattice l = lattice_of(volume);
  const MeshLayout m = mesh_layout(l.count);
  uint8_t *ws = align_ws(d_workspace);
  auto *d_table = reinterpret_cast<TetTable *>(ws + m.table);
  auto *d_tri = reinterpret_cast<uint32_t *>(ws + m.tri);
  auto *d_edge = reinterpret_cast<uint32_t *>(ws + m.edge);
  auto *d_counts64 = reinterpret_cast<unsigned long long *>(d_counts);
  SPZ_HIP_TRY(hipMemcpyAsync(d_table, &tet_table(), sizeof(TetTable), hipMemcpyHostToDevice, st));
  SPZ_HIP_TRY(hipMemsetAsync(d_edge, 0, (size_t)l.count * 28u, st));
  const unsigned blocks = (l.count + kMeshBlock - 1) / kMeshBlock;
  hipLaunchKernelGGL(spz_mesh_classify_kernel, dim3(blocks), dim3(kMeshBlock), 0, st, l, d_grid, min_weight, d_table,
                     ws + m.mask, d_tri, d_edge);
  SPZ_HIP_TRY(hipGetLastError());
  struct Scan {
    uint32_t *a;
    uint32_t n, blocks;
    uint64_t sums, offsets;
    unsigned long long *total;
    uint32_t to_vertex;
  };
  const Scan scans[2] = {{d_edge, 7u * l.count, m.edge_blocks, m.edge_sums, m.edge_offsets, d_counts64, 1u},
                         {d_tri, l.count, m.tri_blocks, m.tri_sums, m.tri_offsets, d_counts64 + 1, 0u}};
  for (const Scan &s : scans) {
    auto *sums = reinterpret_cast<uint32_t *>(ws + s.sums);
    auto *offsets = reinterpret_cast<unsigned long long *>(ws + s.offsets);
    hipLaunchKernelGGL(spz_mesh_scan_reduce_kernel, dim3(s.blocks), dim3(kMeshBlock), 0, st, s.a, s.n, sums);
    SPZ_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(spz_mesh_scan_sums_kernel, dim3(1), dim3(kMeshBlock), 0, st, sums, s.blocks, offsets, s.total);
    SPZ_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(spz_mesh_scan_apply_kernel, dim3(s.blocks), dim3(kMeshBlock), 0, st, s.a, s.n, offsets, s.to_vertex);
    SPZ_HIP_TRY(hipGetLastError());
  }
  return SPZ_AMD_OK;
}

int spz_amd_mesh_emit_device(const spz_amd_tsdf_volume *volume, const float *d_grid, uint64_t num_vertices,
                             uint64_t num_triangles, uint64_t vertex_capacity, uint64_t triangle_capacity,
                             float *d_positions, float *d_colors, uint32_t *d_triangles, const void *d_workspace,
                             void *hip_stream) {
  int rc = spz_amd_tsdf_check(volume);
  if (rc != SPZ_AMD_OK) return rc;
  if (d_grid == nullptr || d_workspace == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  const Lattice l = lattice_of(volume);
  if (num_vertices > 7ull * l.count || num_triangles > 12ull * l.count) return SPZ_AMD_ERR_INVALID_ARG;
  if (num_vertices && (d_positions == nullptr || d_colors == nullptr)) return SPZ_AMD_ERR_INVALID_ARG;
  if (num_triangles && d_triangles == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  if (vertex_capacity < num_vertices || triangle_capacity < num_triangles) return SPZ_AMD_ERR_CAPACITY;
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  if (num_vertices == 0 && num_triangles == 0) return SPZ_AMD_OK;
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  const MeshLayout m = mesh_layout(l.count);
  const uint8_t *ws = align_ws(const_cast<void *>(d_workspace));
  const auto *d_edge = reinterpret_cast<const uint32_t *>(ws + m.edge);
  if (num_vertices) {
    hipLaunchKernelGGL(spz_mesh_vertices_kernel, dim3((7u * l.count + kMeshBlock - 1) / kMeshBlock), dim3(kMeshBlock), 0,
                       st, *volume, l, d_grid, d_edge, (unsigned long long)num_vertices, d_positions, d_colors);
    SPZ_HIP_TRY(hipGetLastError());
  }
  if (num_triangles) {
    hipLaunchKernelGGL(spz_mesh_triangles_kernel, dim3((l.count + kMeshBlock - 1) / kMeshBlock), dim3(kMeshBlock), 0, st, l,
                       reinterpret_cast<const TetTable *>(ws + m.table), ws + m.mask,
                       reinterpret_cast<const uint32_t *>(ws + m.tri),
                       reinterpret_cast<const unsigned long long *>(ws + m.tri_offsets), d_edge,
                       (unsigned long long)num_triangles, d_triangles);
    SPZ_HIP_TRY(hipGetLastError());
  }
  return SPZ_AMD_OK;
}

int spz_amd_mesh_default_options(spz_amd_mesh_options *options) {
  if (options == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  std::memset(options, 0, sizeof(*options));
  options->resolution = 256;
  options->depth_kind = SPZ_AMD_MESH_DEPTH_MEDIAN;
  options->min_alpha = 0.5f;
  options->min_weight = 1.0f;
  return SPZ_AMD_OK;
}

int spz_amd_mesh_check(const spz_amd_mesh_options *o) {
  if (o == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  if (o->has_box) {
    for (int a = 0; a < 3; ++a) {
      if (!std::isfinite(o->box[a]) || !std::isfinite(o->box[3 + a]) || !(o->box[3 + a] > o->box[a])) {
        return SPZ_AMD_ERR_INVALID_ARG;
      }
    }
  }
  const bool by_size = o->voxel_size != 0.0, by_res = o->resolution != 0;
  if (by_size == by_res) return SPZ_AMD_ERR_INVALID_ARG;  // exactly one
  if (by_size && (!(o->voxel_size > 0.0) || !std::isfinite(o->voxel_size))) return SPZ_AMD_ERR_INVALID_ARG;
  if (by_res && (o->resolution < 1 || o->resolution > 2046)) return SPZ_AMD_ERR_INVALID_ARG;
  if (o->truncation != 0.0 && (!(o->truncation > 0.0) || !std::isfinite(o->truncation))) return SPZ_AMD_ERR_INVALID_ARG;
  if (o->depth_kind != SPZ_AMD_MESH_DEPTH_MEDIAN && o->depth_kind != SPZ_AMD_MESH_DEPTH_EXPECTED) return SPZ_AMD_ERR_INVALID_ARG;
  if (!(o->min_alpha >= 0.0f) || !(o->min_alpha <= 1.0f)) return SPZ_AMD_ERR_INVALID_ARG;
  if (!(o->min_weight > 0.0f) || !std::isfinite(o->min_weight)) return SPZ_AMD_ERR_INVALID_ARG;
  return SPZ_AMD_OK;
}

int spz_amd_mesh_open(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, const spz_amd_render_params *views,
                      int num_views, const spz_amd_mesh_options *options, int device, void **ctx, uint64_t *h_counts,
                      spz_amd_tsdf_volume *h_volume, float *h_ms, int32_t *h_bad_view) {
  if (h_bad_view) *h_bad_view = -1;
  if (ctx == nullptr || h_counts == nullptr || d_stream == nullptr || hdr == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  *ctx = nullptr;
  h_counts[0] = h_counts[1] = 0;
  int rc = spz_amd_mesh_check(options);
  if (rc != SPZ_AMD_OK) return rc;
  rc = check_views(views, num_views, SPZ_AMD_MESH_MAX_VIEWS, h_bad_view);
  if (rc != SPZ_AMD_OK) return rc;
  rc = check_render_input(d_stream, size, hdr);
  if (rc != SPZ_AMD_OK) return rc;
  const uint64_t n = hdr->num_points;
  DeviceGuard guard;
  rc = guard.enter(device);
  if (rc != SPZ_AMD_OK) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  std::unique_ptr<MeshResult, MeshResultFree> c(new MeshResult);
  c->device = device;
  SPZ_HIP_TRY(hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking));

  // the maps of the largest view, the small values, the box keys
  uint64_t pixels = 0;
  for (int v = 0; v < num_views; ++v) {
    const uint64_t px = (uint64_t)views[v].width * views[v].height;
    pixels = px > pixels ? px : pixels;
  }
  WorkspaceOffsets o;
  const uint64_t o_image = o.put(16u * pixels), o_depth = o.put(8u * pixels), o_small = o.put(64u);
  SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&c->maps), o.off));
  auto *d_image = reinterpret_cast<float *>(c->maps + o_image);
  auto *d_depth = reinterpret_cast<float *>(c->maps + o_depth);
  auto *d_total = reinterpret_cast<uint64_t *>(c->maps + o_small);
  auto *d_status = reinterpret_cast<uint32_t *>(c->maps + o_small + 8u);
  auto *d_counts = reinterpret_cast<uint64_t *>(c->maps + o_small + 16u);
  auto *d_keys = reinterpret_cast<uint32_t *>(c->maps + o_small + 32u);

  // the volume
  double lo[3], hi[3];
  if (options->has_box) {
    for (int a = 0; a < 3; ++a) {
      lo[a] = options->box[a];
      hi[a] = options->box[3 + a];
    }
  } else {
    spz_amd_layout lay;
    (void)spz_amd_stream_layout(hdr->num_points, hdr->sh_degree, (int)hdr->version, &lay);
    uint32_t keys[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u};
    if (n) {
      SPZ_HIP_TRY(hipMemcpyAsync(d_keys, keys, sizeof(keys), hipMemcpyHostToDevice, c->st));
      const uint64_t want = (n + kMeshBlock - 1) / kMeshBlock;
      hipLaunchKernelGGL(spz_mesh_bounds_kernel, dim3((unsigned)(want < 4096u ? want : 4096u)), dim3(kMeshBlock), 0, c->st,
                         d_stream + lay.offset[SPZ_AMD_SEC_POSITIONS], (uint32_t)n, hdr->version == 1u ? 1u : 0u,
                         (float)(1.0 / (double)(int32_t)(1u << (hdr->fractional_bits & 31))),
                         flip_masks(SPZ_AMD_RUB, views[0].coord).p, d_keys);
      SPZ_HIP_TRY(hipGetLastError());
      SPZ_HIP_TRY(hipMemcpyAsync(keys, d_keys, sizeof(keys), hipMemcpyDeviceToHost, c->st));
      SPZ_HIP_TRY(hipStreamSynchronize(c->st));
    }
    for (int a = 0; a < 3; ++a) {
      if (keys[a] > keys[3 + a]) return SPZ_AMD_ERR_INVALID_ARG;  // no finite position: no box
      lo[a] = (double)order_key_value(keys[a]);
      hi[a] = (double)order_key_value(keys[3 + a]);
    }
  }
  double voxel = options->voxel_size;
  if (options->resolution) {
    double longest = 0.0;
    for (int a = 0; a < 3; ++a) longest = hi[a] - lo[a] > longest ? hi[a] - lo[a] : longest;
    voxel = longest / (double)options->resolution;
  }
  spz_amd_tsdf_volume vol;
  rc = spz_amd_tsdf_volume_from_box(lo, hi, voxel, options->truncation != 0.0 ? options->truncation : 4.0 * voxel, &vol);
  if (rc != SPZ_AMD_OK) return rc;
  if (h_volume) *h_volume = vol;
  const uint64_t grid_bytes = spz_amd_tsdf_bytes(&vol);
  SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&c->grid), grid_bytes));
  SPZ_HIP_TRY(hipMemsetAsync(c->grid, 0, grid_bytes, c->st));
  auto *d_grid = reinterpret_cast<float *>(c->grid);

  // the views: prepare, the depth blend, the fuse
  const RenderSource src = packed_render_source(d_stream, size, hdr);
  uint64_t cap = 0, total = 0;
  double render_ms = 0.0, fuse_ms = 0.0;
  for (int v = 0; v < num_views; ++v) {
    const double a0 = ms_since(t0);
    rc = prepare_view(&c->scratch, &cap, src, &views[v], d_total, c->st, &total);
    if (rc == SPZ_AMD_OK) {
      rc = spz_amd_render_depth_device(n, &views[v], total, d_image, d_depth, nullptr, d_status, c->scratch, c->st);
    }
    if (rc == SPZ_AMD_OK && hipStreamSynchronize(c->st) != hipSuccess) rc = SPZ_AMD_ERR_HIP;
    const double a1 = ms_since(t0);
    if (rc == SPZ_AMD_OK) {
      rc = spz_amd_tsdf_integrate_device(&vol, d_grid, &views[v], d_depth, d_image, options->depth_kind,
                                         options->min_alpha, c->st);
    }
    if (rc == SPZ_AMD_OK && hipStreamSynchronize(c->st) != hipSuccess) rc = SPZ_AMD_ERR_HIP;
    if (rc != SPZ_AMD_OK) {
      if (h_bad_view) *h_bad_view = v;
      return rc;
    }
    render_ms += a1 - a0;
    fuse_ms += ms_since(t0) - a1;
  }
  SPZ_HIP_TRY(hipFree(c->scratch));
  c->scratch = nullptr;

  // the level set
  const double e0 = ms_since(t0);
  SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&c->ws), spz_amd_mesh_workspace_bytes(&vol)));
  rc = spz_amd_mesh_count_device(&vol, d_grid, options->min_weight, d_counts, c->ws, c->st);
  if (rc != SPZ_AMD_OK) return rc;
  uint64_t counts[2] = {0, 0};
  SPZ_HIP_TRY(hipMemcpyAsync(counts, d_counts, sizeof(counts), hipMemcpyDeviceToHost, c->st));
  SPZ_HIP_TRY(hipStreamSynchronize(c->st));
  if (counts[0] > 0xffffffffull) return SPZ_AMD_ERR_CAPACITY;  // vertex numbers are u32
  WorkspaceOffsets oo;
  (void)oo.put(counts[0] * 12u);
  c->o_col = oo.put(counts[0] * 12u);
  c->o_tri = oo.put(counts[1] * 12u);
  SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&c->out), oo.off + 256u));
  rc = spz_amd_mesh_emit_device(&vol, d_grid, counts[0], counts[1], counts[0], counts[1],
                                reinterpret_cast<float *>(c->out), reinterpret_cast<float *>(c->out + c->o_col),
                                reinterpret_cast<uint32_t *>(c->out + c->o_tri), c->ws, c->st);
  if (rc != SPZ_AMD_OK) return rc;
  SPZ_HIP_TRY(hipStreamSynchronize(c->st));
  for (uint8_t **p : {&c->grid, &c->maps, &c->ws}) {
    SPZ_HIP_TRY(hipFree(*p));
    *p = nullptr;
  }
  c->nv = counts[0];
  c->nt = counts[1];
  h_counts[0] = counts[0];
  h_counts[1] = counts[1];
  if (h_ms) {
    h_ms[0] = (float)render_ms;
    h_ms[1] = (float)fuse_ms;
    h_ms[2] = (float)(ms_since(t0) - e0);
  }
  *ctx = c.release();
  return SPZ_AMD_OK;
}

int spz_amd_mesh_fetch(void *ctx, float *h_positions, float *h_colors, uint32_t *h_triangles) {
  MeshResult *r = static_cast<MeshResult *>(ctx);
  if (r == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  if (r->nv && (h_positions == nullptr || h_colors == nullptr)) return SPZ_AMD_ERR_INVALID_ARG;
  if (r->nt && h_triangles == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  DeviceGuard guard;
  const int rc = guard.enter(r->device);
  if (rc != SPZ_AMD_OK) return rc;
  if (r->nv) {
    SPZ_HIP_TRY(hipMemcpyAsync(h_positions, r->out, r->nv * 12u, hipMemcpyDeviceToHost, r->st));
    SPZ_HIP_TRY(hipMemcpyAsync(h_colors, r->out + r->o_col, r->nv * 12u, hipMemcpyDeviceToHost, r->st));
  }
  if (r->nt) SPZ_HIP_TRY(hipMemcpyAsync(h_triangles, r->out + r->o_tri, r->nt * 12u, hipMemcpyDeviceToHost, r->st));
  SPZ_HIP_TRY(hipStreamSynchronize(r->st));
  return SPZ_AMD_OK;
}

void spz_amd_mesh_close(void *ctx) { mesh_result_free(static_cast<MeshResult *>(ctx)); }

}  // extern "C"
