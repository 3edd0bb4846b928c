// spz_filter.hip — a smaller .spz out of a packed stream without requantising (DESIGN §8 "filter"): point selection
// and the subset of the six sections, both byte transforms on a stream that stays in HBM.
//
//   spz_select_kernel       one pass over the position / alpha / mask bytes.  A point's predicates use the decode's own
//                           device code (decode_position_axis, the 256-entry alpha table of spz_decode_gather_kernel) and
//                           compare the decoded float; each wave keeps its __ballot word (1 bit per point) and a tile's
//                           count goes through LDS.
//   spz_select_scan_kernel  one workgroup: exclusive scan of the tile counts, the total.
//   spz_compact_kernel      each tile writes the indices of its set bits at its offset, in point order.  Two passes
//                           with a scan between them: no inter-workgroup flags, no atomics, a deterministic order.
//   spz_subset_kernel       the K-point stream: header + six sections, point k = input point idx[k] with its bytes
//                           (sh: the first 3 * dim(d') of them).  A flat tile list over the OUTPUT sections, one output
//                           dword per thread and unit: lane-contiguous stores, gathered byte loads.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "spz_amd.h"
#include "spz_block_ops.hpp"
#include "spz_common.hpp"
#include "spz_kernel_params.hpp"

namespace spz_amd_detail {
namespace {

constexpr uint32_t kSelBlock = 256;
constexpr uint32_t kSelRounds = 4;
constexpr uint32_t kSelTile = kSelBlock * kSelRounds;       // points per tile
constexpr uint32_t kSelWordsPerTile = kSelTile / 64u;       // ballot words per tile
constexpr uint32_t kScanBlock = 1024;
constexpr uint32_t kSubBlock = 256;
constexpr uint32_t kSubUnroll = 4;
constexpr uint32_t kSubTileBytes = kSubBlock * kSubUnroll * 4u;
constexpr uint32_t kMagic = 0x5053474eu;  // load-spz.cc:132

typedef uint32_t u32_a1 __attribute__((aligned(1)));

struct SelectParams {
  const uint8_t *positions, *alphas, *mask;  // mask: nullptr = none
  const float *tables;
  unsigned long long *words;                 // [tiles * kSelWordsPerTile]
  uint32_t *tile_counts;                     // [tiles]
  uint32_t num_points;
  uint32_t float16;                          // version 1
  uint32_t flip_p;
  float pos_scale;
  uint32_t use_box, use_alpha;
  float lo[3], hi[3];
  float min_alpha;
};

struct CompactParams {
  const unsigned long long *words;
  const uint32_t *tile_offsets;
  uint32_t *indices;
};

struct SubsetSec {
  const uint8_t *src;           // input section base
  uint8_t *dst;                 // output section base
  unsigned long long bytes;     // output bytes of the section
  uint32_t in_bpp, out_bpp;     // bytes per point in and out (sh: out is a prefix of in)
  uint32_t tile_begin;
};

struct SubsetParams {
  SubsetSec sec[SPZ_AMD_NUM_SECTIONS];
  uint32_t n_sec;
  uint32_t total_tiles;
  const uint32_t *indices;
  uint32_t num_points;          // of the input (indices are clamped to num_points - 1)
  uint8_t *header_dst;
  uint32_t header_words[4];
};

}  // namespace

__global__ __launch_bounds__(kSelBlock) void spz_select_kernel(const SelectParams p) {
  __shared__ uint32_t wave_count[kSelBlock / 64u];
  const uint32_t tile = blockIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t count = 0;
#pragma unroll
  for (uint32_t r = 0; r < kSelRounds; ++r) {
    const unsigned long long i = (unsigned long long)tile * kSelTile + r * kSelBlock + threadIdx.x;
    bool keep = i < p.num_points;
    if (keep && p.mask != nullptr) keep = p.mask[i] != 0;
    if (keep && p.use_alpha) keep = p.tables[kTableAlphaDec + p.alphas[i]] >= p.min_alpha;
    if (keep && p.use_box) {
      for (uint32_t a = 0; a < 3; ++a) {
        const float v = decode_position_axis(p.positions, i, a, p.float16 != 0, p.pos_scale, p.flip_p);
        keep = keep && (p.lo[a] <= v) && (v <= p.hi[a]);  // NaN: false
      }
    }
    const unsigned long long bits = __ballot(keep);
    if (lane == 0) p.words[(unsigned long long)tile * kSelWordsPerTile + r * (kSelBlock / 64u) + wave] = bits;
    count += (uint32_t)__popcll(bits);
  }
  if (lane == 0) wave_count[wave] = count;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (uint32_t w = 0; w < kSelBlock / 64u; ++w) s += wave_count[w];
    p.tile_counts[tile] = s;
  }
}

// counts[0 .. tiles) -> exclusive offsets in place; *total = their sum.  One workgroup: thread t owns a contiguous run
// of ceil(tiles / 1024) counts (10 for 10 M points).
__global__ __launch_bounds__(kScanBlock) void spz_select_scan_kernel(uint32_t *counts, uint32_t tiles,
                                                                     unsigned long long *total) {
  __shared__ uint32_t part[kScanBlock];
  const uint32_t sum = block_scan_owned_runs<uint32_t, kScanBlock>(
      tiles, part, [&](uint32_t k) { return counts[k]; }, [&](uint32_t k, uint32_t before) { counts[k] = before; });
  if (threadIdx.x == 0) *total = sum;
}

__global__ __launch_bounds__(kSelBlock) void spz_compact_kernel(const CompactParams p) {
  __shared__ unsigned long long w[kSelWordsPerTile];
  __shared__ uint32_t pre[kSelWordsPerTile];
  const uint32_t tile = blockIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (threadIdx.x < kSelWordsPerTile) w[threadIdx.x] = p.words[(unsigned long long)tile * kSelWordsPerTile + threadIdx.x];
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = p.tile_offsets[tile];
    for (uint32_t j = 0; j < kSelWordsPerTile; ++j) {
      pre[j] = run;
      run += (uint32_t)__popcll(w[j]);
    }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t r = 0; r < kSelRounds; ++r) {
    const uint32_t j = r * (kSelBlock / 64u) + wave;
    const unsigned long long bits = w[j];
    if ((bits >> lane) & 1ull) {
      const uint32_t rank = pre[j] + (uint32_t)__popcll(bits & ((1ull << lane) - 1ull));
      p.indices[rank] = tile * kSelTile + j * 64u + lane;
    }
  }
}

namespace {

// One output dword (or the 1..3 bytes of a section's last one) of section q: byte b of the section is byte b % out_bpp
// of output point b / out_bpp, i.e. of input point idx[b / out_bpp].  IDX: 32-bit while the section's byte count fits.
template <class IDX>
__device__ __forceinline__ void subset_unit(const SubsetParams &p, const SubsetSec &q, unsigned long long b0) {
  const IDX bytes = (IDX)q.bytes;
  const IDX first = (IDX)b0;
  const uint32_t n = (bytes - first) < (IDX)4 ? (uint32_t)(bytes - first) : 4u;
  IDX k = first / (IDX)q.out_bpp;
  uint32_t w = (uint32_t)(first - k * (IDX)q.out_bpp);
  uint32_t i = p.indices[k];
  i = i < p.num_points ? i : p.num_points - 1u;
  uint32_t word = 0;
  for (uint32_t j = 0; j < n; ++j) {
    word |= (uint32_t)q.src[(unsigned long long)i * q.in_bpp + w] << (8u * j);
    if (++w == q.out_bpp && j + 1 < n) {
      w = 0;
      ++k;
      i = p.indices[k];
      i = i < p.num_points ? i : p.num_points - 1u;
    }
  }
  uint8_t *d = q.dst + b0;
  if (n == 4u) {
    *reinterpret_cast<u32_a1 *>(d) = word;  // unaligned dword store (section bases land on any byte)
  } else {
    for (uint32_t j = 0; j < n; ++j) d[j] = (uint8_t)(word >> (8u * j));
  }
}

}  // namespace

__global__ __launch_bounds__(kSubBlock) void spz_subset_kernel(const SubsetParams p) {
  const uint32_t tile = blockIdx.x;
  if (tile == 0 && threadIdx.x < 16 && p.header_dst != nullptr) {
    p.header_dst[threadIdx.x] = (uint8_t)(p.header_words[threadIdx.x >> 2] >> ((threadIdx.x & 3u) * 8u));
  }
  if (tile >= p.total_tiles) return;
  uint32_t si = 0;
  for (uint32_t s = 1; s < p.n_sec; ++s) si = (tile >= p.sec[s].tile_begin) ? s : si;
  const SubsetSec &q = p.sec[si];
  const unsigned long long base = (unsigned long long)(tile - q.tile_begin) * kSubTileBytes;
#pragma unroll
  for (uint32_t r = 0; r < kSubUnroll; ++r) {
    const unsigned long long b0 = base + ((unsigned long long)r * kSubBlock + threadIdx.x) * 4ull;
    if (b0 >= q.bytes) break;
    if (q.bytes <= 0xffffffffull) subset_unit<uint32_t>(p, q, b0);
    else subset_unit<unsigned long long>(p, q, b0);
  }
}

}  // namespace spz_amd_detail

namespace {

using namespace spz_amd_detail;

struct WorkspaceLayout {
  uint64_t tiles, words_off, counts_off, total_off, bytes;
};

WorkspaceLayout workspace_layout(uint64_t num_points) {
  WorkspaceLayout w;
  w.tiles = (num_points + kSelTile - 1) / kSelTile;
  w.words_off = 0;
  w.counts_off = Workspace::aligned(w.tiles * kSelWordsPerTile * 8u);
  w.total_off = w.counts_off + Workspace::aligned(w.tiles * 4u);
  w.bytes = w.total_off + 256 + 256;  // the total, and room to align a caller's pointer up to 256
  return w;
}

bool sh_prefix_degree(int sh_degree, int in_degree, int *out_degree) {
  if (sh_degree == -1) {
    *out_degree = in_degree;
    return true;
  }
  if (sh_degree < 0 || sh_degree > in_degree) return false;
  *out_degree = sh_degree;
  return true;
}

int select_impl(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, const spz_amd_selection *sel,
                const uint8_t *d_mask, uint32_t *d_indices, void *d_workspace, uint64_t *h_count, void *hip_stream) {
  if (h_count == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  *h_count = 0;
  spz_amd_layout lay;
  int rc = check_packed_stream(d_stream, size, hdr, &lay);
  if (rc != SPZ_AMD_OK) return rc;
  SelectParams p = {};
  if (sel != nullptr) {
    if (!valid_coord(sel->to_coord)) return SPZ_AMD_ERR_INVALID_ARG;
    if (sel->use_box) {
      for (int a = 0; a < 3; ++a) {
        if (std::isnan(sel->box_lo[a]) || std::isnan(sel->box_hi[a])) return SPZ_AMD_ERR_INVALID_ARG;
        p.lo[a] = sel->box_lo[a];
        p.hi[a] = sel->box_hi[a];
      }
      p.use_box = 1;
    }
    if (sel->use_min_alpha) {
      if (std::isnan(sel->min_alpha)) return SPZ_AMD_ERR_INVALID_ARG;
      p.min_alpha = sel->min_alpha;
      p.use_alpha = 1;
    }
  }
  const uint64_t n = hdr->num_points;
  if (n == 0) return SPZ_AMD_OK;
  if (d_indices == nullptr || d_workspace == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  rc = ensure_tables(device, &p.tables);
  if (rc != SPZ_AMD_OK) return rc;
  const WorkspaceLayout wl = workspace_layout(n);
  uint8_t *ws = align_ws(d_workspace);
  p.positions = d_stream + lay.offset[SPZ_AMD_SEC_POSITIONS];
  p.alphas = d_stream + lay.offset[SPZ_AMD_SEC_ALPHAS];
  p.mask = d_mask;
  p.words = reinterpret_cast<unsigned long long *>(ws + wl.words_off);
  p.tile_counts = reinterpret_cast<uint32_t *>(ws + wl.counts_off);
  p.num_points = (uint32_t)n;
  p.float16 = hdr->version == 1 ? 1u : 0u;
  p.flip_p = flip_masks(SPZ_AMD_RUB, sel ? sel->to_coord : SPZ_AMD_UNSPECIFIED).p;  // load-spz.cc:529
  // float scale = 1.0 / (1 << fractionalBits) (load-spz.cc:495); x86 masks the shift count to 5 bits
  p.pos_scale = (float)(1.0 / (double)(int32_t)(1u << (hdr->fractional_bits & 31)));
  unsigned long long *total = reinterpret_cast<unsigned long long *>(ws + wl.total_off);
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  hipLaunchKernelGGL(spz_select_kernel, dim3((unsigned)wl.tiles), dim3(kSelBlock), 0, st, p);
  SPZ_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(spz_select_scan_kernel, dim3(1), dim3(kScanBlock), 0, st, p.tile_counts, (uint32_t)wl.tiles, total);
  SPZ_HIP_TRY(hipGetLastError());
  CompactParams c = {p.words, p.tile_counts, d_indices};
  hipLaunchKernelGGL(spz_compact_kernel, dim3((unsigned)wl.tiles), dim3(kSelBlock), 0, st, c);
  SPZ_HIP_TRY(hipGetLastError());
  unsigned long long h = 0;
  SPZ_HIP_TRY(hipMemcpyAsync(&h, total, sizeof(h), hipMemcpyDeviceToHost, st));
  SPZ_HIP_TRY(hipStreamSynchronize(st));
  *h_count = h;
  return SPZ_AMD_OK;
}

int subset_impl(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, const uint32_t *d_indices,
                uint64_t count, int sh_degree, uint8_t *d_out, size_t capacity, void *hip_stream) {
  spz_amd_layout in;
  int rc = check_packed_stream(d_stream, size, hdr, &in);
  if (rc != SPZ_AMD_OK) return rc;
  int out_degree = 0;
  if (!sh_prefix_degree(sh_degree, hdr->sh_degree, &out_degree)) return SPZ_AMD_ERR_INVALID_ARG;
  if (count > 0xffffffffull || d_out == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  if (count > 0 && (d_indices == nullptr || hdr->num_points == 0)) return SPZ_AMD_ERR_INVALID_ARG;
  spz_amd_layout out;
  rc = spz_amd_stream_layout(count, out_degree, (int)hdr->version, &out);
  if (rc != SPZ_AMD_OK) return rc;
  if (capacity < out.total_bytes) return SPZ_AMD_ERR_CAPACITY;
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  SubsetParams p = {};
  p.indices = d_indices;
  p.num_points = hdr->num_points;
  // largest sections first, so that the tail of the grid is made of the small ones
  const int order[SPZ_AMD_NUM_SECTIONS] = {SPZ_AMD_SEC_SH, SPZ_AMD_SEC_POSITIONS, SPZ_AMD_SEC_ROTATIONS,
                                           SPZ_AMD_SEC_SCALES, SPZ_AMD_SEC_COLORS, SPZ_AMD_SEC_ALPHAS};
  unsigned long long tiles = 0;
  for (int s : order) {
    if (out.bytes[s] == 0) continue;
    SubsetSec &q = p.sec[p.n_sec++];
    q.src = d_stream + in.offset[s];
    q.dst = d_out + out.offset[s];
    q.bytes = out.bytes[s];
    q.in_bpp = in.bytes_per_point[s];
    q.out_bpp = out.bytes_per_point[s];
    q.tile_begin = (uint32_t)tiles;
    tiles += (out.bytes[s] + kSubTileBytes - 1) / kSubTileBytes;
  }
  if (tiles > 0x7fffffffull) return SPZ_AMD_ERR_INVALID_ARG;
  p.total_tiles = (uint32_t)tiles;
  // PackedGaussiansHeader (load-spz.cc:131-139): the input's version, fractionalBits and antialiased flag
  p.header_dst = d_out;
  p.header_words[0] = kMagic;
  p.header_words[1] = hdr->version;
  p.header_words[2] = (uint32_t)count;
  p.header_words[3] = (uint32_t)out_degree | ((uint32_t)hdr->fractional_bits << 8) | ((uint32_t)(hdr->flags & 1u) << 16);
  hipLaunchKernelGGL(spz_subset_kernel, dim3(p.total_tiles > 0 ? p.total_tiles : 1u), dim3(kSubBlock), 0,
                     static_cast<hipStream_t>(hip_stream), p);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

}  // namespace

int spz_amd_detail::select_subset_masked(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr,
                                         const uint8_t *d_mask, uint32_t *d_idx, void *d_fws, PackedResult *r,
                                         uint64_t *kept) {
  *kept = 0;
  int rc = select_impl(d_stream, size, hdr, nullptr, hdr->num_points ? d_mask : nullptr, d_idx, d_fws, kept, r->st);
  if (rc != SPZ_AMD_OK) return rc;
  spz_amd_layout ol;
  rc = spz_amd_stream_layout(*kept, hdr->sh_degree, (int)hdr->version, &ol);
  if (rc != SPZ_AMD_OK) return rc;
  r->out_bytes = ol.total_bytes;
  SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&r->out_block), r->out_bytes));
  r->out = r->out_block;
  return subset_impl(d_stream, size, hdr, d_idx, *kept, -1, r->out, r->out_bytes, r->st);
}

extern "C" {

uint64_t spz_amd_filter_workspace_bytes(uint64_t num_points) { return workspace_layout(num_points).bytes; }

int spz_amd_select_device(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, const spz_amd_selection *sel,
                          const uint8_t *d_mask, uint32_t *d_indices, void *d_workspace, uint64_t *h_count,
                          void *hip_stream) {
  return select_impl(d_stream, size, hdr, sel, d_mask, d_indices, d_workspace, h_count, hip_stream);
}

int spz_amd_subset_device(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, const uint32_t *d_indices,
                          uint64_t count, int sh_degree, uint8_t *d_out, size_t capacity, void *hip_stream) {
  return subset_impl(d_stream, size, hdr, d_indices, count, sh_degree, d_out, capacity, hip_stream);
}

int spz_amd_filter_open(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, const spz_amd_selection *sel,
                        const uint8_t *h_mask, int use_indices, const uint32_t *h_indices, uint64_t num_indices,
                        int sh_degree, int device, void **ctx, uint64_t *h_count, uint64_t *h_out_bytes, float *h_ms) {
  if (ctx == nullptr || h_count == nullptr || h_out_bytes == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  *ctx = nullptr;
  *h_count = 0;
  *h_out_bytes = 0;
  spz_amd_layout in;
  int rc = check_packed_stream(d_stream, size, hdr, &in);
  if (rc != SPZ_AMD_OK) return rc;
  int out_degree = 0;
  if (!sh_prefix_degree(sh_degree, hdr->sh_degree, &out_degree)) return SPZ_AMD_ERR_INVALID_ARG;
  const uint64_t n = hdr->num_points;
  if (use_indices) {
    const bool predicates = sel != nullptr && (sel->use_box || sel->use_min_alpha);
    if (h_mask != nullptr || predicates || num_indices > 0xffffffffull || (num_indices > 0 && h_indices == nullptr)) {
      return SPZ_AMD_ERR_INVALID_ARG;
    }
    for (uint64_t k = 0; k < num_indices; ++k) {
      if (h_indices[k] >= n) return SPZ_AMD_ERR_INVALID_ARG;  // rejected before anything is copied
    }
  }
  DeviceGuard guard;
  rc = guard.enter(device);
  if (rc != SPZ_AMD_OK) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  PackedResultPtr c;
  rc = packed_result_open(device, &c);
  if (rc != SPZ_AMD_OK) return rc;
  const uint64_t idx_cap = use_indices ? num_indices : n;
  const WorkspaceLayout wl = workspace_layout(n);
  const uint64_t mask_bytes = (!use_indices && h_mask != nullptr) ? n : 0;
  // the output's size is known once the count is: allocate for the most it can be (idx_cap points)
  spz_amd_layout most;
  rc = spz_amd_stream_layout(idx_cap, out_degree, (int)hdr->version, &most);
  if (rc != SPZ_AMD_OK) return rc;
  const size_t total = Workspace::aligned(idx_cap * 4u) + Workspace::aligned(mask_bytes) +
                       (use_indices ? 0 : Workspace::aligned(wl.bytes)) + Workspace::aligned(most.total_bytes);
  SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&c->block), total));
  uint8_t *q = c->block;
  uint32_t *d_idx = reinterpret_cast<uint32_t *>(q);
  q += Workspace::aligned(idx_cap * 4u);
  uint8_t *d_mask = mask_bytes ? q : nullptr;
  q += Workspace::aligned(mask_bytes);
  void *d_ws = use_indices ? nullptr : q;
  q += use_indices ? 0 : Workspace::aligned(wl.bytes);
  c->out = q;
  uint64_t count = 0;
  if (use_indices) {
    if (num_indices) SPZ_HIP_TRY(hipMemcpyAsync(d_idx, h_indices, num_indices * 4u, hipMemcpyHostToDevice, c->st));
    count = num_indices;
  } else {
    if (mask_bytes) SPZ_HIP_TRY(hipMemcpyAsync(d_mask, h_mask, mask_bytes, hipMemcpyHostToDevice, c->st));
    rc = select_impl(d_stream, size, hdr, sel, d_mask, d_idx, d_ws, &count, c->st);
    if (rc != SPZ_AMD_OK) return rc;
  }
  SPZ_HIP_TRY(hipStreamSynchronize(c->st));
  const double select_ms = ms_since(t0);
  spz_amd_layout out;
  rc = spz_amd_stream_layout(count, out_degree, (int)hdr->version, &out);
  if (rc != SPZ_AMD_OK) return rc;
  rc = subset_impl(d_stream, size, hdr, d_idx, count, sh_degree, c->out, out.total_bytes, c->st);
  if (rc != SPZ_AMD_OK) return rc;
  SPZ_HIP_TRY(hipStreamSynchronize(c->st));
  if (h_ms) {
    h_ms[0] = (float)select_ms;
    h_ms[1] = (float)(ms_since(t0) - select_ms);
  }
  c->out_bytes = out.total_bytes;
  *h_count = count;
  *h_out_bytes = out.total_bytes;
  *ctx = c.release();
  return SPZ_AMD_OK;
}

int spz_amd_filter_fetch(void *ctx, uint8_t *h_out) { return packed_result_fetch(ctx, h_out); }

const uint8_t *spz_amd_filter_device_data(void *ctx) { return packed_result_device_data(ctx); }

void spz_amd_filter_close(void *ctx) { packed_result_close(ctx); }

}  // extern "C"
