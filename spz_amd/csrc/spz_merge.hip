// spz_merge.hip — K packed streams -> one v3 stream (DESIGN "Merge").  Output point order: input 0's points, then
// input 1's, and so on.  Each (output section, input) slice is copied byte for byte unless the input's encoding or its
// placement forces a change; then it is decoded with the decoder's code, placed and re-encoded with the encoder's
// (spz_xf.hpp, the transform's per-point cores):
//
//   alphas, colours  copied
//   scales           copied, or + ln s per byte when the placement scales
//   positions        copied when v2/v3 at the output's fractionalBits and not moved, else decode -> place -> encode
//   rotations        copied when v3 and not rotated, else decode (first three / smallest three) -> q_R * q -> encode
//   sh               records cut or padded (byte 128 = 0.0) to the output degree; rotated at the input's degree and
//                    re-quantised first when the placement rotates
//
// One launch of spz_merge_kernel writes the header and every slice.  The grid is a flat tile list over the slices,
// largest sections first; the slice descriptors and the placement blocks lie in a device table in the caller's
// workspace (K = 1024 inputs do not fit in kernel arguments), and each block finds its slice by binary search over the
// slices' first tiles.  Copy tiles move 16-byte chunks aligned on the destination; the source side is read with
// dword-aligned or unaligned dword loads, whichever the slice's relative alignment allows.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "spz_amd.h"
#include "spz_common.hpp"
#include "spz_kernel_params.hpp"
#include "spz_quant.hpp"
#include "spz_xf.hpp"

#pragma clang fp contract(off)

namespace spz_amd_detail {
namespace {

constexpr uint32_t kMgBlock = 256;                 // threads; point tiles hold one point per thread
constexpr uint32_t kChunk = 16;                    // bytes per lane and step of a copy tile
constexpr uint32_t kCopyUnroll = 4;
constexpr uint32_t kCopyTileChunks = kMgBlock * kCopyUnroll;
constexpr uint32_t kMaxShBytes = 45;               // 3 * 15 at degree 3
constexpr uint32_t kMagic = 0x5053474eu;           // load-spz.cc:132

enum MergeKind : uint32_t { MG_COPY = 0, MG_SCALE, MG_POS, MG_ROT, MG_SH };

// One (output section, input) slice.
struct MergeSeg {
  const uint8_t *src;
  uint8_t *dst;
  unsigned long long bytes;   // output bytes of the slice
  uint32_t kind;
  uint32_t num_points;        // of the input
  uint32_t version;           // of the input
  float in_pos_scale;         // 1 / (1 << input fractionalBits)
  int32_t xf;                 // slot in the placement table, -1: none
  uint32_t in_rec, out_rec;   // sh record bytes of the input and of the output
  uint32_t pad;
};

// The device table: slices, their first tiles (the binary search's keys, apart so that they pack densely), placements.
struct TableLayout {
  size_t segs, tiles, xfs, bytes;
};
TableLayout table_layout(uint64_t k) {
  TableLayout t;
  const size_t n_seg = (size_t)k * SPZ_AMD_NUM_SECTIONS;
  t.segs = 0;
  t.tiles = Workspace::aligned(n_seg * sizeof(MergeSeg));
  t.xfs = t.tiles + Workspace::aligned(n_seg * sizeof(uint32_t));
  t.bytes = t.xfs + Workspace::aligned((size_t)k * sizeof(spz_amd_transform));
  return t;
}

struct MergeParams {
  const MergeSeg *segs;
  const uint32_t *tile_begin;
  const spz_amd_transform *xfs;
  uint32_t n_seg;
  uint32_t total_tiles;
  float out_pos_scale;        // 1 << fractional_bits of the output
  unsigned long long *out_of_range;
  uint8_t *header_dst;
  uint32_t header_words[4];
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_a4 __attribute__((aligned(4)));

// 16-byte chunks on the destination's 16-byte grid; the first and last chunk of a slice may be partial.
__device__ __forceinline__ void copy_tile(const MergeSeg &s, uint32_t tl, const spz_amd_transform *x) {
  const uint32_t lead = (uint32_t)((uintptr_t)s.dst & (kChunk - 1u));
  const bool dword_src = (((uintptr_t)s.src - (uintptr_t)s.dst) & 3u) == 0u;
  const bool scale = s.kind == MG_SCALE;
  const float ln_s = scale ? x->ln_s : 0.0f;
#pragma unroll
  for (uint32_t r = 0; r < kCopyUnroll; ++r) {
    const unsigned long long c = (unsigned long long)tl * kCopyTileChunks + r * kMgBlock + threadIdx.x;
    const long long lo = (long long)(c * kChunk) - (long long)lead;   // output offset of the chunk's first byte
    if (lo >= (long long)s.bytes) break;
    if (lo >= 0 && (unsigned long long)lo + kChunk <= s.bytes) {
      u32x4 w;
      if (dword_src) {
        w = *reinterpret_cast<const u32x4_a4 *>(s.src + lo);
      } else {
        const u32_a1 *p = reinterpret_cast<const u32_a1 *>(s.src + lo);
        w = u32x4{p[0], p[1], p[2], p[3]};
      }
      if (scale) {
        w.x = xf_scale_bytes(w.x, ln_s);
        w.y = xf_scale_bytes(w.y, ln_s);
        w.z = xf_scale_bytes(w.z, ln_s);
        w.w = xf_scale_bytes(w.w, ln_s);
      }
      *reinterpret_cast<u32x4 *>(s.dst + lo) = w;   // 16-byte aligned
    } else {
      const unsigned long long b0 = lo < 0 ? 0ull : (unsigned long long)lo;
      const unsigned long long b1 = ((unsigned long long)(lo + kChunk) < s.bytes) ? (unsigned long long)(lo + kChunk) : s.bytes;
      for (unsigned long long b = b0; b < b1; ++b) {
        const uint32_t v = s.src[b];
        s.dst[b] = (uint8_t)(scale ? xf_scale_bytes(v, ln_s) : v);
      }
    }
  }
}

__device__ __forceinline__ void position_tile(const MergeParams &p, const MergeSeg &s, uint32_t tl, const spz_amd_transform *x) {
  const unsigned long long i = (unsigned long long)tl * kMgBlock + threadIdx.x;
  const bool bad = i < s.num_points &&
                   xf_position_point(s.src, i, s.version == 1u, s.in_pos_scale, x, p.out_pos_scale, s.dst + i * 9ull);
  const unsigned long long ballot = __ballot(bad);
  if ((threadIdx.x & 63u) == 0u && ballot != 0ull && p.out_of_range != nullptr) {
    atomicAdd(p.out_of_range, (unsigned long long)__popcll(ballot));
  }
}

__device__ __forceinline__ void rotation_tile(const MergeSeg &s, uint32_t tl, const spz_amd_transform *x) {
  const unsigned long long i = (unsigned long long)tl * kMgBlock + threadIdx.x;
  if (i >= s.num_points) return;
  *reinterpret_cast<u32_a1 *>(s.dst + i * 4ull) = xf_rotation_point(s.src, i, s.version, x);
}

// 256 input records through LDS (lane-contiguous dword loads), one record per thread rotated (if placed) and cut or
// padded into the output records (LDS), lane-contiguous dword stores.
__device__ __forceinline__ void sh_tile(const MergeSeg &s, uint32_t tl, const spz_amd_transform *x, uint8_t *lin,
                                        uint8_t *lout) {
  const uint32_t irec = s.in_rec, orec = s.out_rec;
  const unsigned long long first = (unsigned long long)tl * kMgBlock;
  const unsigned long long left = s.num_points - first;
  const uint32_t pts = left < kMgBlock ? (uint32_t)left : kMgBlock;
  const uint32_t ibytes = pts * irec, obytes = pts * orec;
  const uint8_t *src = s.src + first * irec;
  uint8_t *dst = s.dst + first * orec;
  for (uint32_t b = threadIdx.x * 4u; b < ibytes; b += kMgBlock * 4u) {
    if (b + 4u <= ibytes) {
      *reinterpret_cast<uint32_t *>(lin + b) = *reinterpret_cast<const u32_a1 *>(src + b);
    } else {
      for (uint32_t j = b; j < ibytes; ++j) lin[j] = src[j];
    }
  }
  __syncthreads();
  if (threadIdx.x < pts) {
    uint8_t *ri = lin + threadIdx.x * irec;
    uint8_t *ro = lout + threadIdx.x * orec;
    const uint32_t keep = irec < orec ? irec : orec;
    if (x != nullptr && x->apply_rotation) xf_sh_record(ri, irec / 3u, keep / 3u, x);
    for (uint32_t j = 0; j < keep; ++j) ro[j] = ri[j];
    for (uint32_t j = keep; j < orec; ++j) ro[j] = 128u;   // decodes to 0.0
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x * 4u; b < obytes; b += kMgBlock * 4u) {
    if (b + 4u <= obytes) {
      *reinterpret_cast<u32_a1 *>(dst + b) = *reinterpret_cast<const uint32_t *>(lout + b);
    } else {
      for (uint32_t j = b; j < obytes; ++j) dst[j] = lout[j];
    }
  }
}

}  // namespace

__global__ __launch_bounds__(kMgBlock) void spz_merge_kernel(const MergeParams p) {
  __shared__ uint32_t lds_in[kMgBlock * kMaxShBytes / 4u];
  __shared__ uint32_t lds_out[kMgBlock * kMaxShBytes / 4u];
  const uint32_t tile = blockIdx.x;
  if (tile == 0 && threadIdx.x < 16 && p.header_dst != nullptr) {
    p.header_dst[threadIdx.x] = (uint8_t)(p.header_words[threadIdx.x >> 2] >> ((threadIdx.x & 3u) * 8u));
  }
  if (tile >= p.total_tiles) return;
  // the last slice whose first tile is <= tile (slices with no tiles are not in the table)
  uint32_t lo = 0, hi = p.n_seg - 1u;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1u) >> 1;
    if (p.tile_begin[mid] <= tile) lo = mid;
    else hi = mid - 1u;
  }
  lo = __builtin_amdgcn_readfirstlane(lo);   // uniform already; this lets the descriptor come in by scalar loads
  const MergeSeg s = p.segs[lo];
  const uint32_t tl = tile - p.tile_begin[lo];
  const spz_amd_transform *x = s.xf >= 0 ? p.xfs + s.xf : nullptr;
  switch (s.kind) {
    case MG_COPY:
    case MG_SCALE: copy_tile(s, tl, x); break;
    case MG_POS: position_tile(p, s, tl, x); break;
    case MG_ROT: rotation_tile(s, tl, x); break;
    case MG_SH: sh_tile(s, tl, x, reinterpret_cast<uint8_t *>(lds_in), reinterpret_cast<uint8_t *>(lds_out)); break;
    default: break;
  }
}

}  // namespace spz_amd_detail

namespace {

using namespace spz_amd_detail;

bool placement_moves(const spz_amd_transform *x) { return x != nullptr && x->apply_positions; }
bool placement_rotates(const spz_amd_transform *x) { return x != nullptr && x->apply_rotation; }
bool placement_scales(const spz_amd_transform *x) { return x != nullptr && x->apply_scales; }

int resolve_impl(const spz_amd_header *hdrs, uint64_t k, int sh_degree, int fractional_bits, int antialiased,
                 spz_amd_header *out_hdr, uint64_t *out_bytes) {
  if (hdrs == nullptr || out_hdr == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  if (k == 0 || k > SPZ_AMD_MERGE_MAX_INPUTS) return SPZ_AMD_ERR_INVALID_ARG;
  if (sh_degree < -1 || sh_degree > 3 || fractional_bits < -1 || fractional_bits > 24 || antialiased < -1 || antialiased > 1) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  uint64_t total = 0;
  int max_degree = 0, common_fb = -1, aa = antialiased;
  bool fb_agree = true;
  for (uint64_t i = 0; i < k; ++i) {
    const spz_amd_header &h = hdrs[i];
    if (h.version < 1 || h.version > 3) return SPZ_AMD_ERR_VERSION;
    if (h.sh_degree > 3) return SPZ_AMD_ERR_SH_DEGREE;
    total += h.num_points;
    if (h.sh_degree > max_degree) max_degree = h.sh_degree;
    if (h.version >= 2) {  // v1 positions are float16: they have no fractionalBits to vote with
      if (common_fb < 0) common_fb = h.fractional_bits;
      else if (common_fb != h.fractional_bits) fb_agree = false;
    }
    if (antialiased < 0 && (h.flags & 1) != (hdrs[0].flags & 1)) return SPZ_AMD_ERR_INVALID_ARG;
  }
  if (total > SPZ_AMD_REFERENCE_MAX_POINTS) return SPZ_AMD_ERR_TOO_MANY_POINTS;
  if (aa < 0) aa = hdrs[0].flags & 1;
  spz_amd_header o = {};
  o.version = 3;
  o.num_points = (uint32_t)total;
  o.sh_degree = (uint8_t)(sh_degree >= 0 ? sh_degree : max_degree);
  o.fractional_bits = (uint8_t)(fractional_bits >= 0 ? fractional_bits : (common_fb >= 0 && fb_agree ? common_fb : 12));
  o.flags = (uint8_t)aa;
  o.reserved = 0;
  spz_amd_layout lay;
  const int rc = spz_amd_stream_layout(o.num_points, o.sh_degree, 3, &lay);
  if (rc != SPZ_AMD_OK) return rc;
  *out_hdr = o;
  if (out_bytes) *out_bytes = lay.total_bytes;
  return SPZ_AMD_OK;
}

// The host image of the device table for `inputs` into `out`; fills the kernel's parameters except the table pointers.
int build_table(const spz_amd_merge_input *inputs, uint64_t k, const spz_amd_header *oh, uint8_t *d_out, uint8_t *img,
                MergeParams *p) {
  const TableLayout tl = table_layout(k);
  MergeSeg *segs = reinterpret_cast<MergeSeg *>(img + tl.segs);
  uint32_t *tiles_at = reinterpret_cast<uint32_t *>(img + tl.tiles);
  spz_amd_transform *xfs = reinterpret_cast<spz_amd_transform *>(img + tl.xfs);
  spz_amd_layout out;
  int rc = spz_amd_stream_layout(oh->num_points, oh->sh_degree, 3, &out);
  if (rc != SPZ_AMD_OK) return rc;
  std::vector<spz_amd_layout> in(k);
  std::vector<uint64_t> first(k);   // output index of each input's first point
  uint64_t at = 0;
  int32_t n_xf = 0;
  std::vector<int32_t> slot(k, -1);
  for (uint64_t i = 0; i < k; ++i) {
    rc = spz_amd_stream_layout(inputs[i].hdr.num_points, inputs[i].hdr.sh_degree, (int)inputs[i].hdr.version, &in[i]);
    if (rc != SPZ_AMD_OK) return rc;
    first[i] = at;
    at += inputs[i].hdr.num_points;
    if (inputs[i].xf != nullptr) {
      xfs[n_xf] = *inputs[i].xf;
      slot[i] = n_xf++;
    }
  }
  // largest sections first, so that the tail of the grid is made of the small ones
  const int order[SPZ_AMD_NUM_SECTIONS] = {SPZ_AMD_SEC_SH, SPZ_AMD_SEC_POSITIONS, SPZ_AMD_SEC_ROTATIONS,
                                           SPZ_AMD_SEC_SCALES, SPZ_AMD_SEC_COLORS, SPZ_AMD_SEC_ALPHAS};
  const uint32_t fb = oh->fractional_bits;
  uint64_t tiles = 0;
  uint32_t n_seg = 0;
  for (int sec : order) {
    const uint32_t obpp = out.bytes_per_point[sec];
    if (obpp == 0) continue;
    for (uint64_t i = 0; i < k; ++i) {
      const spz_amd_header &h = inputs[i].hdr;
      const uint64_t n = h.num_points;
      if (n == 0) continue;
      const spz_amd_transform *x = inputs[i].xf;
      MergeSeg s = {};
      s.src = inputs[i].d_stream + in[i].offset[sec];
      s.dst = d_out + out.offset[sec] + first[i] * obpp;
      s.bytes = n * obpp;
      s.num_points = (uint32_t)n;
      s.version = h.version;
      // float scale = 1.0 / (1 << fractionalBits) (load-spz.cc:495); x86 masks the shift count to 5 bits
      s.in_pos_scale = (float)(1.0 / (double)(int32_t)(1u << (h.fractional_bits & 31)));
      s.xf = slot[i];
      s.in_rec = in[i].bytes_per_point[SPZ_AMD_SEC_SH];
      s.out_rec = out.bytes_per_point[SPZ_AMD_SEC_SH];
      bool per_point = true;
      if (sec == SPZ_AMD_SEC_POSITIONS) {
        s.kind = (h.version >= 2 && h.fractional_bits == fb && !placement_moves(x)) ? MG_COPY : MG_POS;
        per_point = s.kind == MG_POS;
      } else if (sec == SPZ_AMD_SEC_ROTATIONS) {
        s.kind = (h.version >= 3 && !placement_rotates(x)) ? MG_COPY : MG_ROT;
        per_point = s.kind == MG_ROT;
      } else if (sec == SPZ_AMD_SEC_SH) {
        s.kind = (s.in_rec == s.out_rec && !placement_rotates(x)) ? MG_COPY : MG_SH;
        per_point = s.kind == MG_SH;
      } else {
        s.kind = (sec == SPZ_AMD_SEC_SCALES && placement_scales(x)) ? MG_SCALE : MG_COPY;
        per_point = false;
      }
      const uint64_t lead = (uintptr_t)s.dst & (kChunk - 1u);
      const uint64_t t = per_point ? (n + kMgBlock - 1) / kMgBlock
                                   : ((lead + s.bytes + kChunk - 1) / kChunk + kCopyTileChunks - 1) / kCopyTileChunks;
      segs[n_seg] = s;
      tiles_at[n_seg] = (uint32_t)tiles;
      ++n_seg;
      tiles += t;
      if (tiles > 0x7fffffffull) return SPZ_AMD_ERR_INVALID_ARG;
    }
  }
  *p = MergeParams{};
  p->n_seg = n_seg;
  p->total_tiles = (uint32_t)tiles;
  p->out_pos_scale = (float)(1u << fb);
  p->header_dst = d_out;
  p->header_words[0] = kMagic;
  p->header_words[1] = 3u;
  p->header_words[2] = oh->num_points;
  p->header_words[3] = (uint32_t)oh->sh_degree | (fb << 8) | ((uint32_t)(oh->flags & 1u) << 16);
  return SPZ_AMD_OK;
}

void free_host_image(void *p) { std::free(p); }

int merge_impl(const spz_amd_merge_input *inputs, uint64_t k, const spz_amd_header *oh, uint8_t *d_out, size_t capacity,
               void *d_workspace, uint64_t *d_out_of_range, void *hip_stream) {
  if (inputs == nullptr || oh == nullptr || d_out == nullptr || d_workspace == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  if (k == 0 || k > SPZ_AMD_MERGE_MAX_INPUTS) return SPZ_AMD_ERR_INVALID_ARG;
  if (oh->version != 3 || oh->sh_degree > 3 || oh->fractional_bits > 24 || oh->flags > 1) return SPZ_AMD_ERR_INVALID_ARG;
  uint64_t total = 0;
  for (uint64_t i = 0; i < k; ++i) {
    const spz_amd_header &h = inputs[i].hdr;
    if (h.version < 1 || h.version > 3) return SPZ_AMD_ERR_VERSION;
    if (h.sh_degree > 3) return SPZ_AMD_ERR_SH_DEGREE;
    spz_amd_layout lay;
    const int rc = spz_amd_stream_layout(h.num_points, h.sh_degree, (int)h.version, &lay);
    if (rc != SPZ_AMD_OK) return rc;
    if (inputs[i].d_stream == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
    if (inputs[i].size < lay.total_bytes) return SPZ_AMD_ERR_SHORT_STREAM;
    total += h.num_points;
  }
  if (total != oh->num_points) return SPZ_AMD_ERR_INVALID_ARG;
  spz_amd_layout out;
  int rc = spz_amd_stream_layout(oh->num_points, oh->sh_degree, 3, &out);
  if (rc != SPZ_AMD_OK) return rc;
  if (capacity < out.total_bytes) return SPZ_AMD_ERR_CAPACITY;
  int device = 0;
  rc = current_device(&device);
  if (rc != SPZ_AMD_OK) return rc;
  const TableLayout tl = table_layout(k);
  uint8_t *img = static_cast<uint8_t *>(std::calloc(1, tl.bytes));
  if (img == nullptr) return SPZ_AMD_ERR_INVALID_ARG;
  MergeParams p;
  rc = build_table(inputs, k, oh, d_out, img, &p);
  if (rc != SPZ_AMD_OK) {
    std::free(img);
    return rc;
  }
  hipStream_t st = static_cast<hipStream_t>(hip_stream);
  uint8_t *ws = static_cast<uint8_t *>(d_workspace);
  p.segs = reinterpret_cast<const MergeSeg *>(ws + tl.segs);
  p.tile_begin = reinterpret_cast<const uint32_t *>(ws + tl.tiles);
  p.xfs = reinterpret_cast<const spz_amd_transform *>(ws + tl.xfs);
  p.out_of_range = reinterpret_cast<unsigned long long *>(d_out_of_range);
  hipError_t e = hipMemcpyAsync(ws, img, tl.bytes, hipMemcpyHostToDevice, st);
  // the image is freed on the stream once the copy has read it: nothing on the device reads host memory after return
  if (e == hipSuccess) e = hipLaunchHostFunc(st, free_host_image, img);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(st);
    std::free(img);
    g_last_hip_error = (int)e;
    return SPZ_AMD_ERR_HIP;
  }
  if (d_out_of_range) SPZ_HIP_TRY(hipMemsetAsync(d_out_of_range, 0, sizeof(uint64_t), st));
  hipLaunchKernelGGL(spz_merge_kernel, dim3(p.total_tiles > 0 ? p.total_tiles : 1u), dim3(kMgBlock), 0, st, p);
  SPZ_HIP_TRY(hipGetLastError());
  return SPZ_AMD_OK;
}

}  // namespace

extern "C" {

int spz_amd_merge_resolve(const spz_amd_header *headers, uint64_t k, int sh_degree, int fractional_bits, int antialiased,
                          spz_amd_header *out_hdr, uint64_t *out_bytes) {
  return resolve_impl(headers, k, sh_degree, fractional_bits, antialiased, out_hdr, out_bytes);
}

uint64_t spz_amd_merge_workspace_bytes(uint64_t k) {
  return (k == 0 || k > SPZ_AMD_MERGE_MAX_INPUTS) ? 0 : (uint64_t)table_layout(k).bytes;
}

int spz_amd_merge_device(const spz_amd_merge_input *inputs, uint64_t k, const spz_amd_header *out_hdr, uint8_t *d_out,
                         size_t capacity, void *d_workspace, uint64_t *d_out_of_range, void *hip_stream) {
  return merge_impl(inputs, k, out_hdr, d_out, capacity, d_workspace, d_out_of_range, hip_stream);
}

int spz_amd_merge_open(const spz_amd_merge_input *inputs, uint64_t k, int sh_degree, int fractional_bits, int antialiased,
                       int device, void **ctx, spz_amd_header *out_hdr, uint64_t *h_out_bytes, uint64_t *h_out_of_range,
                       float *h_ms) {
  if (ctx == nullptr || out_hdr == nullptr || h_out_bytes == nullptr || h_out_of_range == nullptr || inputs == nullptr) {
    return SPZ_AMD_ERR_INVALID_ARG;
  }
  *ctx = nullptr;
  *h_out_bytes = 0;
  *h_out_of_range = 0;
  if (k == 0 || k > SPZ_AMD_MERGE_MAX_INPUTS) return SPZ_AMD_ERR_INVALID_ARG;
  std::vector<spz_amd_header> hdrs(k);
  for (uint64_t i = 0; i < k; ++i) hdrs[i] = inputs[i].hdr;
  spz_amd_header oh;
  uint64_t bytes = 0;
  int rc = resolve_impl(hdrs.data(), k, sh_degree, fractional_bits, antialiased, &oh, &bytes);
  if (rc != SPZ_AMD_OK) return rc;
  DeviceGuard guard;
  rc = guard.enter(device);
  if (rc != SPZ_AMD_OK) return rc;
  PackedResultPtr c;
  rc = packed_result_open(device, &c);
  if (rc != SPZ_AMD_OK) return rc;
  const size_t stream_bytes = Workspace::aligned(bytes);
  const size_t table_bytes = Workspace::aligned(table_layout(k).bytes);
  SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&c->block), stream_bytes + table_bytes + 256));
  c->out = c->block;
  uint64_t *d_count = reinterpret_cast<uint64_t *>(c->block + stream_bytes + table_bytes);
  const auto t0 = std::chrono::steady_clock::now();
  rc = merge_impl(inputs, k, &oh, c->out, bytes, c->block + stream_bytes, d_count, c->st);
  if (rc != SPZ_AMD_OK) return rc;
  uint64_t h = 0;
  SPZ_HIP_TRY(hipMemcpyAsync(&h, d_count, sizeof(h), hipMemcpyDeviceToHost, c->st));
  SPZ_HIP_TRY(hipStreamSynchronize(c->st));
  if (h_ms) h_ms[0] = (float)ms_since(t0);
  c->out_bytes = bytes;
  *out_hdr = oh;
  *h_out_bytes = bytes;
  *h_out_of_range = h;
  *ctx = c.release();
  return SPZ_AMD_OK;
}

int spz_amd_merge_fetch(void *ctx, uint8_t *h_out) { return packed_result_fetch(ctx, h_out); }

const uint8_t *spz_amd_merge_device_data(void *ctx) { return packed_result_device_data(ctx); }

void spz_amd_merge_close(void *ctx) { packed_result_close(ctx); }

}  // extern "C"
