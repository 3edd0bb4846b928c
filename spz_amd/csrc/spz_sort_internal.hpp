// spz_sort_internal.hpp — the digit passes of the stable radix sort (spz_sort.hip), for other translation units of
// libspz_amd.so that sort keys of their own (spz_render.hip: the tile entries by tile id), and the Morton-sorted points
// of the neighbour searches (spz_clean.hip, spz_align.hip).  The public sorts
// (spz_amd_morton_order_device, spz_amd_argsort_f32_device) are built on the same two functions.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "spz_amd.h"

namespace spz_amd_detail {

// Byte offsets into a 256-aligned workspace of `bytes` bytes for a sort of n keys: the index ping-pong buffer, two
// sets of three u32 key planes, the per-tile digit counts and the digit totals.
struct SortLayout {
  uint64_t tiles, idx_off, planes_off[2][3], counts_off, totals_off, bytes;
};

SortLayout sort_layout(uint64_t n);

// Stable LSD passes over the keys already written into plane 0 of set 0 (ws + planes_off[0][0], n u32), `digits`
// 8-bit digits from bit 0 (digits <= 4 reads plane 0 only); the permutation lands in d_order (n u32).  ws is 256-aligned
// and holds wl = sort_layout(n); n >= 1.  Plane 0 of set 0 is overwritten when digits >= 3.  Enqueues on st.
int radix_passes(uint32_t n, uint32_t digits, uint32_t *d_order, uint8_t *ws, const SortLayout &wl, hipStream_t st);

// The sorted points of one stream, as the neighbour searches read them (spz_morton_walk.hpp): its Morton order into
// d_order (n u32; spz_amd_morton_order_device's checks and errors), then (u_x, u_y, u_z, input index) in that order
// into d_pts (n uint4).  lay is the stream's layout; d_sort_ws holds spz_amd_sort_workspace_bytes(n).  Nothing for an
// empty stream.  Enqueues on st.
int morton_sorted_points(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, const spz_amd_layout &lay,
                         uint32_t *d_order, uint4 *d_pts, void *d_sort_ws, hipStream_t st);

}  // namespace spz_amd_detail
