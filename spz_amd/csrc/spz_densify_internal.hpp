// spz_densify_internal.hpp — what spz_refine.hip uses of spz_densify.hip beyond the C ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace spz_amd_detail {

// d_dst[k] = d_src[d_parent[k]] for k < n_new (d_src NULL: the identity map, so d_dst = d_parent); parents are clamped
// to n_src - 1.  How refine carries each point's index in the input stream through a densify round.
int densify_gather_u32(const uint32_t *d_src, const uint32_t *d_parent, uint64_t n_src, uint64_t n_new, uint32_t *d_dst,
                       hipStream_t st);

}  // namespace spz_amd_detail
