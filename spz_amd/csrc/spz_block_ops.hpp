// spz_block_ops.hpp — reductions and scans over the 256 threads of a workgroup through LDS, for the kernels of
// libspz_amd.so whose sums must repeat their bits: the order of the additions is fixed by the thread index alone.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#pragma clang fp contract(off)

namespace spz_amd_detail {

constexpr uint32_t kOpsBlock = 256;  // the workgroup size of every caller

// The sum of v over the block in a binary tree through s (256 entries), returned to every thread.  T: double or
// unsigned long long.
template <class T>
__device__ __forceinline__ T block_sum(T v, T *s) {
  const uint32_t tid = threadIdx.x;
  s[tid] = v;
  __syncthreads();
  for (uint32_t off = kOpsBlock / 2u; off > 0; off >>= 1) {
    if (tid < off) s[tid] = s[tid] + s[tid + off];
    __syncthreads();
  }
  const T r = s[0];
  __syncthreads();
  return r;
}

// Exclusive scan of v over the block through s (256 entries); returns this thread's prefix.
__device__ __forceinline__ unsigned long long block_exclusive_scan64(unsigned long long v, unsigned long long *s) {
  const uint32_t t = threadIdx.x;
  s[t] = v;
  __syncthreads();
  for (uint32_t off = 1; off < kOpsBlock; off <<= 1) {
    const unsigned long long u = t >= off ? s[t - off] : 0ull;
    __syncthreads();
    s[t] += u;
    __syncthreads();
  }
  const unsigned long long r = s[t] - v;
  __syncthreads();
  return r;
}

}  // namespace spz_amd_detail
