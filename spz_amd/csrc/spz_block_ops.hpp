// spz_block_ops.hpp — reductions and scans over the threads of one workgroup through LDS, for the kernels of
// libspz_amd.so whose sums must repeat their bits: the order of the additions is fixed by the thread index alone.
//
//   block_sum                 the block's sum in a binary tree, 256 threads (clean, align, plane, mesh, densify, seed,
//                             photo).
//   block_exclusive_scan      Hillis–Steele over BLOCK threads: every op that ranks or compacts inside a workgroup.
//   block_scan_owned_runs     one workgroup scans `count` values, a contiguous run per thread: the second level of
//                             every op's two-level scan (filter, sort, decimate, tile, render, densify, seed).
// A new op does not write its own scan: it calls these.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#pragma clang fp contract(off)

namespace spz_amd_detail {

constexpr uint32_t kOpsBlock = 256;  // the workgroup size of block_sum's callers, and the scans' default

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

// Exclusive scan of v over the BLOCK threads of the block through s (BLOCK entries); returns this thread's prefix and,
// when asked, the block's sum to every thread.  s is free again on return.  T: uint32_t or unsigned long long.
template <class T, uint32_t BLOCK = kOpsBlock>
__device__ __forceinline__ T block_exclusive_scan(T v, T *s, T *total = nullptr) {
  static_assert(std::is_same<T, uint32_t>::value || std::is_same<T, unsigned long long>::value, "an integer scan");
  const uint32_t t = threadIdx.x;
  s[t] = v;
  __syncthreads();
  for (uint32_t off = 1; off < BLOCK; off <<= 1) {
    const T u = t >= off ? s[t - off] : T(0);
    __syncthreads();
    s[t] += u;
    __syncthreads();
  }
  const T r = s[t] - v;
  if (total != nullptr) *total = s[BLOCK - 1u];
  __syncthreads();
  return r;
}

// One workgroup of BLOCK threads scans the values load(0), ..., load(count - 1): thread t owns the contiguous run
// [min(t per, count), min(t per + per, count)), per = ceil(count / BLOCK), empty for the trailing threads.  It sums its
// run, one block scan places the runs, and it walks the run again: store(k, the sum of the values before k), once per
// k.  load(k) is called on both walks, on the second before store(k, .), so a scan in place reads before it writes;
// it returns the same value both times and whatever else a kernel does per k belongs in store.  Returns the sum of
// all values to every thread.
template <class T, uint32_t BLOCK = kOpsBlock, class Load, class Store>
__device__ __forceinline__ T block_scan_owned_runs(uint32_t count, T *s, Load load, Store store) {
  const uint32_t t = threadIdx.x;
  const uint32_t per = (count + BLOCK - 1u) / BLOCK;
  const unsigned long long b64 = (unsigned long long)t * per;  // in 64 bits: t per passes 2^32 before count does
  const uint32_t b = b64 < count ? (uint32_t)b64 : count;
  const uint32_t e = (count - b) < per ? count : b + per;
  T sum = 0;
  for (uint32_t k = b; k < e; ++k) sum += load(k);
  T total;
  T run = block_exclusive_scan<T, BLOCK>(sum, s, &total);
  for (uint32_t k = b; k < e; ++k) {
    const T c = load(k);
    store(k, run);
    run += c;
  }
  return total;
}

}  // namespace spz_amd_detail
