// sorted_lists.hpp -- the ascending order of inverse lists (gfx950 only).  A backward pass that gathers over inverse
// lists (who chose me?) instead of scattering with floating-point atomics fills its lists with integer atomics, in
// arbitrary order; the sum is defined over the ascending list, so every list is sorted before it is used.  A list of
// up to kLongList entries is sorted by the lane that owns it (sort_ints); the owner of a longer one registers it
// (register_long_list) and a workgroup of a later kernel takes it (sort_long_list, sorted_entry).  Used by the
// Chamfer backward (chamfer.hip) and the density-aware Chamfer distance (dcd.hip); the ordered accumulation that
// follows the sort differs between them (fp32 by one wave, double by the workgroup) and stays in their kernels.
#pragma once
#include "common.hpp"
#include "lds_sort.hpp"

namespace {

constexpr int kLongList = 64;        // inverse lists longer than this are sorted and summed by a workgroup
constexpr int kLongSortCap = 16384;  // ... in LDS up to this length (64 KiB); longer ones by one thread, in place
constexpr int kLongBlocks = 128;     // workgroups of a long-list kernel: each takes every kLongBlocks-th long list

// the owner of a list of more than kLongList entries: longs[0] counts the long lists, their owners' ids follow
__device__ __forceinline__ void register_long_list(int *longs, int id) { longs[1 + atomicAdd(&longs[0], 1)] = id; }

// in-place ascending sort of an int array in global memory owned by the calling thread
__device__ __forceinline__ void sort_ints(int *a, int n) {
  if (n <= 16) {  // insertion sort
    for (int i = 1; i < n; ++i) {
      const int v = a[i];
      int j = i - 1;
      while (j >= 0 && a[j] > v) {
        a[j + 1] = a[j];
        --j;
      }
      a[j + 1] = v;
    }
    return;
  }
  // heap sort: O(n log n) also for the degenerate case of thousands of queries sharing one neighbour
  auto sift = [&](int start, int end) {
    int root = start;
    for (;;) {
      int child = 2 * root + 1;
      if (child > end) break;
      if (child + 1 <= end && a[child] < a[child + 1]) ++child;
      if (a[root] >= a[child]) break;
      const int t = a[root];
      a[root] = a[child];
      a[child] = t;
      root = child;
    }
  };
  for (int start = (n - 2) / 2; start >= 0; --start) sift(start, n - 1);
  for (int end = n - 1; end > 0; --end) {
    const int t = a[0];
    a[0] = a[end];
    a[end] = t;
    sift(0, end - 1);
  }
}

// A workgroup of kThreads sorts the c entries of lst; keys is its LDS buffer of kLongSortCap ints.  Up to kLongSortCap
// entries: padded to a power of two with 0x7fffffff, lds_sort.hpp's key sort in keys, lst untouched.  Beyond: thread 0
// sorts lst in place.  Opens with a barrier (the previous list's keys are no longer needed) and closes with one:
// afterwards every thread reads entry i through sorted_entry.
template <int kThreads>
__device__ __forceinline__ void sort_long_list(int *lst, int c, int *keys) {
  const int tid = threadIdx.x;
  __syncthreads();
  if (c <= kLongSortCap) {
    int p2 = 1;
    while (p2 < c) p2 <<= 1;
    for (int i = tid; i < p2; i += kThreads) keys[i] = i < c ? lst[i] : 0x7fffffff;
    __syncthreads();
    lds_sort::sort_keys<kThreads>(keys, p2);
  } else {
    if (tid == 0) sort_ints(lst, c);
    __threadfence_block();
    __syncthreads();
  }
}

// Entry i of the c that sort_long_list has sorted, from where it left them.  Thread 0's in-place result is read from
// memory, not from a line another lane's cache may hold: a volatile load.  The fence and the barrier behind the sort
// already order the stores before this load for the waves of one workgroup, which share a compute unit's L1; the
// load is the conservative form and costs one wait per entry read, which the dependent loads behind it need anyway.
__device__ __forceinline__ int sorted_entry(const int *lst, int c, const int *keys, int i) {
  return c <= kLongSortCap ? keys[i] : ((const volatile int *)lst)[i];
}

}  // namespace
