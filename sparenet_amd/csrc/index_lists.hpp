// index_lists.hpp -- the inversion of an index list (gfx950 only).  idx [b, slots] names a target in [0, n) per slot;
// the backward of a gather needs, for every target of a cloud, the slots that point at it.  Built once per call with
// integer atomics only (memset, count, scan, fill), then shared by all channels.  Used by EdgeConv's edge features
// (knn.hip: long long indices, slots = n * k) and by grouping / interpolation (neighbors.hip: int, slots = m * s).
//
// A slot whose index is outside [0, n) -- the -1 padding of the neighbourhood searches -- is in no list.  That holds
// for both users: sn_graph_feature_backward, whose indices come from sn_knn_topk and are always in range, used to index
// with them unchecked.
#pragma once
#include "block_scan.hpp"
#include "common.hpp"

namespace {

struct IndexLists {
  int *offs;  // [b, n] slots arriving at each target, then the lists' starts, after the fill their ENDS
  int *list;  // [b, slots] the slots' numbers inside their cloud, grouped by target (in no order inside a list)
};
inline IndexLists index_lists_layout(sn::Carver &c, int b, int n, long slots) {
  return {c.take256<int>((size_t)b * n * 4), c.take<int>((size_t)b * slots * 4)};
}

template <class Index>
__global__ __launch_bounds__(256) void index_lists_count_kernel(const Index *__restrict__ idx, int n, long slots,
                                                                long total, int *__restrict__ offs) {
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const Index j = idx[e];
    if (j >= 0 && j < n) atomicAdd(&offs[e / slots * n + j], 1);
  }
}

// per cloud: in-place exclusive scan of the n counts
__global__ __launch_bounds__(1024) void index_lists_scan_kernel(int *__restrict__ offs, int n) {
  __shared__ alignas(16) sn::BlockScan<1024> scan;
  int *c = offs + (size_t)blockIdx.x * n;
  scan.reset(0);
  for (int base = 0; base < n; base += 1024) {
    const int i = base + threadIdx.x;
    scan.chunk(i < n ? c[i] : 0, [&](int start) {
      if (i < n) c[i] = start;
    });
  }
}

template <class Index>
__global__ __launch_bounds__(256) void index_lists_fill_kernel(const Index *__restrict__ idx, int n, long slots,
                                                               long total, int *__restrict__ offs,
                                                               int *__restrict__ list) {
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const Index j = idx[e];
    if (j < 0 || j >= n) continue;
    const long b = e / slots;
    const int pos = atomicAdd(&offs[b * n + j], 1);
    list[b * slots + pos] = (int)(e - b * slots);
  }
}

// enqueues the four steps on s; `what` names the entry point in an error's text
template <class Index>
int build_index_lists(const char *what, const Index *idx, int b, int n, long slots, const IndexLists &w,
                      hipStream_t s) {
  constexpr int kMaxBlocks = 65535;  // cap of the grid-stride launches
  const long total = b * slots;
  SN_HIP(hipMemsetAsync(w.offs, 0, (size_t)b * n * 4, s));
  index_lists_count_kernel<<<sn::grid_blocks(total, kMaxBlocks), 256, 0, s>>>(idx, n, slots, total, w.offs);
  index_lists_scan_kernel<<<b, 1024, 0, s>>>(w.offs, n);
  index_lists_fill_kernel<<<sn::grid_blocks(total, kMaxBlocks), 256, 0, s>>>(idx, n, slots, total, w.offs, w.list);
  return sn::launch_status(what);
}

}  // namespace
