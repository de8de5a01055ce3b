// block_scan.hpp -- the prefix sums every count / scan / fill chain needs (gfx950 only): the inclusive scan of a wave, and
// the exclusive scan of a whole workgroup over a sequence of any length, taken in chunks of one value per thread with the
// running total carried from chunk to chunk in LDS.  Also the workgroup's float64 sum in a fixed order (block_sum_f64).
//
//   __shared__ alignas(16) sn::BlockScan<1024> scan;    // aligned: the wave sums are then read four words at a time
//   scan.reset(start);                                  // the sum in front of the first value
//   for (int base = 0; base < n; base += 1024) {
//     const int i = base + threadIdx.x;
//     const int v = i < n ? count[i] : 0;               // EVERY thread takes part in every chunk
//     scan.chunk(v, [&](int exclusive) { if (i < n) start_of[i] = exclusive; });
//   }
//   ... scan.carry is start + the sum of all values, in every thread
#pragma once
#include "common.hpp"

namespace sn {

// inclusive prefix sum of v over the lanes of a wave
__device__ __forceinline__ int wave_inclusive_scan(int v) {
  const int lane = threadIdx.x & (kWave - 1);
  for (int d = 1; d < kWave; d <<= 1) {
    const int u = __shfl_up(v, d);
    if (lane >= d) v += u;
  }
  return v;
}

// The float64 sum of one value per thread over a one-dimensional workgroup of kThreads threads, in an order that
// kThreads alone fixes: a 64-lane xor butterfly (32, 16 .. 1), then the wave sums ascending.  wave_sum: kThreads / kWave
// doubles of LDS.  Every thread calls it; thread 0 returns the sum (the others their wave's).  One barrier inside,
// between the waves' writes and thread 0's reads: the caller leaves wave_sum alone until thread 0 has passed a later
// barrier.
template <int kThreads>
__device__ __forceinline__ double block_sum_f64(double acc, double *wave_sum) {
  static_assert(kThreads % kWave == 0, "whole waves");
  const int tid = threadIdx.x;
  for (int off = kWave / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  if ((tid & (kWave - 1)) == 0) wave_sum[tid / kWave] = acc;
  __syncthreads();
  if (tid == 0) {
    acc = wave_sum[0];
    for (int w = 1; w < kThreads / kWave; ++w) acc += wave_sum[w];
  }
  return acc;
}

// block_sum_f64 for kValues values per thread at once, each in block_sum_f64's order: wave_sums is kThreads / kWave *
// kValues doubles of LDS, and thread k < kValues returns the sum of value k in acc[0] (the other threads' acc is
// spent).  One barrier inside; the caller leaves wave_sums alone until those threads have passed a later barrier.
template <int kThreads, int kValues>
__device__ __forceinline__ void block_sums_f64(double (&acc)[kValues], double *wave_sums) {
  static_assert(kThreads % kWave == 0 && kValues <= kThreads, "whole waves, one summing thread per value");
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < kValues; ++k) {
    double v = acc[k];
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((tid & (kWave - 1)) == 0) wave_sums[(tid / kWave) * kValues + k] = v;
  }
  __syncthreads();
  if (tid < kValues) {
    double v = wave_sums[tid];
    for (int w = 1; w < kThreads / kWave; ++w) v += wave_sums[w * kValues + tid];
    acc[0] = v;
  }
}

// Lives in __shared__ memory of a one-dimensional workgroup of kThreads threads; all of them call reset and chunk.
// The alignment belongs to the variable, not to the type: an aligned type would round these 68 bytes up to 80.
template <int kThreads>
struct BlockScan {
  static_assert(kThreads % kWave == 0, "whole waves");
  int wsum[kThreads / kWave];  // the sum of each wave of the chunk in flight
  int carry;                   // the sum of everything in front of that chunk; after the last chunk, the total

  // only thread 0's `start` counts.  Ends in a barrier.
  __device__ __forceinline__ void reset(int start) {
    if (threadIdx.x == 0) carry = start;
    __syncthreads();
  }

  // body(exclusive prefix of this thread's v) runs between two barriers: it may overwrite what v was read from.  The
  // inclusive prefix is exclusive + v.  Ends in a barrier, behind which carry includes the chunk.
  template <class Body>
  __device__ __forceinline__ void chunk(int v, Body &&body) {
    const int tid = threadIdx.x;
    const int incl = wave_inclusive_scan(v);
    if ((tid & (kWave - 1)) == kWave - 1) wsum[tid / kWave] = incl;
    __syncthreads();
    int pre = carry;
    for (int w = 0; w < tid / kWave; ++w) pre += wsum[w];
    body(pre + incl - v);
    __syncthreads();  // every thread has read carry and wsum
    if (tid == kThreads - 1) carry = pre + incl;
    __syncthreads();
  }
};

}  // namespace sn
