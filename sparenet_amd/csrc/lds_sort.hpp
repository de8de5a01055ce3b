// lds_sort.hpp -- the one place where a workgroup sorts in LDS ("Workgroup sorts in LDS").  Two networks:
// the record sort of swd.hip and voxel_grid.hip and the key sort of sorted_lists.hpp and emd_general.hip.  The index
// arithmetic and the schedules need no HIP runtime: a driver takes `lanes`, the lanes first .. first + kCount - 1 that
// the caller stands for and the barrier() between two passes.  On the device that is Workgroup -- the calling lane and
// __syncthreads(); tools/lds_sort_host.cpp runs the same drivers under sanitizers with every lane of the workgroup one
// after another and an empty barrier, which is exact because within a pass no two lanes touch the same element.
//
// Record sort.  The records are doubles that are unique, normal and of one sign: such doubles order as their bit
// patterns do and v_min_f64 / v_max_f64 return an operand unchanged, so a compare-exchange of two records is one minimum
// and one maximum -- a 64-bit integer compare and four selects otherwise -- and no tie ever has to be broken.  How a
// record is packed, and the pad record that sorts behind all of them, are the caller's.
//   The network's log2(W) (log2(W) + 1) / 2 compare-exchange steps are taken up to kStepsPerPass = 4 at a time: a lane
// loads the 16 records a + t * jlow (t = 0..15) that four consecutive steps of strides 8 jlow .. jlow couple among
// themselves, runs the four steps in registers and stores them -- 32 passes over LDS instead of 105 at W = 16384, one
// barrier each.  Where a merge has a number of steps that is no multiple of four the short pass comes first, at the
// wide strides, so a pass's lowest stride jlow is a power of 16.
//   Slot i lives at record i + i / 16: without the gap the last pass of a merge (jlow = 1, a lane owns 16 consecutive
// records = 128 bytes) puts every lane of a group on the same two bank quarters; with it a lane's stride is 34 dwords
// and the 32 lanes of a ds_read_b64 group fall on 32 different bank pairs.  The passes with jlow >= 16 read consecutive
// records across lanes and meet a gap once per 16 lanes.  A width of 16384 is (16384 + 1024) * 8 = 139264 bytes.
//
// Key sort.  The plain network, one compare-exchange of keys[i] and keys[i ^ j] per lane and step, one barrier per
// step, on plain integer keys that may repeat (a long inverse list of the Chamfer and DCD backward, a chunk of 1024
// bidders of the EMD backward).
#pragma once
#include <cstddef>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif
#if !defined(__HIPCC__) && !defined(__forceinline__)
#define __forceinline__ inline __attribute__((always_inline))
#endif

namespace lds_sort {

constexpr int kThreads = 1024;             // lanes of a workgroup that sorts records
constexpr int kPadShift = 4;               // one empty record behind every 16
constexpr int kStepsPerPass = 4;           // compare-exchange steps a lane runs in registers between two barriers
static_assert(kStepsPerPass == kPadShift, "a pass's lowest stride is a power of 16: whole padded rows, or 1");

__host__ __device__ constexpr int slot(int i) { return i + (i >> kPadShift); }
constexpr size_t lds_bytes(int width) { return (size_t)slot(width) * sizeof(double); }

__host__ __device__ inline int pow2_width(int len) {      // the smallest power of two >= max(len, 2)
  int w = 2;
  while (w < len) w <<= 1;
  return w;
}

// R consecutive steps of the merge of runs of k, strides jtop, jtop / 2 ... jtop >> (R - 1), on 2^R records per lane.
// jlow is a power of 16 (the short pass of a merge comes first), and the R bits of `a` at jlow's position are 0, so
// slot(a + t jlow) = slot(a) + t slot(jlow): one add per record.  A run that is to come out descending is loaded in
// reverse -- register t holds record E - 1 - t -- so the network in the registers is the ascending one for every lane.
template <int R>
__host__ __device__ __forceinline__ void sort_pass(double *rec, int width, int k, int jtop, int tid) {
  constexpr int E = 1 << R;
  const int jlow = jtop >> (R - 1);
  const int stride = slot(jlow);
  for (int q = tid; q < (width >> R); q += kThreads) {
    const int a = ((q & ~(jlow - 1)) << R) | (q & (jlow - 1));      // R zero bits at jlow's position
    const bool up = (a & k) == 0;      // k >= 2 * jtop: the same for all E records
    const int base = slot(a) + (up ? 0 : (E - 1) * stride), step = up ? stride : -stride;
    double e[E];
#pragma unroll
    for (int t = 0; t < E; ++t) e[t] = rec[base + t * step];
#pragma unroll
    for (int d = E >> 1; d >= 1; d >>= 1) {
#pragma unroll
      for (int t = 0; t < E; ++t) {
        if (t & d) continue;
        const double lo = __builtin_fmin(e[t], e[t | d]), hi = __builtin_fmax(e[t], e[t | d]);
        e[t] = lo;
        e[t | d] = hi;
      }
    }
#pragma unroll
    for (int t = 0; t < E; ++t) rec[base + t * step] = e[t];
  }
}

// the records rec[slot(0 .. width - 1)] ascending, width a power of two >= 2: the schedule of the passes
template <class Lanes>
__host__ __device__ __forceinline__ void sort_records(double *rec, int width, Lanes lanes) {
  for (int k = 2, steps = 1; k <= width; k <<= 1, ++steps) {
    int jtop = k >> 1;
    for (int left = steps; left > 0;) {
      const int r = left % kStepsPerPass ? left % kStepsPerPass : kStepsPerPass;
      for (int lane = 0; lane < Lanes::kCount; ++lane) {      // a constant bound: no loop is left where kCount is 1
        const int tid = lanes.first + lane;
        switch (r) {
          case 1: sort_pass<1>(rec, width, k, jtop, tid); break;
          case 2: sort_pass<2>(rec, width, k, jtop, tid); break;
          case 3: sort_pass<3>(rec, width, k, jtop, tid); break;
          default: sort_pass<4>(rec, width, k, jtop, tid); break;
        }
      }
      lanes.barrier();
      jtop >>= r;
      left -= r;
    }
  }
}

// keys[0 .. p2) ascending by operator> of T, p2 a power of two, kLanes lanes that stride over the array
template <int kLanes, class T, class Lanes>
__host__ __device__ __forceinline__ void sort_keys(T *keys, int p2, Lanes lanes) {
  for (int k = 2; k <= p2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int lane = 0; lane < Lanes::kCount; ++lane)
        for (int i = lanes.first + lane; i < p2; i += kLanes) {
          const int ixj = i ^ j;
          if (ixj > i) {
            const T x = keys[i], y = keys[ixj];
            const bool up = (i & k) == 0;
            if ((x > y) == up) {
              keys[i] = y;
              keys[ixj] = x;
            }
          }
        }
      lanes.barrier();
    }
}

#if defined(__HIPCC__)
struct Workgroup {      // the calling lane, and the barrier that ends a pass
  int first;
  static constexpr int kCount = 1;
  __device__ __forceinline__ void barrier() const { __syncthreads(); }
};

// Every lane of the workgroup of kThreads calls it; the records are written and a barrier has been passed.  Ends in a
// barrier.
__device__ __forceinline__ void sort_records(double *rec, int width, int tid) { sort_records(rec, width, Workgroup{tid}); }

// Every lane of the workgroup of kLanes calls it; the caller has padded keys[0 .. p2) to a power of two and passed a
// barrier.  One barrier per step, the last of them the closing one (p2 = 1 has no step: the caller's barrier stands).
template <int kLanes, class T>
__device__ __forceinline__ void sort_keys(T *keys, int p2) {
  sort_keys<kLanes>(keys, p2, Workgroup{(int)threadIdx.x});
}
#endif

}  // namespace lds_sort
