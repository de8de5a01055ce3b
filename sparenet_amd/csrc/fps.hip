// fps.hip -- exact farthest point sampling (include/ops/fps.h states the rule): one workgroup per cloud, M dependent
// arg-max steps, so the kernel is decided by the latency of ONE pick.
//
// Resident path (n <= 24576): thread t of T owns points t, t + T, t + 2T, ... with x, y, z and mind in registers (P of
// them, a template parameter, so the arrays are never indexed at run time).  One pick:
//   1. every thread updates its P points against the last pick and keeps its best {mind, index, x, y, z} -- strict >
//      in ascending index order, so the lowest index of a thread's maxima;
//   2. the wave reduces the 64-bit key (mind bits << 32) | ~index under an unsigned max: mind is never negative, so its
//      bit pattern orders as its value, and ~index makes the lowest index win among equal distances.  Four DPP steps
//      inside the rows of 16 lanes, four v_readlane pairs across them;
//   3. the lane that owns the wave's winner writes {key, x, y, z} to the wave's slot of a double-buffered LDS array;
//   4. ONE __syncthreads();
//   5. every wave reads the (at most 16) slots, one per lane, reduces them the same way and takes the winner's
//      coordinates from the lane that holds them -- redundantly in every wave, so nobody waits for a broadcast.
// The dependent chain carries no global memory access: the winner's coordinates travel with the key, the idx /
// min_dist stores of a pick are issued and never waited for.  The slot array is double-buffered by the pick's parity:
// a wave that writes parity p again has passed the barrier of the pick in between, which every wave reaches only
// after it has read parity p.  A 64-thread workgroup (small clouds) needs neither LDS nor barrier.
//
// Workspace path (n beyond the resident limit): the same workgroup, the same device functions in the same order, with
// mind in global memory (each thread re-reads and re-writes only its own entries, so there is nothing to synchronise)
// and the coordinates re-read for every pick.  Same bits.
//
// No workgroup waits for another, no atomics, no host synchronisation.
#include "common.hpp"
#include "wave_dpp.hpp"
#include "../../include/ops/fps.h"

namespace {

constexpr int kResidentMax = 24576;     // 24 points per thread of a 1024-thread workgroup
constexpr int kMaxWaves = 16;

// a thread's (then a wave's, then the cloud's) best point so far
struct Best {
  float d;      // its mind; -1 while there is none (a thread whose points are all beyond the cloud's length)
  int i;
  float x, y, z;
};

struct alignas(16) Slot {
  unsigned long long key;
  float x, y;
  float z, pad0, pad1, pad2;
};

struct Pick {
  int i;
  float d, x, y, z;
};

__device__ __forceinline__ float sqdist(float x, float y, float z, float cx, float cy, float cz) {
  const float dx = x - cx, dy = y - cy, dz = z - cz;
  return ((dx * dx) + (dy * dy)) + (dz * dz);
}

// point i = (x, y, z) against the last pick c: its mind falls to d(x_i, x_c) where that is smaller, and it becomes the
// thread's best if it beats it (callers visit a thread's points in ascending index order)
__device__ __forceinline__ void visit(float x, float y, float z, float &mind, int i, float cx, float cy, float cz,
                                      Best &best) {
  const float d = sqdist(x, y, z, cx, cy, cz);
  mind = d < mind ? d : mind;
  const bool up = mind > best.d;     // selects, not a branch: one compare and five v_cndmask per point
  best.d = up ? mind : best.d;
  best.i = up ? i : best.i;
  best.x = up ? x : best.x;
  best.y = up ? y : best.y;
  best.z = up ? z : best.z;
}

// distance first, lowest index second; 0 (below every point's key) for a thread without a point
__device__ __forceinline__ unsigned long long key_of(const Best &b) {
  return b.d < 0.f ? 0ull : ((unsigned long long)__float_as_uint(b.d) << 32) | (unsigned)~b.i;
}

template <int kCtrl>
__device__ __forceinline__ unsigned long long dpp_max_step(unsigned long long k) {
  const unsigned lo = (unsigned)__builtin_amdgcn_mov_dpp((int)(unsigned)k, kCtrl, 0xf, 0xf, true);
  const unsigned hi = (unsigned)__builtin_amdgcn_mov_dpp((int)(unsigned)(k >> 32), kCtrl, 0xf, 0xf, true);
  const unsigned long long o = ((unsigned long long)hi << 32) | lo;
  return o > k ? o : k;
}
// maximum over each row of 16 lanes, left in every lane of the row (the steps of sn::row16_max on a 64-bit key)
__device__ __forceinline__ unsigned long long row16_max_key(unsigned long long k) {
  k = dpp_max_step<0xB1>(k);    // quad_perm [1,0,3,2]
  k = dpp_max_step<0x4E>(k);    // quad_perm [2,3,0,1]
  k = dpp_max_step<0x141>(k);   // row_half_mirror
  k = dpp_max_step<0x140>(k);   // row_mirror
  return k;
}
__device__ __forceinline__ unsigned long long lane_key(unsigned long long k, int l) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)k, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(k >> 32), l);
  return ((unsigned long long)hi << 32) | lo;
}
// maximum over the 64 lanes, wave-uniform (all lanes active)
__device__ __forceinline__ unsigned long long wave_max_key(unsigned long long k) {
  k = row16_max_key(k);
  const unsigned long long a = lane_key(k, 0), b = lane_key(k, 16), c = lane_key(k, 32), d = lane_key(k, 48);
  const unsigned long long ab = a > b ? a : b, cd = c > d ? c : d;
  return ab > cd ? ab : cd;
}

// the coordinates held by the first lane of `owners` (a ballot)
__device__ __forceinline__ Pick pick_from(unsigned long long key, unsigned long long owners, float x, float y, float z) {
  const int src = __ffsll((long long)owners) - 1;
  Pick p;
  p.i = (int)~(unsigned)key;
  p.d = __uint_as_float((unsigned)(key >> 32));
  p.x = sn::lane_value(x, src);
  p.y = sn::lane_value(y, src);
  p.z = sn::lane_value(z, src);
  return p;
}

// The cloud's next pick from every thread's best: steps 2-5 of the header.  kWaves = workgroup size / 64, a power of
// two; `slots` holds 2 x kWaves entries, `parity` alternates between consecutive calls.  Every thread of the workgroup
// calls it, and at least one has a point.
template <int kWaves>
__device__ __forceinline__ Pick block_pick(const Best &best, Slot *slots, int parity) {
  const unsigned long long key = key_of(best);
  const unsigned long long wmax = wave_max_key(key);
  if constexpr (kWaves == 1) {
    return pick_from(wmax, __ballot(key == wmax), best.x, best.y, best.z);
  } else {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    Slot *mine = slots + parity * kWaves;
    // keys of points are distinct; a wave without a point has several lanes writing the key 0, which never wins
    if (key == wmax) {
      Slot s;
      s.key = key, s.x = best.x, s.y = best.y, s.z = best.z, s.pad0 = s.pad1 = s.pad2 = 0.f;
      mine[wave] = s;
    }
    __syncthreads();
    const Slot s = mine[lane & (kWaves - 1)];     // every row of 16 lanes holds every slot
    const unsigned long long top = row16_max_key(s.key);
    return pick_from(top, __ballot(s.key == top), s.x, s.y, s.z);
  }
}

// where the sampling starts in a cloud of len points (sn::clamped_length): the device value is held to its range
__device__ __forceinline__ int cloud_start(const int *start, int b, int len) {
  const int s = start ? start[b] : 0;
  return s < 0 ? 0 : (s >= len ? len - 1 : s);
}
// an empty cloud's row: -1 / NaN
__device__ __forceinline__ void empty_row(int m, int *idx, float *min_dist) {
  for (int k = threadIdx.x; k < m; k += blockDim.x) {
    idx[k] = -1;
    if (min_dist) min_dist[k] = __uint_as_float(0x7fc00000u);
  }
}

template <int P, int T>
__global__ __launch_bounds__(T) void fps_resident_kernel(int n, int m, const float *__restrict__ xyz,
                                                         const int *__restrict__ lengths,
                                                         const int *__restrict__ start, int *__restrict__ idx,
                                                         float *__restrict__ min_dist) {
  __shared__ Slot slots[2 * (T / 64)];
  const int b = blockIdx.x, t = threadIdx.x;
  const int len = sn::clamped_length(lengths, b, n);
  idx += (size_t)b * m;
  if (min_dist) min_dist += (size_t)b * m;
  if (len == 0) return empty_row(m, idx, min_dist);
  const float *p = xyz + (size_t)b * n * 3;
  float x[P], y[P], z[P], mind[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const int i = t + j * T;
    const bool in = i < len;
    x[j] = in ? p[3 * i] : 0.f;
    y[j] = in ? p[3 * i + 1] : 0.f;
    z[j] = in ? p[3 * i + 2] : 0.f;
    mind[j] = in ? __builtin_inff() : -1.f;     // -1: never updated (d >= 0), never a thread's best
  }
  Pick c;
  c.i = cloud_start(start, b, len);
  c.d = __builtin_inff();
  c.x = p[3 * c.i], c.y = p[3 * c.i + 1], c.z = p[3 * c.i + 2];
  for (int k = 0;; ++k) {
    if (t == 0) {
      idx[k] = c.i;
      if (min_dist) min_dist[k] = c.d;
    }
    if (k + 1 == m) break;
    Best best{-1.f, 0, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < P; ++j) visit(x[j], y[j], z[j], mind[j], t + j * T, c.x, c.y, c.z, best);
    c = block_pick<T / 64>(best, slots, k & 1);
  }
}

constexpr int kWsThreads = 1024;

__global__ __launch_bounds__(kWsThreads) void fps_workspace_kernel(int n, int m, const float *__restrict__ xyz,
                                                                   const int *__restrict__ lengths,
                                                                   const int *__restrict__ start,
                                                                   int *__restrict__ idx, float *__restrict__ min_dist,
                                                                   float *__restrict__ mind) {
  __shared__ Slot slots[2 * (kWsThreads / 64)];
  const int b = blockIdx.x, t = threadIdx.x;
  const int len = sn::clamped_length(lengths, b, n);
  idx += (size_t)b * m;
  if (min_dist) min_dist += (size_t)b * m;
  if (len == 0) return empty_row(m, idx, min_dist);
  const float *p = xyz + (size_t)b * n * 3;
  mind += (size_t)b * n;
  // entry i is read and written by thread i % kWsThreads alone, here and below
  for (int i = t; i < len; i += kWsThreads) mind[i] = __builtin_inff();
  Pick c;
  c.i = cloud_start(start, b, len);
  c.d = __builtin_inff();
  c.x = p[(size_t)3 * c.i], c.y = p[(size_t)3 * c.i + 1], c.z = p[(size_t)3 * c.i + 2];
  for (int k = 0;; ++k) {
    if (t == 0) {
      idx[k] = c.i;
      if (min_dist) min_dist[k] = c.d;
    }
    if (k + 1 == m) break;
    Best best{-1.f, 0, 0.f, 0.f, 0.f};
    for (int i = t; i < len; i += kWsThreads) {
      const float *q = p + (size_t)3 * i;
      float md = mind[i];
      visit(q[0], q[1], q[2], md, i, c.x, c.y, c.z, best);
      mind[i] = md;
    }
    c = block_pick<kWsThreads / 64>(best, slots, k & 1);
  }
}

// clouds of up to this many points stay in registers: 24576, or what SN_FPS_RESIDENT_MAX lowers it to (tests reach the
// workspace path at small n with it)
int resident_max() {
  const char *e = SN_KNOB("SN_FPS_RESIDENT_MAX");
  if (!e || !*e) return kResidentMax;
  const int v = atoi(e);
  return v >= 0 && v < kResidentMax ? v : kResidentMax;
}

float *workspace_layout(sn::Carver &c, int b, int n) { return c.take<float>((size_t)b * n * 4); }

static_assert(kWsThreads / 64 <= kMaxWaves && kResidentMax == 24 * 1024, "slot count / register buckets");

}  // namespace

extern "C" size_t sn_fps_workspace_bytes(int b, int n) {
  if (b < 1 || n < 1 || n <= resident_max()) return 0;
  return sn::layout_bytes(workspace_layout, b, n);
}

extern "C" int sn_fps(const float *xyz, int b, int n, int m, const int *lengths, const int *start, int *idx,
                      float *min_dist, void *workspace, size_t workspace_bytes, void *stream) {
  SN_REQUIRE(xyz && idx, "sn_fps: null pointer");
  SN_REQUIRE(b >= 1 && n >= 1 && m >= 1, "sn_fps: need b,n,m >= 1 (got %d,%d,%d)", b, n, m);
  SN_REQUIRE(n <= (1 << 30), "sn_fps: cloud too large");
  hipStream_t s = sn::as_stream(stream);
  if (n > resident_max()) {
    sn::Carver carver(workspace);
    float *mind = workspace_layout(carver, b, n);
    SN_REQUIRE(workspace && workspace_bytes >= carver.bytes(), "sn_fps: workspace too small (%zu < %zu)",
               workspace_bytes, carver.bytes());
    fps_workspace_kernel<<<b, kWsThreads, 0, s>>>(n, m, xyz, lengths, start, idx, min_dist, mind);
    return sn::launch_status("sn_fps");
  }
  // per-thread point count P and workgroup size T: the smallest bucket that holds the cloud; small clouds take small
  // workgroups so that many of them share a compute unit
#define FPS_LAUNCH(P, T) fps_resident_kernel<P, T><<<b, T, 0, s>>>(n, m, xyz, lengths, start, idx, min_dist)
  if (n <= 64) FPS_LAUNCH(1, 64);
  else if (n <= 256) FPS_LAUNCH(4, 64);
  else if (n <= 1024) FPS_LAUNCH(4, 256);
  else if (n <= 2048) FPS_LAUNCH(8, 256);
  else if (n <= 4096) FPS_LAUNCH(4, 1024);
  else if (n <= 8192) FPS_LAUNCH(8, 1024);
  else if (n <= 16384) FPS_LAUNCH(16, 1024);
  else FPS_LAUNCH(24, 1024);
#undef FPS_LAUNCH
  return sn::launch_status("sn_fps");
}
