// voxel_cell.hpp -- the cell rule and the per-voxel reductions of voxel_grid.hip, written once for host and device (as
// grid_cell.hpp is for occupancy.hip).  include/ops/voxel_grid.h states the rules; every function below is one of its
// sentences.  Integers and double, nothing contracted (the build has -ffp-contract=off).  The second half is the whole
// operator on HOST arrays, one cloud at a time: what sn_voxel_grid_host and sn_voxel_pool_host run.  Nothing here needs
// the HIP runtime, so a plain C++ program can include the file (tools/voxel_cell_host.cpp does, under sanitizers).
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

namespace voxel_cell {

using u64 = unsigned long long;

constexpr int kCellMin = -32768, kCellMax = 32767;      // 16 bits per axis
constexpr u64 kNoKey = 1ull << 48;                       // above every key: a point in no voxel
constexpr int kSum = 0, kMean = 1, kMax = 2;             // the pooling modes

// neither NaN nor infinite
__host__ __device__ inline bool is_finite(float x) { return fabsf(x) <= 3.40282346638528859812e38f; }

// c = floor(((double)x - (double)o) / (double)size) on one axis, as a double: three separately rounded operations, the
// division correctly rounded.  The ROUNDED quotient decides the cell.
__host__ __device__ inline double axis_cell(float x, float o, float size) {
  const double q = ((double)x - (double)o) / (double)size;
  return floor(q);
}

// the key of a point, or kNoKey where it belongs to no voxel (a non-finite coordinate, a cell outside 16 bits)
__host__ __device__ inline u64 key_of(const float *p, float ox, float oy, float oz, float size) {
  if (!(is_finite(p[0]) && is_finite(p[1]) && is_finite(p[2]))) return kNoKey;
  const double c0 = axis_cell(p[0], ox, size), c1 = axis_cell(p[1], oy, size), c2 = axis_cell(p[2], oz, size);
  const double lo = (double)kCellMin, hi = (double)kCellMax;
  if (!(c0 >= lo && c0 <= hi && c1 >= lo && c1 <= hi && c2 >= lo && c2 <= hi)) return kNoKey;
  // (int)(-0.0) is 0
  return ((u64)((int)c0 - kCellMin) << 32) | ((u64)((int)c1 - kCellMin) << 16) | (u64)((int)c2 - kCellMin);
}

// The centroid of the members order(s) .. order(e - 1) of one voxel (ascending point index): per axis the sum of
// (double)x one addition at a time, divided by the member count in double, rounded once.  The coordinates are read
// kBatch members ahead of the additions -- independent loads in flight instead of one dependent index-then-coordinate
// read per addition, which is what a lane waits for -- and added in the same order.
constexpr int kBatch = 8;
template <class IndexAt>
__host__ __device__ inline void centroid(const float *pts, IndexAt index_at, int s, int e, float *out) {
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  int r = s;
  for (; r + kBatch <= e; r += kBatch) {
    float p[kBatch][3];
#pragma unroll
    for (int t = 0; t < kBatch; ++t) {
      const float *q = pts + 3L * index_at(r + t);
      p[t][0] = q[0], p[t][1] = q[1], p[t][2] = q[2];
    }
#pragma unroll
    for (int t = 0; t < kBatch; ++t) a0 = a0 + (double)p[t][0], a1 = a1 + (double)p[t][1], a2 = a2 + (double)p[t][2];
  }
  for (; r < e; ++r) {
    const float *q = pts + 3L * index_at(r);
    a0 = a0 + (double)q[0], a1 = a1 + (double)q[1], a2 = a2 + (double)q[2];
  }
  const double m = (double)(e - s);
  out[0] = (float)(a0 / m), out[1] = (float)(a1 / m), out[2] = (float)(a2 / m);
}

// One (voxel, channel) of the pooling: the entries order[s .. e) that are point indices (in [0, n)) are the members,
// in that order.  sum / mean: the double sum (mean: over the member count), rounded once; max: the first member, then
// every later one with v > best -- the lowest index wins among equals, a NaN never replaces and is only kept when it
// comes first.  No member: 0.0 and -1.  Entries and values are read kBatch ahead, as in centroid(), and taken in order.
__host__ __device__ inline void pool(const float *row, const int *order, int s, int e, int n, int mode, float *out,
                                     int *argmax) {
  double acc = 0.0;
  float best = 0.f;
  int best_i = -1, members = 0;
  for (int r = s; r < e; r += kBatch) {
    int idx[kBatch];
    float val[kBatch];
#pragma unroll
    for (int t = 0; t < kBatch; ++t) {
      const int i = r + t < e ? order[r + t] : -1;
      idx[t] = i >= 0 && i < n ? i : -1;
    }
#pragma unroll
    for (int t = 0; t < kBatch; ++t) val[t] = idx[t] >= 0 ? row[idx[t]] : 0.f;
#pragma unroll
    for (int t = 0; t < kBatch; ++t) {
      if (idx[t] < 0) continue;
      if (mode == kMax) {
        if (members == 0 || val[t] > best) best = val[t], best_i = idx[t];
      } else {
        acc = acc + (double)val[t];
      }
      ++members;
    }
  }
  if (mode == kMax) {
    *out = best;
  } else {
    *out = members == 0 ? 0.f : (float)(mode == kMean ? acc / (double)members : acc);
  }
  if (argmax) *argmax = mode == kMax ? best_i : -1;
}

// the CSR segment of slot v of a cloud, held inside [0, n]; empty for a slot at or beyond min(count, cap)
__host__ __device__ inline void segment(const int *start, int count, int cap, int v, int n, int *s, int *e) {
  const int kept = count < cap ? (count < 0 ? 0 : count) : cap;
  int a = 0, b = 0;
  if (v < kept) {
    a = start[v], b = start[v + 1];
    a = a < 0 ? 0 : (a > n ? n : a);
    b = b < a ? a : (b > n ? n : b);
  }
  *s = a, *e = b;
}

// ---------------------------------------------------------------------------------------------------- host, one cloud
struct CloudOut {      // one cloud's rows; any may be null except count
  int *count;
  float *centroid;     // [cap, 3]
  int *members, *first;      // [cap]
  int *inverse, *order;      // [n]
  int *start;          // [cap + 1]
};

inline void grid_cloud_host(const float *pts, int len, int n, float size, const float *origin, int cap,
                            const CloudOut &o) {
  struct Rec {
    u64 key;
    int index;
  };
  std::vector<Rec> rec;
  rec.reserve((size_t)len);
  for (int i = 0; i < n; ++i) {
    const u64 key = i < len ? key_of(pts + 3L * i, origin[0], origin[1], origin[2], size) : kNoKey;
    if (key != kNoKey) rec.push_back(Rec{key, i});
    else if (o.inverse) o.inverse[i] = -1;
  }
  std::sort(rec.begin(), rec.end(), [](const Rec &a, const Rec &b) {
    return a.key != b.key ? a.key < b.key : a.index < b.index;
  });
  const int valid = (int)rec.size();
  std::vector<int> starts;
  for (int r = 0; r < valid; ++r) {
    if (r == 0 || rec[r].key != rec[r - 1].key) starts.push_back(r);
    const int rank = (int)starts.size() - 1;
    if (o.order) o.order[r] = rec[r].index;
    if (o.inverse) o.inverse[rec[r].index] = rank < cap ? rank : -1;
  }
  if (o.order)
    for (int r = valid; r < n; ++r) o.order[r] = -1;
  const int count = (int)starts.size(), kept = count < cap ? count : cap;
  starts.push_back(valid);
  *o.count = count;
  for (int k = 0; k < cap; ++k) {
    if (k < kept) {
      if (o.centroid) centroid(pts, [&](int r) { return rec[r].index; }, starts[k], starts[k + 1], o.centroid + 3L * k);
      if (o.members) o.members[k] = starts[k + 1] - starts[k];
      if (o.first) o.first[k] = rec[starts[k]].index;
    } else {
      if (o.centroid) o.centroid[3L * k] = o.centroid[3L * k + 1] = o.centroid[3L * k + 2] = 0.f;
      if (o.members) o.members[k] = 0;
      if (o.first) o.first[k] = -1;
    }
  }
  if (o.start)
    for (int k = 0; k <= cap; ++k) o.start[k] = starts[k < kept ? k : kept];
}

// features[c, n], order[n], start[cap + 1] of one cloud -> out[c, cap] (argmax[c, cap], may be null)
inline void pool_cloud_host(const float *features, int c, int n, const int *order, const int *start, int count, int cap,
                            int mode, float *out, int *argmax) {
  for (int ch = 0; ch < c; ++ch)
    for (int v = 0; v < cap; ++v) {
      int s, e;
      segment(start, count, cap, v, n, &s, &e);
      pool(features + (long)ch * n, order, s, e, n, mode, out + (long)ch * cap + v,
           argmax ? argmax + (long)ch * cap + v : nullptr);
    }
}

}  // namespace voxel_cell
