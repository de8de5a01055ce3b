// dcd.hip -- density-aware Chamfer distance from a finished nearest-neighbour search: counts, loss and gradient in one
// pass over inverse lists built once (include/ops/dcd.h states the rules).  Device and host code in one file: the
// arithmetic of a point is written once, as __host__ __device__ functions, so the two entry points return equal bits.
//
// Per call, after build_index_lists (index_lists.hpp) has inverted idx1 over the m targets and idx2 over the n:
//   dcd_point_kernel    one lane per point of either cloud: the length of its own list (its count), the length of its
//       neighbour's list, from those e, the term of the loss and the coefficient a of the gradient; the owner of a list
//       of more than kLongList entries puts itself on the list of long lists.
//   dcd_gather_kernel   one lane per point: sorts its own list (the fill's order is arbitrary, the defined order is
//       ascending) and adds own term and list terms in double.
//   dcd_long_kernel     one workgroup per long list: bitonic sort in LDS up to kLongSortCap entries, in place by one
//       thread beyond that; the products 256 at a time by the workgroup, the three running sums by three lanes, in order.
//   dcd_sum_kernel      one workgroup per (cloud, side): the 1024 strided partial sums and their binary tree.
// chamfer.hip's backward is the model (gather instead of scatter); the sort of a list, the two thresholds and the rule
// for long lists are sorted_lists.hpp's, shared with it.
#include <algorithm>
#include <cmath>
#include <cstring>      // the host's memcpy, for sn_expf.h
#include <vector>

#include "common.hpp"
#include "host_threads.hpp"
#include "index_lists.hpp"
#include "sorted_lists.hpp"
#include "../../include/ops/dcd.h"
#include "../../include/sn_expf.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSumThreads = 1024;    // the loss's partial sums: part of the definition

enum Power { kPowerZero, kPowerHalf, kPowerOne };      // n_lambda 0, 0.5, 1

struct Rule {
  float alpha;
  int power, ratio;
};

// ---------------------------------------------------------------- the arithmetic of a point, shared by host and device
struct PointTerms {
  double term, a;      // 1 - e W and alpha e W / own_len
};
// a point at squared distance `dist` from a neighbour that c points chose; own_len queries against other_len targets
__host__ __device__ inline PointTerms point_terms(const Rule &r, float dist, int c, int own_len, int other_len) {
  const float e = sn_expf(-(r.alpha * dist));
  const double p = r.power == kPowerZero ? 1.0 : (r.power == kPowerHalf ? sqrt((double)c) : (double)c);
  const double w = (r.ratio ? (double)own_len / (double)other_len : 1.0) / p;
  return {1.0 - (double)e * w, (((double)r.alpha * (double)e) * w) / (double)own_len};
}
// a point whose index names no target: term 1, no gradient
__host__ __device__ inline PointTerms unmatched_terms() { return {1.0, 0.0}; }

__host__ __device__ inline double own_term(double a, float mine, float neighbour) {
  return a * ((double)mine - (double)neighbour);
}
__host__ __device__ inline double list_step(double acc, double a, float theirs, float mine) {
  return acc - a * ((double)theirs - (double)mine);
}

// ---------------------------------------------------------------------------------------------------- device
struct Side {              // a cloud as the one that asks: its points, their neighbours in the other cloud
  const float *xyz;        // [b, size, 3]
  const float *dist;       // [b, size]
  const int *idx;          // [b, size]
  const int *lengths;      // [b] or null
  int size;
  const int *ends;         // [b, size]  where each point's own list ends (index_lists.hpp: the ends after the fill)
  int *list;               // [b, other size]  those lists: the points of the other cloud that chose me
  double *a;               // [b, size]  gradient coefficients
  double *term;            // [b, size]
  int *count;              // [b, size] or null
  float *grad;             // [b, size, 3] or null
};

struct Args {
  Side side[2];
  Rule rule;
  long total1, total;      // b * n, b * (n + m)
  int *longs;              // [0]: how many long lists, then their owners' element numbers
  double *sides;           // [b, 2]
};

struct Point {
  int s, b, i;             // side, cloud, row
  long f;                  // b * size + i
  int own_len, other_len;
  bool valid;              // a point of its cloud, in a pair without an empty side
};
__device__ __forceinline__ Point point_of(const Args &a, long e) {
  Point p;
  p.s = e >= a.total1;
  p.f = p.s ? e - a.total1 : e;
  const int size = a.side[p.s].size;
  p.b = (int)(p.f / size);
  p.i = (int)(p.f - (long)p.b * size);
  p.own_len = sn::clamped_length(a.side[p.s].lengths, p.b, size);
  p.other_len = sn::clamped_length(a.side[1 - p.s].lengths, p.b, a.side[1 - p.s].size);
  p.valid = p.i < p.own_len && p.other_len > 0;
  return p;
}
// start and length of row i's list among cloud b's
__device__ __forceinline__ int list_start(const Side &s, int b, int i) {
  return i ? s.ends[(long)b * s.size + i - 1] : 0;
}
__device__ __forceinline__ int list_length(const Side &s, int b, int i) {
  return s.ends[(long)b * s.size + i] - list_start(s, b, i);
}

__global__ __launch_bounds__(kThreads) void dcd_point_kernel(Args a) {
  const long e = (long)blockIdx.x * kThreads + threadIdx.x;
  if (e >= a.total) return;
  const Point p = point_of(a, e);
  const Side &me = a.side[p.s], &other = a.side[1 - p.s];
  const int chosen_by = p.valid ? list_length(me, p.b, p.i) : 0;
  if (me.count) me.count[p.f] = chosen_by;
  PointTerms t{0.0, 0.0};
  if (p.valid) {
    const int k = me.idx[p.f];
    t = k >= 0 && k < p.other_len ? point_terms(a.rule, me.dist[p.f], list_length(other, p.b, k), p.own_len, p.other_len)
                                  : unmatched_terms();
    if (chosen_by > kLongList && me.grad) register_long_list(a.longs, (int)e);
  }
  me.term[p.f] = t.term;
  me.a[p.f] = t.a;
}

// the own term of a valid point, per component: 0 where its index names no target (nothing of the other cloud is read)
__device__ __forceinline__ void own_terms(const Args &a, const Point &p, const float *mine, double acc[3]) {
  const Side &me = a.side[p.s], &other = a.side[1 - p.s];
  const int k = me.idx[p.f];
  acc[0] = acc[1] = acc[2] = 0.0;
  if (k < 0 || k >= p.other_len) return;
  const float *q = other.xyz + ((long)p.b * other.size + k) * 3;
  const double c = me.a[p.f];
  for (int d = 0; d < 3; ++d) acc[d] = own_term(c, mine[d], q[d]);
}

__global__ __launch_bounds__(kThreads) void dcd_gather_kernel(Args a) {
  const long e = (long)blockIdx.x * kThreads + threadIdx.x;
  if (e >= a.total) return;
  const Point p = point_of(a, e);
  const Side &me = a.side[p.s], &other = a.side[1 - p.s];
  if (!me.grad) return;
  float *out = me.grad + p.f * 3;
  if (!p.valid) {
    out[0] = out[1] = out[2] = 0.f;
    return;
  }
  const int c = list_length(me, p.b, p.i);
  if (c > kLongList) return;      // dcd_long_kernel's
  int *lst = me.list + (long)p.b * other.size + list_start(me, p.b, p.i);
  if (c > 1) sort_ints(lst, c);
  const float mine[3] = {me.xyz[p.f * 3], me.xyz[p.f * 3 + 1], me.xyz[p.f * 3 + 2]};
  double acc[3];
  own_terms(a, p, mine, acc);
  for (int t = 0; t < c; ++t) {
    const long q = (long)p.b * other.size + lst[t];
    const double cq = other.a[q];
    for (int d = 0; d < 3; ++d) acc[d] = list_step(acc[d], cq, other.xyz[q * 3 + d], mine[d]);
  }
  out[0] = (float)acc[0], out[1] = (float)acc[1], out[2] = (float)acc[2];
}

__global__ __launch_bounds__(kThreads) void dcd_long_kernel(Args a) {
  extern __shared__ int keys[];      // kLongSortCap ints
  __shared__ double terms[3][kThreads];
  const int tid = threadIdx.x;
  const int nlong = a.longs[0];
  for (int li = blockIdx.x; li < nlong; li += gridDim.x) {
    const Point p = point_of(a, a.longs[1 + li]);
    const Side &me = a.side[p.s], &other = a.side[1 - p.s];
    const int c = list_length(me, p.b, p.i);
    int *lst = me.list + (long)p.b * other.size + list_start(me, p.b, p.i);
    sort_long_list<kThreads>(lst, c, keys);      // its first barrier also stands behind the previous list's terms
    const float *xyz = me.xyz + p.f * 3;
    const float mine[3] = {xyz[0], xyz[1], xyz[2]};
    double own[3];
    own_terms(a, p, mine, own);
    double acc = tid < 3 ? own[tid] : 0.0;      // lanes 0..2: x, y, z
    for (int base = 0; base < c; base += kThreads) {
      const int t = base + tid;
      if (t < c) {
        const long q = (long)p.b * other.size + sorted_entry(lst, c, keys, t);
        const double cq = other.a[q];
        // list_step's product; its subtraction is taken below, in order
        for (int d = 0; d < 3; ++d) terms[d][tid] = cq * ((double)other.xyz[q * 3 + d] - (double)mine[d]);
      }
      __syncthreads();
      const int lim = c - base < kThreads ? c - base : kThreads;
      if (tid < 3)
        for (int t2 = 0; t2 < lim; ++t2) acc = acc - terms[tid][t2];
      __syncthreads();
    }
    if (tid < 3) me.grad[p.f * 3 + tid] = (float)acc;
  }
}

__global__ __launch_bounds__(kSumThreads) void dcd_sum_kernel(Args a) {
  __shared__ double partial[kSumThreads];
  const int b = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
  const Side &me = a.side[s];
  const int len = sn::clamped_length(me.lengths, b, me.size);
  const int other_len = sn::clamped_length(a.side[1 - s].lengths, b, a.side[1 - s].size);
  double *out = a.sides + (long)b * 2 + s;
  if (len == 0 || other_len == 0) {
    if (tid == 0) *out = 0.0;
    return;
  }
  const double *term = me.term + (long)b * me.size;
  double mine = 0.0;
  for (int i = tid; i < len; i += kSumThreads) mine = mine + term[i];
  partial[tid] = mine;
  __syncthreads();
  for (int h = kSumThreads / 2; h >= 1; h >>= 1) {
    if (tid < h) partial[tid] = partial[tid] + partial[tid + h];
    __syncthreads();
  }
  if (tid == 0) *out = partial[0] / (double)len;
}

struct Workspace {
  IndexLists chosen[2];      // [s]: who chose the points of side s -- the other side's indices inverted
  double *a[2], *term[2];
  int *longs;
};

// the one description of the workspace
Workspace layout(sn::Carver &c, int b, int n, int m) {
  Workspace w;
  const int size[2] = {n, m};
  for (int s = 0; s < 2; ++s) {
    w.chosen[s].offs = c.take256<int>((size_t)b * size[s] * sizeof(int));
    w.chosen[s].list = c.take256<int>((size_t)b * size[1 - s] * sizeof(int));
    w.a[s] = c.take256<double>((size_t)b * size[s] * sizeof(double));
    w.term[s] = c.take256<double>((size_t)b * size[s] * sizeof(double));
  }
  // a list of more than kLongList entries takes that many of the other cloud's points: at most size / 65 per side
  w.longs = c.take256<int>(((size_t)b * ((size_t)n + m) / kLongList + 2) * sizeof(int));
  return w;
}

// shape and rule, the same for both entry points; `power` comes back for the Rule
int check_arguments(const char *what, int b, int n, int m, float alpha, float n_lambda, int ratio, int *power) {
  SN_REQUIRE(b >= 1 && n >= 1 && m >= 1, "%s: need b,n,m >= 1 (got %d,%d,%d)", what, b, n, m);
  SN_REQUIRE((long)b * ((long)n + m) < (1L << 30), "%s: too large (b * (n + m) must stay below 2^30)", what);
  SN_REQUIRE(std::isfinite(alpha) && alpha >= 0.f, "%s: alpha must be finite and >= 0 (got %g)", what, (double)alpha);
  SN_REQUIRE(n_lambda == 0.f || n_lambda == 0.5f || n_lambda == 1.f, "%s: n_lambda must be exactly 0, 0.5 or 1 (got %g)",
             what, (double)n_lambda);
  SN_REQUIRE(ratio == 0 || ratio == 1, "%s: ratio must be 0 or 1 (got %d)", what, ratio);
  *power = n_lambda == 0.f ? kPowerZero : (n_lambda == 0.5f ? kPowerHalf : kPowerOne);
  return 0;
}

// ---------------------------------------------------------------------------------------------------- host
// the points of `mine` that chose each of the `targets` points, ascending inside a list: starts[targets + 1], list
void invert_host(const int *idx, int queries, int targets, std::vector<int> &starts, std::vector<int> &list) {
  starts.assign((size_t)targets + 1, 0);
  for (int i = 0; i < queries; ++i)
    if (idx[i] >= 0 && idx[i] < targets) ++starts[(size_t)idx[i] + 1];
  for (int k = 0; k < targets; ++k) starts[(size_t)k + 1] += starts[k];
  list.resize((size_t)starts[targets]);
  std::vector<int> next(starts.begin(), starts.end() - 1);
  for (int i = 0; i < queries; ++i)
    if (idx[i] >= 0 && idx[i] < targets) list[(size_t)next[idx[i]]++] = i;
}

struct HostSide {
  const float *xyz, *dist;
  const int *idx;
  int size, len;
  int *count;
  float *grad;
  std::vector<int> starts, list;      // who chose my points
  std::vector<double> a;
};

void cloud_host(HostSide (&side)[2], const Rule &rule, double *sides) {
  for (int s = 0; s < 2; ++s) {
    if (side[s].count) std::fill(side[s].count, side[s].count + side[s].size, 0);
    if (side[s].grad) std::fill(side[s].grad, side[s].grad + (size_t)side[s].size * 3, 0.f);
    sides[s] = 0.0;
  }
  if (side[0].len == 0 || side[1].len == 0) return;
  for (int s = 0; s < 2; ++s) {
    const HostSide &other = side[1 - s];
    invert_host(other.idx, other.len, side[s].len, side[s].starts, side[s].list);
  }
  for (int s = 0; s < 2; ++s) {
    HostSide &me = side[s];
    const HostSide &other = side[1 - s];
    me.a.assign((size_t)me.len, 0.0);
    std::vector<double> partial(kSumThreads, 0.0);
    for (int i = 0; i < me.len; ++i) {
      if (me.count) me.count[i] = me.starts[(size_t)i + 1] - me.starts[i];
      const int k = me.idx[i];
      const PointTerms t = k >= 0 && k < other.len
                               ? point_terms(rule, me.dist[i], other.starts[(size_t)k + 1] - other.starts[k], me.len, other.len)
                               : unmatched_terms();
      me.a[i] = t.a;
      partial[i % kSumThreads] = partial[i % kSumThreads] + t.term;
    }
    for (int h = kSumThreads / 2; h >= 1; h >>= 1)
      for (int t = 0; t < h; ++t) partial[t] = partial[t] + partial[t + h];
    sides[s] = partial[0] / (double)me.len;
  }
  for (int s = 0; s < 2; ++s) {
    const HostSide &me = side[s], &other = side[1 - s];
    if (!me.grad) continue;
    for (int i = 0; i < me.len; ++i) {
      const float *mine = me.xyz + (size_t)i * 3;
      const int k = me.idx[i];
      const bool matched = k >= 0 && k < other.len;
      for (int d = 0; d < 3; ++d) {
        double acc = matched ? own_term(me.a[i], mine[d], other.xyz[(size_t)k * 3 + d]) : 0.0;
        for (int t = me.starts[i]; t < me.starts[(size_t)i + 1]; ++t) {
          const int j = me.list[t];
          acc = list_step(acc, other.a[j], other.xyz[(size_t)j * 3 + d], mine[d]);
        }
        me.grad[(size_t)i * 3 + d] = (float)acc;
      }
    }
  }
}

}  // namespace

extern "C" size_t sn_dcd_workspace_bytes(int b, int n, int m) {
  if (b < 1 || n < 1 || m < 1) return 0;
  return sn::layout_bytes(layout, b, n, m);
}

extern "C" int sn_dcd_from_search(const float *xyz1, const float *xyz2, const float *dist1, const int *idx1,
                                  const float *dist2, const int *idx2, int b, int n, int m, const int *lengths1,
                                  const int *lengths2, float alpha, float n_lambda, int ratio, double *sides,
                                  int *count1, int *count2, float *gradxyz1, float *gradxyz2, void *workspace,
                                  size_t workspace_bytes, void *stream) {
  const char *what = "sn_dcd_from_search";
  SN_REQUIRE(xyz1 && xyz2 && dist1 && idx1 && dist2 && idx2 && sides && workspace, "%s: null pointer", what);
  int power = 0;
  if (const int rc = check_arguments(what, b, n, m, alpha, n_lambda, ratio, &power)) return rc;
  sn::Carver carver(workspace);
  const Workspace w = layout(carver, b, n, m);
  SN_REQUIRE(workspace_bytes >= carver.bytes(), "%s: workspace too small (%zu < %zu)", what, workspace_bytes,
             carver.bytes());
  hipStream_t s = sn::as_stream(stream);

  // who chose the points of cloud 1: idx2 over the n targets; of cloud 2: idx1 over the m
  if (const int rc = build_index_lists(what, idx2, b, n, (long)m, w.chosen[0], s)) return rc;
  if (const int rc = build_index_lists(what, idx1, b, m, (long)n, w.chosen[1], s)) return rc;
  SN_HIP(hipMemsetAsync(w.longs, 0, sizeof(int), s));

  Args a{};
  a.side[0] = Side{xyz1, dist1, idx1, lengths1, n, w.chosen[0].offs, w.chosen[0].list, w.a[0], w.term[0], count1, gradxyz1};
  a.side[1] = Side{xyz2, dist2, idx2, lengths2, m, w.chosen[1].offs, w.chosen[1].list, w.a[1], w.term[1], count2, gradxyz2};
  a.rule = Rule{alpha, power, ratio};
  a.total1 = (long)b * n, a.total = (long)b * ((long)n + m);
  a.longs = w.longs;
  a.sides = sides;
  const unsigned blocks = (unsigned)((a.total + kThreads - 1) / kThreads);
  dcd_point_kernel<<<blocks, kThreads, 0, s>>>(a);
  if (const int rc = sn::launch_status(what)) return rc;
  if (gradxyz1 || gradxyz2) {
    dcd_gather_kernel<<<blocks, kThreads, 0, s>>>(a);
    if (const int rc = sn::launch_status(what)) return rc;
    // the lists beyond kLongList entries (none between trained clouds: the kernel then reads one word and leaves)
    SN_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&dcd_long_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, kLongSortCap * (int)sizeof(int)));
    dcd_long_kernel<<<kLongBlocks, kThreads, kLongSortCap * sizeof(int), s>>>(a);
    if (const int rc = sn::launch_status(what)) return rc;
  }
  dcd_sum_kernel<<<dim3((unsigned)b, 2), kSumThreads, 0, s>>>(a);
  return sn::launch_status(what);
}

extern "C" int sn_dcd_from_search_host(const float *xyz1, const float *xyz2, const float *dist1, const int *idx1,
                                       const float *dist2, const int *idx2, int b, int n, int m, const int *lengths1,
                                       const int *lengths2, float alpha, float n_lambda, int ratio, double *sides,
                                       int *count1, int *count2, float *gradxyz1, float *gradxyz2, int threads) {
  const char *what = "sn_dcd_from_search_host";
  SN_REQUIRE(xyz1 && xyz2 && dist1 && idx1 && dist2 && idx2 && sides, "%s: null pointer", what);
  int power = 0;
  if (const int rc = check_arguments(what, b, n, m, alpha, n_lambda, ratio, &power)) return rc;
  const Rule rule{alpha, power, ratio};
  parallel_items(b, threads, [&](long c) {
    const size_t o1 = (size_t)c * n, o2 = (size_t)c * m;
    HostSide side[2] = {
        {xyz1 + o1 * 3, dist1 + o1, idx1 + o1, n, sn::clamped_length(lengths1, c, n), count1 ? count1 + o1 : nullptr,
         gradxyz1 ? gradxyz1 + o1 * 3 : nullptr, {}, {}, {}},
        {xyz2 + o2 * 3, dist2 + o2, idx2 + o2, m, sn::clamped_length(lengths2, c, m), count2 ? count2 + o2 : nullptr,
         gradxyz2 ? gradxyz2 + o2 * 3 : nullptr, {}, {}, {}}};
    cloud_host(side, rule, sides + (size_t)c * 2);
  });
  return 0;
}
