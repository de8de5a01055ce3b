// swd.hip -- sliced Wasserstein distance: project both clouds onto L directions, sort every 1-D projection, solve the
// 1-D transport exactly (include/ops/swd.h states the rules).
//
// Three kernels, launched once per chunk of slices.
//   swd_project_sort_kernel   one workgroup of 1024 lanes per (cloud, slice, side).  A point becomes one 64-bit record
//       in LDS, a double in [1, 2) whose mantissa is (ordered key of its projection) << 14 | index; the records are
//       sorted ascending by a bitonic network, which orders equal keys by index -- the stable order -- because no two
//       records are equal.  -0.0 is made +0.0 before the key is taken (the two compare equal); the array is padded to a
//       power of two W with records 2.0, which sort behind every point, +inf included.  A cloud of 16384 points is
//       128 KiB of records: the sort never leaves LDS.
//       lds_sort.hpp is the network (four steps per pass over LDS in registers, one empty record behind every 16) and
//       says why such records make a compare-exchange one v_min_f64 and one v_max_f64.
//       LDS: (16384 + 1024) * 8 = 139264 bytes, all dynamic (the base stays 16-byte aligned), one workgroup per CU.
//   swd_transport_kernel      one workgroup per (cloud, slice, side), one sorted rank per lane and step: the rank finds
//       its partners on the other side from the mass intervals alone -- no serial merge -- adds its terms in double and
//       drops its gradient coefficient at its point's slot, through the permutation, in an LDS row that is then
//       written out whole; the x side reduces the cost.
//   swd_accumulate_kernel     one lane per point: adds the chunk's coefficient * direction to the gradient in slice
//       order, from 0 in the first chunk, times 1 / L in the last.
#include "common.hpp"
#include "lds_sort.hpp"
#include "../../include/ops/swd.h"

namespace {

using u64 = unsigned long long;
using namespace lds_sort;      // kThreads, slot, lds_bytes, pow2_width, sort_records

constexpr int kMaxPoints = 16384;          // a cloud's records fit one workgroup's LDS
constexpr int kChunkWorkgroups = 512;      // default chunk: this many (cloud, slice) pairs per launch
constexpr int kAccThreads = 256;
constexpr int kIndexBits = 14;             // a record's index field
constexpr u64 kRecordOne = 0x3ff0000000000000ull, kRecordPad = 0x4000000000000000ull;      // 1.0; 2.0 sorts behind all

static_assert(kMaxPoints == 1 << kIndexBits, "the sort's width is a power of two and an index fits its field");
static_assert(lds_bytes(kMaxPoints) == 139264 && lds_bytes(kMaxPoints) <= 160 * 1024, "LDS of one gfx950 CU");

__device__ __forceinline__ float project(const float *pts, int i, float tx, float ty, float tz) {
  const float *q = pts + (size_t)i * 3;
  return ((q[0] * tx) + (q[1] * ty)) + (q[2] * tz);
}

// the record of point i with projection v (-0.0 counts as +0.0): a double in [1, 2) whose mantissa holds
// (ordered key << 14) | index.  Doubles of one sign and exponent order as their bit patterns do, so a compare-exchange
// of two records is one v_min_f64 and one v_max_f64 -- a 64-bit integer compare and four selects otherwise.  Every
// record is a normal number: the minimum and maximum return an operand unchanged.
__device__ __forceinline__ double record(float v, int i) {
  const float c = __float_as_uint(v) == 0x80000000u ? 0.f : v;
  return __longlong_as_double((long long)(kRecordOne | ((u64)sn::ordered_key(c) << kIndexBits) | (unsigned)i));
}
__device__ __forceinline__ int record_index(double r) { return (int)((unsigned)__double_as_longlong(r) & (kMaxPoints - 1)); }

struct SortSide {
  const float *pts;       // [b, n, 3]
  const int *lengths;     // [b] or null
  int n;
  float *sorted;          // [b, stride, n]
  int *perm;              // [b, stride, n]
};

struct SortArgs {
  SortSide side[2];       // blockIdx.y
  const float *dirs;      // [1 or b, slices, 3]
  int slices, dirs_per_cloud;
  int l0, count, stride;  // the chunk: slices l0 .. l0 + count - 1, at rows 0 .. count - 1 of `stride` per cloud
};

__global__ __launch_bounds__(kThreads) void swd_project_sort_kernel(SortArgs a) {
  extern __shared__ __attribute__((aligned(16))) double rec[];
  const SortSide &s = a.side[blockIdx.y];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / a.count, lc = blockIdx.x - b * a.count;
  const int len = sn::clamped_length(s.lengths, b, s.n);
  const float *t = a.dirs + ((size_t)(a.dirs_per_cloud ? b : 0) * a.slices + (a.l0 + lc)) * 3;
  const float tx = t[0], ty = t[1], tz = t[2];
  const float *pts = s.pts + (size_t)b * s.n * 3;
  const int width = pow2_width(len);      // <= pow2_width(s.n): what the launch's LDS holds

  for (int i = tid; i < width; i += kThreads) {
    rec[slot(i)] = i < len ? record(project(pts, i, tx, ty, tz), i) : __longlong_as_double((long long)kRecordPad);
  }
  __syncthreads();
  if (len > 1) sort_records(rec, width, tid);      // uniform over the workgroup
  const size_t row = ((size_t)b * a.stride + lc) * s.n;
  for (int r = tid; r < s.n; r += kThreads) {
    const int i = r < len ? record_index(rec[slot(r)]) : -1;
    s.perm[row + r] = i;
    s.sorted[row + r] = r < len ? project(pts, i, tx, ty, tz) : __builtin_inff();      // the value itself: -0.0 stays
  }
}

struct TransportArgs {
  const float *sorted[2];   // x, y: [b, stride, size]
  const int *perm[2];
  float *coef[2];           // [b, stride, size], by POINT index; null: that side's gradient is not wanted
  const int *lengths[2];
  int size[2];
  int count, stride, l0, slices, p;
  double *cost;             // [b, slices]
};

// LDS, all dynamic: the 1024 partial sums of the cost, then this side's coefficients by point index -- a rank drops its
// coefficient at its point's slot in LDS and the row goes out in whole lines; scattered straight to memory the 4-byte
// writes of a cloud in random order took as long as the rest of the kernel ("Sliced Wasserstein")
constexpr size_t kPartialBytes = kThreads * sizeof(double);
constexpr size_t transport_lds_bytes(int size) { return kPartialBytes + (size_t)size * sizeof(float); }
static_assert(transport_lds_bytes(kMaxPoints) == 73728 && kPartialBytes % 16 == 0, "LDS of the transport");

__global__ __launch_bounds__(kThreads) void swd_transport_kernel(TransportArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char transport_lds[];
  double *partial = reinterpret_cast<double *>(transport_lds);
  float *staged = reinterpret_cast<float *>(transport_lds + kPartialBytes);      // [lq]
  const int q = blockIdx.y, o = 1 - q;      // this side's ranks against the other side
  const int tid = threadIdx.x;
  const int b = blockIdx.x / a.count, lc = blockIdx.x - b * a.count;
  if (q == 1 && !a.coef[1]) return;         // the y side only has a gradient to give
  const int lq = sn::clamped_length(a.lengths[q], b, a.size[q]);
  const int lo_ = sn::clamped_length(a.lengths[o], b, a.size[o]);
  double *cost = a.cost + (size_t)b * a.slices + (a.l0 + lc);
  if (lq == 0 || lo_ == 0) {      // an empty side: cost 0; the accumulation zeroes the gradient without reading coef
    if (q == 0 && tid == 0) *cost = 0.0;
    return;
  }
  const size_t row = (size_t)b * a.stride + lc;
  const float *sq = a.sorted[q] + row * a.size[q];
  const float *so = a.sorted[o] + row * a.size[o];
  const int *perm = a.perm[q] + row * a.size[q];
  float *coef = a.coef[q] ? a.coef[q] + row * a.size[q] : nullptr;
  const double mass = (double)lq * (double)lo_;

  double mine = 0.0;
  for (int i = tid; i < lq; i += kThreads) {
    // rank i's mass interval [i lo_, (i + 1) lo_) in units of 1 / (lq lo_); all of it below 2^28 + 2^14
    const long long begin = (long long)i * lo_, end = begin + lo_;
    const int j0 = (int)((unsigned)begin / (unsigned)lq);
    const int j1 = (int)(((unsigned)end + (unsigned)lq - 1u) / (unsigned)lq);
    const double v = (double)sq[i];
    double t = 0.0, g = 0.0;
    for (int j = j0; j < j1; ++j) {
      const long long ob = (long long)j * lq, oe = ob + lq;
      const double w = (double)((end < oe ? end : oe) - (begin > ob ? begin : ob));
      const double d = v - (double)so[j];
      if (a.p == 2) {
        t = t + w * (d * d);
        g = g + w * (2.0 * d);
      } else {
        t = t + w * __builtin_fabs(d);
        g = g + w * (d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0));
      }
    }
    mine = mine + t;
    if (coef) staged[perm[i]] = (float)(g / mass);      // perm is a bijection of [0, lq): every slot is written
  }
  if (coef) {
    __syncthreads();
    for (int i = tid; i < lq; i += kThreads) coef[i] = staged[i];
  }
  if (q != 0) return;
  partial[tid] = mine;
  __syncthreads();
  for (int h = kThreads / 2; h >= 1; h >>= 1) {
    if (tid < h) partial[tid] = partial[tid] + partial[tid + h];
    __syncthreads();
  }
  if (tid == 0) *cost = partial[0] / mass;
}

struct AccumulateArgs {
  const float *coef;        // [b, stride, n] by point index
  const float *dirs;
  const int *lengths, *other_lengths;
  int n, other_n;
  long total;               // b * n
  int count, stride, l0, slices, dirs_per_cloud;
  int first, last;          // the first chunk starts from 0, the last one scales
  float scale;              // 1 / slices
  float *grad;              // [b, n, 3]
};

__global__ __launch_bounds__(kAccThreads) void swd_accumulate_kernel(AccumulateArgs a) {
  const long gid = (long)blockIdx.x * kAccThreads + threadIdx.x;
  if (gid >= a.total) return;
  const int b = (int)(gid / a.n), i = (int)(gid - (long)b * a.n);
  float *out = a.grad + gid * 3;
  const bool live = i < sn::clamped_length(a.lengths, b, a.n) && sn::clamped_length(a.other_lengths, b, a.other_n) > 0;
  float gx = 0.f, gy = 0.f, gz = 0.f;
  if (live) {
    if (!a.first) gx = out[0], gy = out[1], gz = out[2];
    const float *c = a.coef + (size_t)b * a.stride * a.n + i;
    const float *t = a.dirs + ((size_t)(a.dirs_per_cloud ? b : 0) * a.slices + a.l0) * 3;
    for (int l = 0; l < a.count; ++l) {
      const float w = c[(size_t)l * a.n];
      gx = gx + w * t[l * 3 + 0];
      gy = gy + w * t[l * 3 + 1];
      gz = gz + w * t[l * 3 + 2];
    }
    if (a.last) gx = gx * a.scale, gy = gy * a.scale, gz = gz * a.scale;
  }
  out[0] = gx, out[1] = gy, out[2] = gz;
}

// ---------------------------------------------------------------------------------------------------- host
int chunk_width(int b, int slices) {
  int c = kChunkWorkgroups / b < 1 ? 1 : kChunkWorkgroups / b;
  const char *e = SN_KNOB("SN_SWD_CHUNK");
  if (e && *e) c = atoi(e);
  return c < 1 ? 1 : (c > slices ? slices : c);
}

struct Workspace {
  float *sorted[2];
  int *perm[2];
  float *coef[2];
};

// the one description of the workspace: per side the sorted projections, the permutation and the coefficients of a chunk
Workspace layout(sn::Carver &c, int b, int n, int m, int chunk) {
  Workspace w;
  const int size[2] = {n, m};
  for (int s = 0; s < 2; ++s) {
    const size_t elems = (size_t)b * chunk * size[s];
    w.sorted[s] = c.take256<float>(elems * sizeof(float));
    w.perm[s] = c.take256<int>(elems * sizeof(int));
    w.coef[s] = c.take256<float>(elems * sizeof(float));
  }
  return w;
}

int check_shape(const char *what, int b, int n, int m, int slices) {
  SN_REQUIRE(b >= 1 && n >= 1 && m >= 1 && slices >= 1, "%s: need b,n,m,slices >= 1 (got %d,%d,%d,%d)", what, b, n, m,
             slices);
  SN_REQUIRE(n <= kMaxPoints && m <= kMaxPoints, "%s: a cloud has at most %d points (got %d and %d): one workgroup "
             "sorts a whole cloud in LDS", what, kMaxPoints, n, m);
  SN_REQUIRE((long)b * slices < (1L << 31) && (long)b * (n > m ? n : m) < (1L << 31), "%s: batch too large", what);
  return 0;
}

int launch_sort(const char *what, const SortArgs &a, int b, int sides, int widest, hipStream_t stream) {
  const size_t lds = lds_bytes(pow2_width(widest));
  SN_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&swd_project_sort_kernel),
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(kMaxPoints)));
  swd_project_sort_kernel<<<dim3((unsigned)(b * a.count), sides), kThreads, lds, stream>>>(a);
  return sn::launch_status(what);
}

}  // namespace

extern "C" size_t sn_swd_workspace_bytes(int b, int n, int m, int slices) {
  if (b < 1 || n < 1 || m < 1 || slices < 1) return 0;
  sn::Carver c(nullptr);
  layout(c, b, n, m, chunk_width(b, slices));
  return c.bytes();
}

extern "C" int sn_swd_forward(const float *x, const float *y, const float *dirs, int b, int n, int m, int slices,
                              int dirs_per_cloud, const int *x_lengths, const int *y_lengths, int p, double *cost,
                              float *gradx, float *grady, void *workspace, size_t workspace_bytes, void *stream) {
  SN_REQUIRE(x && y && dirs && cost, "sn_swd_forward: null pointer");
  if (const int rc = check_shape("sn_swd_forward", b, n, m, slices)) return rc;
  SN_REQUIRE(p == 1 || p == 2, "sn_swd_forward: p must be 1 or 2 (got %d)", p);
  const int chunk = chunk_width(b, slices);
  sn::Carver carver(workspace);
  const Workspace w = layout(carver, b, n, m, chunk);
  SN_REQUIRE(workspace && workspace_bytes >= carver.bytes(), "sn_swd_forward: workspace too small (%zu < %zu)",
             workspace_bytes, carver.bytes());
  hipStream_t s = sn::as_stream(stream);
  float *grad[2] = {gradx, grady};
  const float *pts[2] = {x, y};
  const int *lengths[2] = {x_lengths, y_lengths};
  const int size[2] = {n, m};

  for (int l0 = 0; l0 < slices; l0 += chunk) {
    const int count = slices - l0 < chunk ? slices - l0 : chunk;
    SortArgs sa{};
    TransportArgs ta{};
    for (int k = 0; k < 2; ++k) {
      sa.side[k] = SortSide{pts[k], lengths[k], size[k], w.sorted[k], w.perm[k]};
      ta.sorted[k] = w.sorted[k], ta.perm[k] = w.perm[k], ta.coef[k] = grad[k] ? w.coef[k] : nullptr;
      ta.lengths[k] = lengths[k], ta.size[k] = size[k];
    }
    sa.dirs = dirs, sa.slices = slices, sa.dirs_per_cloud = dirs_per_cloud;
    sa.l0 = l0, sa.count = count, sa.stride = chunk;
    if (const int rc = launch_sort("sn_swd_forward", sa, b, 2, n > m ? n : m, s)) return rc;
    ta.count = count, ta.stride = chunk, ta.l0 = l0, ta.slices = slices, ta.p = p, ta.cost = cost;
    SN_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&swd_transport_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)transport_lds_bytes(kMaxPoints)));
    swd_transport_kernel<<<dim3((unsigned)(b * count), 2), kThreads, transport_lds_bytes(n > m ? n : m), s>>>(ta);
    if (const int rc = sn::launch_status("sn_swd_forward")) return rc;
    for (int k = 0; k < 2; ++k) {
      if (!grad[k]) continue;
      AccumulateArgs aa{w.coef[k], dirs, lengths[k], lengths[1 - k], size[k], size[1 - k], (long)b * size[k], count,
                        chunk, l0, slices, dirs_per_cloud, l0 == 0, l0 + count == slices, 1.0f / (float)slices, grad[k]};
      swd_accumulate_kernel<<<(unsigned)sn::ceil_div((int)aa.total, kAccThreads), kAccThreads, 0, s>>>(aa);
      if (const int rc = sn::launch_status("sn_swd_forward")) return rc;
    }
  }
  return 0;
}

extern "C" int sn_swd_project_sort(const float *x, const float *dirs, int b, int n, int slices, int dirs_per_cloud,
                                   const int *lengths, float *sorted, int *perm, void *stream) {
  SN_REQUIRE(x && dirs && sorted && perm, "sn_swd_project_sort: null pointer");
  if (const int rc = check_shape("sn_swd_project_sort", b, n, 1, slices)) return rc;
  SortArgs sa{};
  sa.side[0] = SortSide{x, lengths, n, sorted, perm};
  sa.dirs = dirs, sa.slices = slices, sa.dirs_per_cloud = dirs_per_cloud;
  sa.l0 = 0, sa.count = slices, sa.stride = slices;
  return launch_sort("sn_swd_project_sort", sa, b, 1, n, sn::as_stream(stream));
}
