// voxel_grid.hip -- voxel-grid subsampling and pooling (include/ops/voxel_grid.h states the rules; voxel_cell.hpp is
// the cell rule and the per-voxel reductions, compiled here for the device and for the host entry points).
//
//   voxel_resident_kernel   n <= 16384.  One workgroup of 1024 lanes owns whole clouds and loops over them.  A point
//       becomes the 64-bit record ((key << 14) | index) + 2^52 in LDS: below 2^62 + 2^52 and at least 2^52, so as a double
//       it is positive, finite and NORMAL (without the 2^52 the cells next to -32768 would be denormals) and two records
//       compare as their bit patterns do -- a compare-exchange is one v_min_f64 and one v_max_f64: the records
//       are sorted by lds_sort.hpp's network, as those of swd.hip are.  Padding rows and points in no voxel get the
//       record 4.0, which sorts behind every point.  Behind the sort reduce_cloud() runs on the LDS records.
//   voxel_chunk_sort_kernel, voxel_merge_kernel, voxel_reduce_kernel   n above the resident size.  Chunks of the
//       resident size are sorted the same way (the record's index is the position inside the chunk) and written to the
//       workspace as a key array and an index array; passes of a stable merge double the run length -- one output per
//       lane, its place found by a binary search in the partner run (the merge path of a single element), on equal keys
//       the lower run first; reduce_cloud() then runs on the workspace arrays, one workgroup per cloud.
//   reduce_cloud()   over the sorted records of one cloud, 1024 positions per step: a record starts a voxel where its
//       key differs from its predecessor's, sn::BlockScan ranks the heads, and every lane writes its record's inverse
//       and order entries and, for a head, the voxel's start.  Then one lane per kept voxel walks its segment in order,
//       reads the members' coordinates by index and accumulates in double (voxel_cell::centroid): the sum's order is the
//       header's order whatever the launch.  On the resident path the starts and the sorted indices live in the halves
//       of the records they replace, so LDS holds nothing but the sort's array and the scan.
//   voxel_pool_kernel   one lane per (voxel, channel), neighbouring lanes on neighbouring voxels of one channel.
// No floating-point atomics, nobody waits for another workgroup, no scratch.
#include <cmath>

#include "block_scan.hpp"
#include "common.hpp"
#include "host_threads.hpp"
#include "lds_sort.hpp"
#include "voxel_cell.hpp"
#include "../../include/ops/voxel_grid.h"

namespace {

using namespace lds_sort;      // kThreads, slot, lds_bytes, pow2_width, sort_records
using voxel_cell::kNoKey;
using voxel_cell::u64;

constexpr int kResidentMax = 16384;        // a cloud's records fit one workgroup's LDS
constexpr int kBigMax = 1 << 24;           // the workspace path's limit
constexpr int kIndexBits = 14;             // a record's index field
constexpr int kMergeThreads = 256, kPoolThreads = 256;
constexpr u64 kRecordBias = 1ull << 52;                  // added to every record: the exponent field is never 0
constexpr u64 kRecordPad = (kNoKey << kIndexBits) + kRecordBias;      // behind every record; its key field is kNoKey

static_assert(kResidentMax == 1 << kIndexBits, "the sort's width is a power of two and an index fits its field");
static_assert(lds_bytes(kResidentMax) == 139264 && lds_bytes(kResidentMax) + 256 <= 160 * 1024, "LDS of one gfx950 CU");
static_assert(((kRecordPad - kRecordBias) >> kIndexBits) == kNoKey, "the pad record's key is that of a point in no voxel");
static_assert(kRecordPad == 0x4010000000000000ull, "4.0: a normal, finite double, as every record below it");

struct GridArgs {
  const float *xyz;        // [b, n, 3]
  const int *lengths;      // [b] or null
  int b, n, cap;
  float size, ox, oy, oz;
  int *count;              // [b]
  float *centroid;         // [b, cap, 3] or null
  int *members, *first;    // [b, cap] or null
  int *inverse, *order;    // [b, n] or null
  int *start;              // [b, cap + 1] or null
};

struct Shared {
  sn::BlockScan<kThreads> scan;
  int valid;               // the number of records that have a voxel
  u64 last_key;            // the key of the last position of the step before
};

// the sorted records of a cloud in LDS.  set_index / set_start turn record r into two words: the low one the point
// index of position r, the high one the start of voxel r -- rank <= position, and a step's records are all in
// registers before its first word is replaced.
typedef int __attribute__((may_alias)) record_word;      // a half of a record that has been replaced
struct ResidentView {
  double *rec;
  __device__ u64 key(int r) const { return ((u64)__double_as_longlong(rec[slot(r)]) - kRecordBias) >> kIndexBits; }
  __device__ int index(int r) const { return (int)((unsigned)__double_as_longlong(rec[slot(r)]) & (kResidentMax - 1)); }
  __device__ void set_index(int r, int i) const { reinterpret_cast<record_word *>(rec)[2 * slot(r)] = i; }
  __device__ int sorted_index(int r) const { return reinterpret_cast<const record_word *>(rec)[2 * slot(r)]; }
  __device__ void set_start(int k, int r) const { reinterpret_cast<record_word *>(rec)[2 * slot(k) + 1] = r; }
  __device__ int start(int k) const { return reinterpret_cast<const record_word *>(rec)[2 * slot(k) + 1]; }
};

// the merged arrays of a cloud in the workspace; the starts in a third array
struct WorkspaceView {
  const u64 *keys;
  const int *idx;
  int *starts;
  __device__ u64 key(int r) const { return keys[r]; }
  __device__ int index(int r) const { return idx[r]; }
  __device__ void set_index(int, int) const {}
  __device__ int sorted_index(int r) const { return idx[r]; }
  __device__ void set_start(int k, int r) const { starts[k] = r; }
  __device__ int start(int k) const { return starts[k]; }
};

// Heads, ranks and reductions of cloud `cloud`, whose sorted records are positions 0 .. limit - 1 of `v` (the records
// that have a voxel first).  Every lane of the workgroup calls it; ends in a barrier.
template <class View>
__device__ __forceinline__ void reduce_cloud(const View &v, int limit, Shared &sh, const GridArgs &a, int cloud) {
  const int tid = threadIdx.x, n = a.n, cap = a.cap;
  const float *pts = a.xyz + (long)cloud * n * 3;
  int *inverse = a.inverse ? a.inverse + (long)cloud * n : nullptr;
  int *order = a.order ? a.order + (long)cloud * n : nullptr;
  if (tid == 0) sh.valid = limit;
  sh.scan.reset(0);
  const int end = limit > n ? limit : n;
  for (int base = 0; base < end; base += kThreads) {
    const int r = base + tid;
    const u64 key = r < limit ? v.key(r) : kNoKey;
    const int index = r < limit ? v.index(r) : -1;
    const u64 pred = tid > 0 ? (r - 1 < limit ? v.key(r - 1) : kNoKey) : (base == 0 ? kNoKey : sh.last_key);
    const bool has = key != kNoKey;
    const bool head = has && (r == 0 || key != pred);
    if (!has && r <= limit && (r == 0 || pred != kNoKey)) sh.valid = r;      // the first record without a voxel: one lane
    sh.scan.chunk(head ? 1 : 0, [&](int exclusive) {
      if (has) {
        const int rank = exclusive + (head ? 1 : 0) - 1;
        v.set_index(r, index);
        if (order) order[r] = index;
        if (inverse) inverse[index] = rank < cap ? rank : -1;
        if (head) v.set_start(rank, r);
      } else if (order && r < n) {
        order[r] = -1;
      }
      if (tid == kThreads - 1) sh.last_key = key;
    });
  }
  const int count = sh.scan.carry, valid = sh.valid;
  const int kept = count < cap ? count : cap;
  const int kept_end = kept < count ? v.start(kept) : valid;
  if (tid == 0) a.count[cloud] = count;
  float *centroid = a.centroid ? a.centroid + (long)cloud * cap * 3 : nullptr;
  int *members = a.members ? a.members + (long)cloud * cap : nullptr;
  int *first = a.first ? a.first + (long)cloud * cap : nullptr;
  int *start = a.start ? a.start + (long)cloud * (cap + 1) : nullptr;
  for (int k = tid; k <= cap; k += kThreads) {
    if (k < kept) {
      const int s = v.start(k), e = k + 1 < count ? v.start(k + 1) : valid;
      if (centroid) voxel_cell::centroid(pts, [&](int r) { return v.sorted_index(r); }, s, e, centroid + 3L * k);
      if (members) members[k] = e - s;
      if (first) first[k] = v.sorted_index(s);
      if (start) start[k] = s;
    } else {
      if (k < cap) {
        if (centroid) centroid[3L * k] = centroid[3L * k + 1] = centroid[3L * k + 2] = 0.f;
        if (members) members[k] = 0;
        if (first) first[k] = -1;
      }
      if (start) start[k] = kept_end;
    }
  }
  __syncthreads();      // the view's storage and sh are free again
}

// the record of row i of a cloud of `len` points at position `local` of its sort, or the pad record
__device__ __forceinline__ double record_of(const GridArgs &a, const float *pts, int i, int len, int local) {
  const u64 key = i < len ? voxel_cell::key_of(pts + 3L * i, a.ox, a.oy, a.oz, a.size) : kNoKey;
  return __longlong_as_double((long long)(key == kNoKey ? kRecordPad : ((key << kIndexBits) | (unsigned)local) + kRecordBias));
}

__global__ __launch_bounds__(kThreads) void voxel_resident_kernel(GridArgs a) {
  extern __shared__ __attribute__((aligned(16))) double rec[];
  __shared__ alignas(16) Shared sh;
  const int tid = threadIdx.x;
  for (int cloud = blockIdx.x; cloud < a.b; cloud += gridDim.x) {
    const int len = sn::clamped_length(a.lengths, cloud, a.n);
    const float *pts = a.xyz + (long)cloud * a.n * 3;
    int *inverse = a.inverse ? a.inverse + (long)cloud * a.n : nullptr;
    const int width = pow2_width(len);      // <= pow2_width(a.n): what the launch's LDS holds
    const int end = width > a.n ? width : a.n;
    for (int i = tid; i < end; i += kThreads) {
      const double r = record_of(a, pts, i, len, i);
      if (i < width) rec[slot(i)] = r;
      if (inverse && i < a.n && __double_as_longlong(r) == (long long)kRecordPad) inverse[i] = -1;
    }
    __syncthreads();
    sort_records(rec, width, tid);
    reduce_cloud(ResidentView{rec}, width, sh, a, cloud);
  }
}

struct BigArgs {
  GridArgs g;
  int chunk, chunks;       // points per chunk, chunks per cloud
  u64 *keys[2];            // [b, n] each: the passes go from one to the other
  int *idx[2];
  int *starts;             // [b, n]
  int final;               // which of the two holds the merged arrays
};

__global__ __launch_bounds__(kThreads) void voxel_chunk_sort_kernel(BigArgs a) {
  extern __shared__ __attribute__((aligned(16))) double rec[];
  const int tid = threadIdx.x, n = a.g.n;
  const long total = (long)a.g.b * a.chunks;
  for (long id = blockIdx.x; id < total; id += gridDim.x) {
    const int cloud = (int)(id / a.chunks), base = (int)(id - (long)cloud * a.chunks) * a.chunk;
    const int m = n - base < a.chunk ? n - base : a.chunk;      // this chunk's rows: base .. base + m - 1
    const int len = sn::clamped_length(a.g.lengths, cloud, n);
    const float *pts = a.g.xyz + (long)cloud * n * 3;
    int *inverse = a.g.inverse ? a.g.inverse + (long)cloud * n : nullptr;
    const int width = pow2_width(m);      // <= pow2_width(a.chunk): what the launch's LDS holds
    for (int i = tid; i < width; i += kThreads) {
      const double r = i < m ? record_of(a.g, pts, base + i, len, i) : __longlong_as_double((long long)kRecordPad);
      rec[slot(i)] = r;
      if (inverse && i < m && __double_as_longlong(r) == (long long)kRecordPad) inverse[base + i] = -1;
    }
    __syncthreads();
    sort_records(rec, width, tid);
    u64 *keys = a.keys[0] + (long)cloud * n + base;
    int *idx = a.idx[0] + (long)cloud * n + base;
    for (int i = tid; i < m; i += kThreads) {      // the chunk's pads are at most width - m more than its rows without a voxel
      const u64 r = (u64)__double_as_longlong(rec[slot(i)]);
      keys[i] = (r - kRecordBias) >> kIndexBits;
      idx[i] = r == kRecordPad ? -1 : base + (int)((unsigned)r & (kResidentMax - 1));
    }
    __syncthreads();
  }
}

// one pass: the runs of `run` positions of every cloud, merged in pairs from array `from` into the other
__global__ __launch_bounds__(kMergeThreads) void voxel_merge_kernel(BigArgs a, int run, int from) {
  const int n = a.g.n;
  const long total = (long)a.g.b * n;
  const u64 *kin = a.keys[from];
  const int *iin = a.idx[from];
  u64 *kout = a.keys[from ^ 1];
  int *iout = a.idx[from ^ 1];
  for (long g = (long)blockIdx.x * kMergeThreads + threadIdx.x; g < total; g += (long)gridDim.x * kMergeThreads) {
    const long row = g / n * n;
    const int p = (int)(g - row);
    const int pair0 = p / (2 * run) * (2 * run);      // run <= 2^23: no overflow
    const int mid = pair0 + run < n ? pair0 + run : n, top = pair0 + 2 * run < n ? pair0 + 2 * run : n;
    const u64 *k = kin + row;
    const u64 key = k[p];
    const bool lower = p < mid;
    // the number of records of the partner run in front of this one: those with a smaller key, and for a record of the
    // upper run those with an equal key too
    int lo = lower ? mid : pair0, hi = lower ? top : mid;
    const int from0 = lo;
    while (lo < hi) {
      const int c = lo + (hi - lo) / 2;
      const u64 other = k[c];
      if (lower ? other < key : other <= key) lo = c + 1;
      else hi = c;
    }
    const int dest = pair0 + (p - (lower ? pair0 : mid)) + (lo - from0);
    kout[row + dest] = key;
    iout[row + dest] = iin[g];
  }
}

__global__ __launch_bounds__(kThreads) void voxel_reduce_kernel(BigArgs a) {
  __shared__ alignas(16) Shared sh;
  for (int cloud = blockIdx.x; cloud < a.g.b; cloud += gridDim.x) {
    const long row = (long)cloud * a.g.n;
    reduce_cloud(WorkspaceView{a.keys[a.final] + row, a.idx[a.final] + row, a.starts + row}, a.g.n, sh, a.g, cloud);
  }
}

struct PoolArgs {
  const float *features;   // [b, c, n]
  const int *order;        // [b, n]
  const int *start;        // [b, cap + 1]
  const int *count;        // [b]
  int b, c, n, cap, mode;
  float *out;              // [b, c, cap]
  int *argmax;             // [b, c, cap] or null
};

__global__ __launch_bounds__(kPoolThreads) void voxel_pool_kernel(PoolArgs a) {
  const long total = (long)a.b * a.c * a.cap;
  for (long g = (long)blockIdx.x * kPoolThreads + threadIdx.x; g < total; g += (long)gridDim.x * kPoolThreads) {
    const int v = (int)(g % a.cap);
    const long row = g / a.cap;      // cloud * c + channel
    const int cloud = (int)(row / a.c);
    int s, e;
    voxel_cell::segment(a.start + (long)cloud * (a.cap + 1), a.count[cloud], a.cap, v, a.n, &s, &e);
    voxel_cell::pool(a.features + row * a.n, a.order + (long)cloud * a.n, s, e, a.n, a.mode, a.out + g,
                     a.argmax ? a.argmax + g : nullptr);
  }
}

// ---------------------------------------------------------------------------------------------------- host
// clouds of up to this many points are sorted whole in LDS: 16384, or what SN_VOXEL_RESIDENT_MAX lowers it to (the tests
// reach the workspace path at small sizes with it)
int resident_max() {
  int r = kResidentMax;
  if (const char *e = SN_KNOB("SN_VOXEL_RESIDENT_MAX")) {
    const int v = atoi(e);
    if (v >= 1 && v < r) r = v;
  }
  return r;
}

struct Workspace {
  u64 *keys[2];
  int *idx[2];
  int *starts;
};
// the one description of the workspace: nothing for a resident cloud
Workspace layout(sn::Carver &c, int b, int n, int resident) {
  Workspace w{};
  const size_t elems = n > resident ? (size_t)b * n : 0;
  for (int k = 0; k < 2; ++k) w.keys[k] = c.take256<u64>(elems * sizeof(u64));
  for (int k = 0; k < 2; ++k) w.idx[k] = c.take256<int>(elems * sizeof(int));
  w.starts = c.take256<int>(elems * sizeof(int));
  return w;
}

bool valid_shape(int b, int n) { return b >= 1 && n >= 1 && n <= kBigMax && (long)b * n <= 0x7fffffffL; }

// shape, parameters and pointers, the same for both entry points; fills o[3]
int check_grid(const char *what, const float *xyz, int b, int n, float size, const float *origin, int cap,
               const int *count, float *o) {
  SN_REQUIRE(std::isfinite(size) && size > 0.f, "%s: size must be finite and > 0 (got %g)", what, (double)size);
  SN_REQUIRE(b >= 1 && n >= 1 && cap >= 1, "%s: need b,n,cap >= 1 (got %d,%d,%d)", what, b, n, cap);
  SN_REQUIRE(cap <= n, "%s: cap must not exceed n (got %d > %d)", what, cap, n);
  SN_REQUIRE((long)b * n <= 0x7fffffffL, "%s: too large (b * n must not exceed 2^31 - 1)", what);
  SN_REQUIRE(n <= kBigMax, "%s: a cloud has at most %d points (got %d)", what, kBigMax, n);
  SN_REQUIRE(xyz && count, "%s: null pointer (xyz and count are required)", what);
  for (int k = 0; k < 3; ++k) {
    o[k] = origin ? origin[k] : 0.f;
    SN_REQUIRE(std::isfinite(o[k]), "%s: origin must be finite (origin[%d] = %g)", what, k, (double)o[k]);
  }
  return 0;
}

int check_pool(const char *what, const float *features, int b, int c, int n, const int *order, const int *start,
               const int *count, int cap, int mode, const float *out) {
  SN_REQUIRE(b >= 1 && c >= 1 && n >= 1 && cap >= 1, "%s: need b,c,n,cap >= 1 (got %d,%d,%d,%d)", what, b, c, n, cap);
  SN_REQUIRE(cap <= n, "%s: cap must not exceed n (got %d > %d)", what, cap, n);
  SN_REQUIRE((long)b * n <= 0x7fffffffL, "%s: too large (b * n must not exceed 2^31 - 1)", what);
  SN_REQUIRE(mode >= voxel_cell::kSum && mode <= voxel_cell::kMax, "%s: unknown pooling mode %d (0 sum, 1 mean, 2 max)",
             what, mode);
  SN_REQUIRE(features && order && start && count && out,
             "%s: null pointer (features, order, start, count and out are required)", what);
  return 0;
}

// the workgroups of a launch over `items` independent pieces: SN_VOXEL_BLOCKS, or `cap`; never more than the pieces
int launch_blocks(long items, long cap) {
  long blocks = 0;
  if (const char *e = SN_KNOB("SN_VOXEL_BLOCKS")) blocks = atoi(e);
  if (blocks < 1) blocks = cap;
  return (int)(blocks > items ? items : blocks);
}

}  // namespace

extern "C" size_t sn_voxel_grid_workspace_bytes(int b, int n) {
  if (!valid_shape(b, n)) return 0;
  return sn::layout_bytes(layout, b, n, resident_max());
}

extern "C" int sn_voxel_grid(const float *xyz, const int *lengths, int b, int n, float size, const float *origin,
                             int cap, int *count, float *centroid, int *members, int *first, int *inverse, int *order,
                             int *start, void *workspace, size_t workspace_bytes, void *stream) {
  const char *what = "sn_voxel_grid";
  float o[3];
  if (const int rc = check_grid(what, xyz, b, n, size, origin, cap, count, o)) return rc;
  const int resident = resident_max();
  sn::Carver carver(workspace);
  const Workspace w = layout(carver, b, n, resident);
  SN_REQUIRE(workspace_bytes >= carver.bytes() && (workspace || carver.bytes() == 0),
             "%s: workspace too small (%zu < %zu)", what, workspace_bytes, carver.bytes());
  hipStream_t st = sn::as_stream(stream);
  int dev = 0, cus = 0;
  SN_HIP(hipGetDevice(&dev));
  SN_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  const GridArgs g{xyz, lengths, b, n, cap, size, o[0], o[1], o[2], count, centroid, members, first, inverse, order, start};
  // above the 64 KB a launch may ask for unannounced.  Every call: the attribute belongs to the CURRENT device
  if (n <= resident) {
    SN_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&voxel_resident_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(kResidentMax)));
    SN_TIMED("voxel_grid", st, (voxel_resident_kernel<<<(unsigned)launch_blocks(b, 2L * cus), kThreads,
                                                        lds_bytes(pow2_width(n)), st>>>(g)));
    return sn::launch_status(what);
  }
  BigArgs a{};
  a.g = g, a.chunk = resident, a.chunks = sn::ceil_div(n, resident), a.starts = w.starts;
  for (int k = 0; k < 2; ++k) a.keys[k] = w.keys[k], a.idx[k] = w.idx[k];
  SN_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&voxel_chunk_sort_kernel),
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(kResidentMax)));
  SN_TIMED("voxel_chunk_sort", st, (voxel_chunk_sort_kernel<<<(unsigned)launch_blocks((long)b * a.chunks, 2L * cus), kThreads,
                                                            lds_bytes(pow2_width(resident)), st>>>(a)));
  if (const int rc = sn::launch_status(what)) return rc;
  int from = 0;
  const long merge_items = ((long)b * n + kMergeThreads - 1) / kMergeThreads;
  for (long run = resident; run < n; run *= 2, from ^= 1) {
    SN_TIMED("voxel_merge", st, (voxel_merge_kernel<<<(unsigned)launch_blocks(merge_items, 16L * cus), kMergeThreads, 0,
                                                      st>>>(a, (int)run, from)));
    if (const int rc = sn::launch_status(what)) return rc;
  }
  a.final = from;
  SN_TIMED("voxel_reduce", st, (voxel_reduce_kernel<<<(unsigned)launch_blocks(b, 2L * cus), kThreads, 0, st>>>(a)));
  return sn::launch_status(what);
}

extern "C" int sn_voxel_grid_host(const float *xyz, const int *lengths, int b, int n, float size, const float *origin,
                                  int cap, int *count, float *centroid, int *members, int *first, int *inverse,
                                  int *order, int *start, int threads) {
  float o[3];
  if (const int rc = check_grid("sn_voxel_grid_host", xyz, b, n, size, origin, cap, count, o)) return rc;
  parallel_items(b, threads, [&](long i) {
    const voxel_cell::CloudOut out{count + i,
                                   centroid ? centroid + i * cap * 3 : nullptr,
                                   members ? members + i * cap : nullptr,
                                   first ? first + i * cap : nullptr,
                                   inverse ? inverse + i * n : nullptr,
                                   order ? order + i * n : nullptr,
                                   start ? start + i * (cap + 1) : nullptr};
    voxel_cell::grid_cloud_host(xyz + i * n * 3, sn::clamped_length(lengths, (int)i, n), n, size, o, cap, out);
  });
  return 0;
}

extern "C" int sn_voxel_pool(const float *features, int b, int c, int n, const int *order, const int *start,
                             const int *count, int cap, int mode, float *out, int *argmax, void *stream) {
  const char *what = "sn_voxel_pool";
  if (const int rc = check_pool(what, features, b, c, n, order, start, count, cap, mode, out)) return rc;
  hipStream_t st = sn::as_stream(stream);
  const PoolArgs a{features, order, start, count, b, c, n, cap, mode, out, argmax};
  const long total = (long)b * c * cap;
  const int blocks = launch_blocks((total + kPoolThreads - 1) / kPoolThreads, 1L << 20);
  SN_TIMED("voxel_pool", st, (voxel_pool_kernel<<<(unsigned)blocks, kPoolThreads, 0, st>>>(a)));
  return sn::launch_status(what);
}

extern "C" int sn_voxel_pool_host(const float *features, int b, int c, int n, const int *order, const int *start,
                                  const int *count, int cap, int mode, float *out, int *argmax, int threads) {
  if (const int rc = check_pool("sn_voxel_pool_host", features, b, c, n, order, start, count, cap, mode, out)) return rc;
  parallel_items(b, threads, [&](long i) {
    voxel_cell::pool_cloud_host(features + i * c * n, c, n, order + i * n, start + i * (cap + 1), count[i], cap, mode,
                                out + i * c * cap, argmax ? argmax + i * c * cap : nullptr);
  });
  return 0;
}
