// occupancy.hip -- the occupancy grid of a set of clouds (include/ops/occupancy.h states the rule; grid_cell.hpp is its
// per-point routine, compiled here for the device and for the host entry point).
//
//   sphere_list_kernel   the in-sphere cells of the grid in the order of their linear indices, packed, into the
//       workspace: one thread per row (i, j) counts the row's cells, a workgroup scan places them.  A pure function of
//       res; one workgroup, once per call.
//   occupancy_kernel     a workgroup of kThreads lanes owns whole clouds and loops over them.  The cloud's histogram of
//       res^3 words lives in LDS.  Per chunk of kThreads points: Rule 1 one point per lane (coalesced reads), an LDS
//       atomic on the histogram; a point whose cube cell is clipped away goes into an LDS queue instead.  The queue is
//       then served a wave per point: the 64 lanes stride the 125 cells around the clipped cube cell, each keeps its
//       best (D, cell), a butterfly merges them; where that best D does not prove itself the minimum over the whole
//       sphere (grid_cell.hpp: scan_box) the lanes stride the in-sphere list (coalesced, from L2) the same way -- one
//       slow point never stalls 63 lanes.  After the cloud one pass over the histogram adds every non-empty cell to
//       counts and 1 to occupied with integer global atomics and clears the word behind it, so the clear costs no pass
//       of its own.  No floating-point atomics, nobody waits for another workgroup, no scratch.
#include <algorithm>
#include <mutex>
#include <vector>

#include "block_scan.hpp"
#include "common.hpp"
#include "grid_cell.hpp"
#include "host_threads.hpp"
#include "../../include/ops/occupancy.h"

namespace {

// 16 waves: from res 27 on the histogram leaves room for one workgroup per CU only (139280 B of LDS at res 32, of 160 KB)
constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / sn::kWave;
constexpr int kListThreads = 1024;  // >= kMaxRes^2 rows
static_assert(kListThreads >= grid_cell::kMaxRes * grid_cell::kMaxRes, "one thread per row of the grid");

struct Args {
  const float *xyz;                // [s, n, 3]
  const int *lengths;              // [s] or null
  const int *list;                 // the packed in-sphere cells (in_sphere only)
  unsigned long long *counts;      // [res^3] or null
  int *occupied;                   // [res^3] or null
  int *cells;                      // [s, n] or null
  int s, n, res, in_sphere, list_count;
};

__global__ __launch_bounds__(kListThreads) void sphere_list_kernel(int *list, int res) {
  __shared__ alignas(16) sn::BlockScan<kListThreads> scan;
  const int t = threadIdx.x, i = t / res, j = t % res;
  int first = 0;
  const int count = t < res * res ? grid_cell::row_cells(i, j, res, &first) : 0;
  scan.reset(0);
  scan.chunk(count, [&](int exclusive) {
    for (int k = 0; k < count; ++k) list[exclusive + k] = grid_cell::pack(i, j, first + k);
  });
}

// the best (D, cell) of the 64 lanes, left in every lane
__device__ __forceinline__ void wave_best(double &best_d, int &best) {
  for (int step = sn::kWave / 2; step >= 1; step >>= 1) {
    const double other_d = __shfl_xor(best_d, step);
    const int other = __shfl_xor(best, step);
    if (grid_cell::beats(other_d, other, best_d, best)) best_d = other_d, best = other;
  }
}

__global__ __launch_bounds__(kThreads) void occupancy_kernel(Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned lds[];
  const int tid = threadIdx.x, lane = tid & (sn::kWave - 1), wave = tid / sn::kWave;
  const int res = a.res, res3 = res * res * res;
  const bool want_hist = a.counts || a.occupied;
  unsigned *hist = lds;                                                  // res^3 words (none without counts / occupied)
  int *queue = reinterpret_cast<int *>(lds + (want_hist ? res3 : 0));    // kThreads point indices ...
  int *queue_cube = queue + kThreads;                                    // ... and their packed cube cells
  int *queued = queue_cube + kThreads;                                   // two counters, used in turn
  if (want_hist)
    for (int c = tid; c < res3; c += kThreads) hist[c] = 0;
  if (tid < 2) queued[tid] = 0;
  __syncthreads();
  int turn = 0;
  for (int cloud = blockIdx.x; cloud < a.s; cloud += gridDim.x) {
    const int len = sn::clamped_length(a.lengths, cloud, a.n);
    const float *p = a.xyz + (long)cloud * a.n * 3;
    int *row = a.cells ? a.cells + (long)cloud * a.n : nullptr;
    const int end = row ? a.n : len;      // padding rows are visited only to write their -1
    for (long base = 0; base < end; base += kThreads) {
      const long pt = base + tid;
      int cell = -1;
      if (pt < len) {
        const float x = p[3 * pt], y = p[3 * pt + 1], z = p[3 * pt + 2];
        if (grid_cell::is_finite(x) && grid_cell::is_finite(y) && grid_cell::is_finite(z)) {
          double u0, u1, u2;
          cell = grid_cell::rule1(x, y, z, res, a.in_sphere, &u0, &u1, &u2);
          if (cell < 0) {
            const int slot = atomicAdd(&queued[turn], 1);
            queue[slot] = (int)pt, queue_cube[slot] = -1 - cell;
            cell = -2;      // decided below
          }
        }
      }
      if (cell >= 0 && want_hist) atomicAdd(&hist[cell], 1u);
      if (row && pt < a.n && cell != -2) row[pt] = cell;
      __syncthreads();
      const int waiting = queued[turn];
      if (tid == 0) queued[turn ^ 1] = 0;      // nobody reads or adds to the other counter before the next barrier
      for (int e = wave; e < waiting; e += kWaves) {
        const int q = queue[e];
        const double u0 = grid_cell::scaled(p[3L * q], res), u1 = grid_cell::scaled(p[3L * q + 1], res),
                     u2 = grid_cell::scaled(p[3L * q + 2], res);
        double best_d;
        int best;
        grid_cell::scan_box(u0, u1, u2, queue_cube[e], res, lane, sn::kWave, &best_d, &best);
        wave_best(best_d, best);
        if (!(best_d < grid_cell::kBoxLimit)) {      // wave-uniform: the box does not decide, the whole list does
          grid_cell::scan(u0, u1, u2, a.list, a.list_count, res, lane, sn::kWave, &best_d, &best);
          wave_best(best_d, best);
        }
        if (lane == 0) {
          const int c = grid_cell::linear(best, res);
          if (want_hist) atomicAdd(&hist[c], 1u);
          if (row) row[q] = c;
        }
      }
      __syncthreads();
      turn ^= 1;
    }
    if (want_hist) {
      for (int c = tid; c < res3; c += kThreads) {
        const unsigned v = hist[c];
        if (v) {
          if (a.counts) atomicAdd(a.counts + c, (unsigned long long)v);
          if (a.occupied) atomicAdd(a.occupied + c, 1);
          hist[c] = 0;
        }
      }
      __syncthreads();
    }
  }
}

// the packed in-sphere cells of every res, built at its first use and kept: the host entry point scans it, the device
// entry point needs its length
const std::vector<int> &sphere_list(int res) {
  static std::vector<int> lists[grid_cell::kMaxRes + 1];
  static std::once_flag once[grid_cell::kMaxRes + 1];
  std::call_once(once[res], [res] {
    std::vector<int> &l = lists[res];
    for (int i = 0; i < res; ++i)
      for (int j = 0; j < res; ++j) {
        int first = 0;
        const int count = grid_cell::row_cells(i, j, res, &first);
        for (int k = 0; k < count; ++k) l.push_back(grid_cell::pack(i, j, first + k));
      }
  });
  return lists[res];
}

bool valid_res(int res) { return res >= grid_cell::kMinRes && res <= grid_cell::kMaxRes; }

// the workspace: the in-sphere list
struct Workspace {
  int *list;
};
Workspace layout(sn::Carver &c, int res, int in_sphere) {
  Workspace w;
  w.list = c.take256<int>(in_sphere && valid_res(res) ? sphere_list(res).size() * sizeof(int) : 0);
  return w;
}

// shape and pointers, the same for both entry points
int check_arguments(const char *what, const float *xyz, int s, int n, int res, int in_sphere, const long long *counts,
                    const int *occupied, const int *cells) {
  SN_REQUIRE(valid_res(res), "%s: res must be in %d..%d (got %d)", what, grid_cell::kMinRes, grid_cell::kMaxRes, res);
  SN_REQUIRE(!in_sphere || !sphere_list(res).empty(), "%s: no cell of the grid lies in the sphere at res = %d", what, res);
  SN_REQUIRE(s >= 1 && n >= 1, "%s: need s,n >= 1 (got %d,%d)", what, s, n);
  SN_REQUIRE((long)s * n <= 0x7fffffffL, "%s: too large (s * n must not exceed 2^31 - 1)", what);
  SN_REQUIRE(xyz, "%s: null pointer (xyz is required)", what);
  SN_REQUIRE(counts || occupied || cells, "%s: no output (counts, occupied and cells are all null)", what);
  return 0;
}

}  // namespace

extern "C" size_t sn_occupancy_grid_workspace_bytes(int s, int n, int res, int in_sphere) {
  (void)s, (void)n;
  return sn::layout_bytes(layout, res, in_sphere);
}

extern "C" int sn_occupancy_grid(const float *xyz, const int *lengths, int s, int n, int res, int in_sphere,
                                 long long *counts, int *occupied, int *cells, void *workspace, size_t workspace_bytes,
                                 void *stream) {
  const char *what = "sn_occupancy_grid";
  if (const int rc = check_arguments(what, xyz, s, n, res, in_sphere, counts, occupied, cells)) return rc;
  const size_t need = sn_occupancy_grid_workspace_bytes(s, n, res, in_sphere);
  SN_REQUIRE(workspace_bytes >= need && (workspace || need == 0), "%s: workspace too small (%zu < %zu)", what,
             workspace_bytes, need);
  sn::Carver carver(workspace);
  const Workspace w = layout(carver, res, in_sphere);
  hipStream_t st = sn::as_stream(stream);
  const int res3 = res * res * res;
  Args a{xyz, lengths, w.list, reinterpret_cast<unsigned long long *>(counts), occupied, cells, s, n, res,
         in_sphere ? 1 : 0, in_sphere ? (int)sphere_list(res).size() : 0};
  if (counts) SN_HIP(hipMemsetAsync(counts, 0, (size_t)res3 * sizeof(long long), st));
  if (occupied) SN_HIP(hipMemsetAsync(occupied, 0, (size_t)res3 * sizeof(int), st));
  if (in_sphere) sphere_list_kernel<<<1, kListThreads, 0, st>>>(w.list, res);
  // two workgroups per compute unit where the histogram lets them share one; SN_OCCUPANCY_BLOCKS sets the number (the
  // tests run every case at several: the outputs do not depend on it)
  int blocks = 0;
  if (const char *e = SN_KNOB("SN_OCCUPANCY_BLOCKS")) blocks = atoi(e);
  if (blocks < 1) {
    int dev = 0, cus = 0;
    SN_HIP(hipGetDevice(&dev));
    SN_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    blocks = 2 * cus;
  }
  if (blocks > s) blocks = s;
  const size_t lds = ((size_t)((counts || occupied) ? res3 : 0) + 2 * kThreads + 4) * sizeof(int);
  // above the 64 KB a launch may ask for unannounced.  Every call: the attribute belongs to the CURRENT device
  SN_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&occupancy_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (grid_cell::kMaxRes * grid_cell::kMaxRes * grid_cell::kMaxRes + 2 * kThreads + 4) * (int)sizeof(int)));
  SN_TIMED("occupancy_grid", st, (occupancy_kernel<<<(unsigned)blocks, kThreads, lds, st>>>(a)));
  return sn::launch_status(what);
}

extern "C" int sn_occupancy_grid_host(const float *xyz, const int *lengths, int s, int n, int res, int in_sphere,
                                      long long *counts, int *occupied, int *cells, int threads) {
  const char *what = "sn_occupancy_grid_host";
  if (const int rc = check_arguments(what, xyz, s, n, res, in_sphere, counts, occupied, cells)) return rc;
  const int res3 = res * res * res;
  const std::vector<int> &list = sphere_list(res);
  if (counts) std::fill(counts, counts + res3, 0LL);
  if (occupied) std::fill(occupied, occupied + res3, 0);
  std::mutex merge;
  std::vector<int> stamp;      // the last cloud that touched a cell: guarded by `merge`
  if (occupied) stamp.assign(res3, -1);
  parallel_items(s, threads, [&](long cloud) {
    const int len = sn::clamped_length(lengths, (int)cloud, n);
    const float *p = xyz + cloud * n * 3;
    std::vector<int> own;
    int *row = cells ? cells + cloud * n : (own.resize(len), own.data());
    for (int pt = 0; pt < len; ++pt) {
      const float x = p[3L * pt], y = p[3L * pt + 1], z = p[3L * pt + 2];
      int cell = -1;
      if (grid_cell::is_finite(x) && grid_cell::is_finite(y) && grid_cell::is_finite(z)) {
        double u0, u1, u2;
        cell = grid_cell::rule1(x, y, z, res, in_sphere, &u0, &u1, &u2);
        if (cell < 0) {
          double best_d;
          int best;
          grid_cell::scan_box(u0, u1, u2, -1 - cell, res, 0, 1, &best_d, &best);
          if (!(best_d < grid_cell::kBoxLimit))
            grid_cell::scan(u0, u1, u2, list.data(), (int)list.size(), res, 0, 1, &best_d, &best);
          cell = grid_cell::linear(best, res);
        }
      }
      row[pt] = cell;
    }
    if (cells)
      for (int pt = len; pt < n; ++pt) row[pt] = -1;
    if (!counts && !occupied) return;
    std::lock_guard<std::mutex> hold(merge);
    for (int pt = 0; pt < len; ++pt) {
      const int cell = row[pt];
      if (cell < 0) continue;
      if (counts) ++counts[cell];
      if (occupied && stamp[cell] != (int)cloud) stamp[cell] = (int)cloud, ++occupied[cell];
    }
  });
  return 0;
}
