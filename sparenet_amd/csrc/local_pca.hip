// local_pca.hip -- normals, frames and eigenvalues of the neighbourhoods an index table names (include/ops/local_pca.h
// states the rule; eig3.hpp is its arithmetic, compiled here for the device and for the host entry point).
//
//   local_pca_kernel    one query per lane, kThreads queries per workgroup.  A lane's idx row is k ints at a stride of
//       k, so the workgroup's rows -- one contiguous block of kThreads * k ints -- are loaded coalesced into LDS with an
//       odd row pitch (k | 1: the lanes of a half wave then read 32 different banks for any k) and read from there.
//       The k points are gathered from global memory, once for the centroid and once for the covariance (a cloud
//       stays in L2; the second pass finds most lines in L1); the solver runs in registers.  One launch, no atomics.
#include "common.hpp"
#include "eig3.hpp"
#include "host_threads.hpp"
#include "../../include/ops/local_pca.h"

namespace {

constexpr int kThreads = 128;      // (64 | 1) * 128 ints = 33 KB of LDS at the largest k
constexpr int kMaxK = 64;

struct Args {
  const float *xyz;          // [b, n, 3]
  const int *idx;            // [b, m, k]
  const float *new_xyz;      // [b, m, 3] or null
  const float *viewpoint;    // [b, 3] or null
  double *eigenvalues;       // [b, m, 3] or null
  float *frames;             // [b, m, 3, 3] or null
  float *normals;            // [b, m, 3] or null
  long rows;                 // b * m
  int n, m, k;
};

// the outputs of query `row`, each rounded once
__host__ __device__ inline void store(const Args &a, long row, const eig3::Result &r) {
  if (a.eigenvalues) {
    double *e = a.eigenvalues + row * 3;
    e[0] = r.l0, e[1] = r.l1, e[2] = r.l2;
  }
  if (a.frames) {
    float *f = a.frames + row * 9;
    f[0] = (float)r.e0.x, f[1] = (float)r.e0.y, f[2] = (float)r.e0.z;
    f[3] = (float)r.e1.x, f[4] = (float)r.e1.y, f[5] = (float)r.e1.z;
    f[6] = (float)r.e2.x, f[7] = (float)r.e2.y, f[8] = (float)r.e2.z;
  }
  if (a.normals) {
    float *v = a.normals + row * 3;
    v[0] = (float)r.e0.x, v[1] = (float)r.e0.y, v[2] = (float)r.e0.z;
  }
}

__global__ __launch_bounds__(kThreads) void local_pca_kernel(Args a) {
  extern __shared__ int table[];      // kThreads rows of `pitch` ints
  const int tid = threadIdx.x, k = a.k, pitch = k | 1;
  const long first = (long)blockIdx.x * kThreads;      // the workgroup's first query
  const long left = a.rows - first;
  const int here = left < kThreads ? (int)left : kThreads;
  // element e of the block belongs to row e / k, slot e % k; thread tid takes e = tid, tid + kThreads, ...
  const int *src = a.idx + first * k;
  const int total = here * k, step_row = kThreads / k, step_slot = kThreads % k;
  int row = tid / k, slot = tid % k;
  for (int e = tid; e < total; e += kThreads) {
    table[row * pitch + slot] = src[e];
    row += step_row, slot += step_slot;
    if (slot >= k) slot -= k, ++row;
  }
  __syncthreads();
  if (tid >= here) return;
  const long q = first + tid;
  const int cloud = (int)(q / a.m);
  const int *mine = table + tid * pitch;
  eig3::Result r;
  eig3::neighbourhood(a.xyz + (long)cloud * a.n * 3, a.n, k, [mine](int t) { return mine[t]; },
                      a.viewpoint ? a.new_xyz + q * 3 : nullptr, a.viewpoint ? a.viewpoint + (long)cloud * 3 : nullptr, &r);
  store(a, q, r);
}

// shape and pointers, the same for both entry points
int check_arguments(const char *what, const float *xyz, const int *idx, int b, int n, int m, int k, const float *new_xyz,
                    const float *viewpoint, const double *eigenvalues, const float *frames, const float *normals) {
  SN_REQUIRE(b >= 1 && n >= 1 && m >= 1, "%s: need b,n,m >= 1 (got %d,%d,%d)", what, b, n, m);
  SN_REQUIRE((long)b * m <= (1L << 30), "%s: too large (b * m must not exceed 2^30)", what);
  SN_REQUIRE(k >= 1 && k <= kMaxK, "%s: k must be in 1..%d (got %d)", what, kMaxK, k);
  SN_REQUIRE(xyz && idx, "%s: null pointer (xyz and idx are required)", what);
  SN_REQUIRE(eigenvalues || frames || normals, "%s: no output (eigenvalues, frames and normals are all null)", what);
  SN_REQUIRE(!viewpoint || new_xyz, "%s: a viewpoint needs new_xyz, the query points", what);
  return 0;
}

}  // namespace

extern "C" size_t sn_local_pca_workspace_bytes(int b, int n, int m, int k) {
  (void)b, (void)n, (void)m, (void)k;
  return 0;
}

extern "C" int sn_local_pca(const float *xyz, const int *idx, int b, int n, int m, int k, const float *new_xyz,
                            const float *viewpoint, double *eigenvalues, float *frames, float *normals, void *workspace,
                            size_t workspace_bytes, void *stream) {
  const char *what = "sn_local_pca";
  if (const int rc = check_arguments(what, xyz, idx, b, n, m, k, new_xyz, viewpoint, eigenvalues, frames, normals))
    return rc;
  const size_t need = sn_local_pca_workspace_bytes(b, n, m, k);
  SN_REQUIRE(workspace_bytes >= need && (workspace || need == 0), "%s: workspace too small (%zu < %zu)", what,
             workspace_bytes, need);
  const Args a{xyz, idx, new_xyz, viewpoint, eigenvalues, frames, normals, (long)b * m, n, m, k};
  const unsigned blocks = (unsigned)((a.rows + kThreads - 1) / kThreads);
  const size_t lds = (size_t)kThreads * (k | 1) * sizeof(int);
  local_pca_kernel<<<blocks, kThreads, lds, sn::as_stream(stream)>>>(a);
  return sn::launch_status(what);
}

extern "C" int sn_local_pca_host(const float *xyz, const int *idx, int b, int n, int m, int k, const float *new_xyz,
                                 const float *viewpoint, double *eigenvalues, float *frames, float *normals,
                                 int threads) {
  const char *what = "sn_local_pca_host";
  if (const int rc = check_arguments(what, xyz, idx, b, n, m, k, new_xyz, viewpoint, eigenvalues, frames, normals))
    return rc;
  const Args a{xyz, idx, new_xyz, viewpoint, eigenvalues, frames, normals, (long)b * m, n, m, k};
  parallel_items(b, threads, [&](long cloud) {
    for (long q = cloud * m; q < (cloud + 1) * m; ++q) {
      const int *mine = idx + q * k;
      eig3::Result r;
      eig3::neighbourhood(xyz + cloud * n * 3, n, k, [mine](int t) { return mine[t]; },
                          viewpoint ? new_xyz + q * 3 : nullptr, viewpoint ? viewpoint + cloud * 3 : nullptr, &r);
      store(a, q, r);
    }
  });
  return 0;
}
