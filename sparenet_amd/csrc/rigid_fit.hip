// rigid_fit.hip -- rigid registration: the transform of a cloud and one ICP iteration after the search
// (include/ops/rigid_fit.h states the rule; rigid_solve.hpp is its arithmetic, compiled here for the device and for the
// host entry points).
//
//   rigid_apply_kernel        one row per lane; pose and scale sit at workgroup-uniform addresses (scalar loads).
//   rigid_accumulate_kernel   one workgroup per (cloud, chunk of rigid::kChunk rows), one row per lane per trip: the
//       moved rows, the index row and the weights are read coalesced, the matched target row (and its normal) is
//       gathered; a lane keeps its sums in registers (19 doubles in point mode, 30 in plane mode: one instantiation
//       each), the workgroup adds them in sn::block_sums_f64's fixed order and writes one partial per chunk.
//   rigid_solve_kernel        one lane per cloud: the chunk partials in ascending order, the convergence test, the solve,
//       the composition and the state.  A second plain launch: no atomics, no counters, no workgroup waits for another.
#include "block_scan.hpp"
#include "common.hpp"
#include "host_threads.hpp"
#include "rigid_solve.hpp"
#include "../../include/ops/rigid_fit.h"

namespace {

using rigid::kChunk;
using rigid::kStride;
using rigid::kThreads;
using rigid::kTrips;
constexpr int kWaves = kThreads / sn::kWave;
constexpr int kApplyThreads = 256;
constexpr int kSolveThreads = 64;

struct ApplyArgs {
  const float *xyz;          // [b, n, 3]
  const double *pose;        // [b, 4, 4]
  const double *scale;       // [b] or null
  const int *lengths;        // [b] or null
  float *out;                // [b, n, 3]
  int n;
};

__global__ __launch_bounds__(kApplyThreads) void rigid_apply_kernel(ApplyArgs a) {
  const int cloud = blockIdx.y;
  const int i = blockIdx.x * kApplyThreads + threadIdx.x;
  if (i >= a.n) return;
  const long row = ((long)cloud * a.n + i) * 3;
  if (i >= sn::clamped_length(a.lengths, cloud, a.n)) {
    a.out[row] = 0.0f, a.out[row + 1] = 0.0f, a.out[row + 2] = 0.0f;
    return;
  }
  rigid::apply_row(a.pose + (long)cloud * 16, a.scale ? a.scale[cloud] : 1.0, a.xyz + row, a.out + row);
}

template <int kMode>
__global__ __launch_bounds__(kThreads) void rigid_accumulate_kernel(rigid::Problem P, double *partials) {
  constexpr int kSums = rigid::sums_of<kMode>();
  __shared__ double wave_sums[kWaves * kSums];
  const int cloud = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
  const int src_len = sn::clamped_length(P.src_lengths, cloud, P.n);
  const int dst_len = sn::clamped_length(P.dst_lengths, cloud, P.m);
  const rigid::Pivots v = rigid::pivots_of(P, cloud);
  double acc[kSums];
#pragma unroll
  for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
#pragma unroll
  for (int t = 0; t < kTrips; ++t) {
    const int i = chunk * kChunk + t * kThreads + tid;
    if (i < src_len) rigid::add_row<kMode>(P, cloud, i, dst_len, v, acc);
  }
  sn::block_sums_f64<kThreads, kSums>(acc, wave_sums);
  if (tid < kSums) partials[((long)cloud * gridDim.x + chunk) * kStride + tid] = acc[0];
}

struct SolveArgs {
  rigid::Problem P;
  rigid::Rule rule;
  const double *partials;
  double *pose, *scale, *state, *stats;
  int b, chunks;
};

template <int kMode>
__global__ __launch_bounds__(kSolveThreads) void rigid_solve_kernel(SolveArgs a) {
  const int cloud = blockIdx.x * kSolveThreads + threadIdx.x;
  if (cloud >= a.b) return;
  double acc[rigid::sums_of<kMode>()];
  rigid::sum_chunks<kMode>(a.partials + (long)cloud * a.chunks * kStride, a.chunks, acc);
  rigid::finish_cloud<kMode>(acc, sn::clamped_length(a.P.src_lengths, cloud, a.P.n), rigid::pivots_of(a.P, cloud), a.rule,
                             a.pose ? a.pose + (long)cloud * 16 : nullptr, a.pose ? a.scale + cloud : nullptr,
                             a.pose ? a.state + (long)cloud * 4 : nullptr, a.stats + (long)cloud * 4);
}

// The sums of one chunk on the host, in the workgroup's order: per lane its rows ascending, the 64-lane xor butterfly
// (adds commute, so lane 0 holds a balanced tree over offsets 32, 16 .. 1), then the waves ascending.
template <int kMode>
void chunk_sums_host(const rigid::Problem &P, long cloud, int chunk, int src_len, int dst_len, const rigid::Pivots &v,
                     double *lanes, double *partial) {
  constexpr int kSums = rigid::sums_of<kMode>();
  for (int e = 0; e < kThreads * kSums; ++e) lanes[e] = 0.0;
  for (int t = 0; t < kTrips; ++t)
    for (int tid = 0; tid < kThreads; ++tid) {
      const int i = chunk * kChunk + t * kThreads + tid;
      if (i < src_len) rigid::add_row<kMode>(P, cloud, i, dst_len, v, lanes + tid * kSums);
    }
  for (int k = 0; k < kSums; ++k) {
    double total = 0.0;
    for (int w = 0; w < kWaves; ++w) {
      double lane[sn::kWave];
      for (int l = 0; l < sn::kWave; ++l) lane[l] = lanes[(w * sn::kWave + l) * kSums + k];
      for (int off = sn::kWave / 2; off > 0; off >>= 1)
        for (int l = 0; l < off; ++l) lane[l] = lane[l] + lane[l + off];
      total = w == 0 ? lane[0] : total + lane[0];
    }
    partial[k] = total;
  }
}

template <int kMode>
void step_host(const rigid::Problem &P, const rigid::Rule &rule, int b, double *pose, double *scale, double *state,
               double *stats, int threads) {
  const int chunks = rigid::chunks_of(P.n);
  parallel_items(b, threads, [&](long cloud) {
    std::vector<double> lanes((size_t)kThreads * rigid::sums_of<kMode>()), partials((size_t)chunks * kStride, 0.0);
    const int src_len = sn::clamped_length(P.src_lengths, (int)cloud, P.n);
    const int dst_len = sn::clamped_length(P.dst_lengths, (int)cloud, P.m);
    const rigid::Pivots v = rigid::pivots_of(P, cloud);
    for (int c = 0; c < chunks; ++c)
      chunk_sums_host<kMode>(P, cloud, c, src_len, dst_len, v, lanes.data(), partials.data() + (size_t)c * kStride);
    double acc[rigid::sums_of<kMode>()];
    rigid::sum_chunks<kMode>(partials.data(), chunks, acc);
    rigid::finish_cloud<kMode>(acc, src_len, v, rule, pose ? pose + cloud * 16 : nullptr, pose ? scale + cloud : nullptr,
                               pose ? state + cloud * 4 : nullptr, stats + cloud * 4);
  });
}

int check_apply(const char *what, const float *xyz, const double *pose, int b, int n, const float *out) {
  SN_REQUIRE(b >= 1 && n >= 1, "%s: need b,n >= 1 (got %d,%d)", what, b, n);
  SN_REQUIRE(b <= 65535, "%s: too many clouds (b must not exceed 65535, got %d)", what, b);
  SN_REQUIRE(xyz && pose && out, "%s: null pointer (xyz, pose and out are required)", what);
  return 0;
}

int check_step(const char *what, const float *moved, const float *dst, const int *idx, const float *dst_normals, int b,
               int n, int m, int mode, int with_scale, double rtol, double atol, int freeze, const double *pose,
               const double *scale, const double *state, const double *stats) {
  SN_REQUIRE(b >= 1 && n >= 1 && m >= 1, "%s: need b,n,m >= 1 (got %d,%d,%d)", what, b, n, m);
  SN_REQUIRE(b <= 65535, "%s: too many clouds (b must not exceed 65535, got %d)", what, b);
  SN_REQUIRE(moved && dst && stats, "%s: null pointer (moved, dst and stats are required)", what);
  SN_REQUIRE(!pose || (scale && state), "%s: null pointer (a pose needs scale and state)", what);
  SN_REQUIRE(pose || !freeze, "%s: freeze needs a pose (a null pose measures only)", what);
  SN_REQUIRE(mode == 0 || mode == 1, "%s: mode must be 0 (point) or 1 (plane), got %d", what, mode);
  SN_REQUIRE(mode == 0 || dst_normals, "%s: mode 1 (plane) needs dst_normals", what);
  SN_REQUIRE(mode == 0 || !with_scale, "%s: with_scale is for mode 0 (point) only", what);
  SN_REQUIRE(idx || n == m, "%s: a null idx matches row i to row i and needs n == m (got %d and %d)", what, n, m);
  SN_REQUIRE(rtol >= 0.0 && atol >= 0.0, "%s: rtol and atol must not be negative (got %g and %g)", what, rtol, atol);
  return 0;
}

rigid::Problem problem_of(const float *moved, const float *dst, const int *idx, const float *weight,
                          const float *dst_normals, const int *src_lengths, const int *dst_lengths, int n, int m, int mode,
                          double max_dist) {
  return rigid::Problem{moved, dst, idx, weight, mode == 1 ? dst_normals : nullptr, src_lengths, dst_lengths, n, m,
                        max_dist > 0.0 ? max_dist * max_dist : 0.0};
}

}  // namespace

extern "C" int sn_rigid_apply(const float *xyz, const double *pose, const double *scale, const int *lengths, int b, int n,
                              float *out, void *stream) {
  const char *what = "sn_rigid_apply";
  if (const int rc = check_apply(what, xyz, pose, b, n, out)) return rc;
  const ApplyArgs a{xyz, pose, scale, lengths, out, n};
  rigid_apply_kernel<<<dim3(sn::ceil_div(n, kApplyThreads), b), kApplyThreads, 0, sn::as_stream(stream)>>>(a);
  return sn::launch_status(what);
}

extern "C" int sn_rigid_apply_host(const float *xyz, const double *pose, const double *scale, const int *lengths, int b,
                                   int n, float *out, int threads) {
  const char *what = "sn_rigid_apply_host";
  if (const int rc = check_apply(what, xyz, pose, b, n, out)) return rc;
  parallel_items(b, threads, [&](long cloud) {
    const int len = sn::clamped_length(lengths, (int)cloud, n);
    for (int i = 0; i < n; ++i) {
      const long row = (cloud * n + i) * 3;
      if (i < len)
        rigid::apply_row(pose + cloud * 16, scale ? scale[cloud] : 1.0, xyz + row, out + row);
      else
        out[row] = 0.0f, out[row + 1] = 0.0f, out[row + 2] = 0.0f;
    }
  });
  return 0;
}

extern "C" size_t sn_rigid_step_workspace_bytes(int b, int n) {
  if (b < 1 || n < 1) return 0;
  return (size_t)b * rigid::chunks_of(n) * kStride * sizeof(double);
}

extern "C" int sn_rigid_step(const float *moved, const float *dst, const int *idx, const float *weight,
                             const float *dst_normals, const int *src_lengths, const int *dst_lengths, int b, int n, int m,
                             int mode, int with_scale, double max_dist, double rtol, double atol, int freeze, double *pose,
                             double *scale, double *state, double *stats, void *workspace, size_t workspace_bytes,
                             void *stream) {
  const char *what = "sn_rigid_step";
  if (const int rc = check_step(what, moved, dst, idx, dst_normals, b, n, m, mode, with_scale, rtol, atol, freeze, pose,
                                scale, state, stats))
    return rc;
  const size_t need = sn_rigid_step_workspace_bytes(b, n);
  SN_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace too small (%zu < %zu)", what, workspace_bytes, need);
  const rigid::Problem P = problem_of(moved, dst, idx, weight, dst_normals, src_lengths, dst_lengths, n, m, mode, max_dist);
  const int chunks = rigid::chunks_of(n);
  double *partials = static_cast<double *>(workspace);
  const SolveArgs a{P, rigid::Rule{mode, with_scale, freeze, rtol, atol}, partials, pose, scale, state, stats, b, chunks};
  const dim3 grid(chunks, b);
  const unsigned solve_blocks = (unsigned)sn::ceil_div(b, kSolveThreads);
  hipStream_t s = sn::as_stream(stream);
  if (mode == 0) {
    rigid_accumulate_kernel<0><<<grid, kThreads, 0, s>>>(P, partials);
    rigid_solve_kernel<0><<<solve_blocks, kSolveThreads, 0, s>>>(a);
  } else {
    rigid_accumulate_kernel<1><<<grid, kThreads, 0, s>>>(P, partials);
    rigid_solve_kernel<1><<<solve_blocks, kSolveThreads, 0, s>>>(a);
  }
  return sn::launch_status(what);
}

extern "C" int sn_rigid_step_host(const float *moved, const float *dst, const int *idx, const float *weight,
                                  const float *dst_normals, const int *src_lengths, const int *dst_lengths, int b, int n,
                                  int m, int mode, int with_scale, double max_dist, double rtol, double atol, int freeze,
                                  double *pose, double *scale, double *state, double *stats, int threads) {
  const char *what = "sn_rigid_step_host";
  if (const int rc = check_step(what, moved, dst, idx, dst_normals, b, n, m, mode, with_scale, rtol, atol, freeze, pose,
                                scale, state, stats))
    return rc;
  if (weight)
    for (long e = 0; e < (long)b * n; ++e)
      if ((e % n) < sn::clamped_length(src_lengths, (int)(e / n), n))
        SN_REQUIRE(weight[e] >= 0.0f, "%s: weight must not be negative (cloud %ld, row %ld)", what, e / n, e % n);
  const rigid::Problem P = problem_of(moved, dst, idx, weight, dst_normals, src_lengths, dst_lengths, n, m, mode, max_dist);
  const rigid::Rule rule{mode, with_scale, freeze, rtol, atol};
  if (mode == 0)
    step_host<0>(P, rule, b, pose, scale, state, stats, threads);
  else
    step_host<1>(P, rule, b, pose, scale, state, stats, threads);
  return 0;
}
