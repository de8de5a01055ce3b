// emd_general.hip -- auction EMD for clouds of any size 1 <= n <= m (sn_emd_forward_general /
// sn_emd_backward_general; semantics in include/sparenet_hip.h).
//
// The persistent auction of emd.hip is built around n == m, n % 1024 == 0: teams of workgroups own a cloud and wait
// for each other inside one launch.  This path runs every phase as an ordinary stream-ordered launch, three per
// iteration -- bid, window, assign: the steps of emd_auction.hpp over the cloud's rows of the global workspace -- and
// no workgroup ever waits for another.  The next iteration's unassigned count is final when its bid launch starts, so
// tpu -- and with it the tie rule of the bid -- is read from a settled word.
//
// Bid (the hot path, O(cnt * m) per iteration): a workgroup stages tiles of 1024 targets {x, y, z, A'(price)} in
// LDS; G lanes serve one bidder (G = 1 while the clouds have many bidders, up to a whole wave when few are left) and
// exchange their filter bound after every tile.
#include "block_scan.hpp"
#include "common.hpp"
#include "emd_auction.hpp"
#include "lds_sort.hpp"

namespace {

using namespace sn::emd;

constexpr int kGThreads = 256;
constexpr int kTile = 1024;             // targets per LDS tile (16 KiB)
// lanes a bid launch aims for: 256 CUs x 4 SIMDs x 8 waves x 64.  Measured at B=32, 0.005 / 50 iterations (ms per
// call, 16000 -> 16000 and 3000 -> 16384): 2^17 28.8 / 2.53, 2^18 21.7 / 2.27, 2^19 16.6 / 1.45, 2^20 16.3 / 1.51
constexpr long kLanesWanted = 1L << 19;
// cap of the per-element launches; every total is >= 1 (the entry points require b, n, m >= 1), so the floor of
// sn::grid_blocks never acts
constexpr int kMaxEltBlocks = 2048;

struct GenWs {
  float *price;                 // [b, m]  these six: the rows of sn::emd::AuctionRows, cloud after cloud
  int *assign_inv;              // [b, m]
  unsigned *max_key;            // [b, m]
  unsigned long long *max_idx;  // [b, m]
  int *bid;                     // [b, n]
  float *bid_inc;               // [b, n]
  int *list[2];                 // [b, n] unassigned bidders of an iteration, any order
  int *cnt[2];                  // [b]    their number

  // cloud i's rows; n and m are the strides
  __device__ __forceinline__ AuctionRows rows(int i, int n, int m, int *assignment) const {
    const size_t om = (size_t)i * m, on = (size_t)i * n;
    return AuctionRows{price + om, assign_inv + om, max_key + om, max_idx + om, bid + on, bid_inc + on,
                       assignment ? assignment + on : nullptr};
  }
};

// lanes per bidder: the power of two <= 64 that gives the launch about kLanesWanted lanes (every cloud is assumed to
// have as many bidders as this one).  cnt * G < 2 * kLanesWanted / B whenever G > 1 (see bid_blocks).
__host__ __device__ inline int group_lanes(int cnt, int B) {
  const long want = kLanesWanted / ((long)B * cnt);
  int G = 1;
  while (G < 64 && G < want) G <<= 1;
  return G;
}

// workgroups per cloud that cover cnt * group_lanes(cnt, B) lanes for every cnt <= n
int bid_blocks(int B, int n) {
  long lanes = 2 * kLanesWanted / B;
  if (lanes > 64L * n) lanes = 64L * n;
  if (lanes < n) lanes = n;
  return (int)((lanes + kGThreads - 1) / kGThreads);
}

// the workspace of the stream-ordered auction
GenWs gen_layout(sn::Carver &c, int b, int n, int m) {
  const size_t tm = (size_t)b * m * 4, tn = (size_t)b * n * 4;
  GenWs w;
  w.max_idx = c.take<unsigned long long>(2 * sn::align_up(tm, 256));  // 8-byte words: two word arrays
  w.price = c.take256<float>(tm);
  w.assign_inv = c.take256<int>(tm);
  w.max_key = c.take256<unsigned>(tm);
  w.bid = c.take256<int>(tn);
  w.bid_inc = c.take256<float>(tn);
  w.list[0] = c.take256<int>(tn);
  w.list[1] = c.take256<int>(tn);
  w.cnt[0] = c.take256<int>((size_t)b * 4);
  w.cnt[1] = c.take256<int>((size_t)b * 4);
  return w;
}

// Ragged batches (sn_emd_forward_ragged / sn_emd_backward_ragged): the kernels below take the padded widths as n and m
// -- the strides of every array -- and cloud i has its first lengths1[i] rows as bidders and its first lengths2[i] rows
// as targets.  Dense calls pass no lengths and kRagged = false: every row counts.
struct Ragged {
  const int *lengths1, *lengths2;
};
struct CloudSize {
  int n, m;  // bidders and targets; n == 0: the cloud takes no part (ragged only: lengths1 == 0 or > lengths2)
};
template <bool kRagged>
__device__ __forceinline__ CloudSize cloud_size(Ragged r, long i, int n, int m) {
  if constexpr (kRagged) {
    const int a = r.lengths1[i], b = r.lengths2[i];
    return (a >= 1 && a <= b && a <= n && b <= m) ? CloudSize{a, b} : CloudSize{0, 0};
  } else {
    return CloudSize{n, m};
  }
}

template <bool kRagged>
__global__ __launch_bounds__(kGThreads) void gen_init_kernel(int B, int n, int m, int *__restrict__ assignment, GenWs w,
                                                             Ragged r) {
  const long stride = (long)gridDim.x * blockDim.x, first = (long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long e = first; e < (long)B * m; e += stride) {
    w.price[e] = 0.f;
    w.assign_inv[e] = -1;
    w.max_key[e] = sn::ordered_key(0.f);  // max_increments starts at 0 (emd_module.py:49)
    w.max_idx[e] = 0ull;          // ... and max_idx at 0: a stale index 0 from the start
  }
  for (long e = first; e < (long)B * n; e += stride) {
    assignment[e] = -1;
    w.list[0][e] = (int)(e % n);
  }
  for (long e = first; e < B; e += stride) {
    w.cnt[0][e] = cloud_size<kRagged>(r, e, n, m).n;  // 0: no bid, window or assign launch touches the cloud
    w.cnt[1][e] = 0;
  }
}

struct BidArgs {
  int B, n, m, cur;
  float eps;
  const float *xyz1, *xyz2;
  GenWs w;
  long long *stats;
  Ragged r;
};

// grid (bid_blocks(B, n), B); lane l of cloud i serves bidder l / G with sub-lane l % G
template <bool kRagged>
__global__ __launch_bounds__(kGThreads) void emd_general_bid_kernel(BidArgs a) {
  __shared__ float4 s_t[kTile];  // x, y, z, filter_target(price)
  const int i = blockIdx.y, n = a.n, m = a.m;  // strides
  const int cnt = a.w.cnt[a.cur][i];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.w.cnt[a.cur ^ 1][i] = 0;  // this iteration's assign launch counts the next list into it
    if (cnt > 0 && a.stats) {
      atomicAdd(reinterpret_cast<unsigned long long *>(a.stats),
                (unsigned long long)cnt * cloud_size<kRagged>(a.r, i, n, m).m);
      if (i == 0) atomicAdd(reinterpret_cast<unsigned long long *>(a.stats) + 1, 1ULL);
    }
  }
  if (cnt == 0) return;
  const int G = group_lanes(cnt, a.B);
  const int first = blockIdx.x * kGThreads;
  if (first / G >= cnt) return;  // uniform over the workgroup
  const int lane = first + (int)threadIdx.x, u = lane / G, sub = lane & (G - 1);
  const bool on = u < cnt;
  const CloudSize cs = cloud_size<kRagged>(a.r, i, n, m);  // cnt > 0: the cloud takes part
  const TieGeom g = reference_tie_geom(cs.n, cs.m, cnt);
  const AuctionRows rows = a.w.rows(i, n, m, nullptr);
  int j = 0;
  float x1 = 0.f, y1 = 0.f, z1 = 0.f;
  if (on) {
    j = a.w.list[a.cur][(size_t)i * n + u];
    const float *p = a.xyz1 + ((size_t)i * n + j) * 3;
    x1 = p[0];
    y1 = p[1];
    z1 = p[2];
  }
  const float *p2 = a.xyz2 + (size_t)i * m * 3;
  const float *price = rows.price;
  Top2 t = {-1e9f, -1e9f, -1, -1};
  float cthr = filter_thr(t.better);
  for (int k0 = 0; k0 < cs.m; k0 += kTile) {
    const int tn = cs.m - k0 < kTile ? cs.m - k0 : kTile;
    __syncthreads();  // the previous tile is consumed
    for (int c = threadIdx.x; c < tn; c += kGThreads) {
      const float *q = p2 + (size_t)(k0 + c) * 3;
      s_t[c] = make_float4(q[0], q[1], q[2], filter_target(price[k0 + c]));
    }
    __syncthreads();
    if (on) scan_targets(t, cthr, s_t, price, k0, sub, tn, G, x1, y1, z1, g);
    if (G > 1) cthr = share_filter_bound(t, G, cthr);
  }
  merge_group(t, G, g);
  if (on && sub == 0) post_bid(rows, j, t, a.eps);
}

// grid (x, B): GetMax.  Every bidder inside the window of its target's maximum offers (stamp << 32) | j.
__global__ __launch_bounds__(kGThreads) void emd_general_window_kernel(int n, int m, int cur, unsigned stamp, GenWs w) {
  const int i = blockIdx.y;
  const int cnt = w.cnt[cur][i];
  const AuctionRows rows = w.rows(i, n, m, nullptr);
  for (int u = blockIdx.x * kGThreads + threadIdx.x; u < cnt; u += gridDim.x * kGThreads)
    offer_window(rows, w.list[cur][(size_t)i * n + u], stamp);
}

// grid (x, B): Assign.  Bidders that stay or become unassigned go to the next list (wave-aggregated appends).
__global__ __launch_bounds__(kGThreads) void emd_general_assign_kernel(int n, int m, int cur, int last, GenWs w,
                                                                       int *__restrict__ assignment) {
  const int i = blockIdx.y, lane = threadIdx.x & 63;
  const int cnt = w.cnt[cur][i];
  int *next_list = w.list[cur ^ 1] + (size_t)i * n;
  int *next_cnt = &w.cnt[cur ^ 1][i];
  const AuctionRows rows = w.rows(i, n, m, assignment);
  for (int base = blockIdx.x * kGThreads; base < cnt; base += gridDim.x * kGThreads) {  // uniform over the workgroup
    const int u = base + (int)threadIdx.x;
    const int push = u < cnt ? settle(rows, w.list[cur][(size_t)i * n + u], last).requeue : -1;
    append_unassigned(push, lane, next_list, next_cnt);
  }
}

// CalcDist: every bidder's squared distance to the target it holds
template <bool kRagged>
__global__ __launch_bounds__(kGThreads) void emd_general_dist_kernel(int B, int n, int m, const float *__restrict__ xyz1,
                                                                     const float *__restrict__ xyz2,
                                                                     const int *__restrict__ assignment,
                                                                     float *__restrict__ dist, Ragged r) {
#pragma clang fp contract(off)
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < (long)B * n; e += (long)gridDim.x * blockDim.x) {
    if constexpr (kRagged) {
      if (cloud_size<true>(r, e / n, n, m).n == 0) {  // no auction was held: the whole row says so
        dist[e] = __builtin_nanf("");
        continue;
      }
    }
    const int k = assignment[e];
    dist[e] = matched_sq_dist(k, xyz1 + e * 3, xyz2 + ((e / n) * m + k) * 3);
  }
}

// ---- backward.  gradxyz1 per bidder; gradxyz2[k] = ((0 - t_j1) - t_j2) - ... over the bidders j1 < j2 < ... assigned
// to k, t_j = gradxyz1[j].  The ascending-j sums go through a stable counting sort by target: count per target, an
// exclusive scan per cloud, a stable scatter of the terms into each target's contiguous segment (chunks of 1024
// bidders in ascending j, ranked inside a chunk by a bitonic sort of (target, j)), then one sequential fp32 sum per
// segment.  Linear in n + m: a target shared by every bidder (a collapsed prediction) costs one pass over its segment.
struct BwdWs {
  int *count;   // [b, m] bidders per target
  int *off;     // [b, m] exclusive prefix of count inside the cloud
  int *run;     // [b, m] bidders of the target already placed by earlier chunks
  float *terms; // [b, n, 3] gradxyz1 rows in (target, j) order
};

BwdWs bwd_layout(sn::Carver &c, int b, int n, int m) {
  BwdWs w;
  w.count = c.take256<int>((size_t)b * m * 4);
  w.off = c.take256<int>((size_t)b * m * 4);
  w.run = c.take256<int>((size_t)b * m * 4);
  w.terms = c.take256<float>((size_t)b * n * 12);
  return w;
}

// the target bidder j of cloud c holds, -1 for none: a padding row or a cloud that takes no part holds none whatever
// the assignment array says, and an index beyond the cloud's targets is treated the same
template <bool kRagged>
__device__ __forceinline__ int held_target(const int *__restrict__ assignment, long c, int j, int n, int m, Ragged r) {
  const CloudSize cs = cloud_size<kRagged>(r, c, n, m);
  if (j >= cs.n) return -1;
  const int k = assignment[c * n + j];
  return k < cs.m ? k : -1;
}

// gradxyz1 (the formula of sn_emd_backward) and, when gradxyz2 is wanted, the bidders per target
template <bool kRagged>
__global__ __launch_bounds__(kGThreads) void emd_general_bwd1_kernel(int B, int n, int m, const float *__restrict__ xyz1,
                                                                     const float *__restrict__ xyz2,
                                                                     const float *__restrict__ graddist,
                                                                     const int *__restrict__ assignment,
                                                                     float *__restrict__ grad1, int *count, Ragged r) {
#pragma clang fp contract(off)
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < (long)B * n; e += (long)gridDim.x * blockDim.x) {
    const long c = e / n;
    const int k = kRagged ? held_target<kRagged>(assignment, c, (int)(e - c * n), n, m, r) : assignment[e];
    if (k < 0 || k >= m) {  // unassigned (iters == 0); an index out of range is treated the same
      grad1[e * 3 + 0] = grad1[e * 3 + 1] = grad1[e * 3 + 2] = 0.f;
      continue;
    }
    const float *p = xyz1 + e * 3, *q = xyz2 + (c * m + k) * 3;
    const float g = graddist[e] * 2;
    grad1[e * 3 + 0] = g * (p[0] - q[0]);
    grad1[e * 3 + 1] = g * (p[1] - q[1]);
    grad1[e * 3 + 2] = g * (p[2] - q[2]);
    if (count) atomicAdd(&count[c * m + k], 1);
  }
}

constexpr int kSortThreads = 1024;

// one workgroup per cloud: off = exclusive scan of count over the cloud's targets; run = 0
__global__ __launch_bounds__(kSortThreads) void emd_general_bwd_scan_kernel(int m, BwdWs w) {
  __shared__ alignas(16) sn::BlockScan<kSortThreads> scan;
  const size_t o = (size_t)blockIdx.x * m;
  scan.reset(0);
  for (int k0 = 0; k0 < m; k0 += kSortThreads) {
    const int k = k0 + threadIdx.x;
    scan.chunk(k < m ? w.count[o + k] : 0, [&](int start) {
      if (k < m) {
        w.off[o + k] = start;
        w.run[o + k] = 0;
      }
    });
  }
}

// one workgroup per cloud: the stable scatter.  Chunk after chunk of 1024 bidders in ascending j; the chunk's
// (target << 10 | local j) keys are sorted (lds_sort.hpp's key sort), a bidder's rank among the chunk's bidders of its
// target is its distance from the first key of the target, and the last of them advances the target's run.
template <bool kRagged>
__global__ __launch_bounds__(kSortThreads) void emd_general_bwd_scatter_kernel(int n, int m,
                                                                               const int *__restrict__ assignment,
                                                                               const float *__restrict__ grad1,
                                                                               BwdWs w, Ragged r) {
  __shared__ unsigned sk[kSortThreads];
  const int tid = threadIdx.x;
  const size_t c = blockIdx.x;
  const unsigned kNone = 0xffffffffu;
  for (int j0 = 0; j0 < n; j0 += kSortThreads) {
    const int j = j0 + tid;
    const int k = j >= n ? -1 : kRagged ? held_target<kRagged>(assignment, c, j, n, m, r) : assignment[c * n + j];
    sk[tid] = (k >= 0 && k < m) ? ((unsigned)k << 10) | (unsigned)tid : kNone;  // k < 2^20: fits
    __syncthreads();
    lds_sort::sort_keys<kSortThreads>(sk, kSortThreads);
    const unsigned key = sk[tid];
    int rank = 0, tk = 0;
    if (key != kNone) {
      tk = (int)(key >> 10);
      int lo = 0, hi = tid;  // first position holding target tk
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((sk[mid] >> 10) < (unsigned)tk) lo = mid + 1; else hi = mid;
      }
      rank = tid - lo;
      const size_t ot = c * m + tk;
      const size_t pos = c * n + w.off[ot] + w.run[ot] + rank;
      const size_t src = (c * n + j0 + (key & 1023u)) * 3;
      w.terms[pos * 3 + 0] = grad1[src + 0];
      w.terms[pos * 3 + 1] = grad1[src + 1];
      w.terms[pos * 3 + 2] = grad1[src + 2];
    }
    __syncthreads();  // every rank of this chunk read run[] before it advances
    if (key != kNone && (tid == kSortThreads - 1 || (sk[tid + 1] >> 10) != (unsigned)tk))
      w.run[c * m + tk] += rank + 1;
    __syncthreads();  // run[] and sk[] are reused by the next chunk
  }
}

// one thread per target: the ascending-j sum over its segment
__global__ __launch_bounds__(kGThreads) void emd_general_bwd_sum_kernel(int B, int n, int m, BwdWs w,
                                                                        float *__restrict__ grad2) {
#pragma clang fp contract(off)
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < (long)B * m; e += (long)gridDim.x * blockDim.x) {
    const long c = e / m;
    const float *t = w.terms + (c * n + w.off[e]) * 3;
    const int cnt = w.count[e];
    float sx = 0.f, sy = 0.f, sz = 0.f;
#pragma unroll 4
    for (int p = 0; p < cnt; ++p) {
      sx = sx - t[p * 3 + 0];
      sy = sy - t[p * 3 + 1];
      sz = sz - t[p * 3 + 2];
    }
    grad2[e * 3 + 0] = sx;
    grad2[e * 3 + 1] = sy;
    grad2[e * 3 + 2] = sz;
  }
}

bool persistent_shape(int b, int n, int m) { return n == m && n % 1024 == 0 && b <= 512; }

}  // namespace

extern "C" size_t sn_emd_general_workspace_bytes(int b, int n, int m) {
  if (b < 1 || n < 1 || m < n) return 0;
  const size_t own = sn::layout_bytes(gen_layout, b, n, m);
  if (!persistent_shape(b, n, m)) return own;
  const size_t pers = sn_emd_workspace_bytes(b, n);  // the dispatch may hand the call to sn_emd_forward
  return pers > own ? pers : own;
}

namespace {

// the stream-ordered auction: three launches per iteration, no workgroup waits for another
template <bool kRagged>
int forward_launches(const char *what, const float *xyz1, const float *xyz2, int b, int n, int m, Ragged r, float eps,
                     int iters, float *dist, int *assignment, void *workspace, size_t workspace_bytes, long long *stats,
                     void *stream) {
  hipStream_t s = sn::as_stream(stream);
  sn::Carver carver(workspace);
  const GenWs w = gen_layout(carver, b, n, m);
  SN_REQUIRE(workspace_bytes >= carver.bytes(), "%s: workspace too small (%zu < %zu)", what, workspace_bytes,
             carver.bytes());
  gen_init_kernel<kRagged><<<sn::grid_blocks((long)b * (m > n ? m : n), kMaxEltBlocks, kGThreads), kGThreads, 0, s>>>(
      b, n, m, assignment, w, r);
  BidArgs ba;
  ba.B = b;
  ba.n = n;
  ba.m = m;
  ba.eps = eps;
  ba.xyz1 = xyz1;
  ba.xyz2 = xyz2;
  ba.w = w;
  ba.stats = stats;
  ba.r = r;
  const dim3 bid_grid(bid_blocks(b, n), b);
  int xb = (n + kGThreads - 1) / kGThreads;
  const dim3 list_grid(xb < 64 ? xb : 64, b);
  for (int it = 0; it < iters; ++it) {
    const int cur = it & 1, last = it == iters - 1;
    ba.cur = cur;
    SN_TIMED(kRagged ? "emd_ragged_bid" : "emd_general_bid", s,
             (emd_general_bid_kernel<kRagged><<<bid_grid, kGThreads, 0, s>>>(ba)));
    if (!last) emd_general_window_kernel<<<list_grid, kGThreads, 0, s>>>(n, m, cur, (unsigned)it + 1, w);
    emd_general_assign_kernel<<<list_grid, kGThreads, 0, s>>>(n, m, cur, last, w, assignment);
  }
  emd_general_dist_kernel<kRagged><<<sn::grid_blocks((long)b * n, kMaxEltBlocks, kGThreads), kGThreads, 0, s>>>(
      b, n, m, xyz1, xyz2, assignment, dist, r);
  return sn::launch_status(what);
}

template <bool kRagged>
int backward_launches(const char *what, const float *xyz1, const float *xyz2, const float *graddist,
                      const int *assignment, int b, int n, int m, Ragged r, float *gradxyz1, float *gradxyz2,
                      void *workspace, size_t workspace_bytes, void *stream) {
  hipStream_t s = sn::as_stream(stream);
  BwdWs w{};
  if (gradxyz2) {
    sn::Carver carver(workspace);
    w = bwd_layout(carver, b, n, m);
    SN_REQUIRE(workspace && workspace_bytes >= carver.bytes(), "%s: workspace too small (%zu < %zu)", what,
               workspace_bytes, carver.bytes());
    SN_HIP(hipMemsetAsync(w.count, 0, (size_t)b * m * 4, s));
  }
  emd_general_bwd1_kernel<kRagged><<<sn::grid_blocks((long)b * n, kMaxEltBlocks, kGThreads), kGThreads, 0, s>>>(
      b, n, m, xyz1, xyz2, graddist, assignment, gradxyz1, w.count, r);
  if (gradxyz2) {
    emd_general_bwd_scan_kernel<<<b, kSortThreads, 0, s>>>(m, w);
    emd_general_bwd_scatter_kernel<kRagged><<<b, kSortThreads, 0, s>>>(n, m, assignment, gradxyz1, w, r);
    emd_general_bwd_sum_kernel<<<sn::grid_blocks((long)b * m, kMaxEltBlocks, kGThreads), kGThreads, 0, s>>>(b, n, m, w,
                                                                                                           gradxyz2);
  }
  return sn::launch_status(what);
}

}  // namespace

extern "C" int sn_emd_forward_general(const float *xyz1, const float *xyz2, int b, int n, int m, float eps, int iters,
                                      float *dist, int *assignment, void *workspace, size_t workspace_bytes,
                                      long long *stats, void *stream) {
  SN_REQUIRE(xyz1 && xyz2 && dist && assignment && workspace, "sn_emd_forward_general: null pointer");
  SN_REQUIRE(b >= 1 && b <= 65535, "sn_emd_forward_general: batch size must be in [1,65535] (got %d)", b);
  SN_REQUIRE(n >= 1 && m >= 1, "sn_emd_forward_general: need n, m >= 1 (got n=%d, m=%d)", n, m);
  SN_REQUIRE(n <= m, "sn_emd_forward_general: n=%d > m=%d: pass the smaller cloud first (xyz1 bids for xyz2)", n, m);
  SN_REQUIRE(m <= (1 << 20), "sn_emd_forward_general: m must be <= 2^20 (got %d)", m);
  SN_REQUIRE(iters >= 0, "sn_emd_forward_general: iters must be >= 0");
  // the larger of the two layouts, whichever auction runs; each then checks its own carver
  SN_REQUIRE(workspace_bytes >= sn_emd_general_workspace_bytes(b, n, m),
             "sn_emd_forward_general: workspace too small (%zu < %zu)", workspace_bytes,
             sn_emd_general_workspace_bytes(b, n, m));
  {  // the shapes the persistent auction serves go there, unless SN_EMD_GENERAL=1
    const char *e = SN_KNOB("SN_EMD_GENERAL");
    if (!(e && e[0] == '1') && persistent_shape(b, n, m))
      return sn_emd_forward(xyz1, xyz2, b, n, eps, iters, dist, assignment, workspace, workspace_bytes, stats, stream);
  }
  return forward_launches<false>("sn_emd_forward_general", xyz1, xyz2, b, n, m, Ragged{nullptr, nullptr}, eps, iters, dist,
                                 assignment, workspace, workspace_bytes, stats, stream);
}

// ---- ragged batches: the same launches over the padded widths; never the persistent auction
extern "C" size_t sn_emd_ragged_workspace_bytes(int b, int n, int m) {
  if (b < 1 || n < 1 || m < 1) return 0;
  return sn::layout_bytes(gen_layout, b, n, m);
}

extern "C" int sn_emd_forward_ragged(const float *xyz1, const float *xyz2, int b, int n, int m, const int *lengths1,
                                     const int *lengths2, float eps, int iters, float *dist, int *assignment,
                                     void *workspace, size_t workspace_bytes, long long *stats, void *stream) {
  SN_REQUIRE(xyz1 && xyz2 && lengths1 && lengths2 && dist && assignment && workspace,
             "sn_emd_forward_ragged: null pointer");
  SN_REQUIRE(b >= 1 && b <= 65535, "sn_emd_forward_ragged: batch size must be in [1,65535] (got %d)", b);
  SN_REQUIRE(n >= 1 && m >= 1 && n <= (1 << 20) && m <= (1 << 20),
             "sn_emd_forward_ragged: the padded widths must be in [1, 2^20] (got n=%d, m=%d)", n, m);
  SN_REQUIRE(iters >= 0, "sn_emd_forward_ragged: iters must be >= 0");
  return forward_launches<true>("sn_emd_forward_ragged", xyz1, xyz2, b, n, m, Ragged{lengths1, lengths2}, eps, iters,
                                dist, assignment, workspace, workspace_bytes, stats, stream);
}

extern "C" size_t sn_emd_general_backward_workspace_bytes(int b, int n, int m) {
  if (b < 1 || n < 1 || m < n) return 0;
  return sn::layout_bytes(bwd_layout, b, n, m);
}

extern "C" int sn_emd_backward_general(const float *xyz1, const float *xyz2, const float *graddist,
                                       const int *assignment, int b, int n, int m, float *gradxyz1, float *gradxyz2,
                                       void *workspace, size_t workspace_bytes, void *stream) {
  SN_REQUIRE(xyz1 && xyz2 && graddist && assignment && gradxyz1, "sn_emd_backward_general: null pointer");
  SN_REQUIRE(b >= 1 && b <= 65535 && n >= 1 && n <= m && m <= (1 << 20),
             "sn_emd_backward_general: need 1 <= b <= 65535, 1 <= n <= m <= 2^20 (got b=%d, n=%d, m=%d)", b, n, m);
  return backward_launches<false>("sn_emd_backward_general", xyz1, xyz2, graddist, assignment, b, n, m,
                                  Ragged{nullptr, nullptr}, gradxyz1, gradxyz2, workspace, workspace_bytes, stream);
}

extern "C" size_t sn_emd_ragged_backward_workspace_bytes(int b, int n, int m) {
  if (b < 1 || n < 1 || m < 1) return 0;
  return sn::layout_bytes(bwd_layout, b, n, m);
}

extern "C" int sn_emd_backward_ragged(const float *xyz1, const float *xyz2, const float *graddist,
                                      const int *assignment, int b, int n, int m, const int *lengths1,
                                      const int *lengths2, float *gradxyz1, float *gradxyz2, void *workspace,
                                      size_t workspace_bytes, void *stream) {
  SN_REQUIRE(xyz1 && xyz2 && graddist && assignment && lengths1 && lengths2 && gradxyz1,
             "sn_emd_backward_ragged: null pointer");
  SN_REQUIRE(b >= 1 && b <= 65535 && n >= 1 && m >= 1 && n <= (1 << 20) && m <= (1 << 20),
             "sn_emd_backward_ragged: need 1 <= b <= 65535 and padded widths in [1, 2^20] (got b=%d, n=%d, m=%d)", b, n,
             m);
  return backward_launches<true>("sn_emd_backward_ragged", xyz1, xyz2, graddist, assignment, b, n, m,
                                 Ragged{lengths1, lengths2}, gradxyz1, gradxyz2, workspace, workspace_bytes, stream);
}
