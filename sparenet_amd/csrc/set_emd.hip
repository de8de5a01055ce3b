// set_emd.hip -- the auction EMD between every cloud of one set and every cloud of another (sn_set_emd_sums,
// include/sparenet_hip_ext_set_emd.h): sums[i,j] = sum over the bidders of x_i of sqrt(dist) after the auction of
// x_i for y_j, in float64.  MMD-EMD, COV-EMD and 1-NNA-EMD (sparenet_amd/utils/set_metrics.py) are read off such
// matrices.
//
// The auction is that of emd_general.hip, step for step: both run emd_auction.hpp, which states the semantics.  What
// differs is where the auction lives: at evaluation size (n <= m <= 2048) the whole state of one pair fits in one CU's
// LDS, so
//   * ONE workgroup of 1024 lanes runs the entire auction of one pair in one launch, its phases separated by
//     __syncthreads(); no global workspace, no other workgroup to wait for, nothing to be co-resident with;
//   * G lanes serve one bidder, G the largest power of two <= 64 that keeps cnt * G within the 1024 lanes, cnt the
//     workgroup-uniform unassigned count: as the count shrinks the lanes stay busy;
//   * the workgroup leaves the iteration loop when its count reaches 0 (every later iteration would be a no-op); the
//     count is read from LDS behind a barrier, so the exit is uniform;
//   * after the auction every bidder's dist is evaluated as emd_general_dist_kernel does, its square root is widened
//     to double, and the terms are added lane (bidders tid, tid + 1024) -> sn::block_sum_f64: an order that depends
//     on n alone.  ONE double per pair is written.
#include "block_scan.hpp"
#include "common.hpp"
#include "emd_auction.hpp"
#include "../../include/sparenet_hip_ext_set_emd.h"

namespace {

using namespace sn::emd;

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / sn::kWave;
constexpr int kMaxPoints = 2048;  // per cloud: 36 m + 32 n + 144 bytes of LDS, 139,408 of the 163,840 at 2048 / 2048
constexpr long kMaxGrid = 0xffffffffL / kThreads;  // workgroups per launch: grid x 1024 threads stays below 2^32
constexpr int kGroupSteps = 8;    // targets a lane scans between two exchanges of the group's filter threshold

// The auction state of one pair, carved from the workgroup's dynamic LDS: the one description of its size and places.
// price .. assignment are the rows of sn::emd::AuctionRows.
struct SetEmdLds {
  float4 *target;               // [m] x, y, z, filter_target(price)
  unsigned long long *max_idx;  // [m]
  double *wave_sum;             // [kWaves]
  float *price;                 // [m]
  int *assign_inv;              // [m]
  unsigned *max_key;            // [m]
  float *bidder;                // [n, 3]
  int *bid;                     // [n]
  float *bid_inc;               // [n]
  int *list0, *list1;           // [n] unassigned bidders of an even / odd iteration, any order
  int *assignment;              // [n]
  int *cnt;                     // [2] their number
};

// carves on `base` (16-byte aligned) and returns the bytes taken; the widest elements first, so every array is aligned
__host__ __device__ inline size_t set_emd_layout(char *base, int n, int m, SetEmdLds &L) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char *p = base ? base + off : nullptr;  // a null base only measures
    off += bytes;
    return p;
  };
  L.target = reinterpret_cast<float4 *>(take((size_t)m * 16));
  L.max_idx = reinterpret_cast<unsigned long long *>(take((size_t)m * 8));
  L.wave_sum = reinterpret_cast<double *>(take(kWaves * 8));
  L.price = reinterpret_cast<float *>(take((size_t)m * 4));
  L.assign_inv = reinterpret_cast<int *>(take((size_t)m * 4));
  L.max_key = reinterpret_cast<unsigned *>(take((size_t)m * 4));
  L.bidder = reinterpret_cast<float *>(take((size_t)n * 12));
  L.bid = reinterpret_cast<int *>(take((size_t)n * 4));
  L.bid_inc = reinterpret_cast<float *>(take((size_t)n * 4));
  L.list0 = reinterpret_cast<int *>(take((size_t)n * 4));
  L.list1 = reinterpret_cast<int *>(take((size_t)n * 4));
  L.assignment = reinterpret_cast<int *>(take((size_t)n * 4));
  L.cnt = reinterpret_cast<int *>(take(16));
  return off;
}

bool set_emd_sizes_ok(int n, int m) { return n >= 1 && n <= m && m <= kMaxPoints; }

// lanes per bidder: the largest power of two <= 64 with cnt * G <= kThreads (1 beyond kThreads bidders)
__device__ __forceinline__ int group_lanes(int cnt) {
  int G = 1;
  while (G < sn::kWave && 2 * cnt * G <= kThreads) G <<= 1;
  return G;
}

// grid nx * ny: workgroup i * ny + j holds the auction of x_i for y_j
__global__ __launch_bounds__(kThreads) void set_emd_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                           int n, int ny, int m, float eps, int iters,
                                                           double *__restrict__ sums, int *__restrict__ assignment) {
#pragma clang fp contract(off)
  extern __shared__ float4 set_emd_lds[];
  SetEmdLds L;
  set_emd_layout(reinterpret_cast<char *>(set_emd_lds), n, m, L);
  const int tid = threadIdx.x, lane = tid & (sn::kWave - 1);
  const size_t pair = blockIdx.x;
  const float *__restrict__ p1 = x + (pair / ny) * n * 3;
  const float *__restrict__ p2 = y + (pair % ny) * m * 3;

  for (int k = tid; k < m; k += kThreads) {
    L.target[k] = make_float4(p2[k * 3 + 0], p2[k * 3 + 1], p2[k * 3 + 2], filter_target(0.f));
    L.price[k] = 0.f;
    L.assign_inv[k] = -1;
    L.max_key[k] = sn::ordered_key(0.f);  // max_increments starts at 0
    L.max_idx[k] = 0ull;                  // ... and max_idx at 0: a stale index 0 from the start
  }
  for (int e = tid; e < n * 3; e += kThreads) L.bidder[e] = p1[e];
  for (int j = tid; j < n; j += kThreads) {
    L.assignment[j] = -1;
    L.list0[j] = j;
  }
  if (tid == 0) {
    L.cnt[0] = n;
    L.cnt[1] = 0;
  }
  __syncthreads();

  const AuctionRows rows{L.price, L.assign_inv, L.max_key, L.max_idx, L.bid, L.bid_inc, L.assignment};
  for (int it = 0; it < iters; ++it) {
    const int cur = it & 1, last = it == iters - 1;
    const int cnt = L.cnt[cur];  // settled behind the barrier that ended the previous assign phase
    if (cnt == 0) break;         // uniform: every later iteration is a no-op
    if (tid == 0) L.cnt[cur ^ 1] = 0;  // last read before the previous iteration's barriers; counted into after two more
    const int *list = cur ? L.list1 : L.list0;  // (no array indexed by cur: that would live in scratch)
    int *next_list = cur ? L.list0 : L.list1;

    // ---- bid: G lanes per bidder, kThreads / G bidders per pass; the resident records are scanned kGroupSteps
    // targets per lane between two exchanges of the group's filter bound
    {
      const int G = group_lanes(cnt), sub = tid & (G - 1), per_pass = kThreads / G;
      const int tile = G > 1 ? kGroupSteps * G : m;
      const TieGeom g = reference_tie_geom(n, m, cnt);
      for (int u0 = 0; u0 < cnt; u0 += per_pass) {  // uniform over the workgroup
        const int u = u0 + tid / G;
        const bool on = u < cnt;  // uniform over a group
        int j = 0;
        float x1 = 0.f, y1 = 0.f, z1 = 0.f;
        if (on) {
          j = list[u];
          x1 = L.bidder[j * 3 + 0];
          y1 = L.bidder[j * 3 + 1];
          z1 = L.bidder[j * 3 + 2];
        }
        Top2 t = {-1e9f, -1e9f, -1, -1};
        float cthr = filter_thr(t.better);
        for (int k0 = 0; k0 < m; k0 += tile) {
          if (on)  // the resident records are one tile from target 0
            scan_targets(t, cthr, L.target, L.price, 0, k0 + sub, k0 + tile < m ? k0 + tile : m, G, x1, y1, z1, g);
          if (G > 1) cthr = share_filter_bound(t, G, cthr);
        }
        merge_group(t, G, g);
        if (on && sub == 0) post_bid(rows, j, t, eps);
      }
    }
    __syncthreads();

    // ---- window
    if (!last) {
      for (int u = tid; u < cnt; u += kThreads) offer_window(rows, list[u], (unsigned)(it + 1));
      __syncthreads();
    }

    // ---- assign; a winner's record takes the filter word of its new price
    for (int base = 0; base < cnt; base += kThreads) {  // uniform over the workgroup
      const int u = base + tid;
      int push = -1;
      if (u < cnt) {
        const Settled s = settle(rows, list[u], last);
        if (s.target >= 0) L.target[s.target].w = filter_target(s.price);
        push = s.requeue;
      }
      append_unassigned(push, lane, next_list, &L.cnt[cur ^ 1]);
    }
    __syncthreads();
  }

  // ---- the pair's number: every bidder's dist, its square root in double, added in the fixed order of the file's header
  double acc = 0.0;
  for (int j = tid; j < n; j += kThreads) {
    const int k = L.assignment[j];
    acc += (double)__builtin_sqrtf(matched_sq_dist(k, L.bidder + j * 3, L.target + k));
    if (assignment) assignment[pair * n + j] = k;
  }
  acc = sn::block_sum_f64<kThreads>(acc, L.wave_sum);
  if (tid == 0) sums[pair] = acc;
}

}  // namespace

extern "C" size_t sn_set_emd_lds_bytes(int n, int m) {
  if (!set_emd_sizes_ok(n, m)) return 0;
  SetEmdLds L;
  return set_emd_layout(nullptr, n, m, L);
}

extern "C" int sn_set_emd_sums(const float *x, const float *y, int nx, int n, int ny, int m, float eps, int iters,
                               double *sums, int *assignment, void *stream) {
  SN_REQUIRE(x && y && sums, "sn_set_emd_sums: null pointer");
  SN_REQUIRE(nx >= 1 && ny >= 1 && n >= 1 && m >= 1, "sn_set_emd_sums: need nx,n,ny,m >= 1 (got %d,%d,%d,%d)", nx, n,
             ny, m);
  SN_REQUIRE(n <= m, "sn_set_emd_sums: n=%d > m=%d: pass the smaller clouds first (x bids for y)", n, m);
  SN_REQUIRE(m <= kMaxPoints, "sn_set_emd_sums: at most %d points per cloud (got m=%d)", kMaxPoints, m);
  SN_REQUIRE(iters >= 0, "sn_set_emd_sums: iters must be >= 0");
  SN_REQUIRE((long)nx * ny <= 0x7fffffffL, "sn_set_emd_sums: nx * ny must not exceed 2^31 - 1 (got %d x %d)", nx, ny);
  SN_REQUIRE(!assignment || (long)nx * ny * n <= 0x7fffffffL,
             "sn_set_emd_sums: nx * ny * n must not exceed 2^31 - 1 when the assignment is asked for (got %d x %d x %d)",
             nx, ny, n);
  SN_REQUIRE((long)nx * ny <= kMaxGrid, "sn_set_emd_sums: too large (%ld pairs in one launch, at most %ld)",
             (long)nx * ny, kMaxGrid);
  const size_t lds = sn_set_emd_lds_bytes(n, m);
  // above the 64 KB a launch may ask for unannounced.  Every call: the attribute belongs to the CURRENT device
  SN_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&set_emd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)sn_set_emd_lds_bytes(kMaxPoints, kMaxPoints)));
  hipStream_t s = sn::as_stream(stream);
  SN_TIMED("set_emd", s,
           (set_emd_kernel<<<(unsigned)((long)nx * ny), kThreads, lds, s>>>(x, y, n, ny, m, eps, iters, sums,
                                                                            assignment)));
  return sn::launch_status("sn_set_emd_sums");
}
