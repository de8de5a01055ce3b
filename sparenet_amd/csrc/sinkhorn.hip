// sinkhorn.hip -- entropic optimal transport between two clouds: the streaming softmin that is both half-iterations of
// the log-domain Sinkhorn loop, and the barycentric map of its gradient (include/ops/sinkhorn.h states the rules).
//
// One kernel, sinkhorn_softmin_kernel<WITH_BARY>.  For every query i of a cloud it computes
//   out_i = -e * log( (1 / len_t) sum_{j < len_t} exp( (p_j - C_ij) / e ) )
// over the cloud's targets t_j with potential p_j; with the roles of the two clouds swapped it is the other
// half-iteration.  WITH_BARY also accumulates sum_j w_ij t_j for the normalised weights w.
// The structure is the search of neighbors.hip with other per-pair work.  A query lives in the registers of one lane;
// the targets stream through an LDS tile in the chunk-SoA layout of chamfer_tile.hpp extended by the potential --
// x[8] y[8] z[8] h[8] per chunk = 8 float4, read with wave-uniform 16-byte loads (a broadcast, conflict free).  The
// potential is converted to the exponent's units once, at the tile load: h_j = p_j * k with k = log2(e) / eps, so a
// pair's exponent is s = h_j - C_ij * k, one FMA behind the 8-operation distance, and the exponential is the hardware's
// base-2 one.  The uniform weight is NOT folded into h: the fp32 rounding of log2(1 / len_t), half an ulp of a number
// near 8, would move every output of a half-iteration the same way by up to eps * 3.3e-7, and a common shift of f
// against g is the one direction the iteration never damps -- the large-eps steps of an annealed schedule would leave
// 1.6e-6 in the final potentials that way ("Sinkhorn transport").  The weight enters once per query instead,
// as sum / len_t under the final log2: a correctly rounded division.
// The sum is kept against a running maximum that is rescaled once per chunk: the chunk's maximum by a max3 tree, one
// exp2(m_old - m_new) per chunk, one exp2(s - m_new) per pair.  The maximum starts at the lowest finite float and the
// padding slots of a tile's last chunk carry h = -inf with coordinates 0, so it is finite throughout, every difference
// has a finite right-hand side (never inf - inf) and a padding slot adds exactly 0.  log2 is taken once per query at
// the end.
// A workgroup is S groups of G lanes: group g walks segment g of the S contiguous segments of the targets for the
// workgroup's G queries through a tile of its own.
//   S == 1: G = 256 queries per workgroup, one tile of 1024 targets (the wide path);
//   S >= 2: G = 64, one wave per segment, tiles of 192 targets, then the segments' (max, sum[, 3 sums]) are merged in
//           LDS by segment 0 in segment order.
// No floating-point atomics, no workgroup waits for another, no [b,n,m] intermediate; the order of every sum is fixed
// by the shape and S, so two calls give identical bits.
#include "chamfer_tile.hpp"
#include "common.hpp"
#include "split_launch.hpp"
#include "../../include/ops/sinkhorn.h"

#include <cmath>

namespace {

using sn::ct::dist1;

constexpr int kWideTile = 1024;            // targets per tile, S == 1
constexpr int kSplitTile = 192;            // targets per segment tile, S >= 2: 16 of them are 48 KiB
constexpr int kMaxSplit = 16;              // waves of a 1024-thread workgroup
constexpr int kWavesPerCu = 32;            // what the dispatch fills the device to before it stops splitting
constexpr int kMinSegment = 128;           // ... and the shortest segment it splits down to
constexpr int kMaxPoints = 1 << 30;
constexpr int kFields = 5;                 // what a segment hands to the merge: max, sum, three coordinate sums
constexpr float kLowest = -3.4028234664e38f;

static_assert(sn::ct::kChunk == 8 && kWideTile % 8 == 0 && kSplitTile % 8 == 0, "tile chunks");
static_assert(kMaxSplit * kSplitTile * 16 <= 48 * 1024 && kWideTile * 16 <= 48 * 1024, "LDS of the tiles");
static_assert(64 * kFields * 4 <= kSplitTile * 16, "a segment's merge record fits its own tile");

// float index of component comp (0..2 = x y z, 3 = h) of a tile's target k
__device__ __forceinline__ int slot(int k, int comp) { return (k >> 3) * 32 + comp * 8 + (k & 7); }

__device__ __forceinline__ float max3(float a, float b, float c) { return __builtin_fmaxf(__builtin_fmaxf(a, b), c); }
__device__ __forceinline__ float exp2_hw(float x) { return __builtin_amdgcn_exp2f(x); }      // v_exp_f32, x <= 0 here

struct SoftminArgs {
  const float *q, *t;          // queries [b,nq,3], targets [b,nt,3]
  const float *pot;            // the targets' potential [b,nt]; null = 0 everywhere
  const int *q_lengths, *t_lengths;
  int nq, nt;
  float k;                     // log2(e) / eps
  float c;                     // 1 / k (eps * ln 2 up to one rounding: c * k is 1 to half an ulp)
  int split;                   // S
  int qblocks;                 // workgroups per cloud
  float *out;                  // [b,nq] or null
  float *bary;                 // [b,nq,3] (WITH_BARY)
};

template <bool WITH_BARY>
__global__ __launch_bounds__(1024) void sinkhorn_softmin_kernel(SoftminArgs a) {
  extern __shared__ float4 lds[];
  const int b = blockIdx.x / a.qblocks;
  const int lanes = blockDim.x / a.split;      // G
  const int seg = threadIdx.x / lanes, gt = threadIdx.x - seg * lanes;
  const int len_t = sn::clamped_length(a.t_lengths, b, a.nt);
  const int len_q = sn::clamped_length(a.q_lengths, b, a.nq);
  const int q0 = (blockIdx.x - b * a.qblocks) * lanes;
  const int qi = q0 + gt;
  const size_t row = (size_t)b * a.nq + (qi < a.nq ? qi : 0);

  // a workgroup of padding queries, or a pair with an empty side: zeros (uniform over the workgroup)
  if (q0 >= len_q || len_t == 0) {
    if (seg == 0 && qi < a.nq) {
      if (a.out) a.out[row] = 0.f;
      if (WITH_BARY) a.bary[row * 3 + 0] = a.bary[row * 3 + 1] = a.bary[row * 3 + 2] = 0.f;
    }
    return;
  }

  const bool live = qi < len_q;
  float qx = 0.f, qy = 0.f, qz = 0.f;      // a padding query walks along at the origin; its row is never read
  if (live) {
    const float *q = a.q + row * 3;
    qx = q[0], qy = q[1], qz = q[2];
  }
  const int tile_n = a.split == 1 ? kWideTile : kSplitTile;
  const int seglen = sn::ceil_div(len_t, a.split);
  const int begin = seg * seglen < len_t ? seg * seglen : len_t;
  const int end = begin + seglen < len_t ? begin + seglen : len_t;
  const int ntiles = sn::ceil_div(seglen, tile_n);      // the same for every segment: the tile loop carries barriers
  float4 *tile = lds + seg * tile_n;                    // 8 float4 per 8 targets
  float *tilef = reinterpret_cast<float *>(tile);
  const float *cloud = a.t + (size_t)b * a.nt * 3;
  const float *pot = a.pot ? a.pot + (size_t)b * a.nt : nullptr;
  const float k = a.k;

  // Three levels of sums, so that no accumulator takes more than a tile's worth of additions: the 8 terms of a chunk
  // (a tree), the tile's chunks (ts, tb* at the running maximum m), the tiles (sum, b* at m0, the maximum at the last
  // tile's end).  One accumulator for all targets rounds thousands of near-equal terms the same way at a large eps.
  float m = kLowest, m0 = kLowest, sum = 0.f, bx = 0.f, by = 0.f, bz = 0.f;
  for (int t = 0; t < ntiles; ++t) {
    float ts = 0.f, tbx = 0.f, tby = 0.f, tbz = 0.f;
    const int base = begin + t * tile_n;
    const int count = end - base < tile_n ? (end - base < 0 ? 0 : end - base) : tile_n;
    const int padded = (count + 7) & ~7;                // whole chunks: the tail is (0, 0, 0, -inf)
    __syncthreads();      // the tile's last readers are through
    const float *src = cloud + (size_t)base * 3;
    for (int e = gt; e < 3 * padded; e += lanes) {
      const int j = e / 3;
      tilef[slot(j, e - 3 * j)] = j < count ? src[e] : 0.f;
    }
    for (int j = gt; j < padded; j += lanes)
      tilef[slot(j, 3)] = j < count ? (pot ? pot[base + j] * k : 0.f) : -__builtin_inff();
    __syncthreads();
    const int chunks = __builtin_amdgcn_readfirstlane(padded / 8);      // a segment is one wave, or the workgroup
    for (int c = 0; c < chunks; ++c) {
      const float4 xa = tile[c * 8 + 0], xb = tile[c * 8 + 1];
      const float4 ya = tile[c * 8 + 2], yb = tile[c * 8 + 3];
      const float4 za = tile[c * 8 + 4], zb = tile[c * 8 + 5];
      const float4 ha = tile[c * 8 + 6], hb = tile[c * 8 + 7];
      const float tx[8] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
      const float ty[8] = {ya.x, ya.y, ya.z, ya.w, yb.x, yb.y, yb.z, yb.w};
      const float tz[8] = {za.x, za.y, za.z, za.w, zb.x, zb.y, zb.z, zb.w};
      const float th[8] = {ha.x, ha.y, ha.z, ha.w, hb.x, hb.y, hb.z, hb.w};
      float s[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) s[u] = __builtin_fmaf(-dist1(tx[u], ty[u], tz[u], qx, qy, qz), k, th[u]);
      const float mn = max3(max3(s[0], s[1], s[2]), max3(s[3], s[4], s[5]), max3(s[6], s[7], m));
      const float scale = exp2_hw(m - mn);      // both finite
      float p[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) p[u] = exp2_hw(s[u] - mn);      // s <= mn, mn finite: -inf at a padding slot gives 0
      ts = __builtin_fmaf(ts, scale, ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7])));
      if (WITH_BARY) {
        float cx = p[0] * tx[0], cy = p[0] * ty[0], cz = p[0] * tz[0];
#pragma unroll
        for (int u = 1; u < 8; ++u) {
          cx = __builtin_fmaf(p[u], tx[u], cx);
          cy = __builtin_fmaf(p[u], ty[u], cy);
          cz = __builtin_fmaf(p[u], tz[u], cz);
        }
        tbx = __builtin_fmaf(tbx, scale, cx);
        tby = __builtin_fmaf(tby, scale, cy);
        tbz = __builtin_fmaf(tbz, scale, cz);
      }
      m = mn;
    }
    const float fold = exp2_hw(m0 - m);      // the tile into the totals, at the new maximum
    sum = __builtin_fmaf(sum, fold, ts);
    if (WITH_BARY) {
      bx = __builtin_fmaf(bx, fold, tbx);
      by = __builtin_fmaf(by, fold, tby);
      bz = __builtin_fmaf(bz, fold, tbz);
    }
    m0 = m;
  }

  if (a.split > 1) {
    // every segment leaves its record in LDS (lanes contiguous), segment 0 adds them in segment order
    float *rec = reinterpret_cast<float *>(lds);
    __syncthreads();      // the tiles are read
    rec[(seg * kFields + 0) * 64 + gt] = m;
    rec[(seg * kFields + 1) * 64 + gt] = sum;
    if (WITH_BARY) {
      rec[(seg * kFields + 2) * 64 + gt] = bx;
      rec[(seg * kFields + 3) * 64 + gt] = by;
      rec[(seg * kFields + 4) * 64 + gt] = bz;
    }
    __syncthreads();
    if (seg != 0) return;
    for (int w = 1; w < a.split; ++w) m = __builtin_fmaxf(m, rec[(w * kFields + 0) * 64 + gt]);
    sum = bx = by = bz = 0.f;
    for (int w = 0; w < a.split; ++w) {
      const float scale = exp2_hw(rec[(w * kFields + 0) * 64 + gt] - m);      // an empty segment: (lowest, 0)
      sum = __builtin_fmaf(rec[(w * kFields + 1) * 64 + gt], scale, sum);
      if (WITH_BARY) {
        bx = __builtin_fmaf(rec[(w * kFields + 2) * 64 + gt], scale, bx);
        by = __builtin_fmaf(rec[(w * kFields + 3) * 64 + gt], scale, by);
        bz = __builtin_fmaf(rec[(w * kFields + 4) * 64 + gt], scale, bz);
      }
    }
  }

  if (qi < a.nq) {
    // the term at the maximum is 1, so 1 / len_t <= sum / len_t <= 1: the hardware log2 needs no denormal care
    if (a.out) a.out[row] = live ? -a.c * (m + __builtin_amdgcn_logf(sum / (float)len_t)) : 0.f;
    if (WITH_BARY) {
      a.bary[row * 3 + 0] = live ? bx / sum : 0.f;
      a.bary[row * 3 + 1] = live ? by / sum : 0.f;
      a.bary[row * 3 + 2] = live ? bz / sum : 0.f;
    }
  }
}

// ---------------------------------------------------------------------------------------------------- dispatch
struct Side : sn::SplitLaunch {      // one half-iteration's launch shape
  size_t lds;
};

// nq queries against nt targets: S by the shared rule ("Sinkhorn transport", has the sweep)
int side_of(const char *what, int b, int nq, int nt, Side *s) {
  int split = 1;
  if (const int rc = sn::pick_split(SN_KNOB("SN_SINKHORN_SPLIT"), b, nq, nt, kMaxSplit, kWavesPerCu, kMinSegment, &split))
    return rc;
  if (const int rc = sn::split_launch(what, b, nq, split, s)) return rc;
  s->lds = (size_t)split * (split == 1 ? kWideTile : kSplitTile) * 16;
  return 0;
}

// out (and bary) of the queries q over the targets t with potential pot at eps
int softmin(const char *what, const Side &s, const float *q, const float *t, const float *pot, int nq, int nt,
            const int *q_lengths, const int *t_lengths, float eps, float *out, float *bary, hipStream_t stream) {
  const float k = (float)(1.4426950408889634 / (double)eps);
  const SoftminArgs a{q, t, pot, q_lengths, t_lengths, nq, nt, k, (float)(1.0 / (double)k), s.split, s.qblocks, out, bary};
  if (bary)
    sinkhorn_softmin_kernel<true><<<s.grid, s.threads, s.lds, stream>>>(a);
  else
    sinkhorn_softmin_kernel<false><<<s.grid, s.threads, s.lds, stream>>>(a);
  return sn::launch_status(what);
}

int check_shape(const char *what, int b, int n, int m) {
  SN_REQUIRE(b >= 1 && n >= 1 && m >= 1, "%s: need b,n,m >= 1 (got %d,%d,%d)", what, b, n, m);
  SN_REQUIRE(n <= kMaxPoints && m <= kMaxPoints, "%s: cloud too large", what);
  return 0;
}

bool positive_finite(float v) { return v > 0.f && v <= 3.4028234664e38f; }

}  // namespace

extern "C" size_t sn_sinkhorn_workspace_bytes(int b, int n, int m) {
  (void)b, (void)n, (void)m;
  return 0;      // the potentials are the caller's f and g: nothing else is kept
}

extern "C" int sn_sinkhorn_solve(const float *x, const float *y, int b, int n, int m, const int *x_lengths,
                                 const int *y_lengths, float eps, float eps_start, float decay, int iters,
                                 int warm_start, float *f, float *g, void *workspace, size_t workspace_bytes,
                                 void *stream) {
  SN_REQUIRE(x && y && f && g, "sn_sinkhorn_solve: null pointer");
  if (const int rc = check_shape("sn_sinkhorn_solve", b, n, m)) return rc;
  SN_REQUIRE(positive_finite(eps), "sn_sinkhorn_solve: eps must be finite and > 0");
  SN_REQUIRE(eps_start <= 3.4028234664e38f, "sn_sinkhorn_solve: eps_start must be finite (<= 0: constant eps)");
  SN_REQUIRE(decay > 0.f && decay < 1.f, "sn_sinkhorn_solve: need 0 < decay < 1");
  SN_REQUIRE(iters >= 1, "sn_sinkhorn_solve: need iters >= 1 (got %d)", iters);
  (void)workspace, (void)workspace_bytes;
  hipStream_t s = sn::as_stream(stream);
  Side fs, gs;
  if (const int rc = side_of("sn_sinkhorn_solve", b, n, m, &fs)) return rc;
  if (const int rc = side_of("sn_sinkhorn_solve", b, m, n, &gs)) return rc;
  for (int t = 0; t < iters; ++t) {
    double e = (double)eps;
    if (eps_start > 0.f) {
      const double annealed = (double)eps_start * std::pow((double)decay, t);
      e = annealed > e ? annealed : e;
    }
    const float et = (float)e;
    const float *g_in = t == 0 && !warm_start ? nullptr : g;      // g = 0 without a read
    if (const int rc = softmin("sn_sinkhorn_solve", fs, x, y, g_in, n, m, x_lengths, y_lengths, et, f, nullptr, s))
      return rc;
    if (const int rc = softmin("sn_sinkhorn_solve", gs, y, x, f, m, n, y_lengths, x_lengths, et, g, nullptr, s))
      return rc;
  }
  return 0;
}

extern "C" int sn_sinkhorn_barycenter(const float *q, const float *t, const float *t_potential, int b, int n, int m,
                                      const int *q_lengths, const int *t_lengths, float eps, float *bary,
                                      float *softmin_out, void *workspace, size_t workspace_bytes, void *stream) {
  SN_REQUIRE(q && t && t_potential && bary, "sn_sinkhorn_barycenter: null pointer");
  if (const int rc = check_shape("sn_sinkhorn_barycenter", b, n, m)) return rc;
  SN_REQUIRE(positive_finite(eps), "sn_sinkhorn_barycenter: eps must be finite and > 0");
  (void)workspace, (void)workspace_bytes;
  Side s;
  if (const int rc = side_of("sn_sinkhorn_barycenter", b, n, m, &s)) return rc;
  return softmin("sn_sinkhorn_barycenter", s, q, t, t_potential, n, m, q_lengths, t_lengths, eps, softmin_out, bary,
                 sn::as_stream(stream));
}
