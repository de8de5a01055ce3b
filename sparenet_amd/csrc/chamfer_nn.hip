// chamfer_nn.hip -- Chamfer forward as a spatially pruned nearest-neighbour search (gfx950).
//
// Same contract as chamfer.hip (reference cuda/chamfer_distance/chamfer_distance.cu:7-137,
// CPU statement chamfer_distance.cpp:57-112):
//   dist[b,j] = min_k d(j,k),  d = (dx*dx + dy*dy) + dz*dz, dx = t.x - q.x, separately rounded;
//   idx[b,j]  = LOWEST k attaining the minimum.
// chamfer.hip evaluates all n*m pairs (VALU bound, 2.7 ms at B=32, n=m=16384).  Here both
// clouds are put in Morton order (cloud_sort.hpp) and the search is filtered twice:
//   * superblock level: 64 consecutive sorted targets carry a bounding box; a wave serves 64
//     consecutive sorted QUERIES (spatial neighbours), keeps their bounding box and the largest
//     current best distance R2max, and skips every superblock whose box is farther than that.
//     The test runs for 64 superblocks at a time, lane = superblock.
//   * pair level, on the matrix cores: u = |t|^2 - 2 t.q for 16 targets x 16 queries is one
//     v_mfma_f32_16x16x4_f32 (exact fp32); a pair can only matter if u <= best_q - |q|^2 + slack
//     (formats and margins: pair_filter.hpp).
//   * survivors go to a per-wave LDS queue and are evaluated 64 at a time with the reference's
//     expression; the result meets the query through a 64-bit LDS atomicMin on
//     (bits of d) << 32 | k.  d >= 0, so its bit pattern orders like the value: the minimum key
//     is the minimum distance and, among equal distances, the lowest k -- the reference's rule,
//     independent of the visiting order.
// Every query starts from the best of 8 sorted targets around its own Morton cell, so the ball
// it still has to search is already ~1.5 nearest-neighbour distances wide.
#include "cloud_sort.hpp"
#include "common.hpp"
#include "pair_filter.hpp"

namespace {

using namespace sn::pf;  // f4, the operand stream and box rows, the margins, min16 / hits4 / queue_append

struct NnSide {       // one cloud in Morton order
  const float *xyz;   // [B, n, 3] as given
  int n, nsb;         // points, superblocks of 64
  int *perm;          // [B, n] sorted position -> index
  int *hist;          // [B, 4096] cell END offsets after the scatter
  float *bbox;        // [B, 6]
  f4 *sorted4;        // [B, nsb*64] {x, y, z, index bits}; padding: index -1
  f4 *mstream;        // [B, nsb, 64] MFMA A operand (pair_filter.hpp)
  float *sbbox;       // [B, nsb, 8] box rows (pair_filter.hpp)
};

// one wave per superblock: sorted coordinates, MFMA operand stream, bounding box
__global__ __launch_bounds__(256) void nn_prepare_kernel(int B, NnSide S) {
#pragma clang fp contract(off)
  const long sb_all = (long)B * S.nsb;
  const int lane = threadIdx.x & 63;
  for (long sb = (long)blockIdx.x * 4 + (threadIdx.x >> 6); sb < sb_all; sb += (long)gridDim.x * 4) {
    const long b = sb / S.nsb;
    const int p = (int)(sb - b * S.nsb) * 64 + lane;  // sorted position inside the cloud
    const bool valid = p < S.n;
    const int k = valid ? S.perm[b * S.n + p] : -1;
    const float *t = S.xyz + (b * S.n + (valid ? k : 0)) * 3;
    const float x = valid ? t[0] : 0.f, y = valid ? t[1] : 0.f, z = valid ? t[2] : 0.f;
    S.sorted4[sb * 64 + lane] = f4{x, y, z, __int_as_float(k)};
    store_operand(S.mstream + sb * 64, lane, x, y, z, valid ? norm2(x, y, z) : kFar);  // padding never passes
    float lo[3] = {valid ? x : kFar, valid ? y : kFar, valid ? z : kFar};
    float hi[3] = {valid ? x : -kFar, valid ? y : -kFar, valid ? z : -kFar};
    sn::wave_minmax3(lo, hi);
    store_box_row(S.sbbox, sb, lane, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
  }
}

constexpr int kQueue = 128;

struct NnTab {  // per-wave LDS
  float x[64], y[64], z[64];
  unsigned long long key[64];  // (bits of the best d) << 32 | its lowest k
  unsigned queue[kQueue];      // sorted target position | query lane << 26
};

__global__ __launch_bounds__(256) void nn_search_kernel(int B, NnSide S1, NnSide S2,
                                                        float *__restrict__ dist1,
                                                        int *__restrict__ idx1,
                                                        float *__restrict__ dist2,
                                                        int *__restrict__ idx2, int bpc) {
  __shared__ NnTab tabs[4];
  // XCD-aware: the 2B (direction, cloud) searches are dealt to the XCDs, all workgroups of one
  // search share block id % 8 so that its target streams stay in one L2
  const int lin = blockIdx.x, xcd = lin & 7, rr = lin >> 3;
  const int cidx = (rr / bpc) * 8 + xcd;
  if (cidx >= 2 * B) return;
  const int dir = cidx / B, b = cidx - dir * B;
  const NnSide Q = dir == 0 ? S1 : S2;  // queries
  const NnSide T = dir == 0 ? S2 : S1;  // targets
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int grp = (rr % bpc) * 4 + wave;  // group of 64 sorted queries
  if (grp >= Q.nsb) return;               // whole wave; no workgroup barrier below
  const int row = lane >> 4, col = lane & 15;
  NnTab &W = tabs[wave];
  const f4 *__restrict__ t4 = T.sorted4 + (size_t)b * T.nsb * 64;

  // ---- this wave's queries, their seeds -------------------------------------------------
  const f4 q = Q.sorted4[((size_t)b * Q.nsb + grp) * 64 + lane];
  const int qk = __float_as_int(q.w);
  const bool active = qk >= 0;
  unsigned long long key = ~0ull;
  if (active) {
    int lo = sort_cell_start(T.hist + b * kSortCells, q.x, q.y, q.z, T.bbox + b * 6) - 2;
    lo = lo < 0 ? 0 : (lo > T.n - 8 ? T.n - 8 : lo);
    lo = lo < 0 ? 0 : lo;
    const int cnt = T.n < 8 ? T.n : 8;
    for (int p = lo; p < lo + cnt; ++p) {
      const f4 t = t4[p];
      const float d = sq_dist(t.x, t.y, t.z, q.x, q.y, q.z);
      const unsigned long long kk = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)__float_as_int(t.w);
      key = kk < key ? kk : key;
    }
  }
  W.x[lane] = q.x;
  W.y[lane] = q.y;
  W.z[lane] = q.z;
  W.key[lane] = key;
  float qlo[3] = {active ? q.x : kFar, active ? q.y : kFar, active ? q.z : kFar};
  float qhi[3] = {active ? q.x : -kFar, active ? q.y : -kFar, active ? q.z : -kFar};
  sn::wave_minmax3(qlo, qhi);
  const float tmax = far_corner2(T.bbox + b * 6);

  // the four queries this lane filters for (column col of query group g), MFMA B operand
  float thr[4], base[4], bop[4];
  bool live[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
#pragma clang fp contract(off)
    const int c = 16 * g + col;
    const float x = W.x[c], y = W.y[c], z = W.z[c];
    const float xx = norm2(x, y, z);
    base[g] = kSlack18 * (tmax + xx) - xx;
    live[g] = W.key[c] != ~0ull;
    bop[g] = row == 0 ? x : (row == 1 ? y : (row == 2 ? z : 1.0f));
  }
  float r2max = 0.f;  // wave-uniform: largest current best of the wave's queries
  auto refresh = [&]() {
    const float mine = active ? __uint_as_float((unsigned)(W.key[lane] >> 32)) : 0.f;
    float m = mine;
    for (int s = 1; s < 64; s <<= 1) m = __builtin_fmaxf(m, __shfl_xor(m, s));
    r2max = m;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float best = __uint_as_float((unsigned)(W.key[16 * g + col] >> 32));
      thr[g] = live[g] ? __builtin_fmaf(best, kUp20, base[g]) : -kFar;
    }
  };
  refresh();

  int qcount = 0;  // wave-uniform
  auto batch = [&](int first, int count) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane < count) {
      const unsigned e = W.queue[first + lane];
      const int c = (int)(e >> 26);
      const f4 t = t4[e & 0x3ffffffu];
      const float d = sq_dist(t.x, t.y, t.z, W.x[c], W.y[c], W.z[c]);
      atomicMin(&W.key[c], ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)__float_as_int(t.w));
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  };

  const f4 *__restrict__ ms = T.mstream + (size_t)b * T.nsb * 64;
  const float *__restrict__ sbb = T.sbbox + (size_t)b * T.nsb * 8;
  for (int sb0 = 0; sb0 < T.nsb; sb0 += 64) {
    // which of these 64 superblocks can hold a pair that still matters? (lane = superblock)
    const int sbl = sb0 + lane;
    bool visit = false;
    if (sbl < T.nsb) {
      const f4 lo4 = *reinterpret_cast<const f4 *>(sbb + (size_t)sbl * 8);
      const f4 hi4 = *reinterpret_cast<const f4 *>(sbb + (size_t)sbl * 8 + 4);
      visit = box_gap2(lo4, hi4, qlo, qhi) <= r2max;
    }
    unsigned long long todo = __ballot(visit);
    while (todo) {
      const int sb = sb0 + __builtin_ctzll(todo);
      todo &= todo - 1;
      const f4 a = ms[(size_t)sb * 64 + lane];
      bool drained = false;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f4 zero = {0.f, 0.f, 0.f, 0.f};
        const f4 d0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, bop[g], zero, 0, 0, 0);
        const f4 d1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, bop[g], zero, 0, 0, 0);
        const f4 d2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, bop[g], zero, 0, 0, 0);
        const f4 d3 = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, bop[g], zero, 0, 0, 0);
        if (__builtin_expect(__any(min16(d0, d1, d2, d3) <= thr[g]), 0)) {
          unsigned hm = hits4(d0, thr[g], 0) | hits4(d1, thr[g], 4) | hits4(d2, thr[g], 8) |
                        hits4(d3, thr[g], 12);
          while (__any(hm != 0)) {
            qcount = queue_append(W.queue, qcount, hm, [=](int i) {
              return (unsigned)hit_position(sb * 64, i, row) | ((unsigned)(16 * g + col) << 26);
            });
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            while (qcount >= 64) {
              qcount -= 64;
              batch(qcount, 64);
              drained = true;
            }
          }
        }
      }
      if (drained) {  // tighter bests: fewer superblocks of this chunk remain worth a visit
        refresh();
        if (todo) {
          bool still = false;
          if (sbl < T.nsb && ((todo >> lane) & 1ull)) {
            const f4 lo4 = *reinterpret_cast<const f4 *>(sbb + (size_t)sbl * 8);
            const f4 hi4 = *reinterpret_cast<const f4 *>(sbb + (size_t)sbl * 8 + 4);
            still = box_gap2(lo4, hi4, qlo, qhi) <= r2max;
          }
          todo = __ballot(still);
        }
      }
    }
    if (qcount > 0) {  // keep the bests current between chunks
      batch(0, qcount);
      qcount = 0;
      refresh();
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if (active) {
    const unsigned long long kf = W.key[lane];
    float *dist = dir == 0 ? dist1 : dist2;
    int *idx = dir == 0 ? idx1 : idx2;
    dist[(size_t)b * Q.n + qk] = __uint_as_float((unsigned)(kf >> 32));
    idx[(size_t)b * Q.n + qk] = (int)(unsigned)kf;
  }
}

// the workspace: both sides' arrays, then the two sort-scratch arrays
NnSide side_layout(sn::Carver &c, int b, int n) {
  NnSide s;
  s.xyz = nullptr;  // the entry point's
  s.n = n;
  s.nsb = sn::ceil_div(n, 64);
  s.perm = c.take256<int>((size_t)b * n * 4);
  s.hist = c.take<int>((size_t)b * kSortCells * 4);
  s.bbox = c.take256<float>((size_t)b * 24);
  s.sorted4 = c.take<f4>((size_t)b * s.nsb * 64 * 16);
  s.mstream = c.take<f4>((size_t)b * s.nsb * 64 * 16);
  s.sbbox = c.take<float>((size_t)b * s.nsb * 32);
  return s;
}
struct NnWs {
  NnSide s1, s2;
  int *cell_of, *cell_of2;  // sort scratch of cloud 1 and of cloud 2
};
NnWs nn_layout(sn::Carver &c, int b, int n, int m) {
  const size_t scratch = (size_t)b * (n > m ? n : m) * 4;
  return {side_layout(c, b, n), side_layout(c, b, m), c.take256<int>(scratch), c.take256<int>(scratch)};
}

}  // namespace

extern "C" size_t sn_chamfer_workspace_bytes(int b, int n, int m) {
  if (b < 1 || n < 1 || m < 1) return 0;
  return sn::layout_bytes(nn_layout, b, n, m);
}

extern "C" int sn_chamfer_forward_sorted(const float *xyz1, const float *xyz2, int b, int n, int m,
                                         float *dist1, int *idx1, float *dist2, int *idx2,
                                         void *workspace, size_t workspace_bytes, void *stream) {
  SN_REQUIRE(xyz1 && xyz2 && dist1 && idx1 && dist2 && idx2 && workspace,
             "sn_chamfer_forward_sorted: null pointer");
  SN_REQUIRE(b >= 1 && n >= 1 && m >= 1, "sn_chamfer_forward_sorted: need b,n,m >= 1 (got %d,%d,%d)", b, n, m);
  SN_REQUIRE((long)b * n < (1L << 26) && (long)b * m < (1L << 26) && n < (1 << 26) && m < (1 << 26),
             "sn_chamfer_forward_sorted: too large");
  sn::Carver carver(workspace);
  const NnWs w = nn_layout(carver, b, n, m);
  SN_REQUIRE(workspace_bytes >= carver.bytes(), "sn_chamfer_forward_sorted: workspace too small (%zu < %zu)",
             workspace_bytes, carver.bytes());
  hipStream_t s = sn::as_stream(stream);
  SN_REFUSE_CAPTURE(s, "sn_chamfer_forward_sorted");
  NnSide s1 = w.s1, s2 = w.s2;
  s1.xyz = xyz1;
  s2.xyz = xyz2;
  if (sn::prof_enabled()) sn::prof_begin("chamfer_fwd", s);
  SN_REQUIRE(cloud_sort_pair(b, SortSide{s1.n, s1.xyz, s1.bbox, s1.hist, w.cell_of, s1.perm},
                             SortSide{s2.n, s2.xyz, s2.bbox, s2.hist, w.cell_of2, s2.perm}, s) == 0,
             "sn_chamfer_forward_sorted: cannot size the sort kernel's LDS");
  for (NnSide *side : {&s1, &s2}) {
    const long sbs = (long)b * side->nsb;
    nn_prepare_kernel<<<(int)((sbs + 3) / 4 < 4096 ? (sbs + 3) / 4 : 4096), 256, 0, s>>>(b, *side);
  }
  const int bpc = sn::ceil_div((s1.nsb > s2.nsb ? s1.nsb : s2.nsb), 4);  // workgroups per search
  const int grid = 8 * sn::ceil_div(2 * b, 8) * bpc;
  // (its own bracket inside the call's: bench.py prices the search kernel's counters against ITS time)
  SN_TIMED("nn_search", s, (nn_search_kernel<<<grid, 256, 0, s>>>(b, s1, s2, dist1, idx1, dist2, idx2, bpc)));
  if (sn::prof_enabled()) sn::prof_end("chamfer_fwd", s);
  return sn::launch_status("sn_chamfer_forward_sorted");
}
