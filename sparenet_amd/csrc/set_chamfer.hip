// set_chamfer.hip -- one direction of the Chamfer distance between every cloud of one set and every cloud of another
// (sn_set_chamfer_sums, include/sparenet_hip_ext.h): sums[i,j] = sum_q min_t d(x_i[q], y_j[t]) in float64.  MMD-CD,
// COV-CD and 1-NNA-CD (sparenet_amd/utils/set_metrics.py) are read off two such matrices.
//
// The training kernel (chamfer.hip) would serve a pair of clouds per batch entry and write a distance and an index
// per point; a set metric needs one number per PAIR OF CLOUDS.  So, with the same arithmetic (chamfer_tile.hpp):
//   * a workgroup keeps 2048 queries of one x cloud in VGPRs (8 per lane, packed two by two: the distance chain
//     issues as v_pk_add_f32 / v_pk_mul_f32) and walks a STRIP of consecutive y clouds.  Clouds of at most 1024
//     points take the instantiation with 4 queries per lane: in the wide one half the query slots would be padding,
//     computed and thrown away (measured: 8.6 ms against 4.7 for two sets of 128 clouds of 1024 points);
//   * the y clouds stream through the chunk-SoA LDS tile, tile after tile across cloud boundaries, the next tile's
//     global loads issued before the current tile is consumed;
//   * per chunk of 8 targets only the min3 tree into the running minimum: no chunk index, no epilogue search, no
//     per-point output;
//   * after each y cloud the 2048 minima are widened to double and added lane -> wave -> workgroup, padding queries
//     as 0.0, and ONE double is written.
// Order of the additions: per lane its queries tid + 256 i, i ascending; sn::block_sum_f64 (a 64-lane xor butterfly,
// then the four wave sums ascending); for n > 2048 the query blocks' partial sums (in the workspace) ascending, by a
// second small kernel.  All of it, the choice of the instantiation included, is a function of n alone -- not of nx, ny, m, the strip length or the grid -- which is
// what makes a matrix entry bit-equal to the 1 x 1 call on its pair.  A minimum over fp32 values has no order.
//
// Plain stream-ordered launches: no workgroup waits for another, every loop is bounded by a shape, no floating-point
// atomics.  Blocks that walk the same strip share their blockIdx % 8 (one XCD's L2 serves the strip): an affinity
// hint, nothing depends on it.
#include "block_scan.hpp"
#include "chamfer_tile.hpp"
#include "common.hpp"
#include "../../include/sparenet_hip_ext.h"

namespace {

using sn::ct::dist2;
using sn::ct::f2;
using sn::ct::kChunk;
using sn::ct::kThreads;
using sn::ct::kTile;
using sn::ct::kTileF4;
using sn::ct::min3;

constexpr int kWideQPL = 8;              // queries per lane: 2048 per block, a whole evaluation cloud
constexpr int kNarrowQPL = 4;            // ... for clouds of at most kNarrowPoints points
constexpr int kNarrowPoints = kThreads * kNarrowQPL;
constexpr int kMaxPoints = 1 << 20;      // per cloud
// Strip length.  A block's queries are loaded once per strip (24 KB against 24 KB per target cloud), so a few clouds
// amortise them; beyond that a longer strip only makes the grid coarser.  Small problems take shorter strips so that
// the grid still has kFillBlocks blocks (256 CUs, 3 resident blocks each at 140 VGPRs, between 2 and 3 rounds) where
// the work allows it.
constexpr int kStrip = 8;
constexpr int kFillBlocks = 2048;
constexpr long kMaxGrid = 1L << 24;      // workgroups per launch: grid x 256 threads stays below 2^32

int queries_per_lane(int n) { return n <= kNarrowPoints ? kNarrowQPL : kWideQPL; }
int query_blocks(int n) { return sn::ceil_div(n, kThreads * queries_per_lane(n)); }

int strip_length(long units) {  // units = (x clouds) x (query blocks per cloud) x (y clouds)
  const long s = units / kFillBlocks;
  return (int)(s < 1 ? 1 : (s > kStrip ? kStrip : s));
}

// out[(i ny + j) nqb + qb]: the sums themselves for nqb == 1, the partial sums of the query blocks otherwise
template <int kQPL>
__global__ __launch_bounds__(kThreads) void set_chamfer_kernel(const float *__restrict__ x,
                                                               const float *__restrict__ y, int n, int ny, int m,
                                                               int nqb, int nxq, int strip, int nstrips,
                                                               double *__restrict__ out) {
  constexpr int kQPB = kThreads * kQPL;  // queries per block
  __shared__ float4 tile[kTileF4];
  __shared__ double wsum[kThreads / sn::kWave];

  // block g: strip (g / 8 / nxq) * 8 + g % 8, so the nxq blocks of a strip share g % 8
  const int g = blockIdx.x;
  const int s = ((g >> 3) / nxq) * 8 + (g & 7);
  if (s >= nstrips) return;
  const int xq = (g >> 3) % nxq;
  const int i = xq / nqb, qb = xq - i * nqb;
  const int j0 = s * strip;
  const int j1 = j0 + strip < ny ? j0 + strip : ny;

  const int tid = threadIdx.x;
  const float *__restrict__ q = x + (size_t)i * n * 3;
  const int q0 = qb * kQPB + tid;
  f2 qx[kQPL / 2], qy[kQPL / 2], qz[kQPL / 2];
#pragma unroll
  for (int u = 0; u < kQPL; ++u) {
    int k = q0 + u * kThreads;
    k = k < n ? k : n - 1;  // a padding query repeats the last point; its minimum is not added
    qx[u >> 1][u & 1] = q[k * 3 + 0];
    qy[u >> 1][u & 1] = q[k * 3 + 1];
    qz[u >> 1][u & 1] = q[k * 3 + 2];
  }

  const int ntiles = sn::ceil_div(m, kTile);
  constexpr int kLd = kTile * 3 / kThreads;  // floats per thread per tile (12)
  float stage[kLd];
  const int m3 = m * 3;

  auto load_stage = [&](int cloud, int tile_id) {
    const float *__restrict__ t = y + (size_t)cloud * m3;
    const int base = tile_id * kTile * 3;
#pragma unroll
    for (int u = 0; u < kLd; ++u) {
      const int e = base + u * kThreads + tid;
      stage[u] = e < m3 ? t[e] : __builtin_inff();
    }
  };
  auto store_stage = [&]() {
    float *lds = reinterpret_cast<float *>(tile);
#pragma unroll
    for (int u = 0; u < kLd; ++u) {
      const int e = u * kThreads + tid;
      const int k = e / 3, comp = e - k * 3;
      lds[sn::ct::tile_slot(k, comp)] = stage[u];
    }
  };

  load_stage(j0, 0);
  for (int j = j0; j < j1; ++j) {
    float best[kQPL];
#pragma unroll
    for (int u = 0; u < kQPL; ++u) best[u] = __builtin_inff();

    for (int tile_id = 0; tile_id < ntiles; ++tile_id) {
      __syncthreads();  // previous tile fully consumed
      store_stage();
      __syncthreads();
      if (tile_id + 1 < ntiles) {
        load_stage(j, tile_id + 1);
      } else if (j + 1 < j1) {
        load_stage(j + 1, 0);
      }

      const int rem = m - tile_id * kTile;
      const int nchunks = rem >= kTile ? kTile / kChunk : sn::ceil_div(rem, kChunk);
#pragma unroll 2
      for (int c = 0; c < nchunks; ++c) {
        const float4 xa = tile[c * 6 + 0], xb = tile[c * 6 + 1];
        const float4 ya = tile[c * 6 + 2], yb = tile[c * 6 + 3];
        const float4 za = tile[c * 6 + 4], zb = tile[c * 6 + 5];
        const float tx[8] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
        const float ty[8] = {ya.x, ya.y, ya.z, ya.w, yb.x, yb.y, yb.z, yb.w};
        const float tz[8] = {za.x, za.y, za.z, za.w, zb.x, zb.y, zb.z, zb.w};
#pragma unroll
        for (int p = 0; p < kQPL / 2; ++p) {
          f2 d[8];
#pragma unroll
          for (int k = 0; k < 8; ++k) d[k] = dist2(tx[k], ty[k], tz[k], qx[p], qy[p], qz[p]);
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            float v = min3(d[0][h], d[1][h], d[2][h]);
            v = min3(v, d[3][h], d[4][h]);
            v = min3(v, d[5][h], d[6][h]);
            best[p * 2 + h] = min3(best[p * 2 + h], v, d[7][h]);
          }
        }
      }
    }

    // the cloud's minima, in double: lane, wave, workgroup -- a fixed order (see the top of the file)
    double acc = 0.0;
#pragma unroll
    for (int u = 0; u < kQPL; ++u) acc += q0 + u * kThreads < n ? (double)best[u] : 0.0;
    // wsum is written again only behind the next cloud's tile barriers, which thread 0 reaches after its reads
    acc = sn::block_sum_f64<kThreads>(acc, wsum);
    if (tid == 0) out[((size_t)i * ny + j) * nqb + qb] = acc;
  }
}

// sums[e] = the nqb partial sums of pair e, ascending
__global__ __launch_bounds__(256) void set_chamfer_add_kernel(const double *__restrict__ partials, long pairs, int nqb,
                                                              double *__restrict__ sums) {
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < pairs; e += (long)gridDim.x * blockDim.x) {
    double acc = partials[e * nqb];
    for (int b = 1; b < nqb; ++b) acc += partials[e * nqb + b];
    sums[e] = acc;
  }
}

struct SetChamferWs {
  double *partials;  // [nx, ny, query blocks] for clouds of more than one query block, else nothing
};
SetChamferWs set_chamfer_layout(sn::Carver &c, int nx, int ny, int n) {
  const int nqb = query_blocks(n);
  SetChamferWs L;
  L.partials = c.take256<double>(nqb > 1 ? (size_t)nx * ny * nqb * sizeof(double) : 0);
  return L;
}

bool set_chamfer_sizes_ok(int nx, int ny, int n) {
  return nx >= 1 && ny >= 1 && n >= 1 && n <= kMaxPoints && (long)nx * ny <= 0x7fffffffL;
}

}  // namespace

extern "C" size_t sn_set_chamfer_workspace_bytes(int nx, int ny, int n) {
  if (!set_chamfer_sizes_ok(nx, ny, n)) return 0;
  return sn::layout_bytes(set_chamfer_layout, nx, ny, n);
}

extern "C" int sn_set_chamfer_sums(const float *x, const float *y, int nx, int n, int ny, int m, double *sums,
                                   void *workspace, size_t workspace_bytes, void *stream) {
  SN_REQUIRE(x && y && sums, "sn_set_chamfer_sums: null pointer");
  SN_REQUIRE(nx >= 1 && ny >= 1 && n >= 1 && m >= 1, "sn_set_chamfer_sums: need nx,n,ny,m >= 1 (got %d,%d,%d,%d)", nx,
             n, ny, m);
  SN_REQUIRE(n <= kMaxPoints && m <= kMaxPoints, "sn_set_chamfer_sums: at most %d points per cloud (got %d, %d)",
             kMaxPoints, n, m);
  SN_REQUIRE(set_chamfer_sizes_ok(nx, ny, n), "sn_set_chamfer_sums: nx * ny must not exceed 2^31 - 1 (got %d x %d)",
             nx, ny);
  sn::Carver carver(workspace);
  const SetChamferWs L = set_chamfer_layout(carver, nx, ny, n);
  SN_REQUIRE(workspace_bytes >= carver.bytes() && (workspace || carver.bytes() == 0),
             "sn_set_chamfer_sums: workspace too small (%zu < %zu)", workspace ? workspace_bytes : (size_t)0,
             carver.bytes());
  const int nqb = query_blocks(n);
  const long nxq = (long)nx * nqb;
  const int strip = strip_length(nxq * ny);
  const int nstrips = sn::ceil_div(ny, strip);
  const long grid = 8L * sn::ceil_div(nstrips, 8) * nxq;
  SN_REQUIRE(grid <= kMaxGrid, "sn_set_chamfer_sums: too large (%ld workgroups, at most %ld)", grid, kMaxGrid);
  hipStream_t s = sn::as_stream(stream);
  double *out = nqb > 1 ? L.partials : sums;
  if (queries_per_lane(n) == kNarrowQPL) {
    SN_TIMED("set_chamfer", s, (set_chamfer_kernel<kNarrowQPL><<<(unsigned)grid, kThreads, 0, s>>>(
        x, y, n, ny, m, nqb, (int)nxq, strip, nstrips, out)));
  } else {
    SN_TIMED("set_chamfer", s, (set_chamfer_kernel<kWideQPL><<<(unsigned)grid, kThreads, 0, s>>>(
        x, y, n, ny, m, nqb, (int)nxq, strip, nstrips, out)));
  }
  if (nqb > 1) {
    const long pairs = (long)nx * ny;
    set_chamfer_add_kernel<<<sn::grid_blocks(pairs, 2048), 256, 0, s>>>(L.partials, pairs, nqb, sums);
  }
  return sn::launch_status("sn_set_chamfer_sums");
}
