// neighbors.hip -- k nearest neighbours and ball query between two clouds, grouping, weighted interpolation and the
// backward of both (include/ops/neighbors.h states the rules).
//
// The searches.  A query lives in the registers of one lane; the targets stream through an LDS tile in the chunked SoA
// layout of chamfer_tile.hpp, read with wave-uniform 16-byte loads (a broadcast, conflict free).  A workgroup is S
// groups of G lanes: group g searches segment g of the S contiguous segments of the cloud, for the workgroup's G
// queries, through a tile of its own.
//   S == 1: G = 256 queries per workgroup, one tile of 1024 targets (the wide path);
//   S >= 2: G = 64, one wave per segment, tiles of 256 targets, then the segments' results are merged in LDS.
// k-NN: each lane keeps a sorted list of KB (distance bits, index) pairs in registers -- KB is k rounded up to a
// bucket, every access compile-time indexed -- and inserts only when a distance beats the list's worst.  Distances are
// >= +0, so their bit patterns order as their values and 0xffffffff marks an empty slot that +inf still beats.
// Targets arrive in ascending index order, in the scan and in the merge (a wave merges the list of a HIGHER segment into
// its own), so "strictly smaller than the entry" is the lexicographic (d, j) order of the rule on every path.
// Ball query: a lane writes its hits straight to idx as it finds them and stops once it has nsample; a wave skips a
// tile when all its lanes have, the workgroup leaves the loop when every wave has.  With S >= 2 a first pass counts
// each segment's hits (held to nsample), the counts are exchanged through LDS, and a second pass writes each
// segment's share at its offset: the concatenation in segment order, cut at nsample.
// No workgroup waits for another, no atomics, no [b,m,n] intermediate.
//
// The backward inverts the slot lists once per call (index_lists.hpp: integer atomics only, shared by all channels and
// by grouping and interpolation), then one thread per (b, channel, target) adds its list.
#include "chamfer_tile.hpp"
#include "common.hpp"
#include "index_lists.hpp"
#include "split_launch.hpp"
#include "../../include/ops/neighbors.h"

namespace {

using sn::ct::dist1;
using sn::ct::tile_slot;

constexpr int kMaxK = 32;
constexpr int kWideTile = sn::ct::kTile;   // targets per tile, S == 1
constexpr int kSplitTile = 256;            // targets per segment tile, S >= 2
constexpr int kMaxSplit = 16;              // waves of a 1024-thread workgroup
constexpr int kWavesPerCu = 16;            // what the dispatch fills the device to before it stops splitting
constexpr int kMinSegment = 128;           // ... and the shortest segment it splits down to
constexpr unsigned kEmpty = 0xffffffffu;   // above the bits of every distance, +inf included
constexpr int kMaxBlocks = 65535;          // cap of the grid-stride launches
constexpr int kMaxPoints = 1 << 30;

static_assert(kWideTile % sn::ct::kChunk == 0 && kSplitTile % sn::ct::kChunk == 0 && sn::ct::kChunk == 8, "tile chunks");

struct SearchArgs {
  const float *xyz, *new_xyz;
  const int *lengths, *new_lengths;
  int n, m;
  int split;     // S
  int qblocks;   // workgroups per cloud
};

// where a thread stands: its cloud, its segment of the targets, its query
struct Place {
  int b, seg, gt, lanes;      // cloud, segment, lane inside the segment's group, lanes of a group (G)
  int len, qi;                // the cloud's length; the query's row (may be >= m)
  bool live;                  // the query is one of the cloud's (qi < len_q)
  int tile, begin, end, ntiles;
  const float *cloud;
  float qx, qy, qz;
};

__device__ __forceinline__ Place place_of(const SearchArgs &a) {
  Place p;
  p.b = blockIdx.x / a.qblocks;
  p.lanes = blockDim.x / a.split;
  p.seg = threadIdx.x / p.lanes;
  p.gt = threadIdx.x - p.seg * p.lanes;
  p.len = sn::clamped_length(a.lengths, p.b, a.n);
  p.qi = (blockIdx.x - p.b * a.qblocks) * p.lanes + p.gt;
  p.live = p.qi < sn::clamped_length(a.new_lengths, p.b, a.m);
  p.tile = a.split == 1 ? kWideTile : kSplitTile;
  const int seglen = sn::ceil_div(p.len, a.split);
  p.begin = p.seg * seglen < p.len ? p.seg * seglen : p.len;
  p.end = p.begin + seglen < p.len ? p.begin + seglen : p.len;
  p.ntiles = sn::ceil_div(seglen, p.tile);      // the same for every segment: the tile loops carry barriers
  p.cloud = a.xyz + (size_t)p.b * a.n * 3;
  p.qx = p.qy = p.qz = 0.f;
  if (p.qi < a.m) {
    const float *q = a.new_xyz + ((size_t)p.b * a.m + p.qi) * 3;
    p.qx = q[0], p.qy = q[1], p.qz = q[2];
  }
  return p;
}

// targets [base, base + count) of the cloud into the group's tile
__device__ __forceinline__ void load_tile(float *tile, const Place &p, int base, int count) {
  const float *src = p.cloud + (size_t)base * 3;
  for (int e = p.gt; e < 3 * count; e += p.lanes) {
    const int k = e / 3;
    tile[tile_slot(k, e - 3 * k)] = src[e];
  }
}

// visit(d, j) for the tile's targets in ascending j
template <class Visit>
__device__ __forceinline__ void scan_tile(const float4 *tile, const Place &p, int base, int count, Visit &&visit) {
  const int chunks = sn::ceil_div(count, 8);
  for (int c = 0; c < chunks; ++c) {
    const float4 xa = tile[c * 6 + 0], xb = tile[c * 6 + 1];
    const float4 ya = tile[c * 6 + 2], yb = tile[c * 6 + 3];
    const float4 za = tile[c * 6 + 4], zb = tile[c * 6 + 5];
    const float tx[8] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
    const float ty[8] = {ya.x, ya.y, ya.z, ya.w, yb.x, yb.y, yb.z, yb.w};
    const float tz[8] = {za.x, za.y, za.z, za.w, zb.x, zb.y, zb.z, zb.w};
    const int left = count - c * 8;      // wave-uniform: the tail of the last chunk holds no targets
    if (left >= 8) {
#pragma unroll
      for (int u = 0; u < 8; ++u) visit(dist1(tx[u], ty[u], tz[u], p.qx, p.qy, p.qz), base + c * 8 + u);
    } else {
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (u < left) visit(dist1(tx[u], ty[u], tz[u], p.qx, p.qy, p.qz), base + c * 8 + u);
    }
  }
}

// ------------------------------------------------------------------------------------------------------- k-NN
// (u, j) into the ascending list, behind every entry that is not larger: the caller has checked u < U[KB - 1]
template <int KB>
__device__ __forceinline__ void insert(unsigned (&U)[KB], int (&J)[KB], unsigned u, int j) {
#pragma unroll
  for (int i = KB - 1; i >= 1; --i) {
    const bool shift = u < U[i - 1], here = u < U[i];
    U[i] = shift ? U[i - 1] : (here ? u : U[i]);
    J[i] = shift ? J[i - 1] : (here ? j : J[i]);
  }
  const bool first = u < U[0];
  U[0] = first ? u : U[0];
  J[0] = first ? j : J[0];
}

template <int KB, int kMaxThreads>
__global__ __launch_bounds__(kMaxThreads) void knn_query_kernel(SearchArgs a, int k, int *__restrict__ idx,
                                                                 float *__restrict__ dist2) {
  extern __shared__ float4 lds[];
  const Place p = place_of(a);
  float4 *tile = lds + p.seg * (p.tile / 8 * 6);
  unsigned U[KB];
  int J[KB];
#pragma unroll
  for (int i = 0; i < KB; ++i) U[i] = kEmpty, J[i] = -1;

  for (int t = 0; t < p.ntiles; ++t) {
    const int base = p.begin + t * p.tile;
    const int count = p.end - base < p.tile ? (p.end - base < 0 ? 0 : p.end - base) : p.tile;
    __syncthreads();      // the tile's last readers are through
    load_tile(reinterpret_cast<float *>(tile), p, base, count);
    __syncthreads();
    scan_tile(tile, p, base, count, [&](float d, int j) {
      const unsigned u = __float_as_uint(d);
      if (u < U[KB - 1]) insert<KB>(U, J, u, j);
    });
  }

  // merge tree over the segments: in the round of `stride`, segment w + stride hands its list to segment w
  if (a.split > 1) {
    const int lane = p.gt;
    unsigned *mu = reinterpret_cast<unsigned *>(lds);
    int *mj = reinterpret_cast<int *>(lds) + (a.split + 1) / 2 * KB * 64;
    for (int stride = 1; stride < a.split; stride *= 2) {
      const int slot = p.seg / (2 * stride), role = p.seg % (2 * stride);
      __syncthreads();      // the tiles, or the last round's lists, are read
      if (role == stride) {
#pragma unroll
        for (int i = 0; i < KB; ++i) mu[(slot * KB + i) * 64 + lane] = U[i], mj[(slot * KB + i) * 64 + lane] = J[i];
      }
      __syncthreads();
      if (role == 0 && p.seg + stride < a.split) {
#pragma unroll
        for (int i = 0; i < KB; ++i) {
          const unsigned u = mu[(slot * KB + i) * 64 + lane];
          const bool better = u < U[KB - 1];
          if (!__any(better)) break;      // the incoming list ascends: nothing later enters either
          if (better) insert<KB>(U, J, u, mj[(slot * KB + i) * 64 + lane]);
        }
      }
    }
  }

  if (p.seg == 0 && p.qi < a.m) {
    const size_t row = ((size_t)p.b * a.m + p.qi) * k;
#pragma unroll
    for (int i = 0; i < KB; ++i) {
      if (i < k) {
        const bool has = p.live && U[i] != kEmpty;
        idx[row + i] = has ? J[i] : -1;
        if (dist2) dist2[row + i] = has ? __uint_as_float(U[i]) : __builtin_inff();
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------- ball query
// One pass over the lane's segment: the hits in ascending j until the lane has `limit` of them, written to row[0 ..]
// when row is not null.  Every thread of the workgroup calls it (barriers inside).
__device__ __forceinline__ void ball_pass(float4 *tile, const Place &p, float r2, int limit, int *row, int &hits,
                                          int &first) {
  hits = 0, first = -1;
  for (int t = 0; t < p.ntiles; ++t) {
    if (!__syncthreads_or(hits < limit)) break;      // also: the tile's last readers are through
    const int base = p.begin + t * p.tile;
    const int count = p.end - base < p.tile ? (p.end - base < 0 ? 0 : p.end - base) : p.tile;
    load_tile(reinterpret_cast<float *>(tile), p, base, count);
    __syncthreads();
    if (__any(hits < limit)) {
      scan_tile(tile, p, base, count, [&](float d, int j) {
        if (d < r2 && hits < limit) {
          if (row) row[hits] = j;
          first = hits == 0 ? j : first;
          ++hits;
        }
      });
    }
  }
}

__global__ __launch_bounds__(1024) void ball_query_kernel(SearchArgs a, float r2, int nsample, int pad_first,
                                                          int *__restrict__ idx, int *__restrict__ cnt) {
  extern __shared__ float4 lds[];
  const Place p = place_of(a);
  float4 *tile = lds + p.seg * (p.tile / 8 * 6);
  const bool mine = p.qi < a.m;
  int *row = idx + ((size_t)p.b * a.m + (mine ? p.qi : 0)) * nsample;
  const int want = mine && p.live ? nsample : 0;
  int total, first;
  if (a.split == 1) {
    ball_pass(tile, p, r2, want, row, total, first);
  } else {
    // the exchange arrays lie behind the tiles
    int *counts = reinterpret_cast<int *>(lds + a.split * (kSplitTile / 8 * 6));
    int *firsts = counts + a.split * 64;
    int hits, own_first;
    ball_pass(tile, p, r2, want, nullptr, hits, own_first);
    counts[p.seg * 64 + p.gt] = hits;
    firsts[p.seg * 64 + p.gt] = own_first;
    __syncthreads();
    int before = 0;
    total = 0, first = -1;
    for (int s = 0; s < a.split; ++s) {
      const int c = counts[s * 64 + p.gt];
      before += s < p.seg ? c : 0;
      first = total == 0 && c > 0 ? firsts[s * 64 + p.gt] : first;
      total += c;
    }
    total = total < nsample ? total : nsample;
    const int room = nsample - before;      // what the earlier segments leave of the row
    const int share = room <= 0 ? 0 : (hits < room ? hits : room);
    int written, unused;
    ball_pass(tile, p, r2, share, row + (before < nsample ? before : 0), written, unused);
  }
  if (p.seg == 0 && mine) {
    const int fill = pad_first && total > 0 ? first : -1;
    for (int s = total; s < nsample; ++s) row[s] = fill;
    if (cnt) cnt[(size_t)p.b * a.m + p.qi] = total;
  }
}

// ----------------------------------------------------------------------------------------------------- gathers
__global__ __launch_bounds__(256) void group_fwd_kernel(const float *__restrict__ feat, const int *__restrict__ idx,
                                                        int c, int n, long slots, long total,
                                                        float *__restrict__ out) {
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const long bc = e / slots, b = bc / c;
    const int j = idx[b * slots + (e - bc * slots)];
    out[e] = j == -1 ? 0.f : ((unsigned)j < (unsigned)n ? feat[bc * n + j] : __builtin_nanf(""));
  }
}

__global__ __launch_bounds__(256) void interpolate_fwd_kernel(const float *__restrict__ feat,
                                                              const int *__restrict__ idx,
                                                              const float *__restrict__ weight, int c, int n, int m,
                                                              int s, long total, float *__restrict__ out) {
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const long bc = e / m, b = bc / c;
    const long row = (b * m + (e - bc * m)) * s;
    float acc = 0.f;
    bool any = false;
    for (int t = 0; t < s; ++t) {
      const int j = idx[row + t];
      if (j == -1) continue;
      const float f = (unsigned)j < (unsigned)n ? feat[bc * n + j] : __builtin_nanf("");
      const float term = weight[row + t] * f;
      acc = any ? acc + term : term;
      any = true;
    }
    out[e] = acc;
  }
}

// one thread per (cloud, channel, target): grad_out is [b,c,m,s] (weight null) or [b,c,m]
__global__ __launch_bounds__(256) void group_bwd_kernel(const float *__restrict__ g, const float *__restrict__ weight,
                                                        const int *__restrict__ offs, const int *__restrict__ list,
                                                        int c, int n, int s, long slots, long total,
                                                        float *__restrict__ gf) {
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int j = (int)(e % n);
    const long bc = e / n, b = bc / c;
    const int beg = j > 0 ? offs[b * n + j - 1] : 0, end = offs[b * n + j];
    const int *l = list + b * slots;
    float acc = 0.f;
    if (weight) {
      const float *w = weight + b * slots, *row = g + bc * (slots / s);
      for (int i = beg; i < end; ++i) acc += w[l[i]] * row[l[i] / s];
    } else {
      const float *row = g + bc * slots;
      for (int i = beg; i < end; ++i) acc += row[l[i]];
    }
    gf[e] = acc;
  }
}

// ---------------------------------------------------------------------------------------------------- dispatch
// the widest split a list bucket allows: the merge's lists (half the segments write at a time) fit the tiles' LDS
constexpr int max_split(int kb) { return kb <= 8 ? 16 : (kb <= 16 ? 8 : 4); }

// the launch shape of the m queries of a search against n targets, S at most `cap`: a.split and a.qblocks, workgroups,
// threads.  kWavesPerCu is four waves per SIMD: until the device is that full a wider split is faster at every batch
// size measured ("Neighbourhood queries", has the table).
int search_shape(const char *what, int b, int cap, SearchArgs &a, sn::SplitLaunch *l) {
  int split = 1;
  if (const int rc = sn::pick_split(SN_KNOB("SN_NEIGHBORS_SPLIT"), b, a.m, a.n, cap, kWavesPerCu, kMinSegment, &split))
    return rc;
  if (const int rc = sn::split_launch(what, b, a.m, split, l)) return rc;
  a.split = l->split;
  a.qblocks = l->qblocks;
  return 0;
}

int check_search(const char *what, const float *xyz, const float *new_xyz, int b, int n, int m, const int *idx) {
  SN_REQUIRE(xyz && new_xyz && idx, "%s: null pointer", what);
  SN_REQUIRE(b >= 1 && n >= 1 && m >= 1, "%s: need b,n,m >= 1 (got %d,%d,%d)", what, b, n, m);
  SN_REQUIRE(n <= kMaxPoints && m <= kMaxPoints, "%s: cloud too large", what);
  return 0;
}

size_t tile_bytes(int split) { return (size_t)split * (split == 1 ? kWideTile : kSplitTile) * 12; }

template <int KB>
int launch_knn(SearchArgs a, int b, int k, int *idx, float *dist2, hipStream_t s) {
  constexpr int cap = max_split(KB);
  sn::SplitLaunch l;
  if (const int rc = search_shape("sn_knn_query", b, cap, a, &l)) return rc;
  const size_t merge = (size_t)((l.split + 1) / 2) * KB * 64 * 8;
  const size_t lds = l.split > 1 && merge > tile_bytes(l.split) ? merge : tile_bytes(l.split);
  knn_query_kernel<KB, 64 * cap><<<l.grid, l.threads, lds, s>>>(a, k, idx, dist2);
  return sn::launch_status("sn_knn_query");
}

static_assert(64 * max_split(1) <= 1024 && max_split(kMaxK) * 64 >= sn::kWideLanes, "workgroup sizes of the k-NN buckets");
static_assert((kMaxSplit + 1) / 2 * 8 * 64 * 8 <= 48 * 1024 && kMaxSplit * kSplitTile * 12 + kMaxSplit * 64 * 8 <= 64 * 1024,
              "LDS of the widest split");

}  // namespace

extern "C" size_t sn_neighbors_workspace_bytes(int b, int n, int m, int k) {
  (void)b, (void)n, (void)m, (void)k;
  return 0;      // neither search needs one
}

extern "C" int sn_knn_query(const float *xyz, const float *new_xyz, int b, int n, int m, int k, const int *lengths,
                            const int *new_lengths, int *idx, float *dist2, void *workspace, size_t workspace_bytes,
                            void *stream) {
  if (const int rc = check_search("sn_knn_query", xyz, new_xyz, b, n, m, idx)) return rc;
  SN_REQUIRE(k >= 1 && k <= kMaxK, "sn_knn_query: need 1 <= k <= %d (got %d)", kMaxK, k);
  SN_REQUIRE((long)m * k <= kMaxPoints, "sn_knn_query: m * k too large");
  (void)workspace, (void)workspace_bytes;
  hipStream_t s = sn::as_stream(stream);
  const SearchArgs a{xyz, new_xyz, lengths, new_lengths, n, m, 1, 1};
  if (k <= 1) return launch_knn<1>(a, b, k, idx, dist2, s);
  if (k <= 2) return launch_knn<2>(a, b, k, idx, dist2, s);
  if (k <= 3) return launch_knn<3>(a, b, k, idx, dist2, s);
  if (k <= 4) return launch_knn<4>(a, b, k, idx, dist2, s);
  if (k <= 8) return launch_knn<8>(a, b, k, idx, dist2, s);
  if (k <= 16) return launch_knn<16>(a, b, k, idx, dist2, s);
  return launch_knn<32>(a, b, k, idx, dist2, s);
}

extern "C" int sn_ball_query(const float *xyz, const float *new_xyz, int b, int n, int m, float radius, int nsample,
                             int pad_first, const int *lengths, const int *new_lengths, int *idx, int *cnt,
                             void *workspace, size_t workspace_bytes, void *stream) {
  if (const int rc = check_search("sn_ball_query", xyz, new_xyz, b, n, m, idx)) return rc;
  SN_REQUIRE(nsample >= 1, "sn_ball_query: need nsample >= 1 (got %d)", nsample);
  SN_REQUIRE(radius >= 0.f && radius <= 3.4028234664e38f, "sn_ball_query: radius must be finite and >= 0");
  SN_REQUIRE((long)m * nsample <= kMaxPoints, "sn_ball_query: m * nsample too large");
  (void)workspace, (void)workspace_bytes;
  SearchArgs a{xyz, new_xyz, lengths, new_lengths, n, m, 1, 1};
  sn::SplitLaunch l;
  if (const int rc = search_shape("sn_ball_query", b, kMaxSplit, a, &l)) return rc;
  const size_t lds = tile_bytes(l.split) + (l.split > 1 ? (size_t)l.split * 64 * 8 : 0);
  ball_query_kernel<<<l.grid, l.threads, lds, sn::as_stream(stream)>>>(a, radius * radius, nsample, pad_first, idx, cnt);
  return sn::launch_status("sn_ball_query");
}

extern "C" int sn_group_forward(const float *features, const int *idx, int b, int c, int n, int m, int s, float *out,
                                void *stream) {
  SN_REQUIRE(features && idx && out, "sn_group_forward: null pointer");
  SN_REQUIRE(b >= 1 && c >= 1 && n >= 1 && m >= 1 && s >= 1, "sn_group_forward: need b,c,n,m,s >= 1");
  SN_REQUIRE(n <= kMaxPoints && (long)m * s <= kMaxPoints, "sn_group_forward: cloud too large");
  const long slots = (long)m * s, total = (long)b * c * slots;
  group_fwd_kernel<<<sn::grid_blocks(total, kMaxBlocks), 256, 0, sn::as_stream(stream)>>>(features, idx, c, n, slots,
                                                                                         total, out);
  return sn::launch_status("sn_group_forward");
}

extern "C" int sn_interpolate_forward(const float *features, const int *idx, const float *weight, int b, int c, int n,
                                      int m, int s, float *out, void *stream) {
  SN_REQUIRE(features && idx && weight && out, "sn_interpolate_forward: null pointer");
  SN_REQUIRE(b >= 1 && c >= 1 && n >= 1 && m >= 1 && s >= 1, "sn_interpolate_forward: need b,c,n,m,s >= 1");
  SN_REQUIRE(n <= kMaxPoints && (long)m * s <= kMaxPoints, "sn_interpolate_forward: cloud too large");
  const long total = (long)b * c * m;
  interpolate_fwd_kernel<<<sn::grid_blocks(total, kMaxBlocks), 256, 0, sn::as_stream(stream)>>>(
      features, idx, weight, c, n, m, s, total, out);
  return sn::launch_status("sn_interpolate_forward");
}

extern "C" size_t sn_group_backward_workspace_bytes(int b, int n, int m, int s) {
  if (b < 1 || n < 1 || m < 1 || s < 1) return 0;
  return sn::layout_bytes(index_lists_layout, b, n, (long)m * s);
}

extern "C" int sn_group_backward(const float *grad_out, const int *idx, const float *weight, int b, int c, int n,
                                 int m, int s, float *grad_features, void *workspace, size_t workspace_bytes,
                                 void *stream) {
  SN_REQUIRE(grad_out && idx && grad_features && workspace, "sn_group_backward: null pointer");
  SN_REQUIRE(b >= 1 && c >= 1 && n >= 1 && m >= 1 && s >= 1, "sn_group_backward: need b,c,n,m,s >= 1");
  SN_REQUIRE(n <= kMaxPoints && (long)m * s <= kMaxPoints, "sn_group_backward: cloud too large");
  const long slots = (long)m * s, total = (long)b * c * n;
  sn::Carver carver(workspace);
  const IndexLists w = index_lists_layout(carver, b, n, slots);  // the slots grouped by the target they point at
  SN_REQUIRE(workspace && workspace_bytes >= carver.bytes(), "sn_group_backward: workspace too small (%zu < %zu)",
             workspace_bytes, carver.bytes());
  hipStream_t st = sn::as_stream(stream);
  if (const int rc = build_index_lists("sn_group_backward", idx, b, n, slots, w, st)) return rc;
  group_bwd_kernel<<<sn::grid_blocks(total, kMaxBlocks), 256, 0, st>>>(grad_out, weight, w.offs, w.list, c, n, s,
                                                                       slots, total, grad_features);
  return sn::launch_status("sn_group_backward");
}
