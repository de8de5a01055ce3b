// emd_auction.hpp -- one iteration of the reference's auction, per bidder: the steps the stream-ordered auction
// (emd_general.hip: three launches per iteration, the state in the global workspace) and the set-level auction
// (set_emd.hip: one workgroup per pair, the state in LDS) both run.  Written once over plain pointers to ONE cloud's
// rows; where the rows live is the caller's business, and so are the launches or barriers between the phases.
//
//   bid     an unassigned bidder finds the top two of its bid values (emd_bid.hpp) over all m targets.  G lanes of a
//           wave serve one bidder (G a power of two, 1 .. 64), each scanning every G-th target with the conservative
//           fp32 filter and computing the exact value only where the target can enter its top two; the group merges
//           its partial results with the (thread(k), k) tie key.  The top-2 VALUES do not depend on the partition and
//           tie_key restores the reference's index rule, so G is a pure performance choice.  The increment
//           best - better + eps goes into the target's running maximum through an atomic max on an order-preserving
//           integer key (increments can be negative when eps < 0).  A bidder with a non-finite coordinate passes no
//           filter: its bid is -1, it posts nothing, never wins and is re-queued every iteration.
//   window  the bidders within +-1e-6 of their target's final maximum stamp the target's max_idx with an atomic max
//           on (stamp << 32 | j), stamp = iteration + 1: the highest j of this iteration wins, and a target nobody
//           reached keeps its stale index (the reference never clears max_idx).  Skipped in the last iteration.
//   assign  winners take their target, evict its previous owner, raise its price and reset its maximum; losers and the
//           evicted go to the next iteration's list (unordered: which position a bidder gets never enters a result).
//           The last iteration forces every bid instead: each bidder takes the target it bid for, nothing else moves.
// All bids of an iteration are posted before its window phase starts, and all offers made before its assign phase.
#pragma once
#include "common.hpp"
#include "emd_bid.hpp"

namespace sn {
namespace emd {

// one cloud's auction state
struct AuctionRows {
  float *price;                 // [m]
  int *assign_inv;              // [m] bidder holding the target, -1
  unsigned *max_key;            // [m] running maximum increment, as sn::ordered_key; starts at ordered_key(0)
  unsigned long long *max_idx;  // [m] (stamp << 32) | j of the window's winner; starts at 0: a stale index 0
  int *bid;                     // [n] target of the bidder's last bid, -1 for none
  float *bid_inc;               // [n] its increment
  int *assignment;              // [n] target the bidder holds, -1
};

// the reference's geometry, which only the tie rule sees: ceil(bidders / 1024) blocks share the cloud's cnt
// unassigned bidders, 1024 / (bidders per block) threads serve each
__device__ __forceinline__ TieGeom reference_tie_geom(int bidders, int targets, int cnt) {
  const int block_cnt = (bidders + 1023) / 1024, per_block = (cnt + block_cnt - 1) / block_cnt;
  return TieGeom{targets, 1024 / per_block};
}

// ---- bid.  One lane's share of a tile of targets: tile[c] holds {x, y, z, filter_target(price)} of target k_first + c,
// whose exact price is read from the cloud's price[]; the lane takes c = c_begin, c_begin + G, ... below c_end.  cthr is
// the lane's filter threshold: filter_thr of a lower bound of the bidder's final `better`.
__device__ __forceinline__ void scan_targets(Top2 &t, float &cthr, const float4 *tile, const float *price, int k_first,
                                             int c_begin, int c_end, int G, float x1, float y1, float z1,
                                             const TieGeom &g) {
  for (int c = c_begin; c < c_end; c += G) {
    const float4 q = tile[c];
    if (filter_pass(sq_dist(q.x, q.y, q.z, x1, y1, z1), q.w, cthr)) {  // d_k may enter the top two
      top2_push(t, bid_value(q.x, q.y, q.z, price[k_first + c], x1, y1, z1), k_first + c, g);
      cthr = fmaxf(cthr, filter_thr(t.better));
    }
  }
}

// The second largest of the group's partial top-2 values is a lower bound of the bidder's final `better`: every lane
// filters with it (a lane alone would see each of its m / G targets pass about 2 ln(m / G) times).  All lanes of the
// group call it; returns the raised threshold.
__device__ __forceinline__ float share_filter_bound(const Top2 &t, int G, float cthr) {
  float b1 = t.best, b2 = t.better;
  for (int off = 1; off < G; off <<= 1) {
    const float o1 = __shfl_xor(b1, off), o2 = __shfl_xor(b2, off);
    b2 = fmaxf(fminf(b1, o1), fmaxf(b2, o2));
    b1 = fmaxf(b1, o1);
  }
  return fmaxf(cthr, filter_thr(b2));
}

// butterfly inside the group: every lane ends with the group's result
__device__ __forceinline__ void merge_group(Top2 &t, int G, const TieGeom &g) {
  for (int off = 1; off < G; off <<= 1) {
    const float ob = __shfl_xor(t.best, off), obb = __shfl_xor(t.better, off);
    const int oi = __shfl_xor(t.best_i, off), oi2 = __shfl_xor(t.better_i, off);
    top2_merge(t, ob, obb, oi, oi2, g);
  }
}

// one lane per bidder
__device__ __forceinline__ void post_bid(const AuctionRows &r, int j, const Top2 &t, float eps) {
  const float inc = t.best - t.better + eps;
  r.bid[j] = t.best_i;
  r.bid_inc[j] = inc;
  if (t.best_i >= 0)  // -1 only for non-finite inputs: such a bidder never wins
    atomicMax(&r.max_key[t.best_i], sn::ordered_key(inc));
}

// ---- window (GetMax)
__device__ __forceinline__ void offer_window(const AuctionRows &r, int j, unsigned stamp) {
  const int t = r.bid[j];
  if (t >= 0 && in_window(r.bid_inc[j], sn::ordered_float(r.max_key[t])))
    atomicMax(&r.max_idx[t], ((unsigned long long)stamp << 32) | (unsigned)j);
}

// ---- assign
struct Settled {
  int requeue;  // the bidder that is unassigned after this step (j itself, or the owner it evicted), -1 for none
  int target;   // outside the last iteration, the target j won, at its new ...
  float price;  // ... price; -1 otherwise
};
__device__ __forceinline__ Settled settle(const AuctionRows &r, int j, int last) {
  Settled s{-1, -1, 0.f};
  const int t = r.bid[j];
  if (t >= 0 && (last || (int)(unsigned)r.max_idx[t] == j)) {
    // one winner per target outside the last iteration: the target's words have a single writer
    r.assignment[j] = t;
    if (!last) {
      const int inv = r.assign_inv[t];
      if (inv != -1) {
        r.assignment[inv] = -1;
        s.requeue = inv;
      }
      r.assign_inv[t] = j;
      s.target = t;
      s.price = r.price[t] + r.bid_inc[j];
      r.price[t] = s.price;
      r.max_key[t] = sn::ordered_key(-1e9f);
    }
  } else if (!last) {
    s.requeue = j;
  }
  return s;
}

// wave-aggregated append of every lane's push >= 0 to the next list.  Whole waves call it.
__device__ __forceinline__ void append_unassigned(int push, int lane, int *next_list, int *next_cnt) {
  const unsigned long long mask = __ballot(push >= 0);
  if (mask) {
    const int leader = __ffsll((long long)mask) - 1;
    int pos = 0;
    if (lane == leader) pos = atomicAdd(next_cnt, __popcll(mask));
    pos = __shfl(pos, leader);
    if (push >= 0) next_list[pos + __popcll(mask & ((1ull << lane) - 1))] = push;
  }
}

// ---- CalcDist (emd_cuda.cu:217-226): bidder p minus its target k, which q points to -- three floats, or a record of
// the scan (one aligned load); an unassigned bidder (k < 0: no iterations, or a non-finite row) gets 0, q is not read
__device__ __forceinline__ float4 target_xyz(const float *q) { return make_float4(q[0], q[1], q[2], 0.f); }
__device__ __forceinline__ float4 target_xyz(const float4 *q) { return *q; }
template <class Target>
__device__ __forceinline__ float matched_sq_dist(int k, const float *p, const Target *q) {
#pragma clang fp contract(off)
  if (k < 0) return 0.f;
  const float4 t = target_xyz(q);
  const float dx = p[0] - t.x, dy = p[1] - t.y, dz = p[2] - t.z;
  return dx * dx + dy * dy + dz * dz;
}

}  // namespace emd
}  // namespace sn
