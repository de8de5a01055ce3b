// emd_bid.hpp -- the auction's bid arithmetic, shared by the persistent auction (emd.hip) and the general-size
// auction (emd_general.hip): the exact bid value, its tie rule, the conservative fp32 pre-filter and GetMax's window.
// Build with -ffp-contract=off (the Makefile's FLAGS): every product and sum below is rounded on its own.
#pragma once
#include <hip/hip_runtime.h>

#include "pair_filter.hpp"

namespace sn {
namespace emd {

using pf::sq_dist;  // s of bid_value, on its own

struct Top2 {
  float best, better;
  int best_i, better_i;  // best_i: canonical among exact ties (see tie_key); better_i: a hint
};

__device__ __forceinline__ float bid_value(float tx, float ty, float tz, float p, float x1,
                                           float y1, float z1) {
#pragma clang fp contract(off)
  const float dx = tx - x1, dy = ty - y1, dz = tz - z1;
  const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
  const float s = (xx + yy) + zz;
  return (float)((3.0 - (double)__builtin_sqrtf(s)) - (double)p);
}

// Exact ties at the top.  The reference's Bid resolves d_k == best to
// argmin (thread(k), k): thread(k) = ((k mod 2048) / delta), delta = ceil(end_k / tpu)
// (emd_cuda.cu:136-139, :166-173).  key(k) = thread(k) * 2^20 + k orders those candidates.
struct TieGeom {
  int n, tpu;
};
__device__ __forceinline__ int tie_key(const TieGeom &g, int k) {
  const int k2 = (k / 2048) * 2048;
  const int end_k = (g.n < k2 + 2048 ? g.n : k2 + 2048) - k2;
  const int delta = (end_k + g.tpu - 1) / g.tpu;
  return ((k - k2) / delta) * (1 << 20) + k;  // n <= 2^20 (host check)
}

// if (d > best) {better = best; best = d; best_i = k} else if (d > better) better = d,
// plus: on d == best the candidate with the smaller tie key becomes best_i (values unchanged:
// better becomes best through the "else if").  Runs only on the exact path.
__device__ __forceinline__ void top2_push(Top2 &t, float d, int k, const TieGeom &g) {
  if (__any(d == t.best && t.best_i >= 0)) {  // rare: an exact tie with the running best
    if (d == t.best && t.best_i >= 0 && tie_key(g, k) < tie_key(g, t.best_i)) {
      const int o = t.best_i;
      t.best_i = k;
      k = o;  // the displaced index is an equally valid witness for `better`
    }
  }
  const bool gt = d > t.best;
  const bool mid = !gt && d > t.better;
  t.better_i = gt ? t.best_i : (mid ? k : t.better_i);
  t.better = gt ? t.best : (mid ? d : t.better);
  t.best_i = gt ? k : t.best_i;
  t.best = gt ? d : t.best;
}

// top-2 of the union of two partial results; equal best values keep the smaller tie key
__device__ __forceinline__ void top2_merge(Top2 &a, float b_best, float b_better, int b_i,
                                           int b_i2, const TieGeom &g) {
  if (b_best > a.best) {
    const bool keep_a = a.best >= b_better;
    a.better = keep_a ? a.best : b_better;
    a.better_i = keep_a ? a.best_i : b_i2;
    a.best = b_best;
    a.best_i = b_i;
  } else {
    if (b_best == a.best && b_i >= 0 && a.best_i >= 0 && tie_key(g, b_i) < tie_key(g, a.best_i)) {
      const int o = a.best_i;
      a.best_i = b_i;
      b_i = o;
    }
    const bool take_b = b_best > a.better;
    a.better = take_b ? b_best : a.better;
    a.better_i = take_b ? b_i : a.better_i;
  }
}

// ---- conservative fp32 filter --------------------------------------------------------
// A target k can change a lane's top-2 only if d_k > c, c = the lane's running `better`
// (or any proven lower bound of the bidder's final `better`).  With q = sqrtf(s):
//   d_k > c  =>  3 - q - p_k > c - 1e-15  =>  q < (3 - p_k - c) + 1e-15  =: R
//   =>  s < R^2 (1 + 2^-22).
// The filter evaluates R' = A'_k - c' in fp32 with A'_k = fl(3 - p_k) + eps (3 + |p_k|) and
// c' = c - eps (3 + |c|), eps = 2^-20: the two margins exceed every rounding error of the
// filter itself (<= 2^-22 (6 + |p| + |c|), plus 2^-22 relative on the FMA-evaluated s) and
// the relative slack needed on R, so
// "s <= R' |R'|" is implied by d_k >= c.  Only targets that pass go through the exact
// path (correctly rounded sqrt, fp64 detour, top-2 update); everything else costs
// 8 (distance) + 3 (filter) VALU ops instead of ~45.
constexpr float kFilterEps = 9.5367431640625e-07f;  // 2^-20

__device__ __forceinline__ float filter_target(float p) {
  return (3.0f - p) + (3.0f + __builtin_fabsf(p)) * kFilterEps;
}
__device__ __forceinline__ float filter_thr(float c) {
  return c - (3.0f + __builtin_fabsf(c)) * kFilterEps;
}
__device__ __forceinline__ bool filter_pass(float s, float a_k, float cthr) {
  const float r = a_k - cthr;
  return s <= r * __builtin_fabsf(r);
}

// GetMax's window (emd_cuda.cu:188): bidder increment bi against the target's maximum mi, compared in double
__device__ __forceinline__ bool in_window(float bi, float mi) {
  return (double)bi - 1e-6 <= (double)mi && (double)mi <= (double)bi + 1e-6;
}

}  // namespace emd
}  // namespace sn
