// pair_filter.hpp -- the sorted-stream pair filter shared by the Chamfer search (chamfer_nn.hip) and the persistent
// auction (emd.hip): the two data formats, the numeric margins and the small pieces both search loops are built from.
// The loops themselves stay in their files (the auction's prefetches, carries prices and splits superblocks among
// waves; Chamfer's does none of that).
//
// Both kernels put the targets in Hilbert order (cloud_sort.hpp), prune blocks of consecutive targets by bounding
// box, filter the remaining pairs on the matrix cores and evaluate the rare hits exactly out of a per-wave LDS queue.
//
// Operand stream.  u_kj = |t_k|^2 - 2 t_k . x_j is a [targets x 4] . [4 x queries] product with rows
//   (-2x, -2y, -2z, |t|^2) and columns (x, y, z, 1).  v_mfma_f32_16x16x4_f32 (exact fp32: an fmaf chain) takes ONE
//   float per lane for A: lane l supplies A[i = l & 15][k = l >> 4].  A superblock of 64 targets is 4 such operands;
//   lane l's four values sit in one float4:
//     stream[superblock * 64 + l].q = component (l >> 4) of target 64 sb + 16 q + (l & 15)
//   so a wave fetches 64 targets with one coalesced global_load_dwordx4 per lane (store_operand writes it).  Lane l
//   receives the four targets 16 q + 4 (l >> 4) + r of query 16 g + (l & 15): bit 4 q + r of the lane's hit mask
//   (hits4) is stream position hit_position.  Padding targets carry |t|^2 = kFar and never pass.
// Box rows.  The bounding box of a block of targets is 8 floats, read as two float4:
//     {lo x, lo y, lo z, hi x}, {hi y, hi z, free, free}
//   (store_box_row writes it, box_gap2 reads it; the auction keeps a price bound in the first free word).
//
// Margins.  A pair can only matter if u <= T_j, T_j = (squared reach of query j) (1 + 2^-20) - |x_j|^2 + slack.
//   * slack = 2^-18 (max|t|^2 + |x|^2) covers the fmaf chain's rounding (4 roundings of partial sums
//     <= 2 (|t|^2 + |x|^2)), the rounding of the stored |t|^2 and of |x|^2, and the fp32 evaluation of T itself;
//     max|t|^2 is bounded by the far corner of the targets' box (far_corner2).
//   * (1 + 2^-20) covers the rounding of the squared reach: Chamfer's exact d, the auction's r |r|.
//   * with prices carried through a second MFMA (emd.hip, bid_group) the chain is twice as long and the slack
//     2^-17 (max|t|^2 + |x|^2) + 2^-16 gamma^2; the derivation is beside the code that builds that operand.
//   * a box test compares the squared gap, rounded DOWN by kDown, with a squared reach rounded UP by kUp.
#pragma once
#include <hip/hip_runtime.h>

namespace sn {
namespace pf {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr float kSlack18 = 3.814697265625e-06f;       // 2^-18
constexpr float kSlack17 = 7.62939453125e-06f;        // 2^-17
constexpr float kUp20 = 1.00000095367431640625f;      // 1 + 2^-20
constexpr float kUp16 = 1.0000152587890625f;          // 1 + 2^-16
constexpr float kDown = 0.9999f, kUp = 1.0001f;       // box tests, far_corner2
constexpr float kFar = 3.0e38f;                       // padding |t|^2, closed thresholds (-kFar), empty boxes
static_assert(kSlack18 == 1.0f / (1 << 18) && kSlack17 == 1.0f / (1 << 17), "exact powers of two");
static_assert(kUp20 == 1.0f + 1.0f / (1 << 20) && kUp16 == 1.0f + 1.0f / (1 << 16), "exact");

// the reference's squared distance: every product and sum rounded on its own
__device__ __forceinline__ float sq_dist(float tx, float ty, float tz, float x1, float y1, float z1) {
#pragma clang fp contract(off)
  const float dx = tx - x1, dy = ty - y1, dz = tz - z1;
  const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
  return (xx + yy) + zz;
}

// |v|^2 as the filter stores and bounds it
__device__ __forceinline__ float norm2(float x, float y, float z) {
#pragma clang fp contract(off)
  return (x * x + y * y) + z * z;
}

// upper bound of every stored |t|^2: the far corner of the targets' box {lo xyz, hi xyz}
__device__ __forceinline__ float far_corner2(const float *bbox) {
  float tmax = 0.f;
#pragma unroll
  for (int a = 0; a < 3; ++a) tmax += __builtin_fmaxf(bbox[a] * bbox[a], bbox[3 + a] * bbox[3 + a]);
  return tmax * kUp;
}

// store the target at stream position p of this superblock (tt = |t|^2, kFar for padding): word q = (p >> 4) & 3 of
// the float4 of lane (component k) * 16 + (p & 15)
__device__ __forceinline__ void store_operand(f4 *superblock, int p, float x, float y, float z, float tt) {
  float *m = reinterpret_cast<float *>(superblock) + (p & 15) * 4 + ((p >> 4) & 3);
  m[0 * 64] = -2.f * x;
  m[1 * 64] = -2.f * y;
  m[2 * 64] = -2.f * z;
  m[3 * 64] = tt;
}

// word c of box row r; the lanes c = 0..7 of a group that all hold the box write the row (the corners by value:
// read through pointers the choice becomes a tree of branches)
__device__ __forceinline__ void store_box_row(float *rows, long r, int c, float lx, float ly, float lz, float hx,
                                              float hy, float hz) {
  if (c < 8) rows[r * 8 + c] = c == 0 ? lx : c == 1 ? ly : c == 2 ? lz : c == 3 ? hx : c == 4 ? hy : c == 5 ? hz : 0.f;
}

// squared gap between the box of row {A, B} and the box [qlo, qhi] (a point: qlo == qhi), rounded down
__device__ __forceinline__ float box_gap2(const f4 A, const f4 B, const float *qlo, const float *qhi) {
  const float gx = __builtin_fmaxf(__builtin_fmaxf(A.x - qhi[0], qlo[0] - A.w), 0.f);
  const float gy = __builtin_fmaxf(__builtin_fmaxf(A.y - qhi[1], qlo[1] - B.x), 0.f);
  const float gz = __builtin_fmaxf(__builtin_fmaxf(A.z - qhi[2], qlo[2] - B.y), 0.f);
  return ((gx * gx + gy * gy) + gz * gz) * kDown;
}

__device__ __forceinline__ float min16(const f4 a, const f4 b, const f4 c, const f4 d) {
  const float m0 = __builtin_fminf(__builtin_fminf(a.x, a.y), a.z);
  const float m1 = __builtin_fminf(__builtin_fminf(a.w, b.x), b.y);
  const float m2 = __builtin_fminf(__builtin_fminf(b.z, b.w), c.x);
  const float m3 = __builtin_fminf(__builtin_fminf(c.y, c.z), c.w);
  const float m4 = __builtin_fminf(__builtin_fminf(d.x, d.y), d.z);
  const float m5 = __builtin_fminf(__builtin_fminf(m0, m1), d.w);
  return __builtin_fminf(__builtin_fminf(m2, m3), __builtin_fminf(m4, m5));
}

__device__ __forceinline__ unsigned hits4(const f4 d, float thr, int shift) {
  return ((d.x <= thr ? 1u : 0u) | (d.y <= thr ? 2u : 0u) | (d.z <= thr ? 4u : 0u) |
          (d.w <= thr ? 8u : 0u)) << shift;
}

// stream position of bit i of a lane's hit mask in the superblock that starts at position sb0 (row = lane >> 4)
__device__ __forceinline__ int hit_position(int sb0, int i, int row) {
  return sb0 + 16 * (i >> 2) + 4 * row + (i & 3);
}

// One turn of the hit queue: every lane whose hit mask hm is not empty takes its lowest bit i out of it and appends
// entry(i) to the wave's LDS queue behind the qcount (wave-uniform) entries it holds, in lane order.  Returns the new
// count.  An entry is `stream position | query lane << shift` (the shift is the caller's).  The bit is taken HERE and
// entry captures by value: entry(i) is then computed under the predicate, as the open-coded form was (an entry that
// captures a bit chosen outside costs nn_search_kernel registers and 57 instructions).
template <class Entry>
__device__ __forceinline__ int queue_append(unsigned *queue, int qcount, unsigned &hm, Entry entry) {
  const bool has = hm != 0;
  const int i = has ? __builtin_ctz(hm) : 0;
  hm &= hm - 1;
  const unsigned long long bal = __ballot(has);
  const int pos = qcount + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32),
                                                          __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
  if (has) queue[pos] = entry(i);
  return qcount + __popcll(bal);
}

}  // namespace pf
}  // namespace sn
