// grid_cell.hpp -- the cell of one point in the occupancy grid of occupancy.hip, written once for host and device (as
// eig3.hpp is for local_pca.hip).  include/ops/occupancy.h states the rule; every function below is one of its
// sentences.  Integers and double, nothing contracted (the build has -ffp-contract=off).
#pragma once
#include <cmath>

namespace grid_cell {

constexpr int kMinRes = 2, kMaxRes = 32;

// a = 2 i - (res - 1): the centre of index i, in units of half a spacing
__host__ __device__ inline int coord(int i, int res) { return 2 * i - (res - 1); }

__host__ __device__ inline bool in_sphere(int i, int j, int k, int res) {
  const int a0 = coord(i, res), a1 = coord(j, res), a2 = coord(k, res), r = res - 1;
  return a0 * a0 + a1 * a1 + a2 * a2 <= r * r;
}

// A cell of the in-sphere list is packed as (i << 10) | (j << 5) | k: five bits per index, and packed cells order as
// their linear indices do.
__host__ __device__ inline int pack(int i, int j, int k) { return (i << 10) | (j << 5) | k; }
__host__ __device__ inline int linear(int packed, int res) {
  return ((packed >> 10) * res + ((packed >> 5) & 31)) * res + (packed & 31);
}

// the in-sphere cells of row (i, j): their number, and the lowest k among them (they are contiguous in k)
__host__ __device__ inline int row_cells(int i, int j, int res, int *first) {
  int count = 0;
  *first = 0;
  for (int k = res - 1; k >= 0; --k)
    if (in_sphere(i, j, k, res)) ++count, *first = k;
  return count;
}

// neither NaN nor infinite
__host__ __device__ inline bool is_finite(float x) { return fabsf(x) <= 3.40282346638528859812e38f; }

// u of a coordinate: exact (24 bits times at most 6)
__host__ __device__ inline double scaled(float x, int res) { return (double)x * (double)(2 * (res - 1)); }

// Rule 1 on one axis: the number of midpoints 2 j + 2 - res, j in 0 .. res - 2, below u
__host__ __device__ inline int axis_index(double u, int res) {
  int i = 0;
  for (int j = 0; j < res - 1; ++j) i += u > (double)(2 * j + 2 - res) ? 1 : 0;
  return i;
}

// D of Rule 2 for a packed cell
__host__ __device__ inline double distance(double u0, double u1, double u2, int packed, int res) {
  const double d0 = u0 - (double)coord(packed >> 10, res), d1 = u1 - (double)coord((packed >> 5) & 31, res),
               d2 = u2 - (double)coord(packed & 31, res);
  return (d0 * d0 + d1 * d1) + d2 * d2;
}

// (d, packed) beats (best_d, best): a smaller D, or the same D at a lower index
__host__ __device__ inline bool beats(double d, int packed, double best_d, int best) {
  return d < best_d || (d == best_d && packed < best);
}

// Rule 2 over list[first], list[first + step], ...: the best (D, packed cell) among them, (inf, INT_MAX) where there
// is none.  The host scans the whole list (first 0, step 1); a wave gives each lane a stride and merges with beats().
__host__ __device__ inline void scan(double u0, double u1, double u2, const int *list, int count, int res, int first,
                                     int step, double *best_d, int *best) {
  double bd = HUGE_VAL;
  int bc = 0x7fffffff;
  for (int t = first; t < count; t += step) {
    const int packed = list[t];
    const double d = distance(u0, u1, u2, packed, res);
    if (d < bd) bd = d, bc = packed;      // ascending indices: the first of equal D stays
  }
  *best_d = bd, *best = bc;
}

// Rule 2 bounded: the same scan over the in-sphere cells of the box of kBoxSide^3 cells around the packed cube cell
// `cube` Rule 1 found, cell t of the box for t = first, first + step, ... (ascending linear indices).  A cell OUTSIDE
// the box differs from the cube cell by more than kBoxHalf on some axis, and Rule 1 put u within 1 of the cube cell's
// centre on that side, so |u - a| >= 2 kBoxHalf + 1 there; rounding is monotone and that number and its square are
// representable, so the cell's rounded D is at least kBoxLimit = (2 kBoxHalf + 1)^2.  Hence a best D of the box BELOW
// kBoxLimit beats every cell outside it, ties included, and is Rule 2's answer; otherwise the caller scans the list.
constexpr int kBoxHalf = 2, kBoxSide = 2 * kBoxHalf + 1, kBoxCells = kBoxSide * kBoxSide * kBoxSide;
constexpr double kBoxLimit = (double)(kBoxSide * kBoxSide);
__host__ __device__ inline void scan_box(double u0, double u1, double u2, int cube, int res, int first, int step,
                                         double *best_d, int *best) {
  const int i0 = (cube >> 10) - kBoxHalf, j0 = ((cube >> 5) & 31) - kBoxHalf, k0 = (cube & 31) - kBoxHalf;
  double bd = HUGE_VAL;
  int bc = 0x7fffffff;
  for (int t = first; t < kBoxCells; t += step) {
    const int i = i0 + t / (kBoxSide * kBoxSide), j = j0 + t / kBoxSide % kBoxSide, k = k0 + t % kBoxSide;
    if (i < 0 || i >= res || j < 0 || j >= res || k < 0 || k >= res || !in_sphere(i, j, k, res)) continue;
    const int packed = pack(i, j, k);
    const double d = distance(u0, u1, u2, packed, res);
    if (d < bd) bd = d, bc = packed;
  }
  *best_d = bd, *best = bc;
}

// Rule 1 on the three axes.  Returns the linear cell, or -1 - packed cube cell where that cell lies outside the sphere
// and Rule 2 has to decide (u0, u1, u2 are left for it).
__host__ __device__ inline int rule1(float x, float y, float z, int res, int sphere, double *u0, double *u1,
                                     double *u2) {
  *u0 = scaled(x, res), *u1 = scaled(y, res), *u2 = scaled(z, res);
  const int i = axis_index(*u0, res), j = axis_index(*u1, res), k = axis_index(*u2, res);
  if (!sphere || in_sphere(i, j, k, res)) return (i * res + j) * res + k;
  return -1 - pack(i, j, k);
}

}  // namespace grid_cell
