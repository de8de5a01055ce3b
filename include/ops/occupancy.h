/*
 * ops/occupancy.h -- the occupancy grid of a SET of clouds, of libsparenet_hip.so: every point of every cloud is
 * assigned to the nearest centre of a res x res x res lattice over [-0.5, 0.5]^3 (clipped to the unit sphere where
 * asked), and the set's points per cell and clouds per cell are counted.  It is what the Jensen-Shannon divergence
 * between two sets (Achlioptas et al. 2018; sparenet_amd.utils.set_metrics) is read off.  Conventions as in
 * ops/local_pca.h: raw DEVICE pointers (the _host entry point: HOST pointers), contiguous row-major arrays, sizes in
 * elements, asynchronous launches on `stream`, 0 / positive hipError_t / SN_EINVAL (-22) with a sn_last_error() text;
 * one lower-case base type per parameter, `void *stream` last.  SN_ABI_VERSION is unchanged.
 */
#ifndef SPARENET_HIP_OPS_OCCUPANCY_H
#define SPARENET_HIP_OPS_OCCUPANCY_H

#include "../sparenet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------ the definition
 * The grid.  2 <= res <= 32.  Cell (i, j, k) has the linear index i * res * res + j * res + k and the centre
 * (a0, a1, a2) / (2 (res - 1)) with the integer a = 2 i - (res - 1) per axis: the published i * spacing - 0.5 lattice.
 * A cell is IN THE SPHERE when a0^2 + a1^2 + a2^2 <= (res - 1)^2, decided in integers (the published
 * norm(centre) <= 0.5; equality occurs at res = 3, 5, 9, 17 and is included; res = 28 has 10144 cells in the sphere
 * and none on its boundary).  With in_sphere == 0 every cell counts.
 *
 * The cell of a point (x0, x1, x2), fp32.  A point with a NaN or infinite coordinate belongs to no cell and is counted
 * nowhere.  Otherwise, per axis, u = (double)x * (2 (res - 1)), which is exact.
 *   Rule 1 (per axis, exact).  i = #{ j in 0 .. res - 2 : u > 2 j + 2 - res }: the number of midpoints between
 *     neighbouring centres that lie below u, each compared exactly.  A point exactly on a midpoint goes to the LOWER
 *     index; a point outside the cube goes to the rim.  (x = 0 at res = 28 is a midpoint: cell 13; +1e-30 is cell 14.
 *     u + (res - 1) is never formed: it would round that difference away.)  If in_sphere == 0, or the cell
 *     (i0, i1, i2) is in the sphere, that cell is the answer.
 *   Rule 2 (otherwise).  D(a) = ((u0 - a0) * (u0 - a0) + (u1 - a1) * (u1 - a1)) + (u2 - a2) * (u2 - a2) in double, every
 *     operation separately rounded, no contraction, over ALL cells in the sphere.  The answer is the cell of the
 *     smallest D; among equal D the lowest linear index.  (A point as far away as 1e30, whose D are all equal after
 *     rounding, lands in the lowest in-sphere cell: defined behaviour, not an error.)
 * Rule 1 is the exact nearest centre of the cube; where that centre is in the sphere it is the nearest in-sphere
 * centre too, so Rule 2 decides only points whose cube cell was clipped away.
 *
 * The set.  xyz[s,n,3] (fp32) are s clouds; lengths[s] (int32, may be null: every cloud has n points) makes the batch
 * ragged: cloud c is its first lengths[c] rows (held to [0, n]; 0 is allowed), padding rows are never read.
 * Outputs (each may be null, but not all three):
 *   counts[res^3] (long long)  the number of points of the whole set in each cell;
 *   occupied[res^3] (int32)    the number of CLOUDS with at least one point in the cell;
 *   cells[s,n] (int32)         each point's cell; -1 at padding rows and at non-finite points.
 * Cells outside the sphere stay 0 where in_sphere != 0.  The outputs are written whole: nothing has to be cleared.
 *
 * A workgroup owns whole clouds (it loops when s exceeds the launch): the cloud's histogram lives in LDS, Rule 1 runs
 * one point per lane, the points that need Rule 2 are queued in LDS and then served a wave per point, the 64 lanes
 * striding the candidate cells with a cross-lane arg-min.  Rule 2's scan is bounded where that provably changes
 * nothing: the in-sphere cells of the 5 x 5 x 5 box around the clipped cube cell are scanned first; a cell outside the
 * box is at least 5 half spacings away on some axis, so its rounded D is at least 25 (rounding is monotone, 5 and 25
 * are representable), and a best D of the box BELOW 25 is therefore the minimum over all cells, ties included.
 * Otherwise the whole list of in-sphere cells (a pure function of res, written into the workspace by the call) is
 * scanned.  After a cloud every non-empty cell adds its count to counts and 1 to occupied with INTEGER
 * global atomics.  Plain launches, no floating-point atomics, no workgroup waits for another.  Because every
 * accumulation is an integer addition, the three outputs are bit-identical from call to call, under any permutation
 * of the clouds (cells: row by row) and for any number of workgroups, and sn_occupancy_grid_host -- the same per-point
 * routine (csrc/grid_cell.hpp) compiled for the host, `threads` worker threads sharing the clouds (<= 0: the host
 * Chamfer's default) -- returns the device's bits in all three.
 *
 * SN_EINVAL: res outside 2..32; in_sphere with no cell in the sphere (res = 2: all eight corners lie outside); s or n
 * below 1; s * n above 2^31 - 1; a null xyz; all three outputs null; a workspace smaller than
 * sn_occupancy_grid_workspace_bytes(s, n, res, in_sphere) (which is 0 for arguments that are refused anyway).
 */
size_t sn_occupancy_grid_workspace_bytes(int s, int n, int res, int in_sphere);
int sn_occupancy_grid(const float *xyz, const int *lengths, int s, int n, int res, int in_sphere, long long *counts,
                      int *occupied, int *cells, void *workspace, size_t workspace_bytes, void *stream);
int sn_occupancy_grid_host(const float *xyz, const int *lengths, int s, int n, int res, int in_sphere,
                           long long *counts, int *occupied, int *cells, int threads);

#ifdef __cplusplus
}
#endif

#endif
