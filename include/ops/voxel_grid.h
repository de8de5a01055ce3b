/*
 * ops/voxel_grid.h -- voxel-grid subsampling and pooling of libsparenet_hip.so: every point of a cloud goes to a cell
 * of a regular lattice, every occupied cell gives one output point (the centroid of its members) and one pooled feature
 * column, and every input point learns which output it went to.  One sort and one reduction per cloud, O(n log^2 n)
 * whatever the cloud looks like: no chain of dependent picks (ops/fps.h, sn_mds).  Conventions as in ops/occupancy.h:
 * raw DEVICE pointers (the _host entry points: HOST pointers), contiguous row-major arrays, sizes in elements,
 * asynchronous launches on `stream`, 0 / positive hipError_t / SN_EINVAL (-22) with a sn_last_error() text; one
 * lower-case base type per parameter, `void *stream` last.  SN_ABI_VERSION is unchanged.
 */
#ifndef SPARENET_HIP_OPS_VOXEL_GRID_H
#define SPARENET_HIP_OPS_VOXEL_GRID_H

#include "../sparenet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------ the definition
 * The cell of a point.  `size` (fp32, finite, > 0) is the edge of a cell, origin[3] (fp32, finite) a corner of cell
 * (0, 0, 0).  `origin` is a HOST pointer to 3 floats in every entry point, the device ones included, or null for zeros.
 * Per axis
 *     q = ((double)x - (double)o) / (double)size,        c = floor(q):
 * a subtraction and a division in IEEE double, each rounded separately, the division correctly rounded -- no
 * reciprocal, no contraction.  The cell is defined by the ROUNDED quotient: were the exact quotient to lie just below
 * an integer and round to it, the point would belong to the upper cell (with a dyadic size and moderate coordinates
 * q is exact).  -0.0 goes to cell 0.  A point belongs to NO voxel when a coordinate is NaN or infinite, or
 * when some c lies outside [-32768, 32767]; such a point has inverse = -1 and is counted nowhere.
 * The key of a cell is ((cx + 32768) << 32) | ((cy + 32768) << 16) | (cz + 32768).  The voxels of a cloud are its
 * occupied cells in ascending key order (x slowest); the points inside a voxel are ordered by ascending point index.
 *
 * The batch.  xyz[b,n,3] fp32.  lengths[b] (int32, may be null: every cloud has n points) makes the batch ragged: cloud
 * i is its first min(max(lengths[i], 0), n) rows -- held to that range on the device before it indexes anything -- and
 * later rows are never read.  A cloud of length 0 has count 0.
 *
 * Outputs, per cloud, at the width cap (1 <= cap <= n).  Each may be null except count; each is written whole, so
 * nothing has to be cleared beforehand.  kept = min(count, cap).
 *   count[b]          int32  the number of occupied voxels, NOT clipped to cap: a caller sees truncation at once.
 *   centroid[b,cap,3] fp32   per axis the sum of the members' (double)x in ascending point index, one addition at a
 *                            time from 0.0, divided by the member count in double, rounded once to fp32.  Rows at and
 *                            beyond kept are 0.0.
 *   members[b,cap]    int32  the member count; 0 at and beyond kept.
 *   first[b,cap]      int32  the lowest point index of the voxel; -1 at and beyond kept.
 *   inverse[b,n]      int32  the rank of each point's voxel; -1 for padding rows, points in no voxel and points of a
 *                            voxel whose rank is >= cap.
 *   order[b,n]        int32  the indices of all points that have a voxel (dropped voxels included), sorted by
 *                            (key, index); then -1.
 *   start[b,cap+1]    int32  CSR offsets into order: voxel k < kept is order[start[k] .. start[k+1]); entries at and
 *                            beyond kept repeat the end of the last kept voxel.
 *
 * Pooling.  sn_voxel_pool reads features[b,c,n] fp32 and a grid's order, start, count and cap, and writes out[b,c,cap]
 * and, where not null, argmax[b,c,cap] int32.  The members of slot v < min(count, cap) are the entries of
 * order[start[v] .. start[v+1]) that are point indices (in [0, n); offsets are held to [0, n] and any other entry is
 * skipped, so arrays that did not come from sn_voxel_grid cannot make it read out of bounds), in that order.
 *   mode 0, sum / mode 1, mean:  the sum of (double)f over the members one addition at a time (mean: divided by their
 *                                number in double), rounded once.
 *   mode 2, max:                 the first member is taken; a later member replaces it when v > best, so the lowest
 *                                index wins among equals (a NaN is kept only where it comes first).  argmax records
 *                                the point index (the other modes write -1 there).
 * A slot without members is 0.0 / -1.
 *
 * Guarantees.  Every output is a fixed function of the inputs: bit-identical from call to call, for every launch size
 * (SN_VOXEL_BLOCKS=<workgroups> forces one) and on both kernel paths; row i of a batch equals the one-cloud call on
 * cloud i's first len rows; the _host entry points (the same per-point and per-voxel routines, csrc/voxel_cell.hpp,
 * compiled for the host; `threads` workers share the clouds, <= 0: the host Chamfer's default) return the device's bits
 * in every output.  No floating-point atomics, no workgroup waits for another, every launch is a plain launch.
 *
 * Two paths.  n <= 16384: one workgroup of 1024 lanes per cloud (it loops when b exceeds the launch) builds one 64-bit
 * record ((key << 14) | index) + 2^52 per point in LDS (a positive, finite, normal double: the sort's compare-exchange is
 * a floating-point minimum and maximum), sorts them there, finds the voxels' heads, ranks them with a workgroup
 * scan, and one lane per kept voxel walks its segment in index order: no workspace
 * (sn_voxel_grid_workspace_bytes(b, n) is 0).  16384 < n <= 16777216 (2^24), or n above SN_VOXEL_RESIDENT_MAX, which
 * only lowers the threshold: chunks of the resident size are sorted in LDS and written to `workspace` as separate key
 * and index arrays, merged by stable passes (on equal keys the lower run wins, which keeps ascending index order), and
 * the same head / rank / reduce code runs over the merged arrays.
 *
 * SN_EINVAL: size not finite or not > 0; a non-finite origin; b, n, c or cap below 1; cap > n; b * n above 2^31 - 1;
 * n above 2^24; a null xyz or count (pool: features, order, start, count or out); a workspace smaller than
 * sn_voxel_grid_workspace_bytes(b, n) (which is 0 for arguments that are refused anyway); a pooling mode outside 0..2.
 */
size_t sn_voxel_grid_workspace_bytes(int b, int n);
int sn_voxel_grid(const float *xyz, const int *lengths, int b, int n, float size, const float *origin, int cap,
                  int *count, float *centroid, int *members, int *first, int *inverse, int *order, int *start,
                  void *workspace, size_t workspace_bytes, void *stream);
int sn_voxel_grid_host(const float *xyz, const int *lengths, int b, int n, float size, const float *origin, int cap,
                       int *count, float *centroid, int *members, int *first, int *inverse, int *order, int *start,
                       int threads);
int sn_voxel_pool(const float *features, int b, int c, int n, const int *order, const int *start, const int *count,
                  int cap, int mode, float *out, int *argmax, void *stream);
int sn_voxel_pool_host(const float *features, int b, int c, int n, const int *order, const int *start,
                       const int *count, int cap, int mode, float *out, int *argmax, int threads);

#ifdef __cplusplus
}
#endif

#endif
