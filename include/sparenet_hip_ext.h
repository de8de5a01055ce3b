/*
 * sparenet_hip_ext.h -- entry points of libsparenet_hip.so added after the reference's operators were complete.
 *
 * Why a second header: the function list of sparenet_hip.h is pinned by the test suite (the number of prototypes, the
 * number that take a stream, a recorded table of every size export) and SN_ABI_VERSION with it, so that header
 * describes the drop-in boundary and stays as it is.  Operators the reference does not have are declared HERE, and
 * later additions go here too.  The library is the same one; the Python side binds this header into a registry of its
 * own (sparenet_amd._lib.ext_call / ext_workspace) through the same checked conversion as the main header's calls.
 *
 * The conventions are those of sparenet_hip.h: raw DEVICE pointers, contiguous row-major arrays, sizes in elements,
 * asynchronous launches on `stream`, 0 / positive hipError_t / SN_EINVAL (-22) with a sn_last_error() text, a
 * (workspace, workspace_bytes) pair sized by the matching sn_*_workspace_bytes() and defined by one layout function.
 * The declarations keep to what the binding's parser reads: one lower-case base type per parameter,
 * `void *workspace, size_t workspace_bytes` adjacent, `void *stream` last.
 */
#ifndef SPARENET_HIP_EXT_H
#define SPARENET_HIP_EXT_H

#include "sparenet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------- set-level Chamfer
 * One direction of the Chamfer distance between EVERY cloud of a set x[nx,n,3] and EVERY cloud of a set y[ny,m,3]:
 *   sums[i,j] = sum over the points q of x_i of  min over the points t of y_j of  d(q, t),
 * d = (dx*dx + dy*dy) + dz*dz, dx = t - q, the expression of sn_chamfer_forward: each minimum is bit for bit the
 * dist1 that sn_chamfer_forward returns for (x_i, y_j).  The minima are widened to double and added in an order that
 * depends on n alone -- not on nx, ny, m, or where a cloud stands in its set -- so two calls give identical bits and
 * sums[i,j] equals the 1 x 1 call on (x_i, y_j).  sums[nx,ny] is float64 and fully overwritten.  The other direction
 * is the call with the sets swapped.  (MMD-CD, COV-CD and 1-NNA-CD are read off these matrices:
 * sparenet_amd/utils/set_metrics.py.)
 * nx, ny, n, m >= 1; n, m <= 2^20; nx * ny <= 2^31 - 1, and a launch of more than 2^24 workgroups (one per 2048
 * points of an x cloud and 8 y clouds) is refused as too large.  The workspace holds per-block partial sums of clouds of
 * more than 2048 points; sn_set_chamfer_workspace_bytes is 0 for n <= 2048 (workspace may then be null) and for
 * invalid sizes. */
size_t sn_set_chamfer_workspace_bytes(int nx, int ny, int n);
int sn_set_chamfer_sums(const float *x, const float *y, int nx, int n, int ny, int m,
                        double *sums, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif
