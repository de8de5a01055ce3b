/*
 * sparenet_hip_ext_set_emd.h -- the set-level auction EMD of libsparenet_hip.so.
 *
 * Why a third header: the function list of sparenet_hip_ext.h is pinned by the test suite as well (to its two Chamfer
 * entries), so that header stays as it is and a later group of entry points gets a header of its own,
 * include/sparenet_hip_ext_<topic>.h.  The library is the same one; the Python side binds every such header into a
 * registry per topic (sparenet_amd._lib.topic_call("set_emd", name, ...)) through the same checked conversion as the
 * other two headers' calls.  SN_ABI_VERSION is unchanged.
 *
 * The conventions are those of sparenet_hip.h: raw DEVICE pointers, contiguous row-major arrays, sizes in elements,
 * asynchronous launches on `stream`, 0 / positive hipError_t / SN_EINVAL (-22) with a sn_last_error() text.
 * The declarations keep to what the binding's parser reads: one lower-case base type per parameter, `void *stream`
 * last.
 */
#ifndef SPARENET_HIP_EXT_SET_EMD_H
#define SPARENET_HIP_EXT_SET_EMD_H

#include "sparenet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------ set-level EMD
 * The auction of sn_emd_forward_general between EVERY cloud of a set x[nx,n,3] (the bidders) and EVERY cloud of a set
 * y[ny,m,3] (the targets), 1 <= n <= m <= 2048, one workgroup per pair with the whole auction state in LDS:
 *   sums[i,j] = sum over the bidders q of x_i of  (double)sqrtf(dist[q]),
 * dist and the assignment being bit for bit what sn_emd_forward_general(x_i, y_j, 1, n, m, eps, iters) returns (the
 * same bid / window / assign phases, tie key, 1e-6 window, stale window winners, forced assignment in the last
 * iteration; iters == 0 leaves every bidder unassigned, dist 0; eps may be negative).  The terms are added in an order
 * that depends on n alone -- not on nx, ny, m or where a cloud stands in its set -- so two calls give identical bits
 * and sums[i,j] equals the 1 x 1 call on (x_i, y_j).  sums[nx,ny] is float64 and fully overwritten.  assignment, when
 * not null, is int32 [nx,ny,n] and receives every pair's final assignment (-1: unassigned).
 * No workgroup waits for another, there is no global workspace and no floating-point atomic.
 * nx, ny, n, m >= 1; n <= m ("pass the smaller clouds first"); m <= 2048; iters >= 0; nx * ny <= 2^31 - 1, and
 * nx * ny * n <= 2^31 - 1 when assignment is given; a launch of more than 2^22 - 1 pairs is refused as too large.
 * sn_set_emd_lds_bytes: the dynamic LDS a workgroup takes for (n, m); 0 for sizes the kernel does not take. */
size_t sn_set_emd_lds_bytes(int n, int m);
int sn_set_emd_sums(const float *x, const float *y, int nx, int n, int ny, int m, float eps, int iters,
                    double *sums, int *assignment, void *stream);

#ifdef __cplusplus
}
#endif

#endif
