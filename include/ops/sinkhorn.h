/*
 * ops/sinkhorn.h -- entropic optimal transport (Sinkhorn) between two clouds, of libsparenet_hip.so: the dual
 * potentials of a log-domain Sinkhorn loop and the barycentric maps its gradient needs.  Conventions as in
 * ops/neighbors.h: raw DEVICE pointers, contiguous row-major arrays, sizes in elements, asynchronous launches on
 * `stream`, 0 / positive hipError_t / SN_EINVAL (-22) with a sn_last_error() text; one lower-case base type per
 * parameter, `void *stream` last.  SN_ABI_VERSION is unchanged.
 */
#ifndef SPARENET_HIP_OPS_SINKHORN_H
#define SPARENET_HIP_OPS_SINKHORN_H

#include "../sparenet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------ the definition
 * x[b,n,3] and y[b,m,3] are the clouds (fp32, finite).  x_lengths[b] / y_lengths[b], when not null, make the batch
 * ragged as in ops/neighbors.h: the first len = min(max(lengths[i], 0), size) rows of cloud i are its points, later
 * rows are never read into a result.  The weights are uniform: a_i = 1 / len_x, b_j = 1 / len_y.
 *   C_ij = ((dx * dx) + (dy * dy)) + (dz * dz), dx = y_j.x - x_i.x ..., every product and sum rounded to fp32, no
 *   contraction: the SQUARED distance, as Chamfer's, without a factor 1/2.
 * Schedule: eps_t = max(eps, eps_start * decay^t), computed on the host in double from the fp32 arguments and rounded
 * to fp32 -- decay acts on eps itself; eps_start <= 0 means the constant eps.  eps > 0 and finite, 0 < decay < 1,
 * iters >= 1.
 * Iteration: g = 0 (warm_start != 0: the caller's g, rows j < len_y), then for t = 0 .. iters - 1 with e = eps_t
 *   f_i = -e * log sum_{j < len_y} exp( log b_j + (g_j - C_ij) / e )     for i < len_x
 *   g_j = -e * log sum_{i < len_x} exp( log a_i + (f_i - C_ij) / e )     for j < len_y
 * f[b,n] and g[b,m] are fully overwritten; padding rows are 0, and a cloud pair with len_x == 0 or len_y == 0 gives
 * f = g = 0 -- nothing in it is NaN.  The value is OT_eps = sum_i a_i f_i + sum_j b_j g_j (the dual objective; exact
 * for the plan, whose mass is 1 because g is updated last); the caller takes the sums.
 *
 * sn_sinkhorn_solve enqueues its 2 * iters launches on `stream` and returns: no synchronisation, no device
 * allocation, no host read of device data.
 *
 * sn_sinkhorn_barycenter is one softmin of the queries q[b,n,3] over the targets t[b,m,3] with the targets' potential
 * t_potential[b,m] at `eps`:
 *   w_ij       = softmax_{j < len_t}( log(1 / len_t) + (t_potential_j - C_ij) / eps )
 *   bary[b,n,3] = sum_j w_ij t_j;   softmin[b,n] (may be null) = the update of the iteration above for the same input.
 * Padding rows and pairs with an empty side give 0.  The last-iterate (envelope) gradient of the value is
 *   dOT/dx_i = a_i * 2 * (x_i - bary_x[i])   (q = x, t = y, t_potential = g)
 *   dOT/dy_j = b_j * 2 * (y_j - bary_y[j])   (q = y, t = x, t_potential = f);
 * nothing is differentiated through the loop.
 *
 * A query lives in one lane, the targets and their potential stream through LDS, the sum is kept against a running
 * maximum (clouds far apart relative to eps are fine).  Where b * n is too small to fill the device each query's
 * target range is split into S contiguous segments walked by S waves and merged in LDS in segment order
 * (SN_SINKHORN_SPLIT=<S> forces S, 1 = never split).  Two calls give identical bits; bits may differ between split
 * widths.  Each half-iteration costs O(n * m) whatever the data.  No floating-point atomics, no workgroup waits for
 * another, no [b,n,m] intermediate.  No workspace is needed as built: sn_sinkhorn_workspace_bytes is 0 for every shape
 * and `workspace` may be null.  b, n, m >= 1; n, m <= 2^30. */
size_t sn_sinkhorn_workspace_bytes(int b, int n, int m);
int sn_sinkhorn_solve(const float *x, const float *y, int b, int n, int m, const int *x_lengths, const int *y_lengths,
                      float eps, float eps_start, float decay, int iters, int warm_start, float *f, float *g,
                      void *workspace, size_t workspace_bytes, void *stream);
int sn_sinkhorn_barycenter(const float *q, const float *t, const float *t_potential, int b, int n, int m,
                           const int *q_lengths, const int *t_lengths, float eps, float *bary, float *softmin,
                           void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif
