/*
 * ops/swd.h -- sliced Wasserstein distance between two clouds, of libsparenet_hip.so: both clouds are projected onto
 * L directions, every 1-D projection is sorted, the 1-D transport problem is solved exactly and the caller averages the
 * L costs.  O((n + m) log^2) per slice whatever the clouds look like.  Conventions as in ops/sinkhorn.h: raw DEVICE
 * pointers, contiguous row-major arrays, sizes in elements, asynchronous launches on `stream`, 0 / positive hipError_t /
 * SN_EINVAL (-22) with a sn_last_error() text; one lower-case base type per parameter, `void *stream` last.
 * SN_ABI_VERSION is unchanged.
 */
#ifndef SPARENET_HIP_OPS_SWD_H
#define SPARENET_HIP_OPS_SWD_H

#include "../sparenet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------ the definition
 * x[b,n,3] and y[b,m,3] are the clouds (fp32, finite).  dirs[1 or b, slices, 3] are the fp32 directions, used as given
 * (normalising is the caller's job): dirs_per_cloud == 0 -- one set shared by every cloud, != 0 -- cloud i uses
 * dirs[i].  x_lengths[b] / y_lengths[b], when not null, make the batch ragged as in ops/sinkhorn.h: the first
 * len = min(max(lengths[i], 0), size) rows of cloud i are its points, later rows are never read into a result.
 * p is 1 or 2.  1 <= n, m <= 16384 (one workgroup holds a whole cloud's records in LDS), b, slices >= 1.
 *
 * Projection.  px_i = ((x.x * t.x) + (x.y * t.y)) + (x.z * t.z) for the direction t, every product and sum rounded to
 * fp32, no contraction.
 * Order.  Ascending by projection value; equal values -- -0.0 equals +0.0 -- by ascending point index: the order of
 * np.argsort(kind="stable") on the fp32 projections.  perm[rank] = original index, sorted[rank] = that point's
 * projection (a zero keeps its sign).
 * 1-D transport.  Uniform weights 1/n' and 1/m' (n', m' the valid lengths).  In units of 1/(n' m') sorted atom i of x
 * carries the mass interval [i m', (i+1) m'), sorted atom j of y carries [j n', (j+1) n'); the plan moves
 *   w_ij = min((i+1) m', (j+1) n') - max(i m', j n')      (an exact integer, <= 2^28)
 * between them where that is positive, which is for j in [floor(i m' / n'), ceil((i+1) m' / n')): n' + m' - gcd(n', m')
 * terms.
 * Cost.  cost[b,l] = (sum_i t_i) / (n' m'),  t_i = sum_j w_ij |sx_i - sy_j|^p  (p = 2: w * (d * d)), in double from
 * the fp32 projections widened to double, every product and sum rounded separately: t_i over ascending j; the t_i added
 * per thread over i = thread, thread + 1024, ... and the 1024 partial sums by a binary tree; one division at the end.
 * The order is fixed by (n', m') alone, so two calls give identical bits.  An empty side gives cost 0.
 * Gradient of the MEAN over the slices.  c_il = (sum_j w_ij g(sx_i - sy_j)) / (n' m') with g(d) = 2 d (p = 2) or
 * sign(d) (p = 1, sign(0) = 0), in double over ascending j, rounded once to fp32.  Then
 *   gradx[b, perm_l[i], :] = (sum_l c_il * dirs_l) * (1 / slices)
 * accumulated in fp32 from 0 in ascending l, products and sums rounded separately, 1 / slices the fp32 quotient.  grady
 * is the mirror image (the roles of the clouds swapped: d = sy_j - sx_i).  Padding rows, and every row of a pair with an
 * empty side, get 0 -- nothing is NaN.  No floating-point atomics: inside a slice the permutation makes every write
 * unique, across slices one kernel sums in slice order.
 *
 * sn_swd_forward writes cost[b, slices] (double) and, where not null, gradx[b,n,3] / grady[b,m,3] (either or both may
 * be null: the value only).  The slices are processed in chunks of c, so the workspace is O(b * c * (n + m)) and does
 * not grow with `slices` beyond c: c = min(slices, max(1, 512 / b)), or SN_SWD_CHUNK=<c> (held to [1, slices]).  Results
 * are bit-identical for every chunk width.  Per chunk: one launch that projects and sorts (one workgroup per cloud,
 * slice and side), one for the transport (one rank per lane), one per side that adds the chunk's slices to the gradient.
 * Plain launches: no workgroup waits for another, no host read of device data, no device allocation.
 *
 * sn_swd_project_sort is the first of those launches alone, for one batch of clouds: sorted[b, slices, n] and
 * perm[b, slices, n]; ranks past a cloud's length hold +inf and -1.  The same device code as the forward.
 */
size_t sn_swd_workspace_bytes(int b, int n, int m, int slices);
int sn_swd_forward(const float *x, const float *y, const float *dirs, int b, int n, int m, int slices,
                   int dirs_per_cloud, const int *x_lengths, const int *y_lengths, int p, double *cost, float *gradx,
                   float *grady, void *workspace, size_t workspace_bytes, void *stream);
int sn_swd_project_sort(const float *x, const float *dirs, int b, int n, int slices, int dirs_per_cloud,
                        const int *lengths, float *sorted, int *perm, void *stream);

#ifdef __cplusplus
}
#endif

#endif
