/*
 * ops/dcd.h -- density-aware Chamfer distance (DCD, Wu et al., NeurIPS 2021) of libsparenet_hip.so: everything after the
 * nearest-neighbour search.  Every point's exponential Chamfer term is divided by the number of points that chose the
 * same neighbour, so the value sees density, is bounded in [0, 1] (ratio = 0) and costs a Chamfer call whatever the
 * clouds look like.  Conventions as in ops/swd.h: raw DEVICE pointers (the _host entry point: HOST pointers),
 * contiguous row-major arrays, sizes in elements, asynchronous launches on `stream`, 0 / positive hipError_t /
 * SN_EINVAL (-22) with a sn_last_error() text; one lower-case base type per parameter, `void *stream` last.
 * SN_ABI_VERSION is unchanged.
 */
#ifndef SPARENET_HIP_OPS_DCD_H
#define SPARENET_HIP_OPS_DCD_H

#include "../sparenet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------ the definition
 * xyz1[b,n,3] and xyz2[b,m,3] are the clouds (fp32).  dist1[b,n] / idx1[b,n] are the squared distance and the lowest
 * index of the nearest neighbour of xyz1[i] in xyz2, dist2[b,m] / idx2[b,m] the mirror: what sn_chamfer_forward,
 * sn_chamfer_forward_sorted, sn_chamfer_forward_ragged and sn_chamfer_forward_host write.  lengths1[b] / lengths2[b],
 * when not null, make the batch ragged as in ops/swd.h: n' = min(max(lengths1[i], 0), n) rows of cloud i are its points,
 * m' likewise.  Coordinates and distances of rows past a length are never read (they may hold NaN); their index is -1,
 * as the ragged search leaves it.
 *
 * Counts.  count2[k] = #{i < n' : idx1[i] = k}, count1[i] = #{j < m' : idx2[j] = i} (int32; 0 at padding rows).  A
 * valid row whose index is outside [0, other length) is in no list: its term is 1 and it contributes no gradient.
 * Exponential.  e1_i = sn_expf(-(alpha * dist1_i)): the product rounded to fp32, then negated; sn_expf is the one of
 * include/sn_expf.h, bit-identical on host and device.  e2_j likewise.
 * Weight.  In double, W1 = r1 / p(count2[idx1_i]).  n_lambda must be exactly 0, 0.5 or 1 and no pow is called:
 *   n_lambda = 0: p(c) = 1.0 (the plain exponential Chamfer), 0.5: p(c) = sqrt((double)c), 1: p(c) = (double)c.
 * ratio = 0: r1 = 1.0.  ratio = 1: r1 = (double)n' / (double)m' -- queries over targets, with which an ideal match
 * between clouds of unequal size still reaches 0.  W2 is the mirror, r2 = m' / n'.
 * Loss.  term1_i = 1.0 - (double)e1_i * W1.  L1 = (sum_i term1_i) / n' in double: thread t of 1024 adds the terms
 * i = t, t + 1024, ... in ascending order, the 1024 partial sums are folded by a binary tree with strides 512, 256, ...,
 * 1, one division at the end.  L2 is the mirror.  sides[b,0] = L1, sides[b,1] = L2; the caller's loss is
 * 0.5 * (L1 + L2).  A pair with an empty side gives sides 0, counts 0 and gradients 0.
 * Gradient of 0.5 * (L1 + L2), the counts held constant.  a1_i = (((double)alpha * e1_i) * W1) / n', a2_j the mirror
 * (the 1/2 and the 2 of the squared distance cancel).  gradxyz1[i], per component in double from the fp32 coordinates
 * widened: acc = a1_i * (x_i - y_{idx1_i}), then for the j of x_i's list in ASCENDING j: acc = acc - a2_j * (y_j - x_i);
 * rounded once to fp32.  gradxyz2 is the mirror.  Padding rows get 0.  No floating-point atomics: two calls give
 * identical bits, and the host entry point returns the bits of the device one for every output.
 *
 * sn_dcd_from_search writes sides[b,2] (double) and, where not null, count1[b,n], count2[b,m], gradxyz1[b,n,3] and
 * gradxyz2[b,m,3] (each may be null).  The inverse lists are built once per call and side (integer atomics: count,
 * scan, fill) and give both the counts -- a list's length -- and the gradient's gather; a list is put in ascending
 * order before it is walked: by its owner up to 64 entries, by a workgroup in LDS up to 16384, in place beyond that.
 * Then one launch per step: the per-point terms, the gather, the long lists, the two sums.  Plain launches: no
 * workgroup waits for another, no host read of device data, no device allocation.
 * SN_EINVAL: b, n or m below 1 (or b * (n + m) >= 2^30), alpha not finite or negative, n_lambda not 0 / 0.5 / 1, ratio
 * not 0 / 1, a null required pointer, a workspace smaller than sn_dcd_workspace_bytes(b, n, m).
 *
 * sn_dcd_from_search_host is the same computation on HOST pointers, without a workspace or a stream: `threads` worker
 * threads share the clouds (<= 0: the host Chamfer's default, SN_HOST_THREADS or the hardware's; never more than
 * clouds).
 */
size_t sn_dcd_workspace_bytes(int b, int n, int m);
int sn_dcd_from_search(const float *xyz1, const float *xyz2, const float *dist1, const int *idx1, const float *dist2,
                       const int *idx2, int b, int n, int m, const int *lengths1, const int *lengths2, float alpha,
                       float n_lambda, int ratio, double *sides, int *count1, int *count2, float *gradxyz1,
                       float *gradxyz2, void *workspace, size_t workspace_bytes, void *stream);
int sn_dcd_from_search_host(const float *xyz1, const float *xyz2, const float *dist1, const int *idx1,
                            const float *dist2, const int *idx2, int b, int n, int m, const int *lengths1,
                            const int *lengths2, float alpha, float n_lambda, int ratio, double *sides, int *count1,
                            int *count2, float *gradxyz1, float *gradxyz2, int threads);

#ifdef __cplusplus
}
#endif

#endif
