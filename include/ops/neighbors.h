/*
 * ops/neighbors.h -- neighbourhood queries between two clouds and the gathers over their result, of
 * libsparenet_hip.so: k nearest neighbours and ball query in xyz, grouping, weighted interpolation and the backward of
 * both.  These are the operators PointNet++-style code imports beside furthest_point_sample (ops/fps.h) and
 * gather_operation.  Conventions as in ops/fps.h: raw DEVICE pointers, contiguous row-major arrays, sizes in elements,
 * asynchronous launches on `stream`, 0 / positive hipError_t / SN_EINVAL (-22) with a sn_last_error() text; one
 * lower-case base type per parameter, `void *stream` last.  SN_ABI_VERSION is unchanged.
 */
#ifndef SPARENET_HIP_OPS_NEIGHBORS_H
#define SPARENET_HIP_OPS_NEIGHBORS_H

#include "../sparenet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------ the two searches
 * xyz[b,n,3] are the points searched, new_xyz[b,m,3] the queries (fp32, finite).  lengths[b] / new_lengths[b], when
 * not null, make the batch ragged as in ops/fps.h: the first len = min(max(lengths[i], 0), n) rows of cloud i are its
 * points (len_q of new_lengths and m: its queries), later rows are never read into a result.
 *   d(q, t) = ((dx * dx) + (dy * dy)) + (dz * dz), dx = t.x - q.x ..., every product and sum rounded to fp32, no
 *   contraction; +inf from overflow is an ordinary value.
 *
 * sn_knn_query, 1 <= k <= 32: row i of idx[b,m,k] (int32) and dist2[b,m,k] (fp32, may be null) holds the k smallest
 * pairs (d, j), j < len, in ascending lexicographic order -- equal distances are ordered by the lower index.  Slots
 * beyond len get idx -1, dist2 +inf; so does every slot of a padding query (i >= len_q).
 *
 * sn_ball_query, nsample >= 1, radius >= 0 and finite: r2 = radius * radius rounded to fp32; the hits of query i are
 * the j < len with d < r2 (strict), taken in ascending j.  The first min(hits, nsample) hits fill the first slots of
 * row i of idx[b,m,nsample]; cnt[b,m] (int32, may be null) is min(hits, nsample).  The remaining slots repeat the
 * first hit with pad_first != 0 (the PointNet++ convention) and are -1 with pad_first == 0 (the PyTorch3D one).  A
 * query without a hit, and a padding query, gets -1 in every slot and cnt 0 under both conventions.
 *
 * Both are bit-reproducible and independent of the batch: two calls give identical bits, and row i of cloud b equals
 * the one-cloud call on that cloud's first len rows.  A query lives in one lane, the targets stream through LDS; where
 * b * m is too small to fill the device each query's target range is split into S contiguous segments searched by S
 * waves and merged in LDS (SN_NEIGHBORS_SPLIT=<S> forces S, 1 = never split) -- the same bits by the rule.  No
 * workgroup waits for another, no atomics, no [b,m,n] intermediate.
 * Neither search needs a workspace as built: sn_neighbors_workspace_bytes is 0 for every shape (k is k or nsample),
 * and `workspace` may be null.  b, n, m >= 1; n, m <= 2^30. */
size_t sn_neighbors_workspace_bytes(int b, int n, int m, int k);
int sn_knn_query(const float *xyz, const float *new_xyz, int b, int n, int m, int k, const int *lengths,
                 const int *new_lengths, int *idx, float *dist2, void *workspace, size_t workspace_bytes, void *stream);
int sn_ball_query(const float *xyz, const float *new_xyz, int b, int n, int m, float radius, int nsample, int pad_first,
                  const int *lengths, const int *new_lengths, int *idx, int *cnt, void *workspace,
                  size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------ gathers over idx[b,m,s] and their backward
 * features[b,c,n] fp32.  An index of -1 is an empty slot; any other index outside [0, n) is the caller's error and is
 * treated as sn_gather_forward / sn_gather_backward treat it: NaN in a forward, skipped in the backward, never read.
 *
 * sn_group_forward: out[b,c,m,s] = features[b,c,idx[b,m,s]], 0.0 at an empty slot.
 * sn_interpolate_forward, weight[b,m,s]: out[b,c,m] = (((w0 * f0) + (w1 * f1)) + (w2 * f2)) + ..., every product and
 * sum rounded to fp32, slots left to right, an empty slot skipped (0.0 when every slot is empty) -- bit-equal to that
 * expression for any s >= 1.
 *
 * sn_group_backward: grad_features[b,c,j] = the sum over every slot (i, t) with idx[b,i,t] == j of
 *   grad_out[b,c,i,t]                     weight == null (grouping; grad_out is [b,c,m,s])
 *   weight[b,i,t] * grad_out[b,c,i]       weight != null (interpolation; grad_out is [b,c,m])
 * grad_features is fully overwritten, with 0 where nothing arrives.  No floating-point atomics: the slot lists are
 * inverted once per call for all channels (count, scan, fill with integer atomics), then one thread per (b, c, j) adds
 * its list.  The order inside a list is not fixed, so the backward is accurate to the bound of a recursive fp32 sum of
 * the list's terms, NOT bit-reproducible.  A list may have any length (all m * s slots on one target is legal).
 * workspace: sn_group_backward_workspace_bytes(b, n, m, s) bytes.  b, c, n, m, s >= 1; n, m * s <= 2^30. */
int sn_group_forward(const float *features, const int *idx, int b, int c, int n, int m, int s, float *out,
                     void *stream);
int sn_interpolate_forward(const float *features, const int *idx, const float *weight, int b, int c, int n, int m,
                           int s, float *out, void *stream);
size_t sn_group_backward_workspace_bytes(int b, int n, int m, int s);
int sn_group_backward(const float *grad_out, const int *idx, const float *weight, int b, int c, int n, int m, int s,
                      float *grad_features, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif
