/*
 * ops/fps.h -- exact farthest point sampling of libsparenet_hip.so.
 *
 * Why a directory: the function lists of sparenet_hip.h, sparenet_hip_ext.h and the set of sparenet_hip_ext_<topic>.h
 * files are each pinned by the test suite, so an operator added from here on declares its entry points in a header of
 * its own, include/ops/<name>.h.  The library is the same one; the Python side binds every header of the directory into
 * a registry per file name (sparenet_amd._lib.op_call("fps", name, ...)) through the same checked conversion as the
 * other headers' calls.  SN_ABI_VERSION is unchanged.
 *
 * The conventions are those of sparenet_hip.h: raw DEVICE pointers, contiguous row-major arrays, sizes in elements,
 * asynchronous launches on `stream`, 0 / positive hipError_t / SN_EINVAL (-22) with a sn_last_error() text.
 * The declarations keep to what the binding's parser reads: one lower-case base type per parameter, `void *stream`
 * last.
 */
#ifndef SPARENET_HIP_OPS_FPS_H
#define SPARENET_HIP_OPS_FPS_H

#include "../sparenet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------ farthest point sampling
 * m picks from each cloud of xyz[b,n,3] (fp32, finite).  lengths[b], when not null, makes the batch ragged: the first
 * len = min(max(lengths[i], 0), n) rows of cloud i are its points, later rows are never read into a result.
 * start[b], when not null, is each cloud's first pick, held to [0, max(len, 1) - 1]; null means 0.
 *   d(p, q)  = ((dx * dx) + (dy * dy)) + (dz * dz), dx = p.x - q.x ..., every product and sum rounded to fp32;
 *   mind[i]  = +inf for every i < len;
 *   pick 0   = start; pick c is recorded as idx[i,k] = c, min_dist[i,k] = mind[c] (so min_dist[i,0] = +inf), then
 *              mind[j] = d(x_j, x_c) < mind[j] ? d(x_j, x_c) : mind[j] for every j < len;
 *   the next pick is the LOWEST index among the maxima of mind.
 * Nothing is special-cased: m may exceed len or the number of distinct points (once every mind is 0 the lowest index
 * repeats), +inf distances are ordinary values.  A cloud with len == 0 gets the row idx = -1, min_dist = NaN.
 * idx[b,m] int32 and min_dist[b,m] fp32 (may be null) are fully overwritten.  Two calls give identical bits, and row i
 * equals the one-cloud call on the cloud's first len rows.
 * One workgroup per cloud, no workgroup waits for another, no atomics.  Clouds of n <= 24576 points (lowered by
 * SN_FPS_RESIDENT_MAX) are held in registers and need no workspace; larger ones keep mind in `workspace`
 * (sn_fps_workspace_bytes(b, n) bytes, 0 for the resident sizes) and give the same bits.
 * b, n, m >= 1; n <= 2^30. */
size_t sn_fps_workspace_bytes(int b, int n);
int sn_fps(const float *xyz, int b, int n, int m, const int *lengths, const int *start, int *idx, float *min_dist,
           void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif
