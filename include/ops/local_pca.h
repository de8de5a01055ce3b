/*
 * ops/local_pca.h -- local geometry of a neighbourhood, of libsparenet_hip.so: the centroid, covariance and
 * eigen-decomposition of the points an index table names, per query -- normals, a right-handed frame and the three
 * eigenvalues (surface variation).  It is what turns the tables of sn_knn_query / sn_ball_query (ops/neighbors.h) into
 * geometry.  Conventions as in ops/neighbors.h and ops/dcd.h: raw DEVICE pointers (the _host entry point: HOST
 * pointers), contiguous row-major arrays, sizes in elements, asynchronous launches on `stream`, 0 / positive hipError_t
 * / SN_EINVAL (-22) with a sn_last_error() text; one lower-case base type per parameter, `void *stream` last.
 * SN_ABI_VERSION is unchanged.
 */
#ifndef SPARENET_HIP_OPS_LOCAL_PCA_H
#define SPARENET_HIP_OPS_LOCAL_PCA_H

#include "../sparenet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------ the definition
 * xyz[b,n,3] (fp32) are the points, idx[b,m,k] (int32, 1 <= k <= 64) the table sn_knn_query or sn_ball_query wrote for
 * m queries per cloud.  Slot t of a query is VALID when 0 <= idx < n.  -1 is an empty slot and is skipped; any other
 * value outside [0, n) is the caller's error, is skipped as well and never read through.  A repeated index counts as
 * often as it occurs (so take sn_ball_query's table with pad_first == 0).  c is the number of valid slots, p_t their
 * points in slot order.  Coordinates are widened to double and everything below is double: every product, sum and
 * quotient separately rounded, no contraction.
 *
 * Centroid.  mu = (p_1 + p_2 + ... + p_c) / c per component, the sum from 0.0 left to right, one division.
 * Covariance.  d_t = p_t - mu; Cxx = ((dx_1 * dx_1) + (dx_2 * dx_2) + ...) / c from 0.0 left to right, and likewise Cxy
 * (dx * dy), Cxz (dx * dz), Cyy, Cyz (dy * dz), Czz: six entries, one division each.
 *
 * Eigen-decomposition: cyclic Jacobi.  A = C, V = I.  A sweep visits the pairs (p, q) = (0,1), (0,2), (1,2) in this
 * order.  At a pair: when |A_pq| <= 2^-54 * (|A_pp| + |A_qq|) the entry is set to 0.0 and nothing else changes.
 * Otherwise, with r the third index,
 *   theta = (A_qq - A_pp) / (2.0 * A_pq),  t = 1.0 / (|theta| + sqrt(theta * theta + 1.0)), negated where theta < 0,
 *   co = 1.0 / sqrt(t * t + 1.0),  s = t * co,  tau = s / (1.0 + co),  h = t * A_pq,
 *   A_pp = A_pp - h,  A_qq = A_qq + h,  A_pq = 0.0,
 *   A_rp, A_rq = A_rp - s * (A_rq + tau * A_rp),  A_rq + s * (A_rp - tau * A_rq)      (from the old pair),
 *   and the same pair update for V_jp, V_jq of every row j of V.
 * The sweeps end after the first one in which all three pairs met the "set to 0.0" branch, and after 12 sweeps at the
 * latest, whatever the data: no lane can spin.  (Convergence is quadratic: covariances with axis ratios up to 10^12
 * take at most 4 rotating sweeps and the one that finds nothing to do.)  The eigenvalues are A's diagonal, the
 * eigenvector of A_jj is column j of V; they are put in ascending order of the eigenvalue by the exchanges (0,1), (1,2),
 * (0,1), each made when the later value is strictly smaller.
 *
 * Signs.  The CANONICAL sign of a vector makes its component of largest magnitude positive; equal magnitudes go to the
 * lowest axis.  e2, the eigenvector of the largest eigenvalue (the principal direction), gets the canonical sign.  e0,
 * the NORMAL, gets the canonical sign; with a viewpoint it is then negated when
 *   ((e0x * (vx - qx)) + (e0y * (vy - qy))) + (e0z * (vz - qz)) < 0.0,
 * v = viewpoint[b,3] and q = new_xyz[b,m,3] the query point, both widened: the normal then looks at the viewpoint, and a
 * product of exactly 0 keeps the canonical sign.  e1 = e2 x e0, so the frame is right-handed.  0.0 is added to every
 * component at the end, so a zero is +0.0.
 *
 * Outputs (each may be null, but not all three).  eigenvalues[b,m,3] (double), ascending.  frames[b,m,3,3] (fp32, each
 * component rounded once from double): row r is the unit eigenvector e_r.  normals[b,m,3] (fp32) is row 0.
 * Where eigenvalues coincide the eigenvectors are an orthonormal basis of the eigenspace and no particular one.
 * c == 0: eigenvalues, frame and normal are all 0.  c == 1 (and c copies of one point): the eigenvalues are exactly 0,
 * because every p_t - mu is, and the frame is the identity.
 *
 * One query lives in one lane; a workgroup's idx rows are one contiguous block that is loaded coalesced into LDS with an
 * odd row pitch and read from there; the points are gathered from global memory twice (centroid, covariance); the
 * solver runs in registers.  Plain launches: no atomics, no workgroup waits for another, no [b,m,k,3] intermediate, no
 * workspace -- sn_local_pca_workspace_bytes is 0 for every shape and `workspace` may be null.  Two calls give identical
 * bits, and row i of cloud b equals the one-cloud call on that cloud.
 * SN_EINVAL: b, n or m below 1 (or b * m > 2^30), k outside 1..64, a null xyz or idx, all three outputs null, a
 * viewpoint without new_xyz, a workspace smaller than sn_local_pca_workspace_bytes(b, n, m, k).
 *
 * sn_local_pca_host is the same computation on HOST pointers -- the same routine (csrc/eig3.hpp) compiled for the
 * host -- without a workspace or a stream: `threads` worker threads share the clouds (<= 0: the host Chamfer's
 * default, SN_HOST_THREADS or the hardware's; never more than clouds).
 */
size_t sn_local_pca_workspace_bytes(int b, int n, int m, int k);
int sn_local_pca(const float *xyz, const int *idx, int b, int n, int m, int k, const float *new_xyz,
                 const float *viewpoint, double *eigenvalues, float *frames, float *normals, void *workspace,
                 size_t workspace_bytes, void *stream);
int sn_local_pca_host(const float *xyz, const int *idx, int b, int n, int m, int k, const float *new_xyz,
                      const float *viewpoint, double *eigenvalues, float *frames, float *normals, int threads);

#ifdef __cplusplus
}
#endif

#endif
