/*
 * ops/rigid_fit.h -- rigid registration, of libsparenet_hip.so: the transform of a cloud under a pose, and the step of an
 * ICP iteration that follows the nearest-neighbour search -- inliers, sums, the rigid update (Horn's closed form, or one
 * point-to-plane Gauss-Newton step), composition and the convergence test -- in two plain launches and without a host
 * synchronisation.  Conventions as in ops/local_pca.h: raw DEVICE pointers (the _host entry points: HOST pointers),
 * contiguous row-major arrays, sizes in elements, asynchronous launches on `stream`, 0 / positive hipError_t / SN_EINVAL
 * (-22) with a sn_last_error() text; one lower-case base type per parameter, `void *stream` last.  SN_ABI_VERSION is
 * unchanged.
 */
#ifndef SPARENET_HIP_OPS_RIGID_FIT_H
#define SPARENET_HIP_OPS_RIGID_FIT_H

#include "../sparenet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------ sn_rigid_apply
 * out[b,i] = s_b * R_b * xyz[b,i] + t_b for the rows i < lengths[b] (null: every row; values are held to [0, n]), 0 for
 * the others.  pose[b,4,4] (double, row-major) holds R in its upper left 3 x 3 block and t in its last column; its last
 * row is not read.  scale[b] (double) may be null, which means 1.  The point is widened to double, every product and sum
 * is rounded separately, left to right, and the result is rounded once to fp32:
 *   out_x = (float)((s * (((R00 * x) + (R01 * y)) + (R02 * z))) + t_x), and likewise out_y, out_z.
 * SN_EINVAL: b or n below 1 (or b above 65535), a null xyz, pose or out.
 */
int sn_rigid_apply(const float *xyz, const double *pose, const double *scale, const int *lengths, int b, int n, float *out,
                   void *stream);
int sn_rigid_apply_host(const float *xyz, const double *pose, const double *scale, const int *lengths, int b, int n,
                        float *out, int threads);

/* ------------------------------------------------------------ sn_rigid_step: one ICP iteration after the search
 * moved[b,n,3] (fp32) is the source under the current pose, as sn_rigid_apply wrote it; dst[b,m,3] (fp32) the target;
 * idx[b,n] (int32) the target row matched to each moved row -- null: row i matches row i, which needs n == m.
 * weight[b,n] (fp32, optional) weighs the rows; dst_normals[b,m,3] (fp32) are the target's normals, required for
 * mode == 1 and not read otherwise; src_lengths[b] / dst_lengths[b] (int32, optional, held to [0, n] / [0, m]) make the
 * batch ragged.  mode: 0 = point-to-point, 1 = point-to-plane.  with_scale (mode 0 only) also fits a scale.
 * max_dist <= 0 means no limit.  In/out: pose[b,4,4], scale[b] and state[b,4], all double; state is {previous rmse,
 * previous fitness, iterations done, frozen (0 or 1)} and starts as four zeros.  Output: stats[b,4] (double) = {rmse,
 * fitness, weight sum W, flags}, flags the sum of SN_RIGID_EMPTY, SN_RIGID_SINGULAR and SN_RIGID_FROZEN.
 * A null pose MEASURES only: stats are written, nothing is solved, scale and state are not read (freeze must be 0).
 *
 * Inliers.  Row i < src_length is an inlier when its match j satisfies 0 <= j < dst_length, both points are finite and,
 * with a limit, d^2 <= max_dist * max_dist, d^2 = ((dx * dx) + (dy * dy)) + (dz * dz) recomputed in double from the two
 * fp32 points (p the moved point, q = dst[b,j], dx = px - qx).  In plane mode the normal of row j must be finite too.
 * Every other row contributes nothing and is never read through; -1 is the "no match" value.  A weight that is negative
 * or not finite is refused by sn_rigid_step_host (SN_EINVAL); the device entry point cannot read it and treats such a
 * row as no inlier.  Without weights w = 1.
 *
 * Measures of this correspondence set.  W = sum w over the inliers, rmse = sqrt((sum w d^2) / W) -- the point distance
 * in both modes --, fitness = inliers / src_length.  With W == 0 (or src_length 0): rmse = fitness = W = 0, flag
 * SN_RIGID_EMPTY, and the update is the identity: pose and scale keep every bit.
 *
 * Convergence, tested before solving.  With freeze != 0, a cloud that is not frozen and has taken at least one step
 * becomes frozen when |rmse - rmse_prev| <= rtol * rmse_prev + atol and |fitness - fitness_prev| <= rtol.  A frozen
 * cloud's pose, scale and state keep every bit in this and every later step; its stats are still written, with flag
 * SN_RIGID_FROZEN.  freeze == 0 is a plain fit that never tests.  A cloud that is not frozen ends the step with
 * state = {rmse, fitness, iterations + 1, 0}.
 *
 * Sums.  All about the pivots a = moved[b,0] and c = dst[b,0] (a pivot with a coordinate that is not finite is (0,0,0)):
 * coordinates are widened to double first, u = p - a, v = q - c, and every product and sum below is rounded separately.
 * Raw coordinates are never accumulated: for a unit-sized cloud at (1000, -2000, 500) that costs eight digits of the
 * rotation.  Mode 0: sum w u (3), sum w v (3), sum (w u) v^T (9), sum w |u|^2.  Mode 1: with r = n . (p - q) and the row
 * J = [u x n, n], the 21 entries of the upper triangle of sum (w J)^T J and the 6 of sum (w J) r.
 * The order of the additions is part of the contract.  The rows of a cloud are cut into chunks of 1024 -- a partition
 * that depends on n alone, not on the batch, the grid or the device.  In a chunk, lane l of 256 adds its rows l, l + 256,
 * l + 512, l + 768 of the chunk in this order from 0.0; the 256 lane sums are added by the workgroup's tree (per 64
 * lanes the xor butterfly over offsets 32, 16 .. 1, which is a balanced binary tree because additions commute; then
 * the four waves in ascending order); the chunks' sums are added in ascending order from 0.0.
 *
 * Point-to-point update (Horn 1987).  mu_p - a = (sum w u) / W, mu_q - c = (sum w v) / W, S = sum (w u) v^T -
 * (sum w u)(mu_q - c)^T, and the symmetric N(S) =
 *   [Sxx+Syy+Szz  Syz-Szy       Szx-Sxz       Sxy-Syx     ]
 *   [.            Sxx-Syy-Szz   Sxy+Syx       Szx+Sxz     ]
 *   [.            .            -Sxx+Syy-Szz   Syz+Szy     ]
 *   [.            .             .            -Sxx-Syy+Szz ].
 * Its eigen-decomposition is the cyclic Jacobi of ops/local_pca.h -- the same skip rule (2^-54) and rotation formulas --
 * over the pairs (0,1), (0,2), (0,3), (1,2), (1,3), (2,3), ended by the first sweep that rotates nothing and after 16
 * sweeps at the latest, whatever the data.  The largest eigenvalue's vector (the lowest index among equal values) is
 * normalised, given the sign that makes q0 >= 0, and turned into R.  R is proper by construction and optimal in the
 * reflection case too, so there is no determinant fix.  With with_scale, s = lambda_max / (sum w |p - mu_p|^2)
 * (Umeyama) where both are positive, else 1.  t = mu_q - s R mu_p.  Where S is rank-deficient (collinear points, one
 * pair) R still attains the minimum but is not unique: no particular minimiser is promised.
 *
 * Point-to-plane update: one Gauss-Newton step.  (sum (w J)^T J) x = -(sum (w J) r) is solved by Cholesky in double; a
 * pivot <= 2^-40 * trace sets SN_RIGID_SINGULAR and makes the update the identity (pose and scale keep every bit), and
 * so does a solution that is not finite.  x = (omega, tau): R is the rotation of the rotation vector omega exactly
 * (through the unit quaternion (cos(|omega|/2), sin(|omega|/2) omega/|omega|), sine and cosine by the library's own
 * routine, the same on host and device), and t = a + tau - R a folds the pivot back.
 *
 * Compose.  pose <- update * pose (R <- R' R, t <- s' R' t + t'), scale <- s' * scale, iterations + 1.
 *
 * Two calls give identical bits, a cloud's result does not depend on its batch, and sn_rigid_step_host -- the same
 * routines (csrc/rigid_solve.hpp) compiled for the host, walking the same tree -- agrees with the device in every bit.
 * No floating-point atomics, no workgroup waits for another, no counters: the chunk sums are one launch, the per-cloud
 * solve a second.  workspace: sn_rigid_step_workspace_bytes(b, n) bytes (one partial per cloud and chunk).
 * SN_EINVAL, each with its own text: b, n or m below 1 (b above 65535); a null moved, dst or stats; a pose without scale
 * and state; freeze without a pose; mode outside {0, 1}; mode 1 without dst_normals; mode 1 with with_scale; a null idx
 * with n != m; a negative rtol or atol; a workspace that is null or too small.
 * The _host twins take `threads` worker threads instead of workspace and stream (<= 0: the host Chamfer's default).
 */
#define SN_RIGID_EMPTY 1
#define SN_RIGID_SINGULAR 2
#define SN_RIGID_FROZEN 4

size_t sn_rigid_step_workspace_bytes(int b, int n);
int sn_rigid_step(const float *moved, const float *dst, const int *idx, const float *weight, const float *dst_normals,
                  const int *src_lengths, const int *dst_lengths, int b, int n, int m, int mode, int with_scale,
                  double max_dist, double rtol, double atol, int freeze, double *pose, double *scale, double *state,
                  double *stats, void *workspace, size_t workspace_bytes, void *stream);
int sn_rigid_step_host(const float *moved, const float *dst, const int *idx, const float *weight, const float *dst_normals,
                       const int *src_lengths, const int *dst_lengths, int b, int n, int m, int mode, int with_scale,
                       double max_dist, double rtol, double atol, int freeze, double *pose, double *scale, double *state,
                       double *stats, int threads);

#ifdef __cplusplus
}
#endif

#endif
