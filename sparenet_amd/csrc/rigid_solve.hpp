// rigid_solve.hpp -- the arithmetic of rigid_fit.hip, written once for host and device (as eig3.hpp is for local_pca.hip):
// what one correspondence adds to the sums, the fixed-order sums themselves, Horn's closed form (cyclic Jacobi on the
// symmetric 4 x 4 matrix), the point-to-plane Gauss-Newton step (Cholesky, Rodrigues), the convergence test and the
// composition.  include/ops/rigid_fit.h states the rule; every line below is one of its sentences.  All double, nothing
// contracted (the build has -ffp-contract=off), and no library sine or cosine: host and device give the same bits.
// Arrays are indexed by compile-time values only (every loop over them has constant bounds and is unrolled).
#pragma once
#include <cmath>

namespace rigid {

constexpr int kThreads = 256;             // lanes of a chunk's workgroup
constexpr int kTrips = 4;                 // rows per lane
constexpr int kChunk = kThreads * kTrips; // rows of a chunk: the partition of a cloud's rows depends on n alone
constexpr int kWaveLanes = 64;
constexpr int kMaxSweeps = 16;            // the data-independent bound on the Jacobi solver
constexpr double kSkip = 0x1p-54;         // |A_pq| <= kSkip * (|A_pp| + |A_qq|): the entry is set to 0, no rotation
constexpr double kPivot = 0x1p-40;        // a Cholesky pivot <= kPivot * trace: singular
constexpr double kMaxAngle = 0x1p20;      // a Gauss-Newton rotation vector this long (or not finite): singular

// what a chunk adds up: W, the inlier count, sum w d^2, then the mode's own sums
constexpr int kHead = 3;
constexpr int kPointSums = kHead + 16;    // sum w(p-a) [3], sum w(q-c) [3], sum w(p-a)(q-c)^T [9], sum w|p-a|^2
constexpr int kPlaneSums = kHead + 27;    // J^T J (upper triangle, row-major) [21], J^T r [6]
constexpr int kStride = 32;               // doubles per chunk partial in the workspace, both modes
template <int kMode>
constexpr int sums_of() { return kMode == 0 ? kPointSums : kPlaneSums; }

constexpr int kFlagEmpty = 1, kFlagSingular = 2, kFlagFrozen = 4;

__host__ __device__ inline int chunks_of(int n) { return (n + kChunk - 1) / kChunk; }

struct Problem {
  const float *moved;        // [b, n, 3]
  const float *dst;          // [b, m, 3]
  const int *idx;            // [b, n] or null (row i matches row i)
  const float *weight;       // [b, n] or null
  const float *normals;      // [b, m, 3] or null
  const int *src_lengths, *dst_lengths;
  int n, m;
  double max2;               // max_dist squared; <= 0: no limit
};

struct Pivots {
  double ax, ay, az, cx, cy, cz;
};

__host__ __device__ inline bool finite3(const float *p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }

// a = moved[b, 0], c = dst[b, 0]; a pivot with a coordinate that is not finite is (0, 0, 0)
__host__ __device__ inline Pivots pivots_of(const Problem &P, long cloud) {
  const float *a = P.moved + cloud * P.n * 3, *c = P.dst + cloud * P.m * 3;
  Pivots v{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (finite3(a)) v.ax = (double)a[0], v.ay = (double)a[1], v.az = (double)a[2];
  if (finite3(c)) v.cx = (double)c[0], v.cy = (double)c[1], v.cz = (double)c[2];
  return v;
}

// Row i of `cloud`: where it is an inlier, its terms are added to acc (sums_of<kMode>() doubles), each product and sum
// rounded separately; every other row adds nothing and is not read through.
template <int kMode>
__host__ __device__ inline void add_row(const Problem &P, long cloud, int i, int dst_len, const Pivots &v, double *acc) {
  const long row = cloud * P.n + i;
  const int j = P.idx ? P.idx[row] : i;
  if (j < 0 || j >= dst_len) return;
  const float *pf = P.moved + row * 3, *qf = P.dst + (cloud * P.m + j) * 3;
  if (!finite3(pf) || !finite3(qf)) return;
  const double px = (double)pf[0], py = (double)pf[1], pz = (double)pf[2];
  const double qx = (double)qf[0], qy = (double)qf[1], qz = (double)qf[2];
  const double dx = px - qx, dy = py - qy, dz = pz - qz;
  const double d2 = ((dx * dx) + (dy * dy)) + (dz * dz);
  if (P.max2 > 0.0 && !(d2 <= P.max2)) return;
  double w = 1.0;
  if (P.weight) {
    const float wf = P.weight[row];
    if (!(wf >= 0.0f) || !std::isfinite(wf)) return;      // the entry points refuse these where they can read them
    w = (double)wf;
  }
  const double ux = px - v.ax, uy = py - v.ay, uz = pz - v.az;
  if (kMode == 0) {
    acc[0] = acc[0] + w, acc[1] = acc[1] + 1.0, acc[2] = acc[2] + w * d2;
    const double vx = qx - v.cx, vy = qy - v.cy, vz = qz - v.cz;
    const double wx = w * ux, wy = w * uy, wz = w * uz;
    acc[3] = acc[3] + wx, acc[4] = acc[4] + wy, acc[5] = acc[5] + wz;
    acc[6] = acc[6] + w * vx, acc[7] = acc[7] + w * vy, acc[8] = acc[8] + w * vz;
    acc[9] = acc[9] + wx * vx, acc[10] = acc[10] + wx * vy, acc[11] = acc[11] + wx * vz;
    acc[12] = acc[12] + wy * vx, acc[13] = acc[13] + wy * vy, acc[14] = acc[14] + wy * vz;
    acc[15] = acc[15] + wz * vx, acc[16] = acc[16] + wz * vy, acc[17] = acc[17] + wz * vz;
    acc[18] = acc[18] + w * (((ux * ux) + (uy * uy)) + (uz * uz));
  } else {
    const float *nf = P.normals + (cloud * P.m + j) * 3;
    if (!finite3(nf)) return;
    acc[0] = acc[0] + w, acc[1] = acc[1] + 1.0, acc[2] = acc[2] + w * d2;
    const double nx = (double)nf[0], ny = (double)nf[1], nz = (double)nf[2];
    const double r = ((nx * dx) + (ny * dy)) + (nz * dz);
    const double J[6] = {uy * nz - uz * ny, uz * nx - ux * nz, ux * ny - uy * nx, nx, ny, nz};
    int at = kHead;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      const double wj = w * J[a];
#pragma unroll
      for (int c = a; c < 6; ++c) acc[at] = acc[at] + wj * J[c], ++at;
      acc[kHead + 21 + a] = acc[kHead + 21 + a] + wj * r;
    }
  }
}

// ------------------------------------------------------------------------------------------------ the two solvers
struct Update {
  double r[9];      // row-major, a proper rotation
  double t[3];
  double s;
  int flags;
};

__host__ __device__ inline Update identity_update() { return Update{{1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, {0.0, 0.0, 0.0}, 1.0, 0}; }

// The rotation of the quaternion (w, x, y, z), normalised here with the sign that makes w >= 0.
__host__ __device__ inline void rotation_of(double w, double x, double y, double z, double *r) {
  const double len = sqrt(((w * w) + (x * x)) + ((y * y) + (z * z)));
  w = w / len, x = x / len, y = y / len, z = z / len;
  if (w < 0.0) w = -w, x = -x, y = -y, z = -z;
  r[0] = 1.0 - 2.0 * ((y * y) + (z * z)), r[1] = 2.0 * ((x * y) - (w * z)), r[2] = 2.0 * ((x * z) + (w * y));
  r[3] = 2.0 * ((x * y) + (w * z)), r[4] = 1.0 - 2.0 * ((x * x) + (z * z)), r[5] = 2.0 * ((y * z) - (w * x));
  r[6] = 2.0 * ((x * z) - (w * y)), r[7] = 2.0 * ((y * z) + (w * x)), r[8] = 1.0 - 2.0 * ((x * x) + (y * y));
}

// One Jacobi step of eig3.hpp's rule on the pair (kP, kQ) of the symmetric 4 x 4 matrix A (both triangles kept) and
// the eigenvector matrix V.  Returns whether it rotated.
template <int kP, int kQ>
__host__ __device__ inline bool jacobi_pair4(double (&A)[4][4], double (&V)[4][4]) {
  const double apq = A[kP][kQ];
  if (fabs(apq) <= kSkip * (fabs(A[kP][kP]) + fabs(A[kQ][kQ]))) {
    A[kP][kQ] = 0.0, A[kQ][kP] = 0.0;
    return false;
  }
  const double theta = (A[kQ][kQ] - A[kP][kP]) / (2.0 * apq);
  double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
  if (theta < 0.0) t = -t;
  const double co = 1.0 / sqrt(t * t + 1.0);
  const double s = t * co;
  const double tau = s / (1.0 + co);
  const double h = t * apq;
  A[kP][kP] = A[kP][kP] - h;
  A[kQ][kQ] = A[kQ][kQ] + h;
  A[kP][kQ] = 0.0, A[kQ][kP] = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (r != kP && r != kQ) {
      const double g = A[r][kP], k = A[r][kQ];
      A[r][kP] = A[kP][r] = g - s * (k + tau * g);
      A[r][kQ] = A[kQ][r] = k + s * (g - tau * k);
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double g = V[j][kP], k = V[j][kQ];
    V[j][kP] = g - s * (k + tau * g);
    V[j][kQ] = k + s * (g - tau * k);
  }
  return true;
}

// Horn's closed form from the sums about the pivots (acc as add_row<0> leaves it, W > 0).
__host__ __device__ inline Update solve_point(const double *acc, const Pivots &v, bool with_scale) {
  const double W = acc[0];
  const double mpx = acc[3] / W, mpy = acc[4] / W, mpz = acc[5] / W;      // mu_p - a
  const double mqx = acc[6] / W, mqy = acc[7] / W, mqz = acc[8] / W;      // mu_q - c
  // S = sum w (p - mu_p)(q - mu_q)^T = M - (sum w(p-a)) (mu_q - c)^T
  const double sxx = acc[9] - acc[3] * mqx, sxy = acc[10] - acc[3] * mqy, sxz = acc[11] - acc[3] * mqz;
  const double syx = acc[12] - acc[4] * mqx, syy = acc[13] - acc[4] * mqy, syz = acc[14] - acc[4] * mqz;
  const double szx = acc[15] - acc[5] * mqx, szy = acc[16] - acc[5] * mqy, szz = acc[17] - acc[5] * mqz;
  const double varp = acc[18] - (((acc[3] * mpx) + (acc[4] * mpy)) + (acc[5] * mpz));      // sum w |p - mu_p|^2
  double A[4][4], V[4][4];
  A[0][0] = (sxx + syy) + szz, A[0][1] = syz - szy, A[0][2] = szx - sxz, A[0][3] = sxy - syx;
  A[1][1] = (sxx - syy) - szz, A[1][2] = sxy + syx, A[1][3] = szx + sxz;
  A[2][2] = (syy - sxx) - szz, A[2][3] = syz + szy;
  A[3][3] = (szz - sxx) - syy;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < i) A[i][j] = A[j][i];
      V[i][j] = i == j ? 1.0 : 0.0;
    }
  }
  for (int sweep = 0; sweep < kMaxSweeps; ++sweep) {
    bool rotated = jacobi_pair4<0, 1>(A, V);
    rotated |= jacobi_pair4<0, 2>(A, V);
    rotated |= jacobi_pair4<0, 3>(A, V);
    rotated |= jacobi_pair4<1, 2>(A, V);
    rotated |= jacobi_pair4<1, 3>(A, V);
    rotated |= jacobi_pair4<2, 3>(A, V);
    if (!rotated) break;
  }
  double lambda = A[0][0], q0 = V[0][0], q1 = V[1][0], q2 = V[2][0], q3 = V[3][0];      // the lowest index among equals
  if (A[1][1] > lambda) lambda = A[1][1], q0 = V[0][1], q1 = V[1][1], q2 = V[2][1], q3 = V[3][1];
  if (A[2][2] > lambda) lambda = A[2][2], q0 = V[0][2], q1 = V[1][2], q2 = V[2][2], q3 = V[3][2];
  if (A[3][3] > lambda) lambda = A[3][3], q0 = V[0][3], q1 = V[1][3], q2 = V[2][3], q3 = V[3][3];
  Update u = identity_update();
  rotation_of(q0, q1, q2, q3, u.r);
  if (with_scale && varp > 0.0 && lambda > 0.0) u.s = lambda / varp;
  // t = mu_q - s R mu_p, with mu_p = a + mp and mu_q = c + mq
  const double px = v.ax + mpx, py = v.ay + mpy, pz = v.az + mpz;
  u.t[0] = (v.cx + mqx) - u.s * (((u.r[0] * px) + (u.r[1] * py)) + (u.r[2] * pz));
  u.t[1] = (v.cy + mqy) - u.s * (((u.r[3] * px) + (u.r[4] * py)) + (u.r[5] * pz));
  u.t[2] = (v.cz + mqz) - u.s * (((u.r[6] * px) + (u.r[7] * py)) + (u.r[8] * pz));
  return u;
}

// sine and cosine of any |x| < kMaxAngle: x halved until |x| <= 1/8, the Taylor polynomials there (their first left-out
// terms are below 2^-80), then the double-angle formulas as often as x was halved.
__host__ __device__ inline void sine_cosine(double x, double *sine, double *cosine) {
  int halvings = 0;
  while (fabs(x) > 0.125 && halvings < 32) x = x * 0.5, ++halvings;
  const double z = x * x;
  double s = x * (1.0 - z / 6.0 * (1.0 - z / 20.0 * (1.0 - z / 42.0 * (1.0 - z / 72.0 * (1.0 - z / 110.0 * (1.0 - z / 156.0))))));
  double c = 1.0 - z / 2.0 * (1.0 - z / 12.0 * (1.0 - z / 30.0 * (1.0 - z / 56.0 * (1.0 - z / 90.0 * (1.0 - z / 132.0 * (1.0 - z / 182.0))))));
  for (int i = 0; i < halvings; ++i) {
    const double s2 = 2.0 * (s * c);
    c = 1.0 - 2.0 * (s * s);
    s = s2;
  }
  *sine = s, *cosine = c;
}

// One Gauss-Newton step of the point-to-plane objective from the sums about the pivot (acc as add_row<1> leaves it).
__host__ __device__ inline Update solve_plane(const double *acc, const Pivots &v) {
  double L[6][6], x[6];
  int at = kHead;
  double trace = 0.0;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
#pragma unroll
    for (int c = a; c < 6; ++c) L[c][a] = acc[at], ++at;      // the lower triangle holds J^T J, then its factor
    trace = trace + L[a][a];
  }
  Update u = identity_update();
  bool singular = false;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = L[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d = d - L[j][k] * L[j][k];
    if (!(d > kPivot * trace)) singular = true, d = 1.0;
    const double root = sqrt(d);
    L[j][j] = root;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double e = L[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) e = e - L[i][k] * L[j][k];
      L[i][j] = e / root;
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {      // L y = -J^T r
    double e = -acc[kHead + 21 + i];
#pragma unroll
    for (int k = 0; k < i; ++k) e = e - L[i][k] * x[k];
    x[i] = e / L[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {      // L^T x = y
    double e = x[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) e = e - L[k][i] * x[k];
    x[i] = e / L[i][i];
  }
  const double angle = sqrt(((x[0] * x[0]) + (x[1] * x[1])) + (x[2] * x[2]));
  if (!(angle < kMaxAngle) || !std::isfinite(x[3]) || !std::isfinite(x[4]) || !std::isfinite(x[5])) singular = true;
  if (singular) {
    u.flags = kFlagSingular;
    return u;
  }
  if (angle > 0.0) {
    double sh, ch;
    sine_cosine(0.5 * angle, &sh, &ch);
    const double k = sh / angle;
    rotation_of(ch, k * x[0], k * x[1], k * x[2], u.r);
  }
  // p' = a + R (p - a) + x[3..5] = R p + (a + x[3..5] - R a)
  u.t[0] = (v.ax + x[3]) - (((u.r[0] * v.ax) + (u.r[1] * v.ay)) + (u.r[2] * v.az));
  u.t[1] = (v.ay + x[4]) - (((u.r[3] * v.ax) + (u.r[4] * v.ay)) + (u.r[5] * v.az));
  u.t[2] = (v.az + x[5]) - (((u.r[6] * v.ax) + (u.r[7] * v.ay)) + (u.r[8] * v.az));
  return u;
}

// ------------------------------------------------------------------------------------- one cloud, after its sums
struct Rule {
  int mode, with_scale, freeze;
  double rtol, atol;
};

// The chunks' partials (kStride doubles each) summed in ascending order, from 0.0.
template <int kMode>
__host__ __device__ inline void sum_chunks(const double *partials, int chunks, double *acc) {
  constexpr int kSums = sums_of<kMode>();
#pragma unroll
  for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
  for (int c = 0; c < chunks; ++c) {
#pragma unroll
    for (int k = 0; k < kSums; ++k) acc[k] = acc[k] + partials[(long)c * kStride + k];
  }
}

// pose <- update * pose, scale <- s * scale (pose row-major 4 x 4; its last row is left as it is)
__host__ __device__ inline void compose(const Update &u, double *pose, double *scale) {
  double r[9], t[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
      r[i * 3 + j] = ((u.r[i * 3] * pose[j]) + (u.r[i * 3 + 1] * pose[4 + j])) + (u.r[i * 3 + 2] * pose[8 + j]);
    t[i] = u.s * (((u.r[i * 3] * pose[3]) + (u.r[i * 3 + 1] * pose[7])) + (u.r[i * 3 + 2] * pose[11])) + u.t[i];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) pose[i * 4 + j] = r[i * 3 + j];
    pose[i * 4 + 3] = t[i];
  }
  *scale = u.s * *scale;
}

// The measures, the convergence test, the solve and the composition of one cloud.  pose == null: the measures alone.
template <int kMode>
__host__ __device__ inline void finish_cloud(const double *acc, int src_len, const Pivots &v, const Rule &rule, double *pose,
                                             double *scale, double *state, double *stats) {
  const double W = acc[0];
  const bool empty = !(W > 0.0) || src_len <= 0;
  const double rmse = empty ? 0.0 : sqrt(acc[2] / W);
  const double fitness = empty ? 0.0 : acc[1] / (double)src_len;
  int flags = empty ? kFlagEmpty : 0;
  stats[0] = rmse, stats[1] = fitness, stats[2] = empty ? 0.0 : W;
  if (pose) {
    bool frozen = state[3] != 0.0;
    if (rule.freeze && !frozen && state[2] > 0.0 && fabs(rmse - state[0]) <= rule.rtol * state[0] + rule.atol &&
        fabs(fitness - state[1]) <= rule.rtol) {
      frozen = true;
      state[3] = 1.0;
    }
    if (frozen) {
      flags |= kFlagFrozen;
    } else {
      if (!empty) {
        const Update u = kMode == 0 ? solve_point(acc, v, rule.with_scale != 0) : solve_plane(acc, v);
        flags |= u.flags;
        if (!u.flags) compose(u, pose, scale);
      }
      state[0] = rmse, state[1] = fitness, state[2] = state[2] + 1.0;
    }
  }
  stats[3] = (double)flags;
}

// out = s R x + t of one row, every product and sum rounded separately, left to right, the result rounded once
__host__ __device__ inline void apply_row(const double *pose, double s, const float *x, float *out) {
  const double px = (double)x[0], py = (double)x[1], pz = (double)x[2];
  out[0] = (float)((s * (((pose[0] * px) + (pose[1] * py)) + (pose[2] * pz))) + pose[3]);
  out[1] = (float)((s * (((pose[4] * px) + (pose[5] * py)) + (pose[6] * pz))) + pose[7]);
  out[2] = (float)((s * (((pose[8] * px) + (pose[9] * py)) + (pose[10] * pz))) + pose[11]);
}

}  // namespace rigid
