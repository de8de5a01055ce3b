// eig3.hpp -- the arithmetic of one neighbourhood of local_pca.hip, written once for host and device (the spirit of
// include/sn_expf.h): centroid, covariance, cyclic Jacobi on the symmetric 3 x 3 matrix, order and signs.
// include/ops/local_pca.h states the rule; every line below is one of its sentences.  All double, nothing contracted
// (the build has -ffp-contract=off), no array is indexed by a run-time value: everything stays in registers.
#pragma once
#include <cmath>

namespace eig3 {

constexpr int kMaxSweeps = 12;      // the data-independent bound on the solver
constexpr double kSkip = 0x1p-54;   // |A_pq| <= kSkip * (|A_pp| + |A_qq|): the entry is set to 0, no rotation

struct Vec {
  double x, y, z;
};

struct Result {
  double l0, l1, l2;      // ascending
  Vec e0, e1, e2;         // the frame's rows: normal, e2 x e0, principal direction
};

__host__ __device__ inline void exchange(double &a, double &b) {
  const double t = a;
  a = b;
  b = t;
}
__host__ __device__ inline void exchange(Vec &a, Vec &b) {
  const Vec t = a;
  a = b;
  b = t;
}

// One Jacobi step on the pair (p, q), r the third index: app, aqq, apq and the two entries that couple r to the pair;
// vp, vq are columns p and q of V.  Returns whether it rotated.
__host__ __device__ inline bool jacobi_pair(double &app, double &aqq, double &apq, double &arp, double &arq, Vec &vp,
                                            Vec &vq) {
  if (fabs(apq) <= kSkip * (fabs(app) + fabs(aqq))) {
    apq = 0.0;
    return false;
  }
  const double theta = (aqq - app) / (2.0 * apq);
  double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
  if (theta < 0.0) t = -t;
  const double co = 1.0 / sqrt(t * t + 1.0);
  const double s = t * co;
  const double tau = s / (1.0 + co);
  const double h = t * apq;
  app = app - h;
  aqq = aqq + h;
  apq = 0.0;
  const double g = arp, k = arq;
  arp = g - s * (k + tau * g);
  arq = k + s * (g - tau * k);
  const Vec a = vp, b = vq;
  vp.x = a.x - s * (b.x + tau * a.x), vq.x = b.x + s * (a.x - tau * b.x);
  vp.y = a.y - s * (b.y + tau * a.y), vq.y = b.y + s * (a.y - tau * b.y);
  vp.z = a.z - s * (b.z + tau * a.z), vq.z = b.z + s * (a.z - tau * b.z);
  return true;
}

// the canonical sign: the component of largest magnitude positive, equal magnitudes to the lowest axis
__host__ __device__ inline Vec canonical(const Vec &v) {
  double big = v.x;
  if (fabs(v.y) > fabs(big)) big = v.y;
  if (fabs(v.z) > fabs(big)) big = v.z;
  return big < 0.0 ? Vec{-v.x, -v.y, -v.z} : v;
}

// eigenvalues and frame of the symmetric matrix (cxx cxy cxz; . cyy cyz; . . czz); with `facing` the normal looks
// along (tx, ty, tz); *sweeps, when given, gets the number of sweeps that rotated
__host__ __device__ inline Result solve(double cxx, double cxy, double cxz, double cyy, double cyz, double czz,
                                        bool facing, double tx, double ty, double tz, int *sweeps = nullptr) {
  Vec v0{1.0, 0.0, 0.0}, v1{0.0, 1.0, 0.0}, v2{0.0, 0.0, 1.0};      // the columns of V
  int used = 0;
  for (int sweep = 0; sweep < kMaxSweeps; ++sweep) {
    bool rotated = jacobi_pair(cxx, cyy, cxy, cxz, cyz, v0, v1);      // (0,1), r = 2
    rotated |= jacobi_pair(cxx, czz, cxz, cxy, cyz, v0, v2);          // (0,2), r = 1
    rotated |= jacobi_pair(cyy, czz, cyz, cxy, cxz, v1, v2);          // (1,2), r = 0
    if (!rotated) break;
    ++used;
  }
  if (sweeps) *sweeps = used;
  if (cyy < cxx) exchange(cxx, cyy), exchange(v0, v1);
  if (czz < cyy) exchange(cyy, czz), exchange(v1, v2);
  if (cyy < cxx) exchange(cxx, cyy), exchange(v0, v1);
  Result r;
  r.l0 = cxx, r.l1 = cyy, r.l2 = czz;
  r.e2 = canonical(v2);
  r.e0 = canonical(v0);
  if (facing && ((r.e0.x * tx) + (r.e0.y * ty)) + (r.e0.z * tz) < 0.0)
    r.e0 = Vec{-r.e0.x, -r.e0.y, -r.e0.z};
  r.e1 = Vec{r.e2.y * r.e0.z - r.e2.z * r.e0.y, r.e2.z * r.e0.x - r.e2.x * r.e0.z, r.e2.x * r.e0.y - r.e2.y * r.e0.x};
  r.e0 = Vec{r.e0.x + 0.0, r.e0.y + 0.0, r.e0.z + 0.0};      // a zero is +0.0
  r.e1 = Vec{r.e1.x + 0.0, r.e1.y + 0.0, r.e1.z + 0.0};
  r.e2 = Vec{r.e2.x + 0.0, r.e2.y + 0.0, r.e2.z + 0.0};
  return r;
}

// One neighbourhood: `slot(t)` is the index in slot t of the query's row, `cloud` its n points; query / viewpoint are
// null without a viewpoint.  Returns c, the number of valid slots; with c == 0 everything in *out is 0.
template <class Slot>
__host__ __device__ inline int neighbourhood(const float *cloud, int n, int k, Slot slot, const float *query,
                                             const float *viewpoint, Result *out, int *sweeps = nullptr) {
  int c = 0;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int t = 0; t < k; ++t) {
    const int j = slot(t);
    if (j < 0 || j >= n) continue;
    const float *p = cloud + (long)j * 3;
    sx = sx + (double)p[0], sy = sy + (double)p[1], sz = sz + (double)p[2];
    ++c;
  }
  if (c == 0) {
    *out = Result{0.0, 0.0, 0.0, Vec{0.0, 0.0, 0.0}, Vec{0.0, 0.0, 0.0}, Vec{0.0, 0.0, 0.0}};
    if (sweeps) *sweeps = 0;
    return 0;
  }
  const double count = (double)c;
  const double mx = sx / count, my = sy / count, mz = sz / count;
  double cxx = 0.0, cxy = 0.0, cxz = 0.0, cyy = 0.0, cyz = 0.0, czz = 0.0;
  for (int t = 0; t < k; ++t) {
    const int j = slot(t);
    if (j < 0 || j >= n) continue;
    const float *p = cloud + (long)j * 3;
    const double dx = (double)p[0] - mx, dy = (double)p[1] - my, dz = (double)p[2] - mz;
    cxx = cxx + dx * dx, cxy = cxy + dx * dy, cxz = cxz + dx * dz;
    cyy = cyy + dy * dy, cyz = cyz + dy * dz, czz = czz + dz * dz;
  }
  double tx = 0.0, ty = 0.0, tz = 0.0;      // from the query to the viewpoint
  if (viewpoint) {
    tx = (double)viewpoint[0] - (double)query[0];
    ty = (double)viewpoint[1] - (double)query[1];
    tz = (double)viewpoint[2] - (double)query[2];
  }
  *out = solve(cxx / count, cxy / count, cxz / count, cyy / count, cyz / count, czz / count, viewpoint != nullptr, tx,
               ty, tz, sweeps);
  return c;
}

}  // namespace eig3
