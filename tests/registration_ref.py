"""NumPy float64 reference of sparenet_amd.cuda.registration (include/ops/rigid_fit.h): the transform with the header's
rounding, SVD Kabsch with the determinant fix, Umeyama's scale, the point-to-plane normal equations through
np.linalg.solve, a brute-force nearest neighbour with the lowest-index tie rule, and the ICP loop with the same inlier,
convergence and freeze rules.  One cloud at a time; nothing here is written like the library (mean-centred sums, LAPACK)."""
import collections

import numpy as np

EMPTY, SINGULAR, FROZEN = 1, 2, 4
Fit = collections.namedtuple("Fit", "pose scale rmse fitness flags W inliers")
Icp = collections.namedtuple("Icp", "pose scale rmse fitness flags iterations converged")


def transform(xyz, pose, scale=1.0, length=None):
    """The header's rule: float64, every product and sum rounded separately, left to right; one rounding to fp32; 0 at
    and beyond `length`."""
    p = np.asarray(xyz, np.float32).astype(np.float64)
    pose = np.asarray(pose, np.float64)
    out = np.zeros(p.shape, np.float32)
    for r in range(3):
        rot = ((pose[r, 0] * p[:, 0]) + (pose[r, 1] * p[:, 1])) + (pose[r, 2] * p[:, 2])
        out[:, r] = ((scale * rot) + pose[r, 3]).astype(np.float32)
    if length is not None:
        out[length:] = 0
    return out


def inliers(moved, dst, idx, weight, src_len, dst_len, max_dist, normals=None):
    """(rows, matches, weights, squared distances) of the inlier rows."""
    n = moved.shape[0]
    j = np.arange(n) if idx is None else np.asarray(idx, np.int64)
    ok = (np.arange(n) < src_len) & (j >= 0) & (j < dst_len)
    jj = np.where(ok, j, 0)
    p, q = moved.astype(np.float64), dst.astype(np.float64)[jj]
    with np.errstate(invalid="ignore", over="ignore"):
        ok &= np.isfinite(p).all(axis=1) & np.isfinite(q).all(axis=1)
        d2 = ((p - q) ** 2).sum(axis=1)
        if max_dist is not None and max_dist > 0:
            ok &= d2 <= float(max_dist) * float(max_dist)
    if normals is not None:
        ok &= np.isfinite(normals.astype(np.float64)[jj]).all(axis=1)
    rows = np.nonzero(ok)[0]
    w = np.ones(len(rows)) if weight is None else weight.astype(np.float64)[rows]
    return rows, jj[rows], w, d2[rows]


def kabsch(p, q, w, with_scale=False):
    """(R, t, s) minimising sum w |s R p + t - q|^2: SVD with the determinant fix, Umeyama's scale."""
    W = w.sum()
    mp, mq = (w[:, None] * p).sum(0) / W, (w[:, None] * q).sum(0) / W
    a, b = p - mp, q - mq
    H = (w[:, None] * b).T @ a      # sum w b a^T
    U, D, Vt = np.linalg.svd(H)
    fix = np.ones(3)
    if np.linalg.det(U @ Vt) < 0:
        fix[2] = -1.0
    R = U @ np.diag(fix) @ Vt
    s = 1.0
    var = (w * (a * a).sum(1)).sum()
    if with_scale and var > 0 and (D * fix).sum() > 0:
        s = (D * fix).sum() / var
    return R, mq - s * R @ mp, s


def rodrigues(omega):
    th = np.linalg.norm(omega)
    if th == 0:
        return np.eye(3)
    k = omega / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def plane_step(p, q, nrm, w, c):
    """(R, t, singular) of one Gauss-Newton step of sum w (n . (R p + t - q))^2 in the header's parametrisation: the
    rotation vector turns about the pivot c (the step depends on the pivot in the second order of the angle)."""
    u = p - c
    J = np.concatenate([np.cross(u, nrm), nrm], axis=1)
    r = (nrm * (p - q)).sum(1)
    A, g = (w[:, None] * J).T @ J, (w[:, None] * J).T @ r
    if np.linalg.eigvalsh(A)[0] <= 2.0 ** -40 * np.trace(A) / 6:
        return np.eye(3), np.zeros(3), True
    x = np.linalg.solve(A, -g)
    R = rodrigues(x[:3])
    return R, c + x[3:] - R @ c, False


def step(moved, dst, idx=None, weight=None, src_len=None, dst_len=None, max_dist=None, mode="point", normals=None,
         with_scale=False):
    """The update (R, t, s) of one cloud and the measures of its correspondence set: Fit with pose = the UPDATE."""
    src_len = moved.shape[0] if src_len is None else src_len
    dst_len = dst.shape[0] if dst_len is None else dst_len
    rows, j, w, d2 = inliers(moved, dst, idx, weight, src_len, dst_len, max_dist, normals if mode == "plane" else None)
    W = w.sum()
    pose = np.eye(4)
    if not W > 0 or src_len == 0:
        return Fit(pose, 1.0, 0.0, 0.0, EMPTY, 0.0, rows)
    rmse, fitness = np.sqrt((w * d2).sum() / W), len(rows) / src_len
    p, q = moved.astype(np.float64)[rows], dst.astype(np.float64)[j]
    flags, s = 0, 1.0
    if mode == "point":
        R, t, s = kabsch(p, q, w, with_scale)
    else:
        pivot = moved[0].astype(np.float64) if np.isfinite(moved[0]).all() else np.zeros(3)
        R, t, singular = plane_step(p, q, normals.astype(np.float64)[j], w, pivot)
        flags = SINGULAR if singular else 0
    pose[:3, :3], pose[:3, 3] = R, t
    return Fit(pose, s, rmse, fitness, flags, W, rows)


def compose(update, s_update, pose, scale):
    out = np.eye(4)
    out[:3, :3] = update[:3, :3] @ pose[:3, :3]
    out[:3, 3] = s_update * update[:3, :3] @ pose[:3, 3] + update[:3, 3]
    return out, s_update * scale


def objective(pose, scale, src, dst, rows, j, w):
    """sum w |s R p + t - q|^2 over the given pairs, float64."""
    p, q = src.astype(np.float64)[rows], dst.astype(np.float64)[j]
    e = scale * p @ pose[:3, :3].T + pose[:3, 3] - q
    return float((w * (e * e).sum(1)).sum())


def nearest(moved, dst, src_len, dst_len):
    """idx [n] int32: the lowest index among the nearest rows of dst[:dst_len] by the fp32 squared distance the library's
    search uses (((dx * dx) + (dy * dy)) + (dz * dz) in fp32); -1 at and beyond src_len or where dst is empty."""
    idx = np.full(moved.shape[0], -1, np.int32)
    if src_len == 0 or dst_len == 0:
        return idx
    a, b = moved[:src_len].astype(np.float32), dst[:dst_len].astype(np.float32)
    for lo in range(0, src_len, 512):
        d = a[lo:lo + 512, None, :] - b[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        idx[lo:lo + d2.shape[0]] = d2.argmin(axis=1)
    return idx


def icp(src, dst, iters, mode="point", normals=None, max_dist=None, init=None, with_scale=False, rtol=1e-6, atol=1e-7,
        src_len=None, dst_len=None):
    src_len = src.shape[0] if src_len is None else src_len
    dst_len = dst.shape[0] if dst_len is None else dst_len
    pose, scale = (np.eye(4) if init is None else np.array(init, np.float64)), 1.0
    prev, done, frozen = None, 0, False
    for _ in range(iters):
        moved = transform(src, pose, scale, src_len)
        idx = nearest(moved, dst, src_len, dst_len)
        f = step(moved, dst, idx, None, src_len, dst_len, max_dist, mode, normals, with_scale)
        if prev is not None and abs(f.rmse - prev[0]) <= rtol * prev[0] + atol and abs(f.fitness - prev[1]) <= rtol:
            frozen = True
            break
        if not f.flags:
            pose, scale = compose(f.pose, f.scale, pose, scale)
        prev, done = (f.rmse, f.fitness), done + 1
    moved = transform(src, pose, scale, src_len)
    f = step(moved, dst, nearest(moved, dst, src_len, dst_len), None, src_len, dst_len, max_dist, mode, normals)
    return Icp(pose, scale, f.rmse, f.fitness, (f.flags & EMPTY) | (FROZEN if frozen else 0), done, frozen)
