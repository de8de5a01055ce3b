"""NumPy restatement of the sliced Wasserstein distance (include/ops/swd.h states the definition).

The input of everything after the projection is always the fp32 projection computed by the header's expression
(`project`): the permutation is then the same object in every precision -- a float64 projection would reorder near-ties
and change the gradient discontinuously.  Everything after the sort takes a `dtype`: float64 is the reference, float32
the restatement whose own error E32 sizes the tolerance of a comparison (`tolerance`, the rule of sinkhorn_ref).
"""
import math

import numpy as np

from sinkhorn_ref import tolerance  # noqa: F401  (the one rule: error <= 4 * max(E32, floor))


def project(x, t):
    """fp32 [n] projections of x [n,3] onto t [3]: ((x.x * t.x) + (x.y * t.y)) + (x.z * t.z), every product and sum
    rounded to fp32."""
    x, t = np.asarray(x, np.float32), np.asarray(t, np.float32)
    return ((x[:, 0] * t[0]) + (x[:, 1] * t[1])) + (x[:, 2] * t[2])


def order(proj):
    """perm[rank] = point index: ascending by value, equal values (-0.0 equals +0.0) by index."""
    return np.argsort(proj, kind="stable")


def plan(n, m):
    """The 1-D transport plan of n against m uniform atoms in sorted order, vectorised over the merged breakpoints:
    (i, j, w) with integer masses w in units of 1 / (n m); n + m - gcd(n, m) terms."""
    cuts = np.unique(np.concatenate([np.arange(n + 1, dtype=np.int64) * m, np.arange(m + 1, dtype=np.int64) * n]))
    start, w = cuts[:-1], np.diff(cuts)
    return start // m, start // n, w


def _slope(d, p):
    return 2 * d if p == 2 else np.sign(d)


def transport_1d(sx, sy, p, dtype=np.float64):
    """(cost, cx [n], cy [m]) of the sorted values sx, sy: cost = sum w |sx_i - sy_j|^p / (n m), cx_i = d cost / d sx_i,
    cy_j = d cost / d sy_j, all in `dtype`."""
    n, m = len(sx), len(sy)
    i, j, w = plan(n, m)
    w = w.astype(dtype)
    d = np.asarray(sx, dtype)[i] - np.asarray(sy, dtype)[j]
    mass = dtype(n) * dtype(m)
    terms = w * (d * d if p == 2 else np.abs(d))
    slopes = w * _slope(d, p)
    cx, cy = np.zeros(n, dtype), np.zeros(m, dtype)
    np.add.at(cx, i, slopes)
    np.add.at(cy, j, -slopes)
    return terms.sum(dtype=dtype) / mass, cx / mass, cy / mass


def replicate_and_sort(sx, sy, p):
    """The same cost by the textbook construction: every atom of x m times, every atom of y n times, both sorted."""
    n, m = len(sx), len(sy)
    a = np.sort(np.repeat(np.asarray(sx, np.float64), m))
    b = np.sort(np.repeat(np.asarray(sy, np.float64), n))
    return float(np.mean(np.abs(a - b) ** p))


def term_count(n, m):
    return n + m - math.gcd(n, m)


def swd(x, y, dirs, p, dtype=np.float64, projections=None):
    """One pair of clouds x [n,3], y [m,3] against dirs [L,3]: (cost [L], gradx [n,3], grady [m,3]) with the gradients
    those of the MEAN over the slices, in `dtype`.  `projections` = (px [L,n], py [L,m]) replaces the fp32 projection
    (the finite-difference test hands in float64 ones)."""
    n, m, slices = len(x), len(y), len(dirs)
    cost = np.zeros(slices, dtype)
    gx, gy = np.zeros((n, 3), dtype), np.zeros((m, 3), dtype)
    if n == 0 or m == 0:
        return cost, gx, gy
    for l in range(slices):
        px = project(x, dirs[l]) if projections is None else projections[0][l]
        py = project(y, dirs[l]) if projections is None else projections[1][l]
        ox, oy = order(px), order(py)
        cost[l], cx, cy = transport_1d(px[ox], py[oy], p, dtype)
        t = np.asarray(dirs[l], dtype)
        gx[ox] = gx[ox] + cx[:, None] * t[None, :]
        gy[oy] = gy[oy] + cy[:, None] * t[None, :]
    scale = dtype(1) / dtype(slices)
    return cost, gx * scale, gy * scale
