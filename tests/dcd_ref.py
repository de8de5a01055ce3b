"""NumPy restatement of the density-aware Chamfer distance (include/ops/dcd.h): fp32 distances
(dx*dx + dy*dy) + dz*dz and the fp32 product alpha * dist as the library forms them, np.exp in float64 of that fp32
argument, everything else in float64 with the lists taken in ascending order.  One pair of clouds per call."""
import numpy as np

POWERS = {0.0: lambda c: np.ones_like(c, dtype=np.float64), 0.5: lambda c: np.sqrt(c.astype(np.float64)),
          1.0: lambda c: c.astype(np.float64)}
RATIOS = ("none", "size")


def nearest(q, t):
    """(dist [n] fp32, idx [n] int32): squared distance to, and lowest index of, the nearest of t [m,3] per row of
    q [n,3], every product and sum rounded to fp32."""
    q, t = np.asarray(q, np.float32), np.asarray(t, np.float32)
    dist, idx = np.empty(len(q), np.float32), np.empty(len(q), np.int32)
    step = max(1, (1 << 22) // max(len(t), 1))
    for s in range(0, len(q), step):
        d = t[None, :, :] - q[s:s + step, None, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        idx[s:s + step] = d2.argmin(axis=1)      # the first of equal distances
        dist[s:s + step] = d2[np.arange(d2.shape[0]), idx[s:s + step]]
    return dist, idx


def search(x, y):
    """(dist1, idx1, dist2, idx2) of the Chamfer search both ways."""
    return nearest(x, y) + nearest(y, x)


def _side(dist, idx, count_other, alpha, n_lambda, r, exact=False):
    """(matched, W, term, a) of one side's points; an index outside the other cloud: term 1, a 0."""
    own_len = len(dist)
    matched = (idx >= 0) & (idx < len(count_other))
    c = np.where(matched, count_other[np.where(matched, idx, 0)], 1)
    if exact:
        e, alpha64 = np.exp(-(alpha * dist)), np.float64(alpha)
    else:
        argument = -(np.float32(alpha) * dist.astype(np.float32))      # fp32, as the library forms it
        e, alpha64 = np.exp(argument.astype(np.float64)), np.float64(np.float32(alpha))
    w = r / POWERS[float(n_lambda)](c)
    term = np.where(matched, 1.0 - e * w, 1.0)
    a = np.where(matched, ((alpha64 * e) * w) / own_len, 0.0)
    return matched, w, term, a


def dcd(x, y, alpha=1000.0, n_lambda=1.0, ratio="none", found=None, exact=False):
    """The reference of one pair x [n,3], y [m,3] (fp32): a dict with loss, sides [2], count1, count2, grad1, grad2
    (float64), the search's dist / idx, max_w (the largest weight: the loss's tolerance scales with it) and abs1 / abs2,
    per gradient component the sum of the absolute values of its contributions (the gradient's tolerance scales with
    them).  `found` = (dist1, idx1, dist2, idx2) replaces the search.  `exact`: float64 coordinates, distances and
    products throughout -- the derivative of loss_f64, for the test of the formula itself."""
    dtype = np.float64 if exact else np.float32
    x, y = np.asarray(x, dtype), np.asarray(y, dtype)
    n, m = len(x), len(y)
    dist1, idx1, dist2, idx2 = found if found is not None else search(x, y)
    if exact:
        dist1, dist2 = ((x - y[idx1]) ** 2).sum(axis=1), ((y - x[idx2]) ** 2).sum(axis=1)
    in1, in2 = (idx1 >= 0) & (idx1 < m), (idx2 >= 0) & (idx2 < n)
    count2 = np.bincount(idx1[in1], minlength=m).astype(np.int32)      # who chose y_k
    count1 = np.bincount(idx2[in2], minlength=n).astype(np.int32)
    r1, r2 = (n / m, m / n) if ratio == "size" else (1.0, 1.0)
    _, w1, term1, a1 = _side(dist1, idx1, count2, alpha, n_lambda, r1, exact)
    _, w2, term2, a2 = _side(dist2, idx2, count1, alpha, n_lambda, r2, exact)
    sides = np.array([term1.sum() / n, term2.sum() / m])
    x64, y64 = x.astype(np.float64), y.astype(np.float64)

    def gradient(mine, other, idx_mine, in_mine, a_mine, idx_other, in_other, a_other):
        own = np.where(in_mine[:, None], a_mine[:, None] * (mine - other[np.where(in_mine, idx_mine, 0)]), 0.0)
        grad, total = own.copy(), np.abs(own)
        j = np.nonzero(in_other)[0]      # ascending: np.add.at applies them in this order
        step = a_other[j, None] * (other[j] - mine[idx_other[j]])
        np.add.at(grad, idx_other[j], -step)
        np.add.at(total, idx_other[j], np.abs(step))
        return grad, total

    grad1, abs1 = gradient(x64, y64, idx1, in1, a1, idx2, in2, a2)
    grad2, abs2 = gradient(y64, x64, idx2, in2, a2, idx1, in1, a1)
    return {"loss": 0.5 * (sides[0] + sides[1]), "sides": sides, "count1": count1, "count2": count2, "grad1": grad1,
            "grad2": grad2, "abs1": abs1, "abs2": abs2, "max_w": max(w1.max(), w2.max()), "dist1": dist1, "idx1": idx1,
            "dist2": dist2, "idx2": idx2}


def loss_f64(x, y, idx1, idx2, alpha=1000.0, n_lambda=1.0, ratio="none"):
    """The loss as a float64 function of float64 coordinates with the assignment (and with it the counts) held fixed:
    what the gradient is the derivative of."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    n, m = len(x), len(y)
    count2, count1 = np.bincount(idx1, minlength=m), np.bincount(idx2, minlength=n)
    r1, r2 = (n / m, m / n) if ratio == "size" else (1.0, 1.0)
    p = POWERS[float(n_lambda)]
    d1, d2 = ((x - y[idx1]) ** 2).sum(axis=1), ((y - x[idx2]) ** 2).sum(axis=1)
    l1 = (1.0 - np.exp(-alpha * d1) * r1 / p(count2[idx1])).mean()
    l2 = (1.0 - np.exp(-alpha * d2) * r2 / p(count1[idx2])).mean()
    return 0.5 * (l1 + l2)
