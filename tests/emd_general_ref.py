"""NumPy restatement of the general-size auction EMD (sn_emd_forward_general / sn_emd_backward_general), written from
the semantics in include/sparenet_hip.h.  xyz1 [b, n, 3] bids for xyz2 [b, m, 3], n <= m.  Every fp32 operation is
rounded on its own, as the library builds with -ffp-contract=off.

emd_general(x1, x2, eps, iters) runs several iteration counts from one pass: a run of K iterations equals the first
K - 1 iterations of any longer run followed by a forced last iteration on the same bids (the bids do not depend on
whether the iteration is the last one)."""
import numpy as np

TILE = 2048
SENTINEL = np.float32(-1e9)


def tie_keys(m, tpu):
    """(thread(k), k) as one integer per target: thread(k) = (k mod 2048) // delta of k's 2048-tile."""
    k = np.arange(m, dtype=np.int64)
    k2 = (k // TILE) * TILE
    end_k = np.minimum(m, k2 + TILE) - k2
    delta = (end_k + tpu - 1) // tpu
    return ((k - k2) // delta) * (1 << 20) + k


def bid_values(q, t, price):
    """d[u, k] = (float)((3.0 - (double)sqrtf(s)) - (double)price[k]), s = (dx*dx + dy*dy) + dz*dz, dx = t - q."""
    dx = t[None, :, 0] - q[:, None, 0]
    dy = t[None, :, 1] - q[:, None, 1]
    dz = t[None, :, 2] - q[:, None, 2]
    s = (dx * dx + dy * dy) + dz * dz
    return ((3.0 - np.sqrt(s).astype(np.float64)) - price.astype(np.float64)[None, :]).astype(np.float32)


def top2(d, keys):
    """best, better (second element of the descending multiset, at least -1e9) and best_i per row."""
    best = d.max(1)
    eq = d == best[:, None]
    best_i = np.where(eq, keys[None, :], np.iinfo(np.int64).max).argmin(1)
    rest = np.where(eq, -np.inf, d).max(1) if d.shape[1] > 1 else np.full(d.shape[0], -np.inf)
    better = np.where(eq.sum(1) >= 2, best, np.maximum(rest, SENTINEL)).astype(np.float32)
    low = best <= SENTINEL   # the running values start at -1e9 with a strict '>': nothing at or below it counts
    best = np.where(low, SENTINEL, best)
    better = np.where(low, SENTINEL, better)
    best_i = np.where(low, -1, best_i)
    return best.astype(np.float32), better, best_i


def _dist(p1, p2, a):
    k = np.maximum(a, 0)
    d = p1 - p2[k]
    out = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return np.where(a >= 0, out, np.float32(0)).astype(np.float32)


def _cloud(p1, p2, eps, iters_set, chunk):
    n, m = p1.shape[0], p2.shape[0]
    eps = np.float32(eps)
    block_cnt = (n + 1023) // 1024
    assign = np.full(n, -1, np.int64)
    assign_inv = np.full(m, -1, np.int64)
    price = np.zeros(m, np.float32)
    max_inc = np.zeros(m, np.float32)
    max_idx = np.zeros(m, np.int64)
    out, pairs, last_needed = {}, 0, max(iters_set)
    if 0 in iters_set:
        out[0] = (np.full(n, -1, np.int64), 0)
    for it in range(last_needed):
        unass = np.nonzero(assign == -1)[0]
        cnt = len(unass)
        if cnt == 0:   # every later iteration is a no-op
            for k in iters_set:
                if k > it:
                    out[k] = (assign.copy(), pairs)
            break
        pairs += cnt * m
        tpu = 1024 // ((cnt + block_cnt - 1) // block_cnt)
        keys = tie_keys(m, tpu)
        bid = np.empty(cnt, np.int64)
        inc = np.empty(cnt, np.float32)
        for c0 in range(0, cnt, chunk):
            sel = unass[c0:c0 + chunk]
            best, better, bi = top2(bid_values(p1[sel], p2, price), keys)
            bid[c0:c0 + chunk] = bi
            inc[c0:c0 + chunk] = (best - better) + eps
        ok = bid >= 0
        if it + 1 in iters_set:   # the run of it + 1 iterations: forced assignment of this iteration's bids
            a = assign.copy()
            a[unass[ok]] = bid[ok]
            out[it + 1] = (a, pairs)
        if it + 1 == last_needed:
            break
        # target maximum of the increments
        np.maximum.at(max_inc, bid[ok], inc[ok])
        # GetMax: the highest bidder index inside the window; untouched targets keep a stale max_idx
        bi64 = inc.astype(np.float64)
        mi = max_inc[np.maximum(bid, 0)].astype(np.float64)
        win = ok & (bi64 - 1e-6 <= mi) & (mi <= bi64 + 1e-6)
        top = np.full(m, -1, np.int64)
        np.maximum.at(top, bid[win], unass[win])
        max_idx = np.where(top >= 0, top, max_idx)
        # Assign: one winner per target
        won = ok & (max_idx[np.maximum(bid, 0)] == unass)
        j, t = unass[won], bid[won]
        inv = assign_inv[t]
        assign[inv[inv >= 0]] = -1
        assign_inv[t] = j
        assign[j] = t
        price[t] = price[t] + inc[won]
        max_inc[t] = SENTINEL
    return out


def emd_general(xyz1, xyz2, eps, iters, chunk=None):
    """iters: an int or a list of ints.  Returns {iters: (dist [b, n] f32, assignment [b, n] i32, pairs)} for a list,
    the tuple for an int.  pairs = sum over clouds and iterations of cnt * m."""
    x1 = np.ascontiguousarray(xyz1, np.float32)
    x2 = np.ascontiguousarray(xyz2, np.float32)
    b, n, _ = x1.shape
    m = x2.shape[1]
    assert x2.shape[0] == b and 1 <= n <= m
    many = not np.isscalar(iters)
    iters_set = sorted(set(int(i) for i in (iters if many else [iters])))
    chunk = chunk or max(1, (1 << 22) // m)
    res = {k: (np.zeros((b, n), np.float32), np.zeros((b, n), np.int32), 0) for k in iters_set}
    for i in range(b):
        out = _cloud(x1[i], x2[i], eps, iters_set, chunk)
        for k in iters_set:
            a, p = out[k]
            d, aa, pp = res[k]
            d[i] = _dist(x1[i], x2[i], a)
            aa[i] = a
            res[k] = (d, aa, pp + p)
    return res if many else res[iters_set[0]]


def emd_general_backward(xyz1, xyz2, graddist, assignment, m=None):
    """(gradxyz1 [b, n, 3], gradxyz2 [b, m, 3]): gradxyz1[j] = (2 g_j) * (x1_j - x2_a(j)), 0 where a(j) = -1;
    gradxyz2[k] = ((0 - t_j1) - t_j2) - ... over the bidders j1 < j2 < ... assigned to k."""
    x1 = np.ascontiguousarray(xyz1, np.float32)
    x2 = np.ascontiguousarray(xyz2, np.float32)
    gd = np.ascontiguousarray(graddist, np.float32)
    a = np.asarray(assignment).astype(np.int64)
    b, n, _ = x1.shape
    m = x2.shape[1]
    g1 = np.zeros((b, n, 3), np.float32)
    g2 = np.zeros((b, m, 3), np.float32)
    for i in range(b):
        ok = a[i] >= 0
        g = (gd[i] * np.float32(2))[:, None]
        t = g * (x1[i] - x2[i][np.maximum(a[i], 0)])
        g1[i] = np.where(ok[:, None], t, np.float32(0))
        j = np.nonzero(ok)[0]           # ascending j; ufunc.at applies them in this order
        np.subtract.at(g2[i], a[i][j], g1[i][j])
    return g1, g2
