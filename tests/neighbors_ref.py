"""NumPy restatement of the rules of include/ops/neighbors.h -- the reference of tests/test_neighbors.py and
tests/test_neighbors_gpu.py.  Every array of the searches and the forwards is fp32 and every product and sum is rounded
separately (NumPy never contracts); a stable argsort keeps equal distances in index order; overflow to +inf is an
ordinary value.  The backward is an np.add.at in float64."""
import numpy as np

CHUNK = 256      # queries per block of the distance matrix
PRESELECT_FROM = 4096      # clouds from this size on sort only the candidates of a row (_stable_prefix)


def _length(length, n):
    return n if length is None else min(max(int(length), 0), n)


def dist_matrix(q, t):
    """d[i, j] = ((dx * dx) + (dy * dy)) + (dz * dz) with dx = t[j].x - q[i].x, fp32."""
    q, t = np.asarray(q, np.float32), np.asarray(t, np.float32)
    with np.errstate(all="ignore"):
        dx = t[None, :, 0] - q[:, None, 0]
        dy = t[None, :, 1] - q[:, None, 1]
        dz = t[None, :, 2] - q[:, None, 2]
        return ((dx * dx) + (dy * dy)) + (dz * dz)


def knn_ref(xyz, new_xyz, k, length=None, new_length=None, preselect=True):
    """(idx [M,k] int32, dist2 [M,k] fp32) of one cloud: a stable argsort on d, so equal distances stay in index
    order.  preselect=False sorts whole rows at every size."""
    n, m = xyz.shape[0], new_xyz.shape[0]
    n, lq = _length(length, n), _length(new_length, m)
    idx = np.full((m, k), -1, np.int32)
    dist2 = np.full((m, k), np.inf, np.float32)
    take = min(k, n)
    for lo in range(0, lq, CHUNK):
        hi = min(lo + CHUNK, lq)
        d = dist_matrix(new_xyz[lo:hi], xyz[:n])
        order = _stable_prefix(d, take) if preselect and n >= PRESELECT_FROM else \
            np.argsort(d, axis=1, kind="stable")[:, :take]
        idx[lo:hi, :take] = order
        dist2[lo:hi, :take] = np.take_along_axis(d, order, axis=1)
    return idx, dist2


def _stable_prefix(d, take):
    """The first `take` columns of np.argsort(d, axis=1, kind="stable") without sorting whole rows: only entries that
    are <= a row's take-th smallest value can be among them, and a stable sort of those (they are visited in index
    order) orders them as the full sort does.  For the full-size clouds, where whole rows take seconds."""
    kth = np.partition(d, take - 1, axis=1)[:, take - 1]
    order = np.empty((d.shape[0], take), np.int64)
    for i in range(d.shape[0]):
        cand = np.flatnonzero(d[i] <= kth[i])
        order[i] = cand[np.argsort(d[i, cand], kind="stable")[:take]]
    return order


def ball_ref(xyz, new_xyz, radius, nsample, pad_first=True, length=None, new_length=None):
    """(idx [M,nsample] int32, cnt [M] int32) of one cloud."""
    n, m = xyz.shape[0], new_xyz.shape[0]
    n, lq = _length(length, n), _length(new_length, m)
    r2 = np.float32(radius) * np.float32(radius)
    idx = np.full((m, nsample), -1, np.int32)
    cnt = np.zeros(m, np.int32)
    for lo in range(0, lq, CHUNK):
        hi = min(lo + CHUNK, lq)
        d = dist_matrix(new_xyz[lo:hi], xyz[:n])
        for i in range(lo, hi):
            hits = np.flatnonzero(d[i - lo] < r2)[:nsample]
            cnt[i] = hits.size
            idx[i, :hits.size] = hits
            if hits.size and pad_first:
                idx[i, hits.size:] = hits[0]
    return idx, cnt


def _batch(fn, xyz, new_xyz, lengths, new_lengths):
    rows = [fn(xyz[i], new_xyz[i], None if lengths is None else lengths[i],
               None if new_lengths is None else new_lengths[i]) for i in range(xyz.shape[0])]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


def knn_ref_batch(xyz, new_xyz, k, lengths=None, new_lengths=None):
    return _batch(lambda x, q, ln, lq: knn_ref(x, q, k, ln, lq), xyz, new_xyz, lengths, new_lengths)


def ball_ref_batch(xyz, new_xyz, radius, nsample, pad_first=True, lengths=None, new_lengths=None):
    return _batch(lambda x, q, ln, lq: ball_ref(x, q, radius, nsample, pad_first, ln, lq), xyz, new_xyz, lengths,
                  new_lengths)


def group_ref(features, idx):
    """features [B,C,N], idx [B,M,S] -> [B,C,M,S]; 0.0 where idx is -1."""
    features = np.asarray(features, np.float32)
    b, c, _ = features.shape
    m, s = idx.shape[1:]
    safe = np.where(idx < 0, 0, idx).reshape(b, 1, m * s)
    out = np.take_along_axis(features, np.broadcast_to(safe, (b, c, m * s)), axis=2).reshape(b, c, m, s)
    return np.where(idx[:, None] < 0, np.float32(0), out).astype(np.float32)


def interpolate_ref(features, idx, weight):
    """features [B,C,N], idx / weight [B,M,S] -> [B,C,M] = (((w0 * f0) + (w1 * f1)) + ...), a -1 slot skipped."""
    features, weight = np.asarray(features, np.float32), np.asarray(weight, np.float32)
    f = group_ref(features, idx)
    b, c, m, s = f.shape
    acc = np.zeros((b, c, m), np.float32)
    started = np.zeros((b, 1, m), bool)
    with np.errstate(all="ignore"):
        for t in range(s):
            term = weight[:, None, :, t] * f[:, :, :, t]
            live = (idx[:, None, :, t] >= 0)
            acc = np.where(live, np.where(started, acc + term, term), acc)
            started = started | live
    return acc


def group_backward_ref(grad_out, idx, n, weight=None):
    """float64 (grad_features [B,C,N], magnitude [B,C,N] = the sum of |term|, list length [B,N]).  grad_out is
    [B,C,M,S] (grouping) or, with weight [B,M,S], [B,C,M] (interpolation)."""
    g = np.asarray(grad_out, np.float64)
    b, c = g.shape[:2]
    m, s = idx.shape[1:]
    terms = g if weight is None else np.asarray(weight, np.float64)[:, None] * g[:, :, :, None]
    grad = np.zeros((b, c, n))
    mag = np.zeros((b, c, n))
    length = np.zeros((b, n), np.int64)
    for i in range(b):
        flat = idx[i].reshape(-1)
        live = flat >= 0
        np.add.at(length[i], flat[live], 1)
        for ch in range(c):
            t = terms[i, ch].reshape(-1)[live]
            np.add.at(grad[i, ch], flat[live], t)
            np.add.at(mag[i, ch], flat[live], np.abs(t))
    return grad, mag, length


def sum_bound(length):
    """gamma of a recursive fp32 sum of `length` rounded terms: (L + 2) u / (1 - (L + 2) u), u = 2^-24."""
    lu = (np.asarray(length, np.float64) + 2) * 2.0 ** -24
    return lu / (1 - lu)


def same_bits(a, b):
    """True when two fp32 arrays hold the same bit patterns."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def lattice_points(side=5):
    """side^3 points with coordinates in multiples of 1/8 (shuffled): many equal distances, all exact in fp32, some
    exactly 0.0625 = 0.25^2."""
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32) / 8
    return g[np.random.default_rng(13).permutation(len(g))]
