"""A plain NumPy reference of the GRNet grid ops and of EdgeConv's graph ops (TEST INFRASTRUCTURE).

Independent of oracle/*.c: it states the DEFINITIONS -- corners, indexes, weights, sums -- with vectorised NumPy
and never restates a kernel's loop.  Two kinds of result come out of it:

  * single-writer results (indexes, weights, gathered features, the reverse op's coordinates) are computed with the
    same fp32 operations in the same order as the documented definition, so they are BIT-EQUAL expectations;
  * sums that a GPU forms with atomics (any order) are computed in float64 from the fp32 terms, and come with the
    number of terms k and the sum of absolute terms A of every output element, from which `sum_bound` derives how
    far a correct fp32 result may lie.

Tolerances (derived, not tuned)
-------------------------------
u = 2^-24 is the unit roundoff of fp32 (round to nearest).  A correct implementation forms every term t with r
roundings of its own, so the computed term is t (1 + d_1)...(1 + d_r), |d_i| <= u, i.e. it is off by at most
r u |t| (1 + O(u)).  Adding k such terms in ANY order takes k - 1 fp32 additions; every partial sum is bounded by
the sum of absolute terms A, and every addition adds a relative error of at most u to its partial sum, so the
additions contribute at most (k - 1) u A (1 + O(k u)).  Together

    |got - ref64| <= (k - 1 + r) * 2^-24 * A * (1 + 2^-20)

where the last factor holds the second-order products of roundings and the (far smaller) error of the float64
reference itself.  A fused multiply-add only REMOVES a rounding, so the bound covers contracted code too.  The bound
is elementwise: an element with no terms (k = 0, A = 0) must be exactly zero, an element with one exact term must be
bit-equal.  The r of every op is stated where `sum_bound` is called:

    gridding forward        r = 2   (wx * wy) * wz
    gridding backward       r = 2   (+-g * wy) * wz, k = 8 fixed
    reverse backward        r = 5   each of the three parts g_a * (corner - p_a) / wsum has three roundings (subtract,
                                    multiply, divide) and the two additions that join them add two more; A sums the
                                    absolute PARTS, since the three parts of one term may cancel
    cubic backward          r = 0   the terms are copies of grad_out
    edge feature forward    r = 1, k = 1   one subtraction
    edge feature backward   r = 1   the k own terms are differences g2 - g1 (one rounding), the list terms are copies

A partition-of-unity bound is used where a grid's total is compared with a point count: per axis the two weights
1 - |p - lo| and 1 - |p - up| are four fp32 operations on values of size at most 1, so they sum to 1 within 4 u, and
the product over three axes to 1 within 12 u (1 + 2^-20): `UNITY_BOUND` per point.

Coordinates are held to |p| <= 2^20 (beyond that float -> int conversion differs between host and device) and must
be finite.
"""
import numpy as np

U32 = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20
UNITY_BOUND = 12 * U32 * SLACK

# corner c of a point: bit 4 -> upper x, bit 2 -> upper y, bit 1 -> upper z (LLL, LLU, LUL, LUU, ULL, ULU, UUL, UUU)
_CORNER_BITS = np.array([[(c >> 2) & 1, (c >> 1) & 1, c & 1] for c in range(8)], np.int64)      # [8, 3]


def sum_bound(k, r, a):
    """Elementwise bound of |fp32 sum in any order - float64 sum| for k terms of r roundings each, A = sum |term|."""
    k = np.asarray(k, np.float64)
    return np.maximum(k - 1 + r, 0) * U32 * np.asarray(a, np.float64) * SLACK


def assert_within(got, ref64, bound, what):
    err = np.abs(np.asarray(got, np.float64) - ref64)
    bad = err > bound
    if bad.any():
        i = np.unravel_index(np.argmax(err - bound), err.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements outside the derived bound; worst at "
                             f"{i}: got {np.asarray(got)[i]!r}, ref {ref64[i]!r}, |err| {err[i]:.3e} > {bound[i]:.3e}")


# ------------------------------------------------------------------------------------------------ gridding
def corners(p):
    """p fp32 [...] -> (lo, up) int64: floor and ceil, and up = lo + 1 where p is an integer (-0.0 included)."""
    p = np.asarray(p, np.float32)
    lo = np.floor(p).astype(np.int64)
    up = np.ceil(p).astype(np.int64)
    return lo, np.where(lo == up, up + 1, up)


def _expand(lo_val, up_val):
    """[B, n, 3] values of the lower / upper corner per axis -> [B, n, 8, 3] per corner."""
    return np.where(_CORNER_BITS[None, None].astype(bool), up_val[:, :, None, :], lo_val[:, :, None, :])


def _weights(pt, lo, up):
    """fp32 1 - |p - corner| per axis, [B, n, 8, 3]: the subtraction and then 1 - |.|, each ONE fp32 operation."""
    one = np.float32(1)
    return _expand(one - np.abs(pt - lo.astype(np.float32)), one - np.abs(pt - up.astype(np.float32)))


def padding_rows(pt):
    """The rows the module drops: (x + y) + z == 0 in fp32, in this order (cuda/gridding/__init__.py:45)."""
    pt = np.asarray(pt, np.float32)
    return ((pt[..., 0] + pt[..., 1]) + pt[..., 2]) == np.float32(0)


def _scatter(flat_index, valid, terms, b, nslots):
    """float64 bincount of `terms` [B, n, 8] at `flat_index` where valid -> (sum, count, abs sum), each [B, nslots]."""
    rows = np.arange(b, dtype=np.int64)[:, None, None] * nslots
    at = (rows + np.where(valid, flat_index, 0))[valid]
    t = terms[valid]
    size = b * nslots
    return (np.bincount(at, t, size).reshape(b, nslots), np.bincount(at, None, size).reshape(b, nslots),
            np.bincount(at, np.abs(t), size).reshape(b, nslots))


def _grid(pt, index, nslots, drop):
    b, n = pt.shape[:2]
    lo, up = corners(pt)
    idx = index(_expand(lo, up))                                 # int64 [B, n, 8]
    w = _weights(pt, lo, up)
    assert w.dtype == np.float32
    valid = (idx >= 0) & (idx < nslots)
    if drop is not None:
        valid &= ~drop[:, :, None]
        w = np.where(drop[:, :, None, None], np.float32(0), w)
        idx = np.where(drop[:, :, None], -1, idx)
    terms = w[..., 0].astype(np.float64) * w[..., 1] * w[..., 2]
    grid, k, a = _scatter(idx, valid, terms, b, nslots)
    return dict(grid=grid, k=k, A=a, bound=sum_bound(k, 2, a), weights=w, indexes=idx.astype(np.int32), valid=valid)


def gridding(pt, s, skip_zero_rows=False):
    """pt fp32 [B, n, 3] in vertex units, s = HALF scale: vertices [-s, s - 1] per axis, grid [B, (2 s)^3].
    index = ((cx + s) (2 s) + (cy + s)) (2 s) + (cz + s) in int64; a corner contributes iff 0 <= index < (2 s)^3
    (so a corner past one axis' end may land on a vertex of the next row: the reference's arithmetic).
    Returns grid (float64), k, A, bound, weights (fp32, exact), indexes (int32, exact), valid."""
    pt = np.ascontiguousarray(pt, np.float32)
    ln = 2 * int(s)
    return _grid(pt, lambda cc: ((cc[..., 0] + s) * ln + (cc[..., 1] + s)) * ln + (cc[..., 2] + s), ln ** 3,
                 padding_rows(pt) if skip_zero_rows else None)


def gridding_dist(pt, bounds):
    """The same weights over the integer box bounds = (min_x, max_x, min_y, max_y, min_z, max_z), eight slots per
    vertex: slot = (((cx - min_x) len_y + (cy - min_y)) len_z + (cz - min_z)) 8 + corner; grid [B, nverts * 8]."""
    pt = np.ascontiguousarray(pt, np.float32)
    mnx, mxx, mny, mxy, mnz, mxz = (int(v) for v in bounds)
    ly, lz = mxy - mny + 1, mxz - mnz + 1
    nslots = (mxx - mnx + 1) * ly * lz * 8
    role = np.arange(8, dtype=np.int64)
    return _grid(pt, lambda cc: (((cc[..., 0] - mnx) * ly + (cc[..., 1] - mny)) * lz + (cc[..., 2] - mnz)) * 8 + role,
                 nslots, None)


def gridding_backward(grad_grid, weights, indexes):
    """grad_grid [B, nslots], weights fp32 [B, n, 8, 3], indexes [B, n, 8] -> (grad float64 [B, n, 3], A [B, n, 3]).
    d grid / d p_x of corner c is +-(wy wz) (+ for an upper corner); corners outside [0, nslots) read zero.
    Eight terms of two roundings each: bound = sum_bound(8, 2, A)."""
    gg = np.asarray(grad_grid, np.float64)
    b, nslots = gg.shape
    idx = np.asarray(indexes, np.int64)
    valid = (idx >= 0) & (idx < nslots)
    g = np.where(valid, np.take_along_axis(gg, np.where(valid, idx, 0).reshape(b, -1), 1).reshape(idx.shape), 0.0)
    w = np.asarray(weights, np.float32)
    wx, wy, wz = (w[..., i].astype(np.float64) for i in range(3))
    grad = np.empty(idx.shape[:2] + (3,))
    a = np.empty_like(grad)
    for axis, other in enumerate((wy * wz, wx * wz, wx * wy)):
        t = g * other * (2.0 * _CORNER_BITS[:, axis] - 1.0)
        grad[..., axis] = t.sum(2)
        a[..., axis] = np.abs(t).sum(2)
    return grad, a


# ------------------------------------------------------------------------------------------------ gridding reverse
def _reverse_cells(grid, scale):
    """grid fp32 [B, scale^3] -> per cell j = (x, y, z) with x, y, z >= 1 the eight vertex indexes in the header's
    order ((x-1,y-1,z-1), (x-1,y-1,z), (x-1,y,z-1), (x-1,y,z), (x,y-1,z-1), (x,y-1,z), (x,y,z-1), (x,y,z)), their
    values, the fp32 sequential sum in that order and the float64 sum."""
    grid = np.ascontiguousarray(grid, np.float32).reshape(len(grid), -1)
    n3 = scale ** 3
    j = np.arange(n3, dtype=np.int64)
    x, y, z = j // (scale * scale), j // scale % scale, j % scale
    interior = (x > 0) & (y > 0) & (z > 0)
    vid = np.stack([((x - 1 + dx) * scale + (y - 1 + dy)) * scale + (z - 1 + dz)
                    for dx, dy, dz in _CORNER_BITS], 1)                                        # [n3, 8]
    vid = np.where(interior[:, None], vid, 0)
    vals = grid[:, vid]                                                                        # [B, n3, 8]
    wsum = np.zeros(vals.shape[:2], np.float32)
    for i in range(8):
        wsum = (wsum + vals[..., i]).astype(np.float32)
    sum64 = vals.astype(np.float64).sum(2)
    off = np.stack([x, y, z], 1) - scale // 2                                                   # upper corner's coordinate
    coord = off[:, None, :] - 1 + _CORNER_BITS[None]                                            # [n3, 8, 3]
    return interior, vid, vals, wsum, sum64, coord


def reverse_forward(grid, scale):
    """One point per cell: the weighted mean of the cell's eight corner coordinates (upper corner = cell index -
    scale // 2), weights grid / wsum; cells with x, y or z == 0 or with wsum < 1e-6 (fp32 sum, compared in double)
    give (0, 0, 0).  Returns pts32 (the fixed fp32 chain: w_k = g_k / wsum, acc = w_0 c_0, acc += w_k c_k; bit-exact),
    pts64 (float64 from the fp32 grid and the fp32 wsum; pts32 lies within sum_bound(8, 2, A) of it), A [B, n3, 3],
    wsum (fp32 sequential), sum64, valid [B, n3], interior [n3] -- and `cells`, which reverse_backward reuses."""
    interior, vid, vals, wsum, sum64, coord = _reverse_cells(grid, scale)
    valid = interior[None] & ~(wsum.astype(np.float64) < 1e-6)
    bi, ci = np.nonzero(valid)                                   # the rest only on the valid cells (a sparse grid has few)
    v, ws, cc = vals[bi, ci], wsum[bi, ci], coord[ci]            # [m, 8], [m], [m, 8, 3]
    w32 = v / ws[:, None]
    c32 = cc.astype(np.float32)
    assert w32.dtype == np.float32
    acc = w32[:, 0, None] * c32[:, 0]
    for k in range(1, 8):
        acc = acc + w32[:, k, None] * c32[:, k]
    terms = (v.astype(np.float64) / ws.astype(np.float64)[:, None])[..., None] * cc
    out = {}
    for name, val, dt in (("pts32", acc, np.float32), ("pts64", terms.sum(1), np.float64), ("A", np.abs(terms).sum(1), np.float64)):
        out[name] = np.zeros(valid.shape + (3,), dt)
        out[name][bi, ci] = val
    out.update(wsum=wsum, sum64=sum64, valid=valid, interior=interior, cells=(bi, ci, vid[ci], ws, cc))
    return out


def reverse_backward(grad_ptcloud, grid, ptcloud, scale, fwd=None):
    """grad_grid[v] = sum over the valid cells that read v (as corner k) of sum_a g_a (corner_k,a - p_a) / wsum, from the
    fp32 forward output p and the fp32 wsum, in float64.  Returns grad [B, n3], k, A (absolute PARTS), bound (r = 5)
    and read [B, n3]: whether any valid cell reads the vertex.  fwd: reverse_forward(grid, scale), if at hand."""
    fwd = fwd or reverse_forward(grid, scale)
    bi, ci, vid, ws, cc = fwd["cells"]
    b, n3 = fwd["valid"].shape
    gp = np.asarray(grad_ptcloud, np.float32).reshape(b, n3, 3)[bi, ci].astype(np.float64)
    p = np.asarray(ptcloud, np.float32).reshape(b, n3, 3)[bi, ci].astype(np.float64)
    parts = gp[:, None, :] * (cc - p[:, None, :]) / ws.astype(np.float64)[:, None, None]       # [m, 8, 3]
    at = (bi[:, None] * n3 + vid).reshape(-1)
    size = b * n3
    grad = np.bincount(at, parts.sum(2).reshape(-1), size).reshape(b, n3)
    k = np.bincount(at, None, size).reshape(b, n3)
    a = np.bincount(at, np.abs(parts).sum(2).reshape(-1), size).reshape(b, n3)
    return dict(grad=grad, k=k, A=a, bound=sum_bound(k, 5, a), read=k > 0)


# ------------------------------------------------------------------------------------------------ cubic sampling
def cubic_index(pt, scale, ns):
    """pt fp32 [B, n, 3] in voxel units -> int32 [B, n, (2 ns)^3]: the vertices lo - (ns - 1) .. up + (ns - 1) per axis
    (x major), (j scale + k) scale + m, or -1 where any of j, k, m leaves [0, scale)."""
    lo, up = corners(np.ascontiguousarray(pt, np.float32))
    span = np.arange(2 * ns, dtype=np.int64)
    ax = lo[..., None] - (ns - 1) + span                                                       # [B, n, 3, 2 ns]
    assert (ax[..., -1] == up + (ns - 1)).all()
    j, k, m = ax[:, :, 0, :, None, None], ax[:, :, 1, None, :, None], ax[:, :, 2, None, None, :]
    inside = ((j >= 0) & (j < scale)) & ((k >= 0) & (k < scale)) & ((m >= 0) & (m < scale))
    idx = np.where(inside, (j * scale + k) * scale + m, -1)
    return idx.reshape(pt.shape[0], pt.shape[1], -1).astype(np.int32)


def cubic_gather(feat, idx):
    """feat fp32 [B, C, scale^3 (any shape)], idx [B, n, nv] -> fp32 [B, n, nv, C]: copies, zeros for -1 (bit-exact)."""
    b, c = feat.shape[:2]
    f = np.ascontiguousarray(feat, np.float32).reshape(b, c, -1)
    out = np.stack([f[i][:, np.where(idx[i] < 0, 0, idx[i])] for i in range(b)])               # [B, C, n, nv]
    return np.where((idx >= 0)[:, None], out, np.float32(0)).transpose(0, 2, 3, 1)


def cubic_scatter(grad_out, idx, scale):
    """grad_out [B, n, nv, C], idx [B, n, nv] -> (grad_feat float64 [B, C, scale^3], k [B, scale^3], A like grad_feat)."""
    go = np.asarray(grad_out, np.float64)
    b, _, _, c = go.shape
    cub = scale ** 3
    grad = np.zeros((b, c, cub))
    a = np.zeros((b, c, cub))
    k = np.zeros((b, cub))
    for i in range(b):
        at = idx[i][idx[i] >= 0].astype(np.int64)
        rows = go[i][idx[i] >= 0]                                                              # [hits, C]
        k[i] = np.bincount(at, None, cub)
        for ch in range(c):
            grad[i, ch] = np.bincount(at, rows[:, ch], cub)
            a[i, ch] = np.bincount(at, np.abs(rows[:, ch]), cub)
    return grad, k, a


# ------------------------------------------------------------------------------------------------ k-NN graph
def sqdist(x):
    """x [B, C, N] -> float64 squared distances [B, N, N], as differences (no cancellation of large norms)."""
    x = np.asarray(x, np.float64)
    d = np.zeros((x.shape[0], x.shape[2], x.shape[2]))
    for ch in range(x.shape[1]):
        d += (x[:, ch, :, None] - x[:, ch, None, :]) ** 2
    return d


def knn_exact(x, k):
    """(d [B, N, N] float64, idx [B, N, k]): the point itself first, then ascending distance, equal distances by
    lower index (a stable argsort with the diagonal ranked below every distance)."""
    d = sqdist(x)
    key = d.copy()
    i = np.arange(d.shape[1])
    key[:, i, i] = -1.0
    return d, np.argsort(key, axis=2, kind="stable")[:, :, :k]


def knn_tau(x):
    """The project's bound on the fp32 rounding of the ranking expression |x_j|^2 - 2 x_i.x_j, per cloud [B]:
    2e-5 * 3 * max_j |x_j|^2 (terms of size |x|^2 that cancel)."""
    x = np.asarray(x, np.float64)
    return 2e-5 * 3.0 * (x ** 2).sum(1).max(1)


def graph_feature(x, idx):
    """x [B, C, N], idx [B, N, k] -> float64 [B, 2 C, N, k]: (neighbour - point, point)."""
    x = np.asarray(x, np.float64)
    b, c, n = x.shape
    nb = np.stack([x[i][:, idx[i]] for i in range(b)])                                         # [B, C, N, k]
    own = np.broadcast_to(x[:, :, :, None], nb.shape)
    return np.concatenate([nb - own, own], 1)


def graph_feature_backward(grad_out, idx):
    """grad_out [B, 2 C, N, k] -> (grad_x float64 [B, C, N], terms [B, N], A [B, C, N]).  grad_x[q] = sum_j (g2 - g1)[q, j]
    + sum over edges (p, j) with idx[p, j] == q of g1[p, j]; terms = k + the length of q's incoming list."""
    g = np.asarray(grad_out, np.float32)
    b, c2, n, k = g.shape
    c = c2 // 2
    g1, g2 = g[:, :c], g[:, c:]
    own = g2.astype(np.float64) - g1.astype(np.float64)
    grad = own.sum(3)
    a = np.abs(own).sum(3)
    terms = np.zeros((b, n))
    for i in range(b):
        at = np.asarray(idx[i], np.int64).reshape(-1)
        terms[i] = k + np.bincount(at, None, n)
        for ch in range(c):
            v = g1[i, ch].astype(np.float64).reshape(-1)
            grad[i, ch] += np.bincount(at, v, n)
            a[i, ch] += np.bincount(at, np.abs(v), n)
    return grad, terms, a


def rows_valid(idx, x, k, tau):
    """Check EVERY row of idx [B, N, k] against the exact float64 distances d of x [B, C, N]; d_k = the k-th smallest of
    the row.  Returns {failure: number of rows}, empty when all rows pass:
      duplicates   a neighbour is listed twice;          self_first   the point itself is not first;
      too_far      a returned j has d_j > d_k + tau;     missing      a j with d_j < d_k - tau is not returned;
      order        consecutive neighbours with d[i + 1] < d[i] - tau."""
    idx = np.asarray(idx, np.int64)
    d = sqdist(x)
    n = d.shape[1]
    assert idx.shape == (d.shape[0], n, k) and idx.min() >= 0 and idx.max() < n
    tau = np.asarray(tau, np.float64).reshape(-1, 1)            # one for all clouds, or one per cloud
    dk = np.sort(d, axis=2)[:, :, k - 1]
    picked = np.take_along_axis(d, idx, 2)
    srt = np.sort(idx, 2)
    fails = dict(
        duplicates=(srt[:, :, 1:] == srt[:, :, :-1]).any(2),
        self_first=idx[:, :, 0] != np.arange(n)[None],
        too_far=(picked > (dk + tau)[..., None]).any(2),
        # without duplicates, "every such j is returned" is a count
        missing=(d < (dk - tau)[..., None]).sum(2) != (picked < (dk - tau)[..., None]).sum(2),
        order=(picked[:, :, 1:] < picked[:, :, :-1] - tau[..., None]).any(2))
    return {name: int(bad.sum()) for name, bad in fails.items() if bad.any()}


def band_share(x, k, tau):
    """Share of rows in which a point the exact search does NOT return lies inside [d_k - tau, d_k + tau]: the rows on
    which rows_valid has to accept more than one answer."""
    d = np.sort(sqdist(x), axis=2)
    if d.shape[2] == k:
        return 0.0
    return float(((d[:, :, k] - d[:, :, k - 1]) <= np.asarray(tau, np.float64).reshape(-1, 1)).mean())
