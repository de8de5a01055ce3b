"""What tests/test_normals.py (host entry point, CPU tensors) and tests/test_normals_gpu.py (device) share: the clouds,
their index tables (built in NumPy, so the same on both sides), the reference and the comparison at derived tolerances.

Tolerances.  u = 2^-53, T = trace(C_ref), k the table's width.  Library and reference build C in the same order, each
with a backward error of at most (k + 3) u sum_t |d_t|^2 / c = (k + 3) u T in the 2-norm (c <= k products and sums, one
subtraction and one division per term).  The library's solver makes at most 36 rotations (12 sweeps), each an
orthogonal similarity carried out with an error of at most 6 u ||A|| <= 6 u T: 216 u T; LAPACK's eigh is allowed 34 u T.
Together 2 (k + 3) u T + 250 u T <= 32 (k + 8) u T, so
    E = C1 (k + 8) u T,  C1 = 32
bounds the perturbation of C that explains both results, and by Weyl every eigenvalue is within E of the reference.
    eigenvalues   |l - l_ref| <= E
    residual      ||C v_r - l_r v_r|| <= E + 2^-22 T in np.longdouble, for every row (the second term is the fp32
                  rounding of v: 3 components, 2^-25 each, times ||C - l|| <= T); the reference's own double
                  eigenvectors must meet E alone
    orthonormal   |v_r . v_s - delta_rs| <= 2^-21 for every row with c >= 1
    direction     where (l1 - l0) / T >= 1e-2: sin(angle to the reference normal) <= 2 E / (l1 - l0) + 2^-22
                  (Davis-Kahan), and the SAME sign -- except where the reference's two largest components agree to
                  within 2^-20 in magnitude, where the canonical sign is ill-conditioned (direction only there)
The share of rows the gap rule excludes is capped at 2 % per case.  Every figure is printed before anything is
asserted."""
import functools

import numpy as np

import local_pca_ref as ref
from neighbors_ref import ball_ref, knn_ref

U = 2.0 ** -53
C1 = 32.0
GAP = 1e-2
MAX_EXCLUDED = 0.02
KS = [1, 2, 3, 7, 16, 31, 32, 33, 64]
MS = [1, 63, 64, 65, 257, 1500]
BALL_RADIUS = 0.15


# ---------------------------------------------------------------------------------------------------- clouds
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def cloud(name):
    """The clouds (a) .. (e) of the module's tests, fp32; 'sphere45' is the inner concentric sphere.  The spheres'
    coordinates are multiples of 2^-17, so that (e) = (b) + 100 is an exact translation in fp32."""
    rng = np.random.default_rng({"a": 0, "b": 1, "c": 2, "d": 3, "e": 1, "sphere45": 4}[name])
    if name == "a":
        return _frozen(rng.random((1500, 3)).astype(np.float32))
    if name in ("b", "c", "e", "sphere45"):
        p = rng.standard_normal((2048, 3))
        p = (0.45 if name == "sphere45" else 0.5) * p / np.linalg.norm(p, axis=1, keepdims=True)
        if name == "c":
            p = p + 0.005 * rng.standard_normal(p.shape)
        p = (np.round(p * 2.0 ** 17) / 2.0 ** 17).astype(np.float32)
        if name == "e":
            assert np.array_equal((p + np.float32(100.0)).astype(np.float64), p.astype(np.float64) + 100.0)
            p = p + np.float32(100.0)
        return _frozen(p)
    if name == "d":
        uv = rng.random((1000, 2))
        axes = np.linalg.qr(rng.standard_normal((3, 3)))[0]
        p = uv[:, :1] * axes[0] + uv[:, 1:] * axes[1] + 0.002 * rng.standard_normal((1000, 1)) * axes[2]
        return _frozen(p.astype(np.float32))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def self_table(name, k):
    """The k-NN table of a named cloud against itself (the point is its own first neighbour)."""
    return _frozen(knn_ref(cloud(name), cloud(name), k)[0])


@functools.lru_cache(maxsize=None)
def batch_of(m):
    """Three different clouds of m points -- a slab, a flat Gaussian blob, a thinner slab: a table of 64 slots reaches
    the whole of a small cloud, so each cloud has a thin axis of its own -- and their self-search tables at k = 64 (-1
    beyond the cloud): a table of width k is its first k columns."""
    rng = np.random.default_rng(1000 + m)
    x = np.stack([rng.random((m, 3)) * [1.0, 0.6, 0.1], rng.standard_normal((m, 3)) * [0.3, 0.2, 0.03],
                  rng.random((m, 3)) * [1.0, 0.5, 0.05]])
    x = x.astype(np.float32)
    return _frozen(x, np.stack([knn_ref(x[i], x[i], 64)[0] for i in range(3)]))


@functools.lru_cache(maxsize=None)
def holes_table():
    """Cloud (a)'s table at k = 16 with holes: row 0 empty, rows 1..3 with c = 1, 2, 3, rows 4..19 empty, every other
    slot emptied with probability 0.3."""
    idx = self_table("a", 16).copy()
    rng = np.random.default_rng(7)
    idx[rng.random(idx.shape) < 0.3] = -1
    idx[0] = -1
    for c in (1, 2, 3):
        idx[c] = -1
        idx[c, 16 - c:] = self_table("a", 16)[c, :c]      # the valid slots at the row's end
    idx[4:20] = -1
    return _frozen(idx)


@functools.lru_cache(maxsize=None)
def ball_table():
    """ball_query(pad="none") of cloud (a) against itself: radius 0.15, 32 slots, rows of 2 .. 32 hits."""
    return _frozen(ball_ref(cloud("a"), cloud("a"), BALL_RADIUS, 32, pad_first=False)[0])


def ragged_batch():
    """(xyz [4,700,3] with NaN padding, lengths): a self-search at k = 5, wider than three of the clouds."""
    rng = np.random.default_rng(11)
    lengths = [700, 1, 2, 1]
    x = rng.random((4, 700, 3)).astype(np.float32)
    x[0] = cloud("b")[:700]      # a surface: five neighbours of a point in a cube are too often without a normal
    for i, n in enumerate(lengths):
        x[i, n:] = np.nan
    return x, lengths


def ragged_table(x, lengths, k=5):
    return np.stack([knn_ref(x[i], x[i], k, lengths[i], lengths[i])[0] for i in range(len(x))])


# ---------------------------------------------------------------------------------------------------- running
def run(xyz, idx, device, new_xyz=None, viewpoint=None):
    """local_pca on `device` for a batch [B,n,3] / [B,m,k] (or one cloud [n,3] / [m,k]): (normals, eigenvalues, frames)
    as NumPy arrays of the input's rank."""
    import torch

    from sparenet_amd.cuda.normals import local_pca

    one = xyz.ndim == 2
    put = lambda a: None if a is None else torch.tensor(np.asarray(a)[None] if one else np.asarray(a), device=device)  # noqa: E731
    view = None if viewpoint is None else torch.tensor(np.asarray(viewpoint, np.float32), device=device)
    out = local_pca(put(xyz), put(idx), put(new_xyz), view, return_frames=True)
    assert not any(t.requires_grad for t in out)
    assert out[0].dtype == torch.float32 and out[1].dtype == torch.float64 and out[2].dtype == torch.float32
    return tuple(t.cpu().numpy()[0] if one else t.cpu().numpy() for t in out)


def same_bits(got, want):
    """Two (normals, eigenvalues, frames) triples agree in every bit."""
    return (np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
            and np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64))
            and np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)))


# ---------------------------------------------------------------------------------------------------- checking
def bound(k, trace):
    return C1 * (k + 8) * U * trace


def _residual(C, values, vectors):
    """[m,3] longdouble: ||C v_r - l_r v_r|| for the rows r of vectors [m,3,3]."""
    C, values, vectors = C.astype(np.longdouble), values.astype(np.longdouble), vectors.astype(np.longdouble)
    r = np.einsum("mij,mrj->mri", C, vectors) - values[:, :, None] * vectors
    return np.sqrt((r * r).sum(axis=2))


WORST = {}      # the largest figure of every kind over a test session, in units of its bound: printed by the tests


def _note(kind, value):
    WORST[kind] = max(WORST.get(kind, 0.0), float(value))


def check(out, xyz, idx, label, new_xyz=None, viewpoint=None, signs=True, cap=True):
    """One cloud's (normals, eigenvalues, frames) against the reference at the module's tolerances.  Returns the
    reference's dict with the figures added.  cap=False is for neighbourhoods that define no normal by construction --
    tables of at most 3 slots (one or two points have l0 = l1 = 0, three are often thin) and collinear points: the gap
    rule's share is printed and not capped there; the rows it does not exclude are compared as everywhere."""
    normals, values, frames = out
    k = idx.shape[1]
    want = ref.local_pca(xyz, idx, new_xyz, viewpoint)
    C, c = want["C"], want["c"]
    trace = C[:, 0, 0] + C[:, 1, 1] + C[:, 2, 2]
    E = bound(k, trace)
    unit = np.where(E > 0, E, 1.0)
    assert np.isfinite(values).all() and np.isfinite(frames).all(), f"{label}: not finite"

    value_err = np.abs(values - want["eigenvalues"]).max(axis=1)
    res = _residual(C, values, frames).max(axis=1).astype(np.float64)
    res_tol = E + 2.0 ** -22 * trace
    ref_res = _residual(C, want["eigenvalues"], want["frames"]).max(axis=1).astype(np.float64)
    f64 = frames.astype(np.float64)
    gram = np.einsum("mri,msi->mrs", f64, f64) - np.where(c > 0, 1.0, 0.0)[:, None, None] * np.eye(3)
    ortho = np.abs(gram).max(axis=(1, 2))
    det = np.linalg.det(f64)

    gap = want["eigenvalues"][:, 1] - want["eigenvalues"][:, 0]
    judged = (trace > 0) & (gap >= GAP * np.where(trace > 0, trace, 1.0))
    excluded = float(((c > 0) & (trace > 0) & ~judged).sum()) / max(int(((c > 0) & (trace > 0)).sum()), 1)
    n64, nref = normals.astype(np.float64), want["normals"]
    sin = np.linalg.norm(np.cross(n64, nref), axis=1)
    sin_tol = 2.0 * E / np.where(judged, gap, 1.0) + 2.0 ** -22
    top = np.sort(np.abs(nref), axis=1)
    tie = top[:, 2] - top[:, 1] <= 2.0 ** -20
    same_sign = (n64 * nref).sum(axis=1) > 0

    figures = {"eigenvalue err / E": (value_err / unit).max(), "residual / (E + 2^-22 T)": (res / np.where(res_tol > 0, res_tol, 1.0)).max(),
               "reference residual / E": (ref_res / unit).max(), "orthonormality / 2^-21": ortho.max() / 2.0 ** -21,
               "sin / bound": (sin / sin_tol)[judged].max() if judged.any() else 0.0}
    print(f"{label}: k {k} rows {len(c)} " + "; ".join(f"{name} {v:.3g}" for name, v in figures.items())
          + f"; excluded by the gap rule {100 * excluded:.2f} %; sign ties {int((tie & judged).sum())}")
    for name, v in figures.items():
        _note(name, v)
    if cap:
        _note("excluded share", excluded)

    assert (value_err <= E).all(), f"{label}: eigenvalues outside E (worst {figures['eigenvalue err / E']:.3g} E)"
    assert (np.diff(values, axis=1) >= 0).all(), f"{label}: eigenvalues not ascending"
    assert (ref_res <= E).all(), f"{label}: the reference's own residual exceeds E"
    assert (res <= res_tol).all(), f"{label}: residual"
    assert (ortho <= 2.0 ** -21).all(), f"{label}: frame not orthonormal"
    assert (det[c > 0] > 0).all(), f"{label}: a frame is left-handed"
    assert np.array_equal(normals.view(np.uint32), frames[:, 0].view(np.uint32)), f"{label}: normals are not row 0"
    empty = c == 0
    assert (values[empty] == 0).all() and (frames[empty] == 0).all(), f"{label}: an empty row is not 0"
    assert (values[c == 1] == 0).all(), f"{label}: c == 1 must give eigenvalues of exactly 0"
    assert not cap or excluded <= MAX_EXCLUDED, f"{label}: the gap rule excludes {100 * excluded:.2f} % of the rows"
    assert (sin <= sin_tol)[judged].all(), f"{label}: normal direction"
    if signs:
        assert same_sign[judged & ~tie].all(), f"{label}: normal sign"
    want.update(trace=trace, E=E, judged=judged, excluded=excluded)
    return want


def check_batch(out, xyz, idx, label, **kw):
    return [check(tuple(t[i] for t in out), xyz[i], idx[i], f"{label} cloud {i}", **kw) for i in range(len(xyz))]


def check_shapes(m, device):
    """Every k of KS on the three clouds of m points: the reference, a second call and the one-cloud calls."""
    x, table = batch_of(m)
    for k in KS:
        idx = np.ascontiguousarray(table[:, :, :k])
        out = run(x, idx, device)
        check_batch(out, x, idx, f"m {m} k {k}", cap=k > 3)
        assert same_bits(run(x, idx, device), out), f"m {m} k {k}: a second call differs"
        for i in range(3):
            alone = run(x[i], idx[i], device)
            assert same_bits(alone, tuple(t[i] for t in out)), f"m {m} k {k}: cloud {i} depends on the batch"


def check_named_clouds(device):
    """Clouds (a) .. (e); returns {name: check's dict}."""
    done = {}
    for name, k in (("a", 16), ("b", 16), ("b", 5), ("c", 16), ("d", 8), ("e", 16)):
        x, idx = cloud(name), self_table(name, k)
        out = run(x, idx, device)
        done[(name, k)] = check(out, x, idx, f"cloud ({name}) k {k}")
        done[(name, k)]["out"] = out
    # (e) is (b) translated by +100: the centroid is subtracted in double, so the normals agree at the angle bound
    # of (e)'s own neighbourhoods (their coordinates were rounded to fp32 after the translation: E is (e)'s)
    b, e = done[("b", 16)], done[("e", 16)]
    judged = b["judged"] & e["judged"]
    nb, ne = b["out"][0].astype(np.float64), e["out"][0].astype(np.float64)
    sin = np.linalg.norm(np.cross(nb, ne), axis=1)
    gap = np.minimum(b["eigenvalues"][:, 1] - b["eigenvalues"][:, 0], e["eigenvalues"][:, 1] - e["eigenvalues"][:, 0])
    tol = 2.0 * (b["E"] + e["E"]) / np.where(judged, gap, 1.0) + 2.0 ** -21
    top = np.sort(np.abs(b["normals"]), axis=1)
    print(f"(e) against (b): sin / bound {(sin / tol)[judged].max():.3g} on {int(judged.sum())} rows")
    _note("(e) against (b): sin / bound", (sin / tol)[judged].max())
    assert (sin <= tol)[judged].all(), "(b) + 100 must have (b)'s normals: the centroid is subtracted in double"
    assert ((nb * ne).sum(axis=1) > 0)[judged & (top[:, 2] - top[:, 1] > 2.0 ** -20)].all()
    return done


def check_degenerate(device):
    x = cloud("a")
    # k copies of one point
    for k in (1, 5, 64):
        idx = np.repeat(np.arange(40, dtype=np.int32)[:, None], k, axis=1)
        out = run(x, idx, device)
        check(out, x, idx, f"{k} copies of one point")
        assert (out[1] == 0).all()
        assert np.array_equal(out[2], np.broadcast_to(np.eye(3, dtype=np.float32), out[2].shape))
    # exactly collinear points: integer multiples of a vector of small integers over 2^8
    t = np.arange(-20, 21, dtype=np.float64)
    line = (t[:, None] * np.array([1.0, 2.0, -1.0]) / 256.0 + np.array([0.5, 0.25, 0.125])).astype(np.float32)
    assert np.array_equal(line.astype(np.float64), t[:, None] * np.array([1.0, 2.0, -1.0]) / 256.0 + np.array([0.5, 0.25, 0.125]))
    idx = knn_ref(line, line, 7)[0]
    out = run(line, idx, device)
    want = check(out, line, idx, "collinear", cap=False)
    assert (np.abs(out[1][:, :2]) <= want["E"][:, None]).all(), "collinear: l0, l1 must be within E of 0"
    direction = out[2][:, 2].astype(np.float64)
    assert np.abs(np.abs(direction @ np.array([1.0, 2.0, -1.0]) / np.sqrt(6.0)) - 1.0).max() <= 2.0 ** -21
    # an exactly axis-aligned plane
    rng = np.random.default_rng(21)
    plane = np.concatenate([rng.random((400, 2)), np.full((400, 1), 0.25)], axis=1).astype(np.float32)
    for k in (3, 16, 33):
        idx = knn_ref(plane, plane, k)[0]
        out = run(plane, idx, device)
        check(out, plane, idx, f"plane z = 0.25, k {k}", cap=k > 3)
        up = np.broadcast_to(np.array([0.0, 0.0, 1.0], np.float32), out[0].shape)
        assert np.array_equal(out[0].view(np.uint32), up.view(np.uint32)), "plane: the normal is not (0, 0, 1) bit for bit"
        assert (out[1][:, 0] == 0).all()


def check_holes(device):
    x = cloud("a")
    idx = holes_table()
    out = run(x, idx, device)
    want = check(out, x, idx, "table with holes")
    assert sorted(set(want["c"][:4].tolist())) == [0, 1, 2, 3] and (want["c"][4:20] == 0).all()
    assert (out[0][0] == 0).all() and (out[1][0] == 0).all() and (out[2][0] == 0).all()
    ball = ball_table()
    hits = (ball >= 0).sum(axis=1)
    assert 1 <= hits.min() < 8 and hits.max() == 32 and (ball[hits < 32, -1] == -1).all()
    check(run(x, ball, device), x, ball, "ball_query(pad='none') table")
    xr, lengths = ragged_batch()
    table = ragged_table(xr, lengths)
    out = run(xr, table, device)
    assert not np.isnan(out[0]).any() and not np.isnan(out[1]).any() and not np.isnan(out[2]).any()
    for i, n in enumerate(lengths):
        check(tuple(t[i, :n] for t in out), xr[i, :n], table[i, :n], f"ragged cloud {i} ({n} points)", cap=n > 3)
        assert all((t[i, n:] == 0).all() for t in out), "padding rows must be 0"
        assert same_bits(tuple(t[i, :n] for t in out), run(xr[i, :n], table[i, :n], device)), "ragged against the cloud alone"


def check_queries_apart(device):
    """m = 130 farthest-point picks of a 700-point cloud as queries, their k = 8 table."""
    from fps_ref import fps_ref

    rng = np.random.default_rng(31)
    x = rng.random((700, 3)).astype(np.float32)
    q = x[fps_ref(x, 130)[0]]
    idx = knn_ref(x, q, 8)[0]
    out = run(x, idx, device)
    check(out, x, idx, "130 queries into 700 points")
    return x, q, idx, out


def check_signs(device):
    x, idx = cloud("b"), self_table("b", 16)
    plain = run(x, idx, device)
    # a viewpoint at the sphere's centre: every normal looks inward
    inward = run(x, idx, device, new_xyz=x, viewpoint=[0.0, 0.0, 0.0])
    check(inward, x, idx, "viewpoint at the centre", new_xyz=x, viewpoint=[0.0, 0.0, 0.0])
    assert ((inward[0].astype(np.float64) * x.astype(np.float64)).sum(axis=1) < 0).all()
    assert np.array_equal(np.abs(inward[0]), np.abs(plain[0])) and np.array_equal(inward[1], plain[1])
    assert np.array_equal(inward[2][:, 2], plain[2][:, 2]), "the principal direction does not depend on the viewpoint"
    # far outside along +x: exactly the rows with n_x < 0 in the canonical result are flipped
    far = run(x, idx, device, new_xyz=x, viewpoint=[1e8, 0.0, 0.0])
    flipped = (far[0] != plain[0]).any(axis=1)
    assert np.array_equal(flipped, plain[0][:, 0] < 0), "a far viewpoint along +x flips the rows with n_x < 0"
    assert np.array_equal(far[0][flipped], -plain[0][flipped]) and (far[0][:, 0] > 0).all()
    for out in (plain, inward, far):
        assert (np.linalg.det(out[2].astype(np.float64)) > 0).all(), "right-handed"
        assert (np.abs(out[2][:, 2]).max(axis=1) == out[2][:, 2].max(axis=1)).all(), "row 2 has the canonical sign"
    assert (np.abs(plain[0]).max(axis=1) == plain[0].max(axis=1)).all(), "the normal has the canonical sign"
    # [3] and [B,3] agree
    xb, tb = batch_of(257)
    tb = np.ascontiguousarray(tb[:, :, :16])
    view = np.array([0.3, -2.0, 0.7], np.float32)
    assert same_bits(run(xb, tb, device, new_xyz=xb, viewpoint=view), run(xb, tb, device, new_xyz=xb, viewpoint=np.tile(view, (3, 1))))
    views = np.array([[0.3, -2.0, 0.7], [5.0, 5.0, 5.0], [-1.0, 0.0, 0.0]], np.float32)
    per_cloud = run(xb, tb, device, new_xyz=xb, viewpoint=views)
    for i in range(3):
        assert same_bits(tuple(t[i] for t in per_cloud), run(xb[i], tb[i], device, new_xyz=xb[i], viewpoint=views[i]))
        check(tuple(t[i] for t in per_cloud), xb[i], tb[i], f"viewpoint of cloud {i}", new_xyz=xb[i], viewpoint=views[i], signs=False)


# ---------------------------------------------------------------------------------------------------- metrics
def plane_pair():
    """x on the exact plane z = 0.5 and y = the same plane's other points: (x, y, normals of y)."""
    rng = np.random.default_rng(41)
    x = np.concatenate([rng.random((300, 2)), np.full((300, 1), 0.5)], axis=1).astype(np.float32)
    y = np.concatenate([rng.random((260, 2)), np.full((260, 1), 0.5)], axis=1).astype(np.float32)
    n = np.broadcast_to(np.array([0.0, 0.0, 1.0], np.float32), y.shape).copy()
    return x, y, n


def check_point_to_plane(device):
    """Value and gradient of point_to_plane_chamfer against float64 with the indices held, at fp32-sum bounds."""
    import torch

    from sparenet_amd.cuda.normals import point_to_plane_chamfer

    u32 = 2.0 ** -24
    rng = np.random.default_rng(43)
    x = np.stack([cloud("c")[:700], cloud("a")[:700]])
    y = np.stack([cloud("b")[:900], rng.random((900, 3)).astype(np.float32)])
    n2 = rng.standard_normal((2, 900, 3))
    n2 = (n2 / np.linalg.norm(n2, axis=2, keepdims=True)).astype(np.float32)
    n2[0] = (y[0] / np.linalg.norm(y[0], axis=1, keepdims=True)).astype(np.float32)      # the sphere's own normals
    xt = torch.tensor(x, device=device, requires_grad=True)
    yt = torch.tensor(y, device=device, requires_grad=True)
    value = point_to_plane_chamfer(xt, yt, torch.tensor(n2, device=device))
    weights = torch.tensor([1.0, -0.5], device=device)
    (value * weights).sum().backward()
    value, gx, gy = value.detach().cpu().numpy(), xt.grad.cpu().numpy(), yt.grad.cpu().numpy()
    for i in range(2):
        idx1, idx2 = ref.chamfer_indices(x[i], y[i])
        xd = torch.tensor(x[i], dtype=torch.float64, requires_grad=True)
        yd = torch.tensor(y[i], dtype=torch.float64, requires_grad=True)
        nd = torch.tensor(n2[i], dtype=torch.float64)
        i1, i2 = torch.tensor(idx1, dtype=torch.long), torch.tensor(idx2, dtype=torch.long)
        off1 = (nd[i1] * (xd - yd[i1])).sum(dim=1)
        off2 = (nd * (yd - xd[i2])).sum(dim=1)
        want = (off1 * off1).mean() + (off2 * off2).mean()
        (want * float(weights[i])).backward()
        assert abs(want.item() - ref.point_to_plane(x[i], y[i], n2[i], idx1, idx2)) <= 1e-15
        # value: a dot product of 3 fp32 terms (4 roundings of sum |n_i d_i| = A), its square, an fp32 sum of the terms
        xn, yn, nn = x[i].astype(np.float64), y[i].astype(np.float64), n2[i].astype(np.float64)
        A1, A2 = (np.abs(nn[idx1]) * np.abs(xn - yn[idx1])).sum(axis=1), (np.abs(nn) * np.abs(yn - xn[idx2])).sum(axis=1)
        o1, o2 = off1.detach().numpy(), off2.detach().numpy()
        tol = u32 * ((8 * np.abs(o1) * A1 + 2 * o1 * o1).mean() + (8 * np.abs(o2) * A2 + 2 * o2 * o2).mean()) \
            + u32 * (len(x[i]) * (o1 * o1).mean() + len(y[i]) * (o2 * o2).mean())
        err = abs(float(value[i]) - want.item())
        # gradient: per point the own term and the terms of the points that chose it, an fp32 sum of 1 + list terms
        sx = np.abs(float(weights[i])) * 2 * A1[:, None] * np.abs(nn[idx1]) / len(x[i])
        sy = np.abs(float(weights[i])) * 2 * A2[:, None] * np.abs(nn) / len(y[i])
        np.add.at(sx, idx2, np.abs(float(weights[i])) * 2 * A2[:, None] * np.abs(nn) / len(y[i]))
        np.add.at(sy, idx1, np.abs(float(weights[i])) * 2 * A1[:, None] * np.abs(nn[idx1]) / len(x[i]))
        lx, ly = 1 + np.bincount(idx2, minlength=len(x[i])), 1 + np.bincount(idx1, minlength=len(y[i]))
        ex, ey = np.abs(gx[i] - xd.grad.numpy()), np.abs(gy[i] - yd.grad.numpy())
        tx, ty = u32 * (lx[:, None] + 10) * sx, u32 * (ly[:, None] + 10) * sy
        print(f"point to plane cloud {i}: value {value[i]:.9g} ref {want.item():.9g} err {err:.3g} tol {tol:.3g}; grad err / bound "
              f"{(ex / np.where(tx > 0, tx, 1)).max():.3g} {(ey / np.where(ty > 0, ty, 1)).max():.3g}")
        assert err <= tol, f"point to plane value, cloud {i}"
        assert (ex <= tx).all() and (ey <= ty).all(), f"point to plane gradient, cloud {i}"
    # points displaced inside the tangent plane of an exact plane: value 0, gradient 0
    px, py, pn = plane_pair()
    xt = torch.tensor(px[None], device=device, requires_grad=True)
    yt = torch.tensor(py[None], device=device, requires_grad=True)
    value = point_to_plane_chamfer(xt, yt, torch.tensor(pn[None], device=device))
    value.sum().backward()
    assert value.item() == 0.0 and (xt.grad == 0).all() and (yt.grad == 0).all()
