"""Gridding, gridding distance, GriddingReverse and CubicFeatureSampling (csrc/gridding.hip) on the GPU, at the inputs the
goldens and the GRNet-size tests do not reach: coordinates on the lattice and at the grid's edge, the padding rule,
launches past the grid-stride cap, cubic neighbourhoods at the volume's faces, sparse / threshold / mixed-sign grids for
the reverse op, and the size refusals of the two gridding entry points.

Every expectation comes from tests/grnet_ref.py: indexes, weights and single-writer outputs bit for bit, atomic sums
inside the bound derived there (no rtol / atol).  tests/test_grnet_ref.py checks on the CPU that grnet_ref and oracle
agree on these very inputs (tests/grnet_cases.py builds them for both)."""
import ctypes

import numpy as np
import pytest
import torch

import grnet_cases as C
import grnet_ref as R

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


def _check_grid(got, r, what):
    """(grid, weights, indexes) of the GPU against a grnet_ref result."""
    grid, w, ix = got
    assert np.array_equal(_np(ix), r["indexes"]), what + ": indexes"
    assert np.array_equal(_np(w), r["weights"]), what + ": weights"
    R.assert_within(_np(grid).reshape(r["grid"].shape), r["grid"], r["bound"], what + ": grid")


def _check_grad(got, grad_grid, r, dropped, what):
    g, a = R.gridding_backward(grad_grid.reshape(len(grad_grid), -1), r["weights"], r["indexes"])
    got = _np(got)
    R.assert_within(got, g, R.sum_bound(8, 2, a), what + ": backward")
    assert (got[dropped] == 0).all(), what + ": a dropped row has a gradient"


def _gridding(pt, s, padded, grad_grid, dev):
    """GriddingFunction forward + backward -> ((grid, weights, indexes), grad_ptcloud)."""
    from sparenet_amd.cuda.gridding import GriddingFunction

    p = torch.from_numpy(np.array(pt)).to(dev).requires_grad_(True)
    grid = GriddingFunction.apply(s, p, padded)
    w, ix = grid.grad_fn.saved_tensors
    grid.backward(torch.from_numpy(grad_grid).to(dev))
    return (grid, w, ix), p.grad


def _gridding_dist(pt, bounds, grad_grid, dev):
    """GriddingDistanceFunction (the cloud as prediction and as ground truth) -> the same."""
    from sparenet_amd.cuda.gridding_loss import GriddingDistanceFunction

    p = torch.from_numpy(np.array(pt)).to(dev).requires_grad_(True)
    q = p.detach().clone().requires_grad_(True)
    pg, qg = GriddingDistanceFunction.apply(*bounds, p, q)
    pw, pi, qw, qi = pg.grad_fn.saved_tensors
    gg = torch.from_numpy(grad_grid).to(dev).view(pg.shape)
    torch.autograd.backward([pg, qg], [gg, gg])
    assert torch.equal(pw, qw) and torch.equal(pi, qi) and torch.equal(p.grad, q.grad)
    return (pg, pw, pi), p.grad, qg


# ------------------------------------------------------------------------------------------------ a. lattice and edges
@pytest.mark.parametrize("s", C.LATTICE_HALF_SCALES)
def test_lattice_and_edge_coordinates(s, dev):
    """Integer coordinates (up = lo + 1), -0.0, points in [s - 1, s) whose upper corner wraps into the next row or leaves
    the slab, points outside on one axis or on all: the `0 <= idx < nverts` guards of the forward, distance and backward
    kernels are all that keeps sample 2's grid clean."""
    pt = C.lattice_batch(s)
    nverts = (2 * s) ** 3
    gg = C.grad_like((3, nverts), 3)
    alone = R.gridding(pt[2:3], s)
    for padded in (False, True):
        what = f"s={s} padded={padded}"
        r = R.gridding(pt, s, skip_zero_rows=padded)
        got, grad = _gridding(pt, s, padded, gg, dev)
        _check_grid(got, r, what)
        _check_grad(grad, gg, r, ~r["valid"].any(2), what)
        if not padded:      # nothing leaks across slabs: sample 2 against sample 2 gridded alone
            R.assert_within(_np(got[0])[2], alone["grid"][0], alone["bound"][0], what + ": sample 2 alone")
    for tighter in (False, True):
        bounds = C.lattice_bounds(s, tighter)
        what = f"dist s={s} tighter={tighter}"
        r = R.gridding_dist(pt, bounds)
        gg8 = C.grad_like(r["grid"].shape, 4)
        got, grad, twin = _gridding_dist(pt, bounds, gg8, dev)
        _check_grid(got, r, what)
        R.assert_within(_np(twin).reshape(r["grid"].shape), r["grid"], r["bound"], what + ": second cloud")
        _check_grad(grad, gg8, r, ~r["valid"].any(2), what)
        alone8 = R.gridding_dist(pt[2:3], bounds)
        R.assert_within(_np(got[0]).reshape(3, -1)[2], alone8["grid"][0], alone8["bound"][0], what + ": sample 2 alone")


# ------------------------------------------------------------------------------------------------ b. padding rule
def test_padding_rule(dev):
    """Rows whose scaled coordinates sum to zero in fp32 -- (x + y) + z, the reference's torch.sum(p * scale, dim=2).ne(0)
    taken on the CPU -- are dropped by the Gridding module (in the kernel) and by GriddingDistance (on the host): zeros,
    -0.0, rows that cancel exactly, rows that cancel only through underflow-free tiny values; (3e-4, -1e-4, -2e-4) does not
    cancel in fp32 and stays."""
    from sparenet_amd.cuda.gridding import Gridding
    from sparenet_amd.cuda.gridding_loss import GriddingDistance

    pt, where = C.padding_batch()
    half = C.PADDING_SCALE // 2
    keep = torch.sum(torch.from_numpy(pt.copy()) * half, dim=2).ne(0).numpy()
    assert keep.sum(1).tolist() == [201, 201]
    scaled = (pt * np.float32(half)).astype(np.float32)
    kept = [scaled[b:b + 1][:, keep[b]] for b in range(2)]

    p = torch.from_numpy(pt.copy()).to(dev).requires_grad_(True)
    grid = Gridding(scale=C.PADDING_SCALE)(p)
    w, ix = grid.grad_fn.saved_tensors
    gg = C.grad_like(tuple(grid.shape), 8)
    grid.backward(torch.from_numpy(gg).to(dev))
    w, ix, g, grad = _np(w), _np(ix), _np(grid), _np(p.grad)
    assert (w[~keep] == 0).all() and (ix[~keep] == -1).all()
    assert (grad[~keep] == 0).all()
    for b in range(2):
        r = R.gridding(kept[b], half)
        assert np.array_equal(ix[b][keep[b]], r["indexes"][0]) and np.array_equal(w[b][keep[b]], r["weights"][0])
        R.assert_within(g[b], r["grid"][0], r["bound"][0], f"padding: grid of sample {b}")
        gr, a = R.gridding_backward(gg[b:b + 1], r["weights"], r["indexes"])
        # the module multiplies by scale // 2 (a power of two: exact) on the way in, so the chain rule does on the way out
        R.assert_within(grad[b][keep[b]], gr[0] * half, R.sum_bound(8, 2, a[0]) * half, f"padding: backward of sample {b}")
        total = g[b].astype(np.float64).sum()
        print(f"padding: sample {b} grid total {total!r} for {keep[b].sum()} kept rows")
        assert abs(total - keep[b].sum()) <= r["bound"][0].sum() + keep[b].sum() * R.UNITY_BOUND

    pg, qg = GriddingDistance(scale=C.PADDING_SCALE)(torch.from_numpy(pt.copy()).to(dev),
                                                     torch.from_numpy(pt[::-1].copy()).to(dev))
    bounds = C.dist_bounds(scaled)
    for b in range(2):
        for got, cloud in ((pg, kept[b]), (qg, kept[1 - b])):
            r = R.gridding_dist(cloud, bounds)
            assert got[b].numel() == r["grid"].size
            R.assert_within(_np(got[b]).reshape(-1), r["grid"][0], r["bound"][0], f"padding: distance grid {b}")
            total = _np(got[b]).astype(np.float64).sum()
            assert abs(total - cloud.shape[1]) <= r["bound"][0].sum() + cloud.shape[1] * R.UNITY_BOUND


# ------------------------------------------------------------------------------------------------ c. cap crossings
def test_cap_crossing_gridding(dev):
    """2,100,003 points: gridding_fwd_kernel and gridding_bwd_kernel run their grid-stride loop a second time (2,851
    elements: 11 full blocks and one of 35 threads)."""
    pt = C.cap_points()
    s = C.CAP_SCALE // 2
    gg = C.grad_like((C.CAP_BATCH, C.CAP_SCALE ** 3), 3)
    r = R.gridding(pt, s)
    got, grad = _gridding(pt, s, False, gg, dev)
    _check_grid(got, r, "cap")
    _check_grad(grad, gg, r, ~r["valid"].any(2), "cap")


def test_cap_crossing_gridding_distance(dev):
    """The same points through gridding_dist_fwd_kernel and the backward with eight slots per vertex."""
    pt = C.cap_points()
    bounds = C.lattice_bounds(C.CAP_SCALE // 2, False)
    r = R.gridding_dist(pt, bounds)
    gg = C.grad_like(r["grid"].shape, 4)
    got, grad, _ = _gridding_dist(pt, bounds, gg, dev)
    _check_grid(got, r, "cap dist")
    _check_grad(grad, gg, r, ~r["valid"].any(2), "cap dist")


def _reverse(grid, scale, dev, what):
    """GriddingReverseFunction forward + backward on one grid against grnet_ref; returns the forward reference."""
    from sparenet_amd.cuda.gridding import GriddingReverseFunction

    f = R.reverse_forward(grid, scale)
    assert C.threshold_clearance(grid, scale, f) >= C.THRESHOLD_CLEARANCE, what
    g = torch.from_numpy(grid.copy()).to(dev).view(-1, scale, scale, scale).requires_grad_(True)
    pts = GriddingReverseFunction.apply(scale, g)
    got = _np(pts)
    assert np.array_equal(got, f["pts32"]), what + ": forward"
    assert (got[~f["valid"]] == 0).all()
    gp = C.grad_like(got.shape, 5)
    pts.backward(torch.from_numpy(gp).to(dev))
    bw = R.reverse_backward(gp, grid, f["pts32"], scale, f)
    gg = _np(g.grad).reshape(bw["grad"].shape)
    R.assert_within(gg, bw["grad"], bw["bound"], what + ": backward")
    assert (gg[~bw["read"]] == 0).all(), what + ": a vertex no valid cell reads has a gradient"
    return f


def test_cap_crossing_reverse(dev):
    """3 x 96^3 = 2,654,208 cells of a sparse grid (3,000 gridded points per sample): gridding_rev_fwd_kernel and
    gridding_rev_bwd_kernel loop twice.  (96^3 is a multiple of 256, so the second pass has no partial block; the
    gridding case above covers that.)"""
    f = _reverse(C.cap_reverse_grid(), C.CAP_REVERSE_SCALE, dev, "cap reverse")
    assert f["valid"][2].any()           # the last sample, past the cap, produces points


def test_cap_crossing_cubic(dev):
    """The 2,100,003 points in a scale-8 volume, c = 1, ns = 1: cubic_index_kernel loops twice, the gather and the scatter
    (16.8 M elements) nine times."""
    from sparenet_amd.cuda.cubic_feature_sampling import CubicFeatureSamplingFunction

    pt = C.cap_cubic_points()
    feat = C.cubic_feat(C.CAP_BATCH, 1, C.CAP_SCALE, 21)
    idx = R.cubic_index(pt, C.CAP_SCALE, 1)
    ft = torch.from_numpy(feat).to(dev).requires_grad_(True)
    out = CubicFeatureSamplingFunction.apply(torch.from_numpy(np.array(pt)).to(dev), ft, 1)
    assert np.array_equal(_np(out.grad_fn.saved_tensors[0]), idx)
    assert np.array_equal(_np(out), R.cubic_gather(feat, idx))
    go = C.grad_like(tuple(out.shape), 22)
    out.backward(torch.from_numpy(go).to(dev))
    g, k, a = R.cubic_scatter(go, idx, C.CAP_SCALE)
    R.assert_within(_np(ft.grad).reshape(g.shape), g, R.sum_bound(k[:, None], 0, a), "cap cubic backward")


def test_edge_features_largest_case(dev):
    """Edge features forward + backward at b = 2, c = 3, n = 3000, k = 20: 360,000 elements.  Their launches are capped at
    65,535 blocks of 256 = 16.7 M elements; a case past that cap would need a 16.7 M-element edge tensor per channel pair
    and a [b, n, n] search to build it, far beyond a few seconds, so the grid-stride loops of graph_feature_fwd_kernel,
    index_lists_count_kernel, index_lists_fill_kernel and graph_feature_bwd_kernel stay UNTESTED past their first pass."""
    from sparenet_amd.cuda.knn import get_graph_feature

    b, c, n, k = C.CAP_EDGE
    x = np.random.default_rng(31).standard_normal((b, c, n)).astype(np.float32)
    _, idx = R.knn_exact(x, k)
    xt = torch.from_numpy(x).to(dev).requires_grad_(True)
    out = get_graph_feature(xt, k=k, idx=torch.from_numpy(idx).to(dev))
    ref = R.graph_feature(x, idx)
    R.assert_within(_np(out), ref, R.sum_bound(1, 1, np.abs(ref)), "edge features")
    go = C.grad_like(tuple(out.shape), 32)
    out.backward(torch.from_numpy(go).to(dev))
    g, terms, a = R.graph_feature_backward(go, idx)
    R.assert_within(_np(xt.grad), g, R.sum_bound(terms[:, None], 1, a), "edge features backward")


# ------------------------------------------------------------------------------------------------ d. cubic sampling
@pytest.mark.parametrize("scale", C.CUBIC_SCALES)
@pytest.mark.parametrize("ns", C.CUBIC_NS)
def test_cubic_sampling_at_the_faces(scale, ns, dev):
    """Integer points (0 and scale - 1 included), points up to ns + 1 cells outside every face, interior points; a volume
    that is no power of two; channel counts that are no multiple of the wave.  Indexes and outputs bit for bit."""
    from sparenet_amd.cuda.cubic_feature_sampling import CubicFeatureSamplingFunction

    pt = C.cubic_points(scale, ns)
    idx = R.cubic_index(pt, scale, ns)
    pd = torch.from_numpy(pt).to(dev)
    for c in C.CUBIC_CHANNELS:
        feat = C.cubic_feat(2, c, scale, c)
        out = CubicFeatureSamplingFunction.apply(pd, torch.from_numpy(feat).to(dev).requires_grad_(True), ns)
        assert np.array_equal(_np(out.grad_fn.saved_tensors[0]), idx), (scale, ns, c)
        assert np.array_equal(_np(out), R.cubic_gather(feat, idx)), (scale, ns, c)


@pytest.mark.parametrize("single", (False, True))
def test_cubic_backward_contention(single, dev):
    """600 points in one cell (ns = 2: every one of the 64 destinations takes 600 atomic adds per channel) inside the bound;
    one point in every second cell (every destination has a single writer) bit for bit."""
    from sparenet_amd.cuda.cubic_feature_sampling import CubicFeatureSamplingFunction

    pt, ns = (C.cubic_single_writer_points(), 1) if single else (C.cubic_one_cell_points(), 2)
    idx = R.cubic_index(pt, 8, ns)
    ft = torch.from_numpy(C.cubic_feat(1, 3, 8, 9)).to(dev).requires_grad_(True)
    out = CubicFeatureSamplingFunction.apply(torch.from_numpy(pt).to(dev), ft, ns)
    go = C.grad_like(tuple(out.shape), 6)
    out.backward(torch.from_numpy(go).to(dev))
    g, k, a = R.cubic_scatter(go, idx, 8)
    assert k.max() == (1 if single else 600)
    got = _np(ft.grad).reshape(g.shape)
    R.assert_within(got, g, R.sum_bound(k[:, None], 0, a), "cubic backward")
    if single:
        assert np.array_equal(got, g.astype(np.float32))


# ------------------------------------------------------------------------------------------------ e. GriddingReverse
@pytest.mark.parametrize("scale", C.REVERSE_SCALES)
def test_gridding_reverse_grids(scale, dev):
    """A sparse grid (what Gridding produces), a grid whose 8-cell sums sit on both sides of the 1e-6 threshold (never
    closer than 5 %), and a mixed-sign grid with |sum| >= 0.1, at scale 1 (no cell), 2 (one cell), odd 5 and 32."""
    for name, grid in C.reverse_grids(scale).items():
        f = _reverse(grid, scale, dev, f"reverse {name} scale={scale}")
        if name != "mixed":          # (a mixed-sign grid of one cell may hold two negative sums)
            assert f["valid"].any() == (scale > 1), name


# ------------------------------------------------------------------------------------------------ f. size refusals
def test_gridding_size_refusals(dev):
    """Host code only: both gridding entry points take an even scale in [2, 1024] and refuse anything else."""
    from sparenet_amd import SparenetHipError, _lib

    one, grid, w = (torch.zeros(64, device=dev) for _ in range(3))
    ione = torch.zeros(64, dtype=torch.int32, device=dev)
    for name in ("sn_gridding_forward", "sn_gridding_forward_padded"):
        for scale in (3, 7, 1, 0, -2, 1026, 1 << 20):
            with pytest.raises(SparenetHipError, match=name + ": bad sizes"):
                _lib.call(name, one, 1, 1, scale, grid, w, ione)
        with pytest.raises(SparenetHipError, match="an even scale in \\[2, 1024\\]"):
            _lib.call(name, one, 1, 1, 5, grid, w, ione)
        with pytest.raises(SparenetHipError, match=name + ": bad sizes"):
            _lib.call(name, one, 0, 1, 2, grid, w, ione)
        _lib.call(name, one, 1, 1, 2, grid, w, ione)            # the smallest accepted size: 8 vertices, one point
    lib = _lib.lib()
    p = ctypes.c_void_p(one.data_ptr())
    assert lib.sn_gridding_forward(p, 1, 1, 1025, p, p, p, None) == -22
    assert b"sn_gridding_forward: bad sizes" in lib.sn_last_error()
