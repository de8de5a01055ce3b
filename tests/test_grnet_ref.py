"""tests/grnet_ref.py (the plain NumPy reference of the GRNet grid ops and the graph ops) against the goldens and
against oracle/*.c, on EVERY input tests/test_grnet_edges.py gives the HIP kernels (tests/grnet_cases.py builds
them for both files).  Exact parts bit for bit, sums inside the derived bound (grnet_ref's docstring).  CPU only."""
import glob
import os
import re

import numpy as np
import pytest

import grnet_cases as C
import grnet_ref as R
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden(golden_dir, pat):
    files = sorted(glob.glob(os.path.join(golden_dir, pat)))
    assert files
    return files


# ------------------------------------------------------------------------------------------------ goldens
def test_ref_reproduces_gridding_goldens(golden_dir):
    for f in _golden(golden_dir, "gridding_*.npz"):
        z = np.load(f)
        scale = int(z["scale"])
        r = R.gridding(z["ptcloud"], scale // 2)
        assert np.array_equal(r["weights"], z["weights"]) and np.array_equal(r["indexes"], z["indexes"]), f
        R.assert_within(z["grid"], r["grid"], r["bound"], f)
        g, a = R.gridding_backward(z["grad_grid"], z["weights"], z["indexes"])
        R.assert_within(z["grad_ptcloud"], g, R.sum_bound(8, 2, a), f + " backward")
        fw = R.reverse_forward(z["rev_grid"], scale)
        assert np.array_equal(fw["pts32"], z["rev_ptcloud"]), f
        bw = R.reverse_backward(z["rev_grad_ptcloud"], z["rev_grid"], z["rev_ptcloud"], scale)
        R.assert_within(z["rev_grad_grid"], bw["grad"], bw["bound"], f + " reverse backward")
        assert C.threshold_clearance(z["rev_grid"], scale) >= C.THRESHOLD_CLEARANCE


def test_ref_reproduces_griddist_goldens(golden_dir):
    for f in _golden(golden_dir, "griddist_*.npz"):
        z = np.load(f)
        r = R.gridding_dist(z["ptcloud"], z["bounds"])
        assert np.array_equal(r["weights"], z["weights"]) and np.array_equal(r["indexes"], z["indexes"]), f
        R.assert_within(z["grid"].reshape(r["grid"].shape), r["grid"], r["bound"], f)
        g, a = R.gridding_backward(z["grad_grid"], z["weights"], z["indexes"])
        R.assert_within(z["grad_ptcloud"], g, R.sum_bound(8, 2, a), f + " backward")


def test_ref_reproduces_cubic_goldens(golden_dir):
    for f in _golden(golden_dir, "cubic_*.npz"):
        z = np.load(f)
        ns, scale = int(z["neighborhood_size"]), z["feat"].shape[2]
        idx = R.cubic_index(z["ptcloud"], scale, ns)
        assert np.array_equal(idx, z["indexes"]), f
        assert np.array_equal(R.cubic_gather(z["feat"], idx), z["out"]), f
        g, k, a = R.cubic_scatter(z["grad_out"], idx, scale)
        R.assert_within(z["grad_feat"].reshape(g.shape), g, R.sum_bound(k[:, None], 0, a), f + " backward")


def test_ref_reproduces_knn_goldens(golden_dir):
    for f in _golden(golden_dir, "knn_*.npz"):
        z = np.load(f)
        k = int(z["k"])
        assert R.rows_valid(z["idx"], z["x"], k, R.knn_tau(z["x"])) == {}, f
        ref = R.graph_feature(z["x"], z["idx"])
        R.assert_within(z["feature"], ref, R.sum_bound(1, 1, np.abs(ref)), f)


# ------------------------------------------------------------------------------------------------ ref vs oracle
def _same_gridding(pt, s, what):
    """grnet_ref vs oracle on one cloud: plain, padded (oracle on the kept rows of every sample) and the backward."""
    r = R.gridding(pt, s)
    og, ow, oi = oracle.gridding_forward(pt, 2 * s)
    assert np.array_equal(r["weights"], ow) and np.array_equal(r["indexes"], oi), what
    R.assert_within(og, r["grid"], r["bound"], what)
    gg = C.grad_like(og.shape, 3)
    g, a = R.gridding_backward(gg, r["weights"], r["indexes"])
    R.assert_within(oracle.gridding_backward(gg, ow, oi), g, R.sum_bound(8, 2, a), what + " backward")
    p = R.gridding(pt, s, skip_zero_rows=True)
    drop = R.padding_rows(pt)
    assert (p["weights"][drop] == 0).all() and (p["indexes"][drop] == -1).all()
    for b in range(len(pt)):
        kg, kw, ki = oracle.gridding_forward(pt[b:b + 1][:, ~drop[b]], 2 * s)
        assert np.array_equal(p["weights"][b][~drop[b]], kw[0]) and np.array_equal(p["indexes"][b][~drop[b]], ki[0])
        R.assert_within(kg[0], p["grid"][b], p["bound"][b], what + " padded")
    g, a = R.gridding_backward(gg, p["weights"], p["indexes"])
    assert (g[drop] == 0).all() and (a[drop] == 0).all()
    return r


def _same_dist(pt, bounds, what):
    r = R.gridding_dist(pt, bounds)
    og, ow, oi = oracle.gridding_dist_forward(pt, bounds)
    assert np.array_equal(r["weights"], ow) and np.array_equal(r["indexes"], oi), what
    R.assert_within(og.reshape(r["grid"].shape), r["grid"], r["bound"], what)
    gg = C.grad_like(r["grid"].shape, 4)
    g, a = R.gridding_backward(gg, r["weights"], r["indexes"])
    R.assert_within(oracle.gridding_backward(gg, ow, oi), g, R.sum_bound(8, 2, a), what + " backward")


@pytest.mark.parametrize("s", C.LATTICE_HALF_SCALES)
def test_ref_agrees_with_oracle_on_lattice_inputs(s):
    pt = C.lattice_batch(s)
    r = _same_gridding(pt, s, f"lattice s={s}")
    # the guards are reached: corners below 0, past the end, and wrapped into a neighbouring row
    ix = r["indexes"].astype(np.int64)
    assert (ix < 0).any() and (ix >= (2 * s) ** 3).any() and r["valid"][0].any()
    alone = R.gridding(pt[2:3], s)
    assert np.array_equal(alone["grid"][0], r["grid"][2])
    for tighter in (False, True):
        _same_dist(pt, C.lattice_bounds(s, tighter), f"lattice dist s={s} tighter={tighter}")


def test_ref_agrees_with_oracle_on_padding_inputs():
    import torch

    pt, where = C.padding_batch()
    half = C.PADDING_SCALE // 2
    scaled = (pt * np.float32(half)).astype(np.float32)
    # the rule as the reference's Python writes it, fp32 on the CPU
    keep = torch.sum(torch.from_numpy(pt.copy()) * half, dim=2).ne(0).numpy()
    assert np.array_equal(keep, ~R.padding_rows(scaled))
    for b in range(2):
        special = dict(zip(map(tuple, pt[b, where[b]].tolist()), keep[b, where[b]]))
        assert sum(special.values()) == 1 and keep[b].sum() == 201     # only (3e-4, -1e-4, -2e-4) survives
    _same_gridding(scaled, half, "padding")
    bounds = C.dist_bounds(scaled)
    for b in range(2):
        _same_dist(scaled[b:b + 1][:, keep[b]], bounds, "padding dist")


def test_ref_agrees_with_oracle_on_cap_inputs():
    pt = C.cap_points()
    s = C.CAP_SCALE // 2
    _same_gridding(pt, s, "cap gridding")
    _same_dist(pt, C.lattice_bounds(s, False), "cap dist")
    cp = C.cap_cubic_points()
    feat = C.cubic_feat(C.CAP_BATCH, 1, C.CAP_SCALE, 21)
    out, oi = oracle.cubic_forward(cp, feat, 1)
    idx = R.cubic_index(cp, C.CAP_SCALE, 1)
    assert np.array_equal(idx, oi) and np.array_equal(R.cubic_gather(feat, idx), out)
    go = C.grad_like(out.shape, 22)
    g, k, a = R.cubic_scatter(go, idx, C.CAP_SCALE)
    R.assert_within(oracle.cubic_backward(go, oi, 1, C.CAP_SCALE, 1).reshape(g.shape), g, R.sum_bound(k[:, None], 0, a),
                    "cap cubic backward")


def _same_reverse(grid, scale, what):
    f = R.reverse_forward(grid, scale)
    assert C.threshold_clearance(grid, scale, f) >= C.THRESHOLD_CLEARANCE, what
    op = oracle.gridding_reverse_forward(grid, scale)
    assert np.array_equal(f["pts32"], op), what
    R.assert_within(f["pts32"], f["pts64"], R.sum_bound(8, 2, f["A"]), what + " fp32 chain vs float64")
    gp = C.grad_like(op.shape, 5)
    bw = R.reverse_backward(gp, grid, op, scale, f)
    og = oracle.gridding_reverse_backward(gp, grid, op, scale).reshape(bw["grad"].shape)
    R.assert_within(og, bw["grad"], bw["bound"], what + " backward")
    assert (og[~bw["read"]] == 0).all()
    return f


def test_ref_agrees_with_oracle_on_cap_reverse_input():
    f = _same_reverse(C.cap_reverse_grid(), C.CAP_REVERSE_SCALE, "cap reverse")
    assert 0 < f["valid"].mean() < 0.2                                  # sparse


@pytest.mark.parametrize("scale", C.REVERSE_SCALES)
def test_ref_agrees_with_oracle_on_reverse_inputs(scale):
    grids = C.reverse_grids(scale)
    for name, grid in grids.items():
        f = _same_reverse(grid, scale, f"reverse {name} scale={scale}")
        if scale == 1:
            assert not f["valid"].any()
    if scale >= 5:
        m = np.broadcast_to(R.reverse_forward(grids["mixed"], scale)["interior"][None], (2, scale ** 3))
        s64 = R.reverse_forward(grids["mixed"], scale)["sum64"][m]
        assert (np.abs(s64) >= 0.1).all() and (s64 < 0).any() and (s64 > 0).any()
        t = R.reverse_forward(grids["threshold"], scale)
        levels = np.unique(t["wsum"][m])
        assert set(levels.tolist()) == {float(np.float32(v)) for v in C.THRESHOLD_LEVELS}   # one isolated vertex per cell
        assert t["valid"].any() and (~t["valid"][m]).any()


@pytest.mark.parametrize("scale", C.CUBIC_SCALES)
@pytest.mark.parametrize("ns", C.CUBIC_NS)
def test_ref_agrees_with_oracle_on_cubic_inputs(scale, ns):
    pt = C.cubic_points(scale, ns)
    idx = R.cubic_index(pt, scale, ns)
    assert (idx == -1).any() and (idx == scale ** 3 - 1).any() and (idx == 0).any()
    for c in C.CUBIC_CHANNELS:
        feat = C.cubic_feat(2, c, scale, c)
        out, oi = oracle.cubic_forward(pt, feat, ns)
        assert np.array_equal(idx, oi) and np.array_equal(R.cubic_gather(feat, idx), out), (scale, ns, c)


def test_ref_agrees_with_oracle_on_cubic_backward_inputs():
    for pt, ns, single in ((C.cubic_one_cell_points(), 2, False), (C.cubic_single_writer_points(), 1, True)):
        idx = R.cubic_index(pt, 8, ns)
        go = C.grad_like(idx.shape + (3,), 6)
        g, k, a = R.cubic_scatter(go, idx, 8)
        assert k.max() == (1 if single else 600)
        og = oracle.cubic_backward(go, idx, 3, 8, ns).reshape(g.shape)
        R.assert_within(og, g, R.sum_bound(k[:, None], 0, a), "cubic backward")
        if single:
            assert np.array_equal(og, g.astype(np.float32))


def test_ref_agrees_with_oracle_on_edge_feature_inputs():
    b, c, n, k = C.CAP_EDGE
    x = np.random.default_rng(31).standard_normal((b, c, n)).astype(np.float32)
    _, idx = R.knn_exact(x, k)
    assert np.array_equal(idx, oracle.knn(x, k))
    ref = R.graph_feature(x, idx)
    R.assert_within(oracle.graph_feature(x, idx), ref, R.sum_bound(1, 1, np.abs(ref)), "edge features")


# ------------------------------------------------------------------------------------------------ the caps
def test_cap_crossing_sizes_still_cross_the_caps():
    """The sizes of the cap-crossing cases are chosen against the launch caps in the kernels' source; a later change of a
    cap must flag them as stale."""
    def constant(path, name):
        m = re.search(r"constexpr int %s = (\d+);" % name, open(os.path.join(ROOT, "sparenet_amd", "csrc", path)).read())
        assert m, (path, name)
        return int(m.group(1))

    lin = constant("gridding.hip", "kMaxLinBlocks") * 256
    assert C.CAP_BATCH * C.CAP_POINTS > lin and (C.CAP_BATCH * C.CAP_POINTS - lin) % 256 != 0
    assert C.CAP_REVERSE_BATCH * C.CAP_REVERSE_SCALE ** 3 > lin
    assert C.CAP_BATCH * C.CAP_POINTS * 8 > lin                          # cubic gather / scatter, c = 1, ns = 1
    # the edge-feature launches stay far below their cap on purpose (tests/test_grnet_edges.py says why)
    b, c, n, k = C.CAP_EDGE
    assert b * c * n * k == 360000 and b * 2 * c * n * k < constant("knn.hip", "kMaxBlocks") * 256
