"""Sinkhorn transport on the GPU against the NumPy reference (tests/sinkhorn_ref.py).

The tolerance is the rule of sinkhorn_ref.tolerance(): for every compared quantity q the float64 reference q64 and the
same code in fp32, q32, are computed on the CPU, and the kernel must satisfy
    max|q_gpu - q64| <= 4 * max(E32, floor),   E32 = max|q32 - q64|,   floor = 2^-22 * max(1, max|q64|).
Every case runs with SN_SINKHORN_SPLIT = 1 (the wide path: 256 queries per workgroup, tiles of 1024 targets), 3 and 16
(the split path: one wave per segment, tiles of 192 targets, merged in LDS) and unset (the dispatch); sizes sit at the
edges of lanes (64), workgroups (256 / 64 queries), chunks (8 targets) and tiles.  Every check prints its figures
(`pytest -s`).

Measured on an MI355X: the largest error over the four split settings as a multiple of max(E32, floor) -- 4 is allowed
-- with the absolute error in brackets ("Sinkhorn transport", has the full table):
    edges 1/1 ... 1023/257            f, g <= 0.60 (1.4e-7), value <= 0.03
    1/1025 (one query)                f 0.68 (3.8e-7), g 0.73 (4.5e-7), value 0.14
    1025/1 (one target)               f 2.01 (8.3e-7), g 3.10 (7.4e-7), value 0.03     the closest case: g = C - f exactly,
                                      the iteration has no restoring force and every half-step adds its rounding
    2049/2047 eps=0.0025              f 0.24 (5.8e-8), g 0.23, value 0.01
    257/255 eps=0.001                 f 0.35 (1.1e-7), g 0.36, value 0.01
    far apart 65/63                   f 0.61 (2.7e-6; E32 4.4e-6), g 0.64, value 0.05
    coincident / collapsed            f 0.22 / 1.69 (4.8e-7), g 0.21 / 1.65, value 0.01 / 0.10
    ragged                            f 0.58, g 0.64, value 0.02, x.grad 1.59 (3.8e-7), y.grad 0.04
    warm start                        f 0.32, g 0.29
    barycentres 257/255, 1025/63      bary 1.36 (3.2e-7) / 1.20, softmin 0.08 / 0.10
    gradients, divergence             <= 0.03; S(x, x) exactly 0
    eps=1e4 65/63                     f 0.14 (2.5e-3; E32 1.8e-2), g 0.10, value 0.03, value against mean(C) 0.03 (6e-5)
    eps=1e-4 permuted copies          <P,C> equals the optimal assignment cost to 6 digits (allowed gap 4.2e-4)
"""
import functools

import numpy as np
import pytest
import torch

import sinkhorn_ref as ref

pytestmark = pytest.mark.gpu

SPLITS = ("1", "3", "16", None)      # the wide path, two split widths, the dispatch
ANNEALED = dict(eps=0.01, iters=12, eps_start=3.0)


def _cloud(seed, b, n):
    return np.random.default_rng(seed).random((b, n, 3)).astype(np.float32)


def _t(a, dev):
    return torch.from_numpy(np.array(a, copy=True)).to(dev)


def _set_split(monkeypatch, split):
    if split is None:
        monkeypatch.delenv("SN_SINKHORN_SPLIT", raising=False)
    else:
        monkeypatch.setenv("SN_SINKHORN_SPLIT", split)


def _within(what, got, q32, q64):
    """Assert the rule for one quantity; prints the figures first."""
    got, q64 = np.asarray(got, np.float64), np.asarray(q64, np.float64)
    bound, e32, floor = ref.tolerance(q32, q64)
    err = float(np.max(np.abs(got - q64))) if q64.size else 0.0
    print(f"{what}: err {err:.3g}  E32 {e32:.3g}  floor {floor:.3g}  = {err / max(e32, floor):.2f} x max(E32, floor)")
    assert np.isfinite(got).all(), f"{what}: not finite"
    assert err <= bound, f"{what}: error {err:.3g} above 4 * max(E32 {e32:.3g}, floor {floor:.3g})"


@functools.lru_cache(maxsize=None)
def _solved(seed, b, n, m, eps, iters, eps_start, kind="uniform"):
    """The clouds of a case and the reference's potentials and values in float64 and fp32 (computed once)."""
    x, y = _cloud(seed, b, n), _cloud(seed + 1000, b, m)
    if kind == "far":
        y[:, :, 0] += 4
    elif kind == "coincident":
        y = x.copy()
    elif kind == "collapsed":
        y[:] = y[:, :1]
    out = {"x": x, "y": y}
    for name, dtype in (("64", np.float64), ("32", np.float32)):
        f, g = ref.solve_batch(x, y, eps, iters, eps_start, dtype=dtype)
        out["f" + name], out["g" + name] = f, g
        out["v" + name] = np.array([ref.value(f[i], g[i]) for i in range(b)])
    for a in out.values():
        a.setflags(write=False)
    return out


def _check_solve(dev, monkeypatch, case, eps, iters, eps_start, what):
    from sparenet_amd.cuda.sinkhorn import sinkhorn_ot, sinkhorn_potentials

    x, y = _t(case["x"], dev), _t(case["y"], dev)
    for split in SPLITS:
        _set_split(monkeypatch, split)
        f, g = sinkhorn_potentials(x, y, eps, iters=iters, eps_start=eps_start)
        assert f.shape == case["f64"].shape and g.shape == case["g64"].shape and f.dtype == g.dtype == torch.float32
        _within(f"{what} split={split} f", f.cpu().numpy(), case["f32"], case["f64"])
        _within(f"{what} split={split} g", g.cpu().numpy(), case["g32"], case["g64"])
        v = sinkhorn_ot(x, y, eps, iters=iters, eps_start=eps_start)
        assert v.shape == (x.size(0),) and v.dtype == torch.float32
        _within(f"{what} split={split} value", v.cpu().numpy(), case["v32"], case["v64"])


# ------------------------------------------------------------------ edges of lanes, waves, workgroups and tiles
# every size on both sides; no pair puts a multiple of the workgroup's queries against a multiple of a tile
EDGES = [(1, 1), (1, 1025), (63, 64), (64, 255), (65, 63), (255, 1023), (257, 65), (1023, 257), (1025, 1)]


def test_edge_pairs_cover_every_size_on_both_sides():
    sizes = {1, 63, 64, 65, 255, 257, 1023, 1025}
    assert {n for n, _ in EDGES} == sizes == {m for _, m in EDGES}
    for n, m in EDGES:      # one direction of the pair: queries off the workgroup (64 and 256), targets off the tiles
        assert any(q % 64 and t % 192 and t % 1024 for q, t in ((n, m), (m, n)))


@pytest.mark.parametrize("n,m", EDGES)
def test_lane_wave_workgroup_and_tile_edges(dev, monkeypatch, n, m):
    case = _solved(n * 7 + m, 3, n, m, ANNEALED["eps"], ANNEALED["iters"], ANNEALED["eps_start"])
    _check_solve(dev, monkeypatch, case, what=f"{n}/{m}", **ANNEALED)


def test_two_tiles_on_every_path(dev, monkeypatch):
    case = _solved(5, 1, 2049, 2047, 0.0025, 12, 3.0)
    _check_solve(dev, monkeypatch, case, 0.0025, 12, 3.0, "2049/2047 eps=0.0025")


def test_small_eps(dev, monkeypatch):
    iters = ref.default_iters(0.001, 3.0)
    case = _solved(6, 2, 257, 255, 0.001, iters, 3.0)
    _check_solve(dev, monkeypatch, case, 0.001, None, 3.0, "257/255 eps=0.001")      # iters=None: the default count


def test_clouds_far_apart(dev, monkeypatch):
    """min C / eps > 900: every term of exp((g - C) / eps) underflows unless the sum is kept against its own maximum."""
    case = _solved(7, 2, 65, 63, 0.01, 5, None, "far")
    assert ref.cost_matrix(case["x"][0], case["y"][0]).min() / 0.01 > 900
    _check_solve(dev, monkeypatch, case, 0.01, 5, None, "far apart 65/63")


@pytest.mark.parametrize("kind", ["coincident", "collapsed"])
def test_coincident_and_collapsed_clouds(dev, monkeypatch, kind):
    case = _solved(8, 2, 130, 130, ANNEALED["eps"], ANNEALED["iters"], ANNEALED["eps_start"], kind)
    _check_solve(dev, monkeypatch, case, what=kind, **ANNEALED)


# -------------------------------------------------------------------------------------------------------- ragged
def test_ragged_batch(dev, monkeypatch):
    from sparenet_amd.cuda.sinkhorn import sinkhorn_ot, sinkhorn_potentials

    lx, ly = [300, 257, 1, 0], [64, 300, 300, 5]
    x, y = _cloud(9, 4, 300), _cloud(10, 4, 300)
    eps, iters, eps_start = 0.01, 12, 3.0
    want = {}
    for name, dtype in (("64", np.float64), ("32", np.float32)):
        f, g = ref.solve_batch(x, y, eps, iters, eps_start, dtype=dtype, x_lengths=lx, y_lengths=ly)
        grads = [ref.gradients(x[i], y[i], f[i], g[i], eps, dtype, lx[i], ly[i]) for i in range(4)]
        want[name] = (f, g, np.array([ref.value(f[i], g[i], lx[i], ly[i]) for i in range(4)]),
                      np.stack([a for a, _ in grads]), np.stack([b for _, b in grads]))
    for i in range(4):      # rows past the lengths are never read: poison them
        x[i, lx[i]:] = np.nan
        y[i, ly[i]:] = np.nan
    for split in SPLITS:
        _set_split(monkeypatch, split)
        xt, yt = _t(x, dev).requires_grad_(True), _t(y, dev).requires_grad_(True)
        f, g = sinkhorn_potentials(xt, yt, eps, iters=iters, eps_start=eps_start, x_lengths=lx, y_lengths=ly)
        f, g = f.cpu().numpy(), g.cpu().numpy()
        for i in range(4):
            what = f"ragged split={split} cloud {i} ({lx[i]}/{ly[i]})"
            _within(what + " f", f[i, :lx[i]], want["32"][0][i, :lx[i]], want["64"][0][i, :lx[i]])
            _within(what + " g", g[i, :ly[i]], want["32"][1][i, :ly[i]], want["64"][1][i, :ly[i]])
            assert not f[i, lx[i]:].any() and not g[i, ly[i]:].any(), what + ": padding rows must be 0"
        assert not f[3].any() and not g[3].any(), "the zero-length pair gives f = g = 0"
        v = sinkhorn_ot(xt, yt, eps, iters=iters, eps_start=eps_start, x_lengths=torch.tensor(lx, device=dev),
                        y_lengths=torch.tensor(ly, dtype=torch.int32, device=dev))
        _within(f"ragged split={split} value", v.detach().cpu().numpy(), want["32"][2], want["64"][2])
        assert v[3].item() == 0.0
        v.sum().backward()
        gx, gy = xt.grad.cpu().numpy(), yt.grad.cpu().numpy()
        _within(f"ragged split={split} x.grad", gx, want["32"][3], want["64"][3])
        _within(f"ragged split={split} y.grad", gy, want["32"][4], want["64"][4])
        assert not gx[3].any() and not gy[3].any(), "the zero-length pair has a zero gradient"
        for i in range(4):
            assert not gx[i, lx[i]:].any() and not gy[i, ly[i]:].any(), "padding rows have a zero gradient"


# ----------------------------------------------------------------------------------------------- reproducibility
def test_two_calls_give_identical_bits(dev, monkeypatch):
    from sparenet_amd import _lib
    from sparenet_amd.cuda.sinkhorn import sinkhorn_potentials

    x, y = _t(_cloud(11, 3, 1025), dev), _t(_cloud(12, 3, 513), dev)
    for split in SPLITS:
        _set_split(monkeypatch, split)
        runs = []
        for _ in range(2):
            f, g = sinkhorn_potentials(x, y, 0.01, iters=6, eps_start=1.0)
            bary, soft = torch.empty(3, 1025, 3, device=dev), torch.empty(3, 1025, device=dev)
            _lib.op_call("sinkhorn", "sn_sinkhorn_barycenter", x, y, g, 3, 1025, 513, None, None, 0.01, bary, soft, None)
            runs.append([t.cpu().numpy().view(np.int32) for t in (f, g, bary, soft)])
        for a, b, name in zip(runs[0], runs[1], ("f", "g", "bary", "softmin")):
            assert np.array_equal(a, b), f"split={split}: {name} differs between two calls"


# ---------------------------------------------------------------------------------------------------- warm start
def test_warm_start_continues_the_sequence(dev, monkeypatch):
    from sparenet_amd.cuda.sinkhorn import sinkhorn_potentials

    case = _solved(13, 2, 257, 255, ANNEALED["eps"], ANNEALED["iters"], ANNEALED["eps_start"])
    x, y = _t(case["x"], dev), _t(case["y"], dev)
    for split in SPLITS:
        _set_split(monkeypatch, split)
        _, g11 = sinkhorn_potentials(x, y, 0.01, iters=11, eps_start=3.0)      # step 11 of 12 runs at eps itself
        f, g = sinkhorn_potentials(x, y, 0.01, iters=1, g0=g11)
        _within(f"warm start split={split} f", f.cpu().numpy(), case["f32"], case["f64"])
        _within(f"warm start split={split} g", g.cpu().numpy(), case["g32"], case["g64"])
        f12, g12 = sinkhorn_potentials(x, y, **ANNEALED)      # the same launches on the same inputs
        assert torch.equal(f.view(torch.int32), f12.view(torch.int32))
        assert torch.equal(g.view(torch.int32), g12.view(torch.int32))


# ------------------------------------------------------------------------------------- barycentres and gradients
@pytest.mark.parametrize("n,m", [(257, 255), (1025, 63)])
def test_barycenter_entry(dev, monkeypatch, n, m):
    from sparenet_amd import _lib

    case = _solved(14 + n, 2, n, m, ANNEALED["eps"], ANNEALED["iters"], ANNEALED["eps_start"])
    x, y, pot = case["x"], case["y"], case["g64"].astype(np.float32)      # the potential is an input here
    want = {}
    for name, dtype in (("64", np.float64), ("32", np.float32)):
        rows = [ref.barycenter(x[i], y[i], pot[i], 0.01, dtype) for i in range(2)]
        want[name] = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    for split in SPLITS:
        _set_split(monkeypatch, split)
        bary, soft = torch.full((2, n, 3), np.nan, device=dev), torch.full((2, n), np.nan, device=dev)
        _lib.op_call("sinkhorn", "sn_sinkhorn_barycenter", _t(x, dev), _t(y, dev), _t(pot, dev), 2, n, m, None, None,
                     0.01, bary, soft, None)
        _within(f"barycenter {n}/{m} split={split} bary", bary.cpu().numpy(), want["32"][0], want["64"][0])
        _within(f"barycenter {n}/{m} split={split} softmin", soft.cpu().numpy(), want["32"][1], want["64"][1])
        only = torch.full((2, n, 3), np.nan, device=dev)      # softmin may be null
        _lib.op_call("sinkhorn", "sn_sinkhorn_barycenter", _t(x, dev), _t(y, dev), _t(pot, dev), 2, n, m, None, None,
                     0.01, only, None, None)
        assert torch.equal(only.view(torch.int32), bary.view(torch.int32))


def test_gradients_of_the_value(dev, monkeypatch):
    from sparenet_amd.cuda.sinkhorn import sinkhorn_ot

    case = _solved(13, 2, 257, 255, ANNEALED["eps"], ANNEALED["iters"], ANNEALED["eps_start"])
    x, y = case["x"], case["y"]
    want = {}
    for name, dtype in (("64", np.float64), ("32", np.float32)):      # the formula fed with that precision's potentials
        grads = [ref.gradients(x[i], y[i], case["f" + name][i], case["g" + name][i], 0.01, dtype) for i in range(2)]
        want[name] = np.stack([a for a, _ in grads]), np.stack([b for _, b in grads])
    for split in SPLITS:
        _set_split(monkeypatch, split)
        xt, yt = _t(x, dev).requires_grad_(True), _t(y, dev).requires_grad_(True)
        sinkhorn_ot(xt, yt, **ANNEALED).sum().backward()
        _within(f"gradient split={split} x.grad", xt.grad.cpu().numpy(), want["32"][0], want["64"][0])
        _within(f"gradient split={split} y.grad", yt.grad.cpu().numpy(), want["32"][1], want["64"][1])
        # one input only: that side alone is computed, and it is the same side
        x1, y1 = _t(x, dev).requires_grad_(True), _t(y, dev)
        sinkhorn_ot(x1, y1, **ANNEALED).sum().backward()
        assert y1.grad is None and torch.equal(x1.grad.view(torch.int32), xt.grad.view(torch.int32))
        x2, y2 = _t(x, dev), _t(y, dev).requires_grad_(True)
        sinkhorn_ot(x2, y2, **ANNEALED).sum().backward()
        assert x2.grad is None and torch.equal(y2.grad.view(torch.int32), yt.grad.view(torch.int32))
        # an upstream gradient scales each cloud's rows
        x3 = _t(x, dev).requires_grad_(True)
        (sinkhorn_ot(x3, y1, **ANNEALED) * torch.tensor([2.0, -0.5], device=dev)).sum().backward()
        scaled = want["64"][0] * np.array([2.0, -0.5])[:, None, None]
        _within(f"gradient split={split} scaled x.grad", x3.grad.cpu().numpy(),
                want["32"][0] * np.array([2.0, -0.5], np.float32)[:, None, None], scaled)


def test_divergence(dev, monkeypatch):
    from sparenet_amd.cuda.sinkhorn import SinkhornDistance, sinkhorn_divergence

    x, y = _cloud(15, 2, 130), _cloud(16, 2, 97)      # unequal widths: the three problems are padded to 130
    want = {}
    for name, dtype in (("64", np.float64), ("32", np.float32)):
        rows = [ref.divergence(x[i], y[i], dtype=dtype, **ANNEALED) for i in range(2)]
        want[name] = [np.stack([r[k] for r in rows]) for k in range(3)]
    same = [ref.divergence(x[i], x[i], **ANNEALED)[0] for i in range(2)]
    assert same == [0.0, 0.0] and (want["64"][0] > 0).all()
    for split in SPLITS:
        _set_split(monkeypatch, split)
        xt, yt = _t(x, dev).requires_grad_(True), _t(y, dev).requires_grad_(True)
        s = sinkhorn_divergence(xt, yt, **ANNEALED)
        s.sum().backward()
        _within(f"divergence split={split} value", s.detach().cpu().numpy(), want["32"][0], want["64"][0])
        _within(f"divergence split={split} x.grad", xt.grad.cpu().numpy(), want["32"][1], want["64"][1])
        _within(f"divergence split={split} y.grad", yt.grad.cpu().numpy(), want["32"][2], want["64"][2])
        bound = ref.tolerance(want["32"][0], want["64"][0])[0]
        assert (s.detach().cpu().numpy() >= -bound).all(), "S(x, y) >= 0 within the rule"
        module = SinkhornDistance(debias=True, **ANNEALED)
        assert torch.equal(module(_t(x, dev), _t(y, dev)).view(torch.int32), s.detach().view(torch.int32))
        zero = sinkhorn_divergence(_t(x, dev), _t(x, dev), **ANNEALED)
        _within(f"divergence split={split} S(x, x)", zero.cpu().numpy(), np.zeros(2, np.float32), np.zeros(2))


# ------------------------------------------------------------------------------------ limits with a known answer
def test_small_eps_approaches_the_optimal_assignment(dev, monkeypatch):
    from scipy.optimize import linear_sum_assignment

    from sparenet_amd.cuda.sinkhorn import sinkhorn_potentials

    rng = np.random.default_rng(17)
    n, eps = 64, 1e-4
    x = rng.random((2, n, 3)).astype(np.float32)
    y = np.stack([(x[i] + 0.01 * rng.standard_normal((n, 3)).astype(np.float32))[rng.permutation(n)] for i in range(2)])
    for split in SPLITS:
        _set_split(monkeypatch, split)
        f, g = sinkhorn_potentials(_t(x, dev), _t(y, dev), eps, eps_start=1.0)      # annealed, the default step count
        f, g = f.cpu().numpy(), g.cpu().numpy()
        for i in range(2):
            P, C = ref.plan(x[i], y[i], f[i], g[i], eps)
            rows, cols = linear_sum_assignment(C)
            best, primal = C[rows, cols].mean(), (P * C).sum()
            print(f"assignment limit split={split} cloud {i}: <P,C> {primal:.6g}  optimal {best:.6g}  mass {P.sum():.9f}  "
                  f"allowed gap {eps * np.log(n):.3g}")
            assert abs(primal - best) <= eps * np.log(n)


def test_large_eps_gives_the_mean_cost(dev, monkeypatch):
    from sparenet_amd.cuda.sinkhorn import sinkhorn_ot

    case = _solved(18, 2, 65, 63, 1e4, 5, None)
    mean_cost = np.array([ref.cost_matrix(case["x"][i], case["y"][i]).mean() for i in range(2)])
    assert np.abs(case["v64"] - mean_cost).max() < 1e-4      # the reference's own distance from the limit
    _check_solve(dev, monkeypatch, case, 1e4, 5, None, "eps=1e4 65/63")
    for split in SPLITS:
        _set_split(monkeypatch, split)
        v = sinkhorn_ot(_t(case["x"], dev), _t(case["y"], dev), 1e4, iters=5)
        _within(f"eps=1e4 split={split} value against the mean of C", v.cpu().numpy(), case["v32"], mean_cost)
