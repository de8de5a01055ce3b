"""Sliced Wasserstein distance on the GPU against the NumPy reference (tests/swd_ref.py).

Order: `sorted_projections` must equal the stable argsort of the fp32 projections bit for bit, in values and in
permutation.  Cost: relative 1e-10 against the float64 reference -- (n + m) <= 32768 double additions at 2^-53 each are
3.6e-12, the factor 30 covers the summation order.  Gradients: the rule of sinkhorn_ref.tolerance(),
    max|q_gpu - q64| <= 4 * max(E32, floor),   E32 = max|q32 - q64|,   floor = 2^-22 * max(1, max|q64|),
with q32 the reference's fp32 restatement.  Ragged batches, chunk widths, repeated calls, shared against per-cloud
directions and the upstream gradient are compared bit for bit.  Every check prints its figures (`pytest -s`).

Measured on an MI355X ("Sliced Wasserstein"): the cost's relative error is at most 1.4e-14 (1/1025, p = 2)
and 2e-16 or exactly 0 in every other case -- 1e-10 is allowed.  The gradients' error as a multiple of max(E32, floor) --
4 is allowed -- with the absolute error in brackets, p = 1 / p = 2:
    1/1               gradx, grady 0.17 / 0.14 (4.0e-8 / 3.3e-8)
    1/1025            gradx 0.14 / 0.07 (3.4e-8 / 1.6e-8), grady 0.00 (2e-11 / 1e-10)
    1025/1            gradx 0.00, grady 0.10 / 0.04 (2.4e-8 / 1.1e-8)
    257/255, 1024/1024, 4096/1000, 16384/16383        0.00 (8e-12 ... 3e-10: the fp32 restatement's own error)
    lattice 512/384   0.00 (6e-11 / 5e-10)
The floor, 2.4e-7, is what the rule allows in every case: the coefficient is summed in double and rounded once, so the
kernel's error is that of the fp32 accumulation over the slices.
"""
import functools

import numpy as np
import pytest
import torch

import swd_ref as ref

pytestmark = pytest.mark.gpu

PAIRS = [(1, 1), (1, 1025), (1025, 1), (257, 255), (1024, 1024), (4096, 1000), (16384, 16383)]
ORDER_SIZES = [1, 2, 63, 64, 65, 1023, 1024, 1025, 16383, 16384]


def _t(a, dev):
    return torch.from_numpy(np.array(a, copy=True)).to(dev)


def _dirs(seed, slices):
    d = np.random.default_rng(seed).standard_normal((slices, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def _cloud(seed, b, n, shift=0.0):
    return (np.random.default_rng(seed).random((b, n, 3)) + shift).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _within(what, got, q32, q64):
    """Assert the rule for one quantity; prints the figures first."""
    got, q64 = np.asarray(got, np.float64), np.asarray(q64, np.float64)
    bound, e32, floor = ref.tolerance(q32, q64)
    err = float(np.max(np.abs(got - q64))) if q64.size else 0.0
    print(f"{what}: err {err:.3g}  E32 {e32:.3g}  floor {floor:.3g}  = {err / max(e32, floor):.2f} x max(E32, floor)")
    assert np.isfinite(got).all(), f"{what}: not finite"
    assert err <= bound, f"{what}: error {err:.3g} above 4 * max(E32 {e32:.3g}, floor {floor:.3g})"


def _reference(x, y, dirs, p):
    """The float64 reference and its fp32 restatement for a batch (shared directions)."""
    out = {}
    for name, dtype in (("64", np.float64), ("32", np.float32)):
        rows = [ref.swd(x[i], y[i], dirs, p, dtype=dtype) for i in range(len(x))]
        out["c" + name] = np.stack([r[0] for r in rows])
        out["gx" + name] = np.stack([r[1] for r in rows])
        out["gy" + name] = np.stack([r[2] for r in rows])
    return out


def _run(x, y, dirs, p=2, upstream=None, **kw):
    """(value [B], x.grad, y.grad) of one differentiable call."""
    from sparenet_amd.cuda.swd import sliced_wasserstein

    x, y = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    v = sliced_wasserstein(x, y, p=p, directions=dirs, **kw)
    (v.sum() if upstream is None else (v * upstream).sum()).backward()
    return v.detach(), x.grad, y.grad


def _slice_costs(x, y, dirs, p):
    """float64 [B, L]: every slice's cost, from the library call itself."""
    from sparenet_amd.cuda import swd

    d, slices, per_cloud = swd._directions("test", dirs, x.size(0), x.device)
    return swd._forward(x.contiguous(), y.contiguous(), d, slices, per_cloud, None, None, p, False)[0]


# ------------------------------------------------------------------------------------------------------- order
def _check_order(dev, x, dirs, lengths=None):
    from sparenet_amd.cuda.swd import sorted_projections

    values, perm = sorted_projections(_t(x, dev), _t(dirs, dev), lengths)
    b, n, slices = x.shape[0], x.shape[1], dirs.shape[-2]
    assert values.shape == perm.shape == (b, slices, n) and values.dtype == torch.float32 and perm.dtype == torch.int32
    values, perm = values.cpu().numpy(), perm.cpu().numpy()
    for i in range(b):
        ln = n if lengths is None else int(lengths[i])
        for l in range(slices):
            proj = ref.project(x[i, :ln], dirs[l] if dirs.ndim == 2 else dirs[i, l])
            want = ref.order(proj)
            assert np.array_equal(perm[i, l, :ln], want), f"cloud {i} slice {l}: permutation"
            assert np.array_equal(values[i, l, :ln].view(np.uint32), proj[want].view(np.uint32)), f"cloud {i} slice {l}"
            assert np.array_equal(values[i, l, :ln], np.sort(proj))
            assert (perm[i, l, ln:] == -1).all() and np.isposinf(values[i, l, ln:]).all()


@pytest.mark.parametrize("n", ORDER_SIZES)
def test_order_at_lane_workgroup_and_width_edges(dev, n):
    _check_order(dev, _cloud(n, 2, n) - 0.5, _dirs(n + 1, 3))


def test_order_on_a_lattice_where_most_keys_are_equal(dev):
    g = np.arange(8, dtype=np.float32)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    x = np.stack([lattice, lattice[np.random.default_rng(0).permutation(512)]])
    dirs = np.array([[1, 0, 0], [0, 0, 1], [1, 1, 0], [1, -1, 1], [1, 1, 1]], np.float32)
    assert len(np.unique(ref.project(x[0], dirs[0]))) == 8 and len(np.unique(ref.project(x[0], dirs[4]))) == 22
    _check_order(dev, x, dirs)


def test_order_with_signed_zeros(dev):
    rng = np.random.default_rng(4)
    x = (rng.integers(-2, 3, (2, 300, 3))).astype(np.float32)
    x[:, ::3] = -0.0
    x[:, 1::7] = 0.0
    x[0, 2::5, 0] = -0.0
    dirs = np.array([[1, 2, 3], [-1, -2, -3], [1, 0, 0], [0, -1, 0]], np.float32)
    proj = ref.project(x[0], dirs[0])
    zeros = proj[proj == 0]
    assert np.signbit(zeros).any() and not np.signbit(zeros).all()      # both zeros are among the keys
    mixed = np.signbit(zeros)
    assert (mixed[:-1] & ~mixed[1:]).any() and (~mixed[:-1] & mixed[1:]).any()      # and interleaved in index order
    _check_order(dev, x, dirs)


def test_order_ragged_with_nan_padding(dev):
    n, lengths = 130, [0, 1, 130, 64, 65, 97]
    x = _cloud(9, len(lengths), n) - 0.5
    for i, ln in enumerate(lengths):
        x[i, ln:] = np.nan
    _check_order(dev, x, _dirs(10, 3), lengths)
    per_cloud = np.stack([_dirs(20 + i, 2) for i in range(len(lengths))])
    _check_order(dev, x, per_cloud, lengths)


# ------------------------------------------------------------------------------------------- cost and gradients
@functools.lru_cache(maxsize=None)
def _case(n, m, p, b=2, slices=3):
    x, y, dirs = _cloud(n * 3 + m, b, n), _cloud(n * 5 + m + 1, b, m, 0.25), _dirs(n + m, slices)
    out = dict(x=x, y=y, dirs=dirs, **_reference(x, y, dirs, p))
    for a in out.values():
        a.setflags(write=False)
    return out


def _check_case(dev, case, p, what):
    x, y, dirs = _t(case["x"], dev), _t(case["y"], dev), _t(case["dirs"], dev)
    cost = _slice_costs(x, y, dirs, p).cpu().numpy()
    rel = np.abs(cost - case["c64"]) / np.maximum(np.abs(case["c64"]), 1e-300)
    print(f"{what} cost: largest relative error {rel.max():.3g}")
    assert cost.dtype == np.float64 and rel.max() <= 1e-10
    v, gx, gy = _run(x, y, dirs, p)
    assert v.dtype == torch.float32 and v.shape == (x.size(0),)
    assert np.allclose(v.cpu().numpy(), cost.mean(axis=1), rtol=2.0 ** -23, atol=0)      # the double mean, rounded once
    _within(f"{what} gradx", gx.cpu().numpy(), case["gx32"], case["gx64"])
    _within(f"{what} grady", gy.cpu().numpy(), case["gy32"], case["gy64"])


@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("n,m", PAIRS)
def test_cost_and_gradients(dev, n, m, p):
    _check_case(dev, _case(n, m, p), p, f"{n}/{m} p={p}")


@pytest.mark.parametrize("p", [1, 2])
def test_cost_and_gradients_on_a_lattice(dev, p):
    """Most projections tie: the permutation, and with it which point gets which coefficient, is the tie rule's."""
    g = np.arange(8, dtype=np.float32)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(1)
    x = np.stack([lattice[rng.permutation(512)], lattice])
    y = np.stack([lattice[rng.permutation(512)[:384]] + np.float32(0.5), lattice[rng.permutation(512)[:384]]])
    dirs = np.array([[1, 0, 0], [0, 0, 1], [1, 1, 0], [1, -1, 1], [1, 1, 1]], np.float32)
    case = dict(x=x, y=y, dirs=dirs, **_reference(x, y, dirs, p))
    _check_case(dev, case, p, f"lattice 512/384 p={p}")


@pytest.mark.parametrize("p", [1, 2])
def test_a_cloud_against_itself_is_exactly_zero(dev, p):
    x = _t(_cloud(2, 3, 1000), dev)
    v, gx, gy = _run(x, x.clone(), _t(_dirs(3, 5), dev), p)
    assert (v == 0).all() and (gx == 0).all() and (gy == 0).all()


# ------------------------------------------------------------------------------------------------------ ragged
@pytest.mark.parametrize("p", [1, 2])
def test_ragged_equals_the_dense_call_on_the_compacted_pair(dev, p):
    n, m = 70, 50
    lx, ly = [0, 1, 70, 37, 20, 9], [50, 50, 50, 1, 0, 9]
    x, y = _cloud(11, len(lx), n), _cloud(12, len(lx), m, 0.25)
    for i in range(len(lx)):
        x[i, lx[i]:] = np.nan
        y[i, ly[i]:] = np.nan
    dirs = _t(_dirs(13, 4), dev)
    v, gx, gy = _run(_t(x, dev), _t(y, dev), dirs, p, x_lengths=lx, y_lengths=ly)
    assert torch.isfinite(v).all() and torch.isfinite(gx).all() and torch.isfinite(gy).all()
    for i in range(len(lx)):
        assert (gx[i, lx[i]:] == 0).all() and (gy[i, ly[i]:] == 0).all(), f"cloud {i}: padding rows"
        if lx[i] == 0 or ly[i] == 0:
            assert v[i] == 0 and (gx[i] == 0).all() and (gy[i] == 0).all(), f"cloud {i}: an empty side"
            continue
        dv, dgx, dgy = _run(_t(x[i:i + 1, :lx[i]], dev), _t(y[i:i + 1, :ly[i]], dev), dirs, p)
        assert _same_bits(v[i:i + 1], dv), f"cloud {i}: value"
        assert _same_bits(gx[i:i + 1, :lx[i]], dgx) and _same_bits(gy[i:i + 1, :ly[i]], dgy), f"cloud {i}: gradients"


# ------------------------------------------------------------------------------ chunks and reproducibility
def test_chunk_widths_and_repeated_calls_give_identical_bits(dev, monkeypatch):
    x, y, dirs = _t(_cloud(21, 2, 300), dev), _t(_cloud(22, 2, 200, 0.1), dev), _t(_dirs(23, 7), dev)
    results = []
    for chunk in ("1", "3", None, None):
        if chunk is None:
            monkeypatch.delenv("SN_SWD_CHUNK", raising=False)
        else:
            monkeypatch.setenv("SN_SWD_CHUNK", chunk)
        results.append(_run(x, y, dirs) + (_slice_costs(x, y, dirs, 2),))
    for got in results[1:]:
        for a, b in zip(results[0], got):
            assert torch.equal(a, b) and _same_bits(a.float(), b.float())
    assert (results[0][0] > 0).all()


def test_permuting_the_points_permutes_the_gradient_rows(dev):
    x, y, dirs = _cloud(31, 2, 500), _cloud(32, 2, 333, 0.1), _dirs(33, 5)
    for l in range(5):      # tie-free: the permutation of the sort is then the only thing that changes
        assert len(np.unique(ref.project(x[0], dirs[l]))) == 500 and len(np.unique(ref.project(x[1], dirs[l]))) == 500
    order = np.random.default_rng(34).permutation(500)
    d = _t(dirs, dev)
    v, gx, gy = _run(_t(x, dev), _t(y, dev), d)
    vp, gxp, gyp = _run(_t(x[:, order], dev), _t(y, dev), d)
    assert _same_bits(v, vp) and _same_bits(gy, gyp)
    assert _same_bits(gx[:, torch.from_numpy(order).to(dev)], gxp)
    assert torch.equal(_slice_costs(_t(x, dev), _t(y, dev), d, 2), _slice_costs(_t(x[:, order], dev), _t(y, dev), d, 2))


# ------------------------------------------------------- shared and per-cloud directions; the max reduction
def test_per_cloud_directions_with_identical_rows_equal_the_shared_call(dev):
    x, y, dirs = _t(_cloud(41, 3, 257), dev), _t(_cloud(42, 3, 129, 0.1), dev), _t(_dirs(43, 4), dev)
    shared = _run(x, y, dirs)
    own = _run(x, y, dirs[None].expand(3, 4, 3).contiguous())
    for a, b in zip(shared, own):
        assert _same_bits(a, b)


@pytest.mark.parametrize("p", [1, 2])
def test_max_reduction_is_the_largest_slice_and_its_gradient(dev, p):
    x, y, dirs = _t(_cloud(51, 3, 200), dev), _t(_cloud(52, 3, 150, 0.1), dev), _t(_dirs(53, 5), dev)
    costs = _slice_costs(x, y, dirs, p)
    best = costs.argmax(dim=1)
    v, gx, gy = _run(x, y, dirs, p, reduction="max")
    assert _same_bits(v, costs.max(dim=1).values.float())
    for i in range(3):
        sv, sgx, sgy = _run(x[i:i + 1], y[i:i + 1], dirs[best[i]:best[i] + 1], p)
        assert _same_bits(v[i:i + 1], sv) and _same_bits(gx[i:i + 1], sgx) and _same_bits(gy[i:i + 1], sgy)


# ---------------------------------------------------------------------------------------------------- autograd
def test_upstream_gradient_scales_the_saved_gradients_exactly(dev):
    from sparenet_amd.cuda.swd import SlicedWassersteinDistance
    from sparenet_amd.utils import metrics

    x, y, dirs = _t(_cloud(61, 3, 100), dev), _t(_cloud(62, 3, 90, 0.1), dev), _t(_dirs(63, 4), dev)
    v, gx, gy = _run(x, y, dirs)
    up = torch.tensor([0.5, -3.0, 1.7], device=dev)
    v2, gx2, gy2 = _run(x, y, dirs, upstream=up)
    assert _same_bits(v, v2)
    assert _same_bits(gx2, up[:, None, None] * gx) and _same_bits(gy2, up[:, None, None] * gy)
    # only one side asks for a gradient; the module and the metric are the same call
    xr = x.clone().requires_grad_(True)
    module = SlicedWassersteinDistance(4, p=2)
    module(xr, y, directions=dirs).sum().backward()
    assert _same_bits(xr.grad, gx)
    assert _same_bits(metrics.swd(x, y, directions=dirs), torch.sqrt(v))
    g = torch.Generator(device=dev).manual_seed(7)
    a = module(x, y, generator=g)
    b = module(x, y, generator=torch.Generator(device=dev).manual_seed(7))
    assert _same_bits(a, b) and (a > 0).all()
