"""EMD for clouds of any size n <= m (sn_emd_forward_general / sn_emd_backward_general, sparenet_amd.cuda.emd.emd_general)
on the GPU: the general kernels against every emulated-reference golden and against the persistent auction (same
contract for n == m, n % 1024 == 0), and against the NumPy restatement (tests/emd_general_ref.py) bit for bit on
sizes the persistent auction cannot take.  Gradients for both inputs."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from emd_general_ref import emd_general as ref_forward
from emd_general_ref import emd_general_backward as ref_backward

pytestmark = pytest.mark.gpu


def _clouds(b, n, m, seed, kind="uniform"):
    r = np.random.default_rng(seed)
    x = r.random((b, n, 3), dtype=np.float32)
    y = r.random((b, m, 3), dtype=np.float32)
    if kind == "contested":   # duplicate points on both sides: exact ties in the bid values
        x = x[:, r.integers(0, max(1, n // 8), n)]
        y = y[:, r.integers(0, max(1, m // 4), m)]
    return np.ascontiguousarray(x), np.ascontiguousarray(y)


def _run(x, y, eps, iters, dev):
    from sparenet_amd.cuda.emd.emd_general import emd_general_forward_raw

    st = torch.zeros(2, dtype=torch.int64, device=dev)
    d, a = emd_general_forward_raw(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), eps, iters, st)
    return d.cpu().numpy(), a.cpu().numpy(), st.cpu().numpy()


def test_general_kernels_match_every_emulated_golden(golden_dir, dev, monkeypatch):
    monkeypatch.setenv("SN_EMD_GENERAL", "1")
    files = sorted(glob.glob(os.path.join(golden_dir, "emd_*.npz")))
    assert len(files) >= 10
    for f in files:
        z = np.load(f)
        d, a, st = _run(z["xyz1"], z["xyz2"], float(z["eps"]), int(z["iters"]), dev)
        assert np.array_equal(a, z["assignment"]), f
        assert np.array_equal(d, z["dist"]), f
        assert st[0] == int(z["unass"].astype(np.int64).sum()) * z["xyz1"].shape[1], f


def test_general_kernels_equal_persistent_auction_at_16384(dev, monkeypatch):
    from sparenet_amd.cuda.emd.emd_module import emd_forward_raw

    g = torch.Generator().manual_seed(5)
    x = torch.rand(32, 16384, 3, generator=g).to(dev)
    y = torch.rand(32, 16384, 3, generator=g).to(dev)
    s0 = torch.zeros(2, dtype=torch.int64, device=dev)
    d0, a0 = emd_forward_raw(x, y, 0.005, 50, s0)
    monkeypatch.setenv("SN_EMD_GENERAL", "1")
    from sparenet_amd.cuda.emd.emd_general import emd_general_forward_raw

    s1 = torch.zeros(2, dtype=torch.int64, device=dev)
    d1, a1 = emd_general_forward_raw(x, y, 0.005, 50, s1)
    assert torch.equal(a0, a1)
    assert torch.equal(d0, d1)
    assert torch.equal(s0, s1)


def _launches(lib, name, fn):
    """(result of fn(), number of `name` launches it made) through the library's optional per-kernel timing."""
    lib.sn_prof_reset()
    lib.sn_prof_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        lib.sn_prof_enable(0)
    ms = ctypes.c_double(0)
    count = lib.sn_prof_read(name.encode(), ctypes.byref(ms))
    lib.sn_prof_reset()
    return out, count


def test_dispatch_hands_persistent_shapes_to_the_persistent_auction(dev, monkeypatch):
    import sparenet_amd
    from sparenet_amd.cuda.emd.emd_general import emd_general
    from sparenet_amd.cuda.emd.emd_module import emdModule

    lib = sparenet_amd.lib()
    x, y = _clouds(2, 1024, 1024, 11)
    xt, yt = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    d0, a0 = emdModule()(xt, yt, 0.005, 20)
    # which kernels ran: the persistent auction's launch or the general bid launches (one per iteration)
    (d1, a1), n_auction = _launches(lib, "emd_auction", lambda: emd_general(xt, yt, 0.005, 20))
    _, n_bid = _launches(lib, "emd_general_bid", lambda: emd_general(xt, yt, 0.005, 20))
    assert (n_auction, n_bid) == (1, 0)
    assert torch.equal(a0, a1) and torch.equal(d0, d1)
    monkeypatch.setenv("SN_EMD_GENERAL", "1")
    _, n_auction = _launches(lib, "emd_auction", lambda: emd_general(xt, yt, 0.005, 20))
    _, n_bid = _launches(lib, "emd_general_bid", lambda: emd_general(xt, yt, 0.005, 20))
    assert (n_auction, n_bid) == (0, 20)
    # a size the persistent auction refuses never reaches it
    monkeypatch.delenv("SN_EMD_GENERAL")
    _, n_auction = _launches(lib, "emd_auction", lambda: emd_general(xt[:, :1000], yt, 0.005, 20))
    assert n_auction == 0


SIZES = [(1, 1, 1, "uniform"), (3, 7, 7, "uniform"), (2, 1000, 1000, "uniform"), (2, 1000, 3000, "uniform"),
         (4, 2500, 2500, "contested"), (2, 3000, 16384, "uniform"), (9, 1500, 2048, "uniform")]


@pytest.mark.parametrize("b,n,m,kind", SIZES)
@pytest.mark.parametrize("eps", [0.005, 0.002, -0.001])
def test_general_matches_restatement(b, n, m, kind, eps, dev):
    x, y = _clouds(b, n, m, 1000 * b + n + m, kind)
    iters = [0, 1, 3, 50]
    ref = ref_forward(x, y, eps, iters)
    for k in iters:
        d, a, st = _run(x, y, eps, k, dev)
        d0, a0, pairs = ref[k]
        assert np.array_equal(a, a0), (k, np.argwhere(a != a0)[:5])
        assert np.array_equal(d, d0), k
        assert st[0] == pairs, k


@pytest.mark.parametrize("b,n,m,kind,eps,iters", [
    (2, 1000, 3000, "uniform", 0.005, 1),        # forced assignment: targets shared by several bidders
    (2, 700, 700, "contested", 0.005, 1),
    (4, 2500, 2500, "contested", 0.005, 3),
    (2, 3000, 16384, "uniform", 0.002, 50),
    (3, 7, 7, "uniform", -0.001, 50),
])
def test_general_backward_bit_equal_to_restatement(b, n, m, kind, eps, iters, dev):
    from sparenet_amd.cuda.emd.emd_general import emd_general_backward_raw

    x, y = _clouds(b, n, m, 77 + n, kind)
    _, a, _ = _run(x, y, eps, iters, dev)
    gd = np.random.default_rng(n).standard_normal((b, n)).astype(np.float32)
    g1, g2 = emd_general_backward_raw(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev),
                                      torch.from_numpy(gd).to(dev), torch.from_numpy(a).to(dev))
    r1, r2 = ref_backward(x, y, gd, a)
    assert np.array_equal(g1.cpu().numpy(), r1)
    assert np.array_equal(g2.cpu().numpy(), r2)
    if iters == 1 and kind == "contested":
        assert max(np.bincount(a[i]).max() for i in range(b)) > 1   # the case of several bidders per target


@pytest.mark.parametrize("b,n,m,iters", [(2, 1000, 3000, 1), (2, 1000, 3000, 50), (3, 1500, 2048, 3)])
def test_autograd_gradients_for_both_inputs(b, n, m, iters, dev):
    from sparenet_amd.cuda.emd.emd_general import EmdGeneral

    x, y = _clouds(b, n, m, 5 + iters, "uniform")
    x1 = torch.from_numpy(x).to(dev).requires_grad_(True)
    x2 = torch.from_numpy(y).to(dev).requires_grad_(True)
    dist, a = EmdGeneral()(x1, x2, 0.005, iters)
    w = torch.rand(b, n, device=dev)
    (dist * w).sum().backward()
    r1 = x1.detach().clone().requires_grad_(True)
    r2 = x2.detach().clone().requires_grad_(True)
    sel = torch.gather(r2, 1, a.long().unsqueeze(-1).expand(-1, -1, 3))
    (((r1 - sel) ** 2).sum(-1) * w).sum().backward()
    torch.testing.assert_close(x1.grad, r1.grad, rtol=0, atol=1e-6)
    torch.testing.assert_close(x2.grad, r2.grad, rtol=0, atol=1e-6)
    assert x2.grad.abs().sum() > 0


def test_refusals(dev):
    import sparenet_amd
    from sparenet_amd import SparenetHipError
    from sparenet_amd.cuda.emd.emd_general import emd_general
    from sparenet_amd.cuda.emd.emd_module import emdModule

    a = torch.rand(1, 20, 3, device=dev)
    b = torch.rand(1, 10, 3, device=dev)
    with pytest.raises(ValueError, match="smaller cloud first"):
        emd_general(a, b, 0.005, 5)
    lib = sparenet_amd.lib()
    one, null = ctypes.c_void_p(8), ctypes.c_void_p(0)
    assert lib.sn_emd_forward_general(one, one, 1, 20, 10, ctypes.c_float(0.005), 5, one, one, one,
                                      ctypes.c_size_t(1 << 30), null, null) == -22
    assert b"smaller cloud first" in lib.sn_last_error()
    assert lib.sn_emd_forward_general(one, one, 1, 20, (1 << 20) + 1, ctypes.c_float(0.005), 5, one, one, one,
                                      ctypes.c_size_t(1 << 40), null, null) == -22
    assert lib.sn_emd_forward_general(one, one, 0, 20, 30, ctypes.c_float(0.005), 5, one, one, one,
                                      ctypes.c_size_t(1 << 30), null, null) == -22
    need = lib.sn_emd_general_workspace_bytes(2, 1000, 3000)
    assert need > 0 and lib.sn_emd_general_workspace_bytes(2, 3000, 1000) == 0
    assert lib.sn_emd_forward_general(one, one, 2, 1000, 3000, ctypes.c_float(0.005), 5, one, one, one,
                                      ctypes.c_size_t(need - 1), null, null) == -22
    assert b"workspace too small" in lib.sn_last_error()
    with pytest.raises(SparenetHipError):
        emd_general(torch.rand(1, 10, 3), torch.rand(1, 20, 3), 0.005, 5)
    with pytest.raises(AssertionError):   # the reference's module keeps its limits
        emdModule()(torch.rand(1, 1000, 3, device=dev), torch.rand(1, 1000, 3, device=dev), 0.005, 5)


def test_validation_metrics_any_size(dev):
    from sparenet_amd.utils.metrics import fused_validation_metrics

    g = torch.Generator().manual_seed(3)
    pred = torch.rand(2, 1024, 3, generator=g).to(dev)
    gt = torch.rand(2, 1024, 3, generator=g).to(dev)
    m0 = fused_validation_metrics(pred, gt)
    m1 = fused_validation_metrics(pred, gt, emd_any_size=True)
    assert torch.equal(m0["EMD"], m1["EMD"])
    partial = torch.rand(2, 3000, 3, generator=g).to(dev)
    big = torch.rand(2, 16384, 3, generator=g).to(dev)
    for p, q in ((partial, big), (big, partial)):
        out = fused_validation_metrics(p, q, emd_any_size=True)
        assert out["EMD"].shape == (2,) and torch.isfinite(out["EMD"]).all()
    # the value is the smaller cloud's mean matched distance, through the general kernels (the default path refuses it)
    d, _ = _run(partial.cpu().numpy(), big.cpu().numpy(), 0.005, 50, dev)[:2]
    expect = torch.sqrt(torch.from_numpy(d).to(dev)).mean(dim=1) * 100
    assert torch.equal(fused_validation_metrics(big, partial, emd_any_size=True)["EMD"], expect)
    with pytest.raises(AssertionError):
        fused_validation_metrics(partial[:, :1000], partial[:, 1000:2000])


@pytest.mark.parametrize("n,m,kind", [(16000, 16000, "uniform"), (16000, 16000, "near"), (3000, 16384, "uniform")])
def test_full_size(n, m, kind, dev):
    """One 50-iteration call at full size: finite, in range, and a bijection in every cloud that converged.  A cloud
    has converged when the run's last iteration found no bidder left: stats[0] grows by (bidders) * m per cloud and
    iteration, so a run of 51 iterations counts no more pairs than one of 50 exactly when every cloud converged.
    Uniform 16000-point clouds do not converge within 50 iterations at eps 0.005 (thousands of bidders remain after
    800); a prediction near its ground truth ("near") and 3000 -> 16384 do, and there every cloud must be a bijection."""
    from sparenet_amd.cuda.emd.emd_general import emd_general_forward_raw

    g = torch.Generator().manual_seed(n + m)
    y = torch.rand(32, m, 3, generator=g)
    if kind == "near":
        x = (y[:, torch.randperm(m, generator=g)[:n]] + 1e-3 * torch.randn(32, n, 3, generator=g)).clamp(0, 1)
    else:
        x = torch.rand(32, n, 3, generator=g)
    x, y = x.to(dev), y.to(dev)
    s0 = torch.zeros(2, dtype=torch.int64, device=dev)
    s1 = torch.zeros(2, dtype=torch.int64, device=dev)
    d, a = emd_general_forward_raw(x, y, 0.005, 50, s0)
    emd_general_forward_raw(x, y, 0.005, 51, s1)
    assert torch.isfinite(d).all()
    assert ((a >= 0) & (a < m)).all()
    if kind == "uniform" and n == m:
        return
    assert s1[0].item() == s0[0].item(), "some cloud still had bidders after 50 iterations"
    for i in range(32):
        assert torch.unique(a[i]).numel() == n, i


@pytest.mark.parametrize("b,n,m,kind", [(1, 16384, 16384, "identical"), (2, 3000, 3000, "cluster"),
                                        (2, 3000, 3000, "offset")])
def test_backward_with_most_bidders_on_one_target(b, n, m, kind, dev):
    """A collapsed or offset prediction: bidders with the same preferences lose to each other in every iteration and
    the last one forces nearly all of them onto one target.  The gradxyz2 sum over that target stays linear and
    bit-equal to the ascending-j restatement."""
    import time

    from sparenet_amd.cuda.emd.emd_general import emd_general_backward_raw

    r = np.random.default_rng(n + len(kind))
    y = r.random((b, m, 3), dtype=np.float32)
    if kind == "identical":
        x = np.full((b, n, 3), 0.5, np.float32)
    elif kind == "cluster":
        x = (0.5 + 1e-3 * r.standard_normal((b, n, 3))).astype(np.float32)
    else:
        x = (1.3 + 0.05 * r.standard_normal((b, n, 3))).astype(np.float32)
    _, a, _ = _run(x, y, 0.005, 50, dev)
    longest = max(np.bincount(a[i]).max() for i in range(b))
    assert longest > 500, longest
    gd = r.standard_normal((b, n)).astype(np.float32)
    args = [torch.from_numpy(v).to(dev) for v in (x, y, gd, a)]
    emd_general_backward_raw(*args)   # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g1, g2 = emd_general_backward_raw(*args)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    r1, r2 = ref_backward(x, y, gd, a)
    assert np.array_equal(g1.cpu().numpy(), r1)
    assert np.array_equal(g2.cpu().numpy(), r2)
    assert elapsed < 0.5, (elapsed, longest)
