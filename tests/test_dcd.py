"""Density-aware Chamfer distance without a GPU: the header and its binding, every refusal, and the host entry point
(sn_dcd_from_search_host, through the wrapper's CPU path) against the NumPy reference at the derived tolerances of
tests/dcd_cases.py.  tests/test_dcd_gpu.py runs the kernels and compares them with this host path bit for bit."""
import ctypes
import os

import numpy as np
import pytest
import torch

import dcd_cases as cases
import dcd_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ops", "dcd.h")
NAMES = ["sn_dcd_from_search", "sn_dcd_from_search_host", "sn_dcd_workspace_bytes"]
DATA = ["xyz1", "xyz2", "dist1", "idx1", "dist2", "idx2", "b", "n", "m", "lengths1", "lengths2", "alpha", "n_lambda",
        "ratio", "sides", "count1", "count2", "gradxyz1", "gradxyz2"]
CPU = torch.device("cpu")


# ------------------------------------------------------------------------------------------ header and binding
def test_header_and_exports():
    from sparenet_amd import _lib

    protos = _lib.prototypes(HEADER)
    assert sorted(protos) == NAMES
    assert [p.name for p in protos["sn_dcd_from_search"][1]] == DATA + ["workspace", "workspace_bytes", "stream"]
    assert protos["sn_dcd_from_search"][1][-1] == _lib.Param("stream", "void", True, False)
    assert _lib.Param("sides", "double", True, False) in protos["sn_dcd_from_search"][1]
    assert [p.name for p in protos["sn_dcd_from_search_host"][1]] == DATA + ["threads"]
    assert protos["sn_dcd_workspace_bytes"][0] == "size_t"
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name), f"{name} declared in include/ops/dcd.h but not exported"
    assert _lib.op_headers()["dcd"] == HEADER
    assert sorted(_lib._op_calls["dcd"]) == NAMES
    assert _lib.signature("sn_dcd_from_search") == DATA + ["workspace"]
    assert _lib.signature("sn_dcd_from_search_host") == DATA + ["threads"]
    assert _lib.signature("sn_dcd_workspace_bytes") == ["b", "n", "m"]
    assert L.sn_abi_version() == 4
    size = lambda *shape: _lib.op_call("dcd", "sn_dcd_workspace_bytes", *shape)      # noqa: E731
    assert size(0, 1, 1) == size(1, 0, 1) == size(1, 1, 0) == 0
    # per side: ends and list (int), a and term (double); then the long lists' owners
    assert size(32, 16384, 16384) == 2 * 32 * 16384 * (4 + 4 + 8 + 8) + (32 * 32768 // 64 + 2) * 4 + 248
    assert size(1, 1, 1) == 8 * 256 + 256


def test_library_refuses_bad_arguments():
    import sparenet_amd

    L = sparenet_amd.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(8)      # `one` is never dereferenced: validation fails first

    def data(b=2, n=8, m=4, alpha=1000.0, n_lambda=1.0, ratio=0, **pointers):
        p = {k: one for k in ("xyz1", "xyz2", "dist1", "idx1", "dist2", "idx2", "sides")}
        p.update(pointers)
        return (p["xyz1"], p["xyz2"], p["dist1"], p["idx1"], p["dist2"], p["idx2"], b, n, m, null, null, alpha, n_lambda,
                ratio, p["sides"], null, null, null, null)

    def device(ws=one, nbytes=1 << 30, **kw):
        return L.sn_dcd_from_search(*data(**kw), ws, ctypes.c_size_t(nbytes), null)

    def host(**kw):
        return L.sn_dcd_from_search_host(*data(**kw), 1)

    for fn in (device, host):
        def refused(text, **kw):
            assert fn(**kw) == -22
            assert text in L.sn_last_error(), L.sn_last_error()

        for missing in ("xyz1", "xyz2", "dist1", "idx1", "dist2", "idx2", "sides"):
            refused(b"null pointer", **{missing: null})
        for size in ("b", "n", "m"):
            refused(b">= 1", **{size: 0})
            refused(b">= 1", **{size: -3})
        refused(b"too large", b=1 << 15, n=1 << 14, m=1 << 14)
        for alpha in (-1.0, float("inf"), float("-inf"), float("nan")):
            refused(b"alpha must be finite", alpha=alpha)
        for n_lambda in (0.25, 2.0, -1.0, 0.75, float("nan")):
            refused(b"n_lambda must be exactly 0, 0.5 or 1", n_lambda=n_lambda)
        for ratio in (2, -1):
            refused(b"ratio must be 0 or 1", ratio=ratio)
    assert device(nbytes=16) == -22 and b"workspace too small" in L.sn_last_error()
    assert device(ws=null) == -22 and b"null pointer" in L.sn_last_error()


def test_wrapper_refuses_bad_arguments_before_the_library_is_called(monkeypatch):
    from sparenet_amd import _lib
    from sparenet_amd.cuda import dcd
    from sparenet_amd.utils import metrics

    def no_call(*a, **k):
        raise AssertionError("the library was called")

    for name in ("op_call", "op_workspace", "call"):
        monkeypatch.setattr(_lib, name, no_call)
    x, y = torch.zeros(2, 8, 3), torch.zeros(2, 4, 3)
    for fn in (dcd.density_aware_chamfer, metrics.dcd):
        for alpha in (-1.0, float("inf"), float("nan"), "1000", True, None):
            with pytest.raises(ValueError, match="alpha must be a finite number"):
                fn(x, y, alpha=alpha)
        for n_lambda in (0.25, 2, -1, "1", True, None):
            with pytest.raises(ValueError, match="n_lambda must be 0, 0.5 or 1"):
                fn(x, y, n_lambda=n_lambda)
        for ratio in ("mean", 1, None):
            with pytest.raises(ValueError, match="ratio must be one of none, size"):
                fn(x, y, ratio=ratio)
        for bad in (torch.zeros(2, 8, 2), torch.zeros(8, 3), torch.zeros(2, 0, 3), torch.zeros(0, 8, 3)):
            with pytest.raises(ValueError, match=r"\[B, N, 3\]"):
                fn(bad, y)
            with pytest.raises(ValueError, match=r"\[B, N, 3\]"):
                fn(x, bad)
        with pytest.raises(TypeError, match="floating-point"):
            fn(x.int(), y)
        with pytest.raises(ValueError, match="batch sizes differ"):
            fn(x, torch.zeros(3, 4, 3))
    with pytest.raises(ValueError, match="n_lambda"):
        dcd.DensityAwareChamferDistance(n_lambda=0.3)
    with pytest.raises(ValueError, match="ratio"):
        dcd.DensityAwareChamferDistance(ratio="sizes")
    found = (torch.zeros(2, 8), torch.zeros(2, 8, dtype=torch.int), torch.zeros(2, 4), torch.zeros(2, 4, dtype=torch.int))
    with pytest.raises(ValueError, match=r"dist2 must be a \[2, 4\] tensor"):
        dcd.dcd_from_search(x, y, found[0], found[1], found[0], found[3])
    with pytest.raises(ValueError, match="alpha"):
        dcd.dcd_from_search(x, y, *found, alpha=-2.0)


def test_wrapper_refuses_bad_lengths():
    from sparenet_amd.cuda.dcd import density_aware_chamfer

    x, y = torch.rand(2, 8, 3), torch.rand(2, 4, 3)
    with pytest.raises(ValueError, match="lengths1"):
        density_aware_chamfer(x, y, lengths1=[9, 1], lengths2=[4, 4])
    with pytest.raises(ValueError, match="lengths2"):
        density_aware_chamfer(x, y, lengths1=[8, 1], lengths2=[4])


def test_exported_from_the_package():
    import sparenet_amd
    from sparenet_amd.cuda import dcd

    for name in ("density_aware_chamfer", "dcd_from_search", "DensityAwareChamferDistance"):
        assert getattr(sparenet_amd, name) is getattr(dcd, name)


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("n_lambda,ratio", cases.RULES)
def test_reference_gradient_equals_central_differences(n_lambda, ratio):
    """float64 throughout, the assignment held fixed: the gradient formula of the header is the derivative of its loss."""
    rng = np.random.default_rng(11)
    n, m, alpha = 12, 9, 40.0
    x, y = 0.5 * rng.random((n, 3)), 0.5 * rng.random((m, 3))
    _, idx1, _, idx2 = ref.search(x, y)
    want = ref.dcd(x, y, alpha, n_lambda, ratio, found=(None, idx1, None, idx2), exact=True)
    assert want["count1"].max() > 1 or want["count2"].max() > 1
    assert abs(want["loss"] - ref.loss_f64(x, y, idx1, idx2, alpha, n_lambda, ratio)) <= 1e-15
    h = 1e-6
    for pts, grad, side in ((x, want["grad1"], 0), (y, want["grad2"], 1)):
        for i in range(len(pts)):
            for c in range(3):
                hi, lo = pts.copy(), pts.copy()
                hi[i, c] += h
                lo[i, c] -= h
                value = lambda p: ref.loss_f64(*((p, y) if side == 0 else (x, p)), idx1, idx2, alpha, n_lambda, ratio)  # noqa: E731
                fd = (value(hi) - value(lo)) / (2 * h)
                assert abs(fd - grad[i, c]) <= 1e-8 * max(1.0, abs(fd)), (side, i, c, fd, grad[i, c])


# ------------------------------------------------------------------------------------------- host against reference
@pytest.mark.parametrize("n_lambda,ratio", cases.RULES)
@pytest.mark.parametrize("n,m", cases.SHAPES)
def test_host_against_reference(n, m, n_lambda, ratio):
    cases.check_shape_against_ref(n, m, n_lambda, ratio, CPU)


@pytest.mark.parametrize("n,m", [(1500, 1), (20000, 1)])
def test_host_one_target_for_everyone(n, m):
    rng = np.random.default_rng(n)
    x, y = (0.1 * rng.random((1, n, 3))).astype(np.float32), (0.1 * rng.random((1, m, 3))).astype(np.float32)
    for n_lambda, ratio in ((1.0, "none"), (0.5, "size")):
        _, raw, g1, g2 = cases.run(x, y, 1000.0, n_lambda, ratio, CPU)
        assert raw["count2"][0, 0] == n and (raw["idx1"] == 0).all()
        want = ref.dcd(x[0], y[0], 1000.0, n_lambda, ratio)
        cases.check_cloud((raw["sides"][0], raw["count1"][0], raw["count2"][0], g1[0], g2[0]), want, f"{n}x{m} {n_lambda} {ratio}")


def test_host_copies_of_one_point_choose_index_zero():
    rng = np.random.default_rng(5)
    x = (0.1 * rng.random((1, 700, 3))).astype(np.float32)
    y = np.repeat((0.1 * rng.random((1, 1, 3))).astype(np.float32), 1500, axis=1)
    _, raw, g1, g2 = cases.run(x, y, 1000.0, 1.0, "none", CPU)
    assert (raw["idx1"] == 0).all() and raw["count2"][0, 0] == 700 and (raw["count2"][0, 1:] == 0).all()
    assert raw["count1"].sum() == 1500
    want = ref.dcd(x[0], y[0], 1000.0, 1.0, "none")
    cases.check_cloud((raw["sides"][0], raw["count1"][0], raw["count2"][0], g1[0], g2[0]), want, "700 x 1500 copies")


# ------------------------------------------------------------------------------------------------- exact values
@pytest.mark.parametrize("n_lambda,ratio", cases.RULES)
def test_host_permutation_gives_exactly_zero(n_lambda, ratio):
    rng = np.random.default_rng(2)
    x = rng.random((2, 257, 3)).astype(np.float32)
    y = np.stack([x[i][rng.permutation(257)] for i in range(2)])
    value, raw, g1, g2 = cases.run(x, y, 1000.0, n_lambda, ratio, CPU)
    assert (value == 0.0).all() and (raw["sides"] == 0.0).all()
    assert (raw["count1"] == 1).all() and (raw["count2"] == 1).all()
    assert (g1 == 0.0).all() and (g2 == 0.0).all()


@pytest.mark.parametrize("n_lambda,ratio", cases.RULES)
def test_host_distant_clouds_give_exactly_one(n_lambda, ratio):
    """alpha = 1000 and every distance above sqrt(0.104): the argument is below -104, where sn_expf returns 0."""
    rng = np.random.default_rng(3)
    x = (0.1 * rng.random((2, 65, 3))).astype(np.float32)
    y = (0.1 * rng.random((2, 40, 3)) + np.array([0.45, 0.0, 0.0])).astype(np.float32)
    value, raw, g1, g2 = cases.run(x, y, 1000.0, n_lambda, ratio, CPU)
    assert raw["dist1"].min() > 0.104 and raw["dist2"].min() > 0.104
    assert (value == 1.0).all() and (raw["sides"] == 1.0).all()
    assert (g1 == 0.0).all() and (g2 == 0.0).all()


# ------------------------------------------------------------------------------------------------------- ragged
def test_host_ragged_equals_dense_on_every_slice():
    cases.check_ragged(CPU)


def test_host_index_outside_the_other_cloud_is_in_no_list():
    """dcd_from_search on a caller's search: a valid row whose index names no target has term 1 and no gradient."""
    from sparenet_amd.cuda.dcd import dcd_from_search

    rng = np.random.default_rng(9)
    x, y = (0.1 * rng.random((1, 6, 3))).astype(np.float32), (0.1 * rng.random((1, 4, 3))).astype(np.float32)
    dist1, idx1, dist2, idx2 = (t.copy() for t in ref.search(x[0], y[0]))
    idx1[2], idx2[1] = 4, -1
    args = [torch.tensor(t[None]) for t in (dist1, idx1, dist2, idx2)]
    sides, count1, count2, g1, g2 = dcd_from_search(torch.tensor(x), torch.tensor(y), *args, alpha=1000.0)
    want = ref.dcd(x[0], y[0], 1000.0, found=(dist1, idx1, dist2, idx2))
    cases.check_cloud((sides[0].numpy(), count1[0].numpy(), count2[0].numpy(), g1[0].numpy(), g2[0].numpy()), want,
                      "unmatched rows")
    assert count2.sum() == 5 and count1.sum() == 3


# ----------------------------------------------------------------------------------------------------- autograd
def test_host_autograd_scales_the_stored_gradient():
    from sparenet_amd.cuda.dcd import DensityAwareChamferDistance, dcd_from_search, density_aware_chamfer

    x, y, alpha, _ = cases.case(200, 130)
    module = DensityAwareChamferDistance(alpha, 0.5, "size")
    weights = torch.tensor([0.25, -3.0, 1.7])      # the upstream gradient differs per cloud
    grads = []
    for _ in range(2):
        xt, yt = torch.tensor(x).requires_grad_(True), torch.tensor(y).requires_grad_(True)
        value = module(xt, yt)
        assert value.dtype == torch.float32 and value.shape == (3,)
        (value * weights).sum().backward()
        grads.append((value.detach(), xt.grad, yt.grad))
    assert all(torch.equal(a, b) for a, b in zip(*grads)), "two calls differ"
    _, raw = density_aware_chamfer(torch.tensor(x), torch.tensor(y), alpha, 0.5, "size", return_raw=True)
    _, _, _, g1, g2 = dcd_from_search(torch.tensor(x), torch.tensor(y), raw["dist1"], raw["idx1"], raw["dist2"],
                                      raw["idx2"], alpha, 0.5, "size")
    assert torch.equal(grads[0][1], weights[:, None, None] * g1) and torch.equal(grads[0][2], weights[:, None, None] * g2)
    # only one input needs a gradient: the other gets none
    xt = torch.tensor(x).requires_grad_(True)
    module(xt, torch.tensor(y)).sum().backward()
    assert torch.equal(xt.grad, g1)
    # no gradient wanted: nothing is stored, the value is the same
    assert torch.equal(module(torch.tensor(x), torch.tensor(y)), grads[0][0])


# ------------------------------------------------------------------------------------------------------ metrics
def test_fused_validation_metrics_flag_on_cpu():
    from sparenet_amd.cuda.dcd import density_aware_chamfer
    from sparenet_amd.utils.metrics import dcd, fused_validation_metrics

    x, y, _, _ = cases.case(200, 130)
    pred, gt = torch.tensor(x), torch.tensor(y)
    plain = fused_validation_metrics(pred, gt, with_emd=False)
    assert sorted(plain) == ["ChamferDistance", "F-Score"]
    flagged = fused_validation_metrics(pred, gt, with_emd=False, with_dcd=True, dcd_alpha=200.0, dcd_n_lambda=0.5)
    assert sorted(flagged) == ["ChamferDistance", "DCD", "F-Score"]
    for key in plain:
        assert torch.equal(plain[key], flagged[key]), key
    assert torch.equal(flagged["DCD"], density_aware_chamfer(pred, gt, 200.0, 0.5))
    assert torch.equal(flagged["DCD"], dcd(pred, gt, 200.0, 0.5))
    # ragged
    xr, yr, lengths1, lengths2 = cases.ragged_batch()
    pred, gt = torch.tensor(xr), torch.tensor(yr)
    plain = fused_validation_metrics(pred, gt, with_emd=False, pred_lengths=lengths1, gt_lengths=lengths2)
    flagged = fused_validation_metrics(pred, gt, with_emd=False, pred_lengths=lengths1, gt_lengths=lengths2, with_dcd=True)
    assert sorted(plain) == ["ChamferDistance", "F-Score"] and sorted(flagged) == ["ChamferDistance", "DCD", "F-Score"]
    for key in plain:
        assert torch.equal(plain[key], flagged[key]), key
    assert torch.equal(flagged["DCD"], density_aware_chamfer(pred, gt, lengths1=lengths1, lengths2=lengths2))
