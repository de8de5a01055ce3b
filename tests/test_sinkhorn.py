"""Sinkhorn transport without a GPU: self-checks of the NumPy reference (tests/sinkhorn_ref.py: marginals, the
formula gradient against central differences, the value against <P,C> + eps KL), the operator header
(include/ops/sinkhorn.h) and its call path in sparenet_amd._lib, every SN_EINVAL case through direct ctypes with nothing
dereferenced, the Python wrappers' refusals before any device call, and the schedule arithmetic of the wrapper against
the reference's."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import sinkhorn_ref as ref
from lib_stub import _scalars, install

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ops", "sinkhorn.h")
NAMES = sorted(["sn_sinkhorn_workspace_bytes", "sn_sinkhorn_solve", "sn_sinkhorn_barycenter"])


def _cloud(seed, n):
    return np.random.default_rng(seed).random((n, 3)).astype(np.float32)


# ------------------------------------------------------------------------------------------ the reference itself
def test_reference_column_marginals():
    x, y = _cloud(1, 257), _cloud(2, 255)
    f, g = ref.solve(x, y, 0.01, 12, 3.0)
    P, _ = ref.plan(x, y, f, g, 0.01)
    # g is updated last: the column marginals are exact whatever the number of steps, so the plan's mass is 1
    assert np.max(np.abs(P.sum(axis=0) - 1.0 / 255)) * 255 < 1e-6
    assert abs(P.sum() - 1.0) < 1e-9


def test_reference_value_is_primal_cost_plus_entropy():
    x, y = _cloud(3, 24), _cloud(4, 31)
    eps = 0.05
    f, g = ref.solve(x, y, eps, 2000)
    P, C = ref.plan(x, y, f, g, eps)
    ab = 1.0 / (24 * 31)
    primal = (P * C).sum() + float(np.float32(eps)) * (P * np.log(P / ab)).sum()
    assert abs(ref.value(f, g) - primal) <= 1e-9 * max(1.0, abs(primal))


def test_reference_gradient_equals_central_differences():
    x, y = _cloud(5, 24).astype(np.float64), _cloud(6, 31).astype(np.float64)
    eps, steps, h = 0.05, 2000, 1e-5

    def ot(a, b):      # the value with the cost in float64: central differences need a smooth cost
        C = ((a[:, None, :] - b[None, :, :]) ** 2).sum(axis=2)
        g = np.zeros(len(b))
        for _ in range(steps):
            f = ref.softmin(C, g, eps, np.float64)
            g = ref.softmin(C.T, f, eps, np.float64)
        return f.mean() + g.mean(), f, g

    _, f, g = ot(x, y)
    gx, gy = ref.gradients(x.astype(np.float32), y.astype(np.float32), f, g, eps)
    worst = 0.0
    for cloud, grad, which in ((x, gx, 0), (y, gy, 1)):
        for i in (0, len(cloud) - 1):
            numeric = np.zeros(3)
            for c in range(3):
                up, down = cloud.copy(), cloud.copy()
                up[i, c] += h
                down[i, c] -= h
                pair = ((up, y), (down, y)) if which == 0 else ((x, up), (x, down))
                numeric[c] = (ot(*pair[0])[0] - ot(*pair[1])[0]) / (2 * h)
            worst = max(worst, np.linalg.norm(numeric - grad[i]) / np.linalg.norm(grad[i]))
    print(f"formula gradient against central differences: worst relative error of a point's gradient {worst:.3g}")
    assert worst < 1e-4, worst


def test_reference_conventions():
    x, y = _cloud(7, 9), _cloud(8, 6)
    f, g = ref.solve(x, y, 0.1, 3, x_length=4, y_length=6)
    assert not f[4:].any() and f[:4].all() and g.all()
    for lx, ly in ((0, 6), (4, 0), (-3, 2)):
        f, g = ref.solve(x, y, 0.1, 3, x_length=lx, y_length=ly)
        assert not f.any() and not g.any() and ref.value(f, g, lx, ly) == 0
        gx, gy = ref.gradients(x, y, f, g, 0.1, x_length=lx, y_length=ly)
        assert not gx.any() and not gy.any()
    # the restatement is the reference's code in fp32: close, not equal
    f64, g64 = ref.solve(x, y, 0.1, 5)
    f32, g32 = ref.solve(x, y, 0.1, 5, dtype=np.float32)
    assert f32.dtype == np.float32 and 0 < np.abs(f32 - f64).max() < 1e-5
    bound, e32, floor = ref.tolerance(f32, f64)
    assert bound == 4 * max(e32, floor) and floor == 2.0 ** -22 * max(1.0, np.abs(f64).max())
    # a warm start continues the sequence
    fa, ga = ref.solve(x, y, 0.1, 4)
    fb, gb = ref.solve(x, y, 0.1, 1, g0=ref.solve(x, y, 0.1, 3)[1])
    assert np.array_equal(fa, fb) and np.array_equal(ga, gb)


# ------------------------------------------------------------------------------------------ header and binding
def _declared(path):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"^(?:int|size_t|void|long long|const char \*)\s*(sn_[a-z0-9_]+)\s*\(", txt, re.M)))


def test_header_functions_are_exported_and_registered():
    from sparenet_amd import _lib

    assert _declared(HEADER) == NAMES
    L = _lib.lib()
    for n in NAMES:
        assert hasattr(L, n), f"{n} declared in include/ops/sinkhorn.h but not exported"
    assert _lib.op_headers()["sinkhorn"] == HEADER
    assert sorted(_lib._op_calls["sinkhorn"]) == NAMES == sorted(_lib.prototypes(HEADER))
    assert _lib.signature("sn_sinkhorn_workspace_bytes") == ["b", "n", "m"]
    assert _lib.signature("sn_sinkhorn_solve") == ["x", "y", "b", "n", "m", "x_lengths", "y_lengths", "eps",
                                                   "eps_start", "decay", "iters", "warm_start", "f", "g", "workspace"]
    assert _lib.signature("sn_sinkhorn_barycenter") == ["q", "t", "t_potential", "b", "n", "m", "q_lengths",
                                                        "t_lengths", "eps", "bary", "softmin", "workspace"]
    assert L.sn_abi_version() == 4
    for shape in ((1, 1, 1), (3, 2049, 2047), (32, 16384, 16384), (0, 0, 0)):
        assert _lib.op_call("sinkhorn", "sn_sinkhorn_workspace_bytes", *shape) == 0


def test_exported_from_the_package():
    import sparenet_amd
    from sparenet_amd.cuda import sinkhorn

    for name in ("sinkhorn_potentials", "sinkhorn_ot", "sinkhorn_divergence", "SinkhornDistance"):
        assert getattr(sparenet_amd, name) is getattr(sinkhorn, name)
    with pytest.raises(AttributeError):
        sparenet_amd.sinkhorn_nothing


def test_argument_validation_without_gpu():
    import sparenet_amd

    L = sparenet_amd.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(8)      # `one` is never dereferenced: validation fails first
    c = ctypes.c_float

    def refused(fn, text, *args):
        assert fn(*args) == -22
        assert text in L.sn_last_error(), L.sn_last_error()

    # sn_sinkhorn_solve(x, y, b, n, m, x_lengths, y_lengths, eps, eps_start, decay, iters, warm_start, f, g, ws, bytes,
    #                   stream)
    def solve(x=one, y=one, b=2, n=8, m=4, eps=0.01, eps_start=0.0, decay=0.5, iters=3, f=one, g=one):
        return (x, y, b, n, m, null, null, c(eps), c(eps_start), c(decay), iters, 0, f, g, null, 0, null)

    for missing in ("x", "y", "f", "g"):
        refused(L.sn_sinkhorn_solve, b"null pointer", *solve(**{missing: null}))
    for size in ("b", "n", "m"):
        for v in (0, -3):
            refused(L.sn_sinkhorn_solve, b">= 1", *solve(**{size: v}))
    for eps in (0.0, -0.01, float("inf"), float("nan")):
        refused(L.sn_sinkhorn_solve, b"eps must be finite and > 0", *solve(eps=eps))
    for eps_start in (float("inf"), float("nan")):
        refused(L.sn_sinkhorn_solve, b"eps_start must be finite", *solve(eps_start=eps_start))
    for decay in (0.0, 1.0, -0.5, 1.5, float("nan")):
        refused(L.sn_sinkhorn_solve, b"0 < decay < 1", *solve(decay=decay))
    for iters in (0, -1):
        refused(L.sn_sinkhorn_solve, b"iters >= 1", *solve(iters=iters))

    # sn_sinkhorn_barycenter(q, t, t_potential, b, n, m, q_lengths, t_lengths, eps, bary, softmin, ws, bytes, stream)
    def bary(q=one, t=one, pot=one, b=2, n=8, m=4, eps=0.01, out=one):
        return (q, t, pot, b, n, m, null, null, c(eps), out, null, null, 0, null)

    for missing in ("q", "t", "pot", "out"):
        refused(L.sn_sinkhorn_barycenter, b"null pointer", *bary(**{missing: null}))
    for size in ("b", "n", "m"):
        for v in (0, -3):
            refused(L.sn_sinkhorn_barycenter, b">= 1", *bary(**{size: v}))
    for eps in (0.0, -1.0, float("inf"), float("nan")):
        refused(L.sn_sinkhorn_barycenter, b"eps must be finite and > 0", *bary(eps=eps))


# ------------------------------------------------------------------------------------------------ the wrappers
def test_wrapper_refusals_before_any_device_call(monkeypatch):
    from sparenet_amd import SparenetHipError, _lib
    from sparenet_amd.cuda import sinkhorn as sk

    def no_device_call(*args, **kwargs):
        raise AssertionError("the library was called before the arguments were validated")

    monkeypatch.setattr(_lib, "op_call", no_device_call)
    monkeypatch.setattr(_lib, "op_workspace", no_device_call)
    x, y = torch.rand(2, 16, 3), torch.rand(2, 5, 3)
    module = sk.SinkhornDistance(0.01, eps_start=1.0)
    for call in (sk.sinkhorn_potentials, sk.sinkhorn_ot, sk.sinkhorn_divergence):
        for eps in (0.0, -1.0, float("inf"), float("nan"), 1e-60):
            with pytest.raises(ValueError, match="eps must be finite and > 0"):
                call(x, y, eps)
        for decay in (0.0, 1.0, -0.5, 2.0, float("nan")):
            with pytest.raises(ValueError, match=r"decay must be in \(0, 1\)"):
                call(x, y, 0.01, decay=decay)
        for iters in (0, -1, 2.5, True):
            with pytest.raises(ValueError, match="iters must be an integer >= 1"):
                call(x, y, 0.01, iters=iters)
        for eps_start in (float("inf"), float("nan")):
            with pytest.raises(ValueError, match="eps_start must be finite"):
                call(x, y, 0.01, eps_start=eps_start)
        with pytest.raises(ValueError, match="batch sizes differ"):
            call(x, torch.rand(3, 5, 3), 0.01)
        for bad in (torch.rand(16, 3), torch.rand(2, 16, 2), torch.rand(0, 16, 3), torch.rand(2, 0, 3)):
            with pytest.raises(ValueError, match=r"\[B, N, 3\]"):
                call(bad, y, 0.01)
            with pytest.raises(ValueError, match=r"\[B, N, 3\]"):
                call(x, bad, 0.01)
        with pytest.raises(TypeError, match="floating-point"):
            call(torch.zeros(2, 16, 3, dtype=torch.int32), y, 0.01)
        with pytest.raises(SparenetHipError, match="no CPU path"):
            call(x, y, 0.01)
    with pytest.raises(SparenetHipError, match="no CPU path"):
        module(x, y)
    with pytest.raises(SparenetHipError, match="no CPU path"):
        sk.SinkhornDistance(0.01, debias=False)(x, y)
    for bad in (dict(eps=0.0), dict(eps=0.01, decay=1.0), dict(eps=0.01, iters=0)):
        with pytest.raises(ValueError):
            sk.SinkhornDistance(**bad)


@pytest.fixture()
def stub(monkeypatch):
    """The converting, recording stub of tests/lib_stub.py in place of the library (its workspace size is 0)."""
    return install(monkeypatch, ("_op_calls",), size_t=0)


def test_wrappers_pass_what_they_were_given(stub):
    from sparenet_amd.cuda import sinkhorn as sk

    x = torch.rand(3, 40, 3, dtype=torch.float64)[:, ::2]      # neither fp32 nor contiguous: the wrapper converts
    y = torch.rand(3, 7, 3)
    f, g = sk.sinkhorn_potentials(x, y, 0.25, iters=4, eps_start=2.0, decay=0.5)
    assert f.shape == (3, 20) and g.shape == (3, 7) and f.dtype == g.dtype == torch.float32
    assert stub[0] == ("sn_sinkhorn_workspace_bytes", (3, 20, 7))
    name, a = stub[1]
    #                                   x     y    b   n  m  xl     yl     eps  start decay it warm f     g    ws   bytes
    assert name == "sn_sinkhorn_solve" and _scalars(a) == (True, True, 3, 20, 7, False, False, 0.25, 2.0, 0.5, 4, 0,
                                                           True, True, True, 0)
    del stub[:]
    sk.sinkhorn_potentials(x, y, 0.25, x_lengths=[0, 5, 20], y_lengths=torch.tensor([7, 0, 1]), g0=torch.rand(3, 7))
    assert _scalars(stub[1][1]) == (True, True, 3, 20, 7, True, True, 0.25, 0.0, 0.5, 20, 1, True, True, True, 0)
    with pytest.raises(ValueError, match="g0"):
        sk.sinkhorn_potentials(x, y, 0.25, g0=torch.rand(3, 8))
    with pytest.raises(ValueError, match="expected 3 lengths"):
        sk.sinkhorn_potentials(x, y, 0.25, x_lengths=[1, 2])
    with pytest.raises(ValueError, match=r"y_lengths: lengths must be in \[0, 7\]"):
        sk.sinkhorn_ot(x, y, 0.25, y_lengths=[1, 8, 3])

    # the backward calls the barycentre entry only for the inputs that need a gradient
    for need_x, need_y in ((True, True), (True, False), (False, True)):
        del stub[:]
        xs = torch.rand(3, 20, 3, requires_grad=need_x)
        ys = torch.rand(3, 7, 3, requires_grad=need_y)
        sk.sinkhorn_ot(xs, ys, 0.5, iters=2).sum().backward()
        names = [c[0] for c in stub if c[0] != "sn_sinkhorn_workspace_bytes"]
        assert names == ["sn_sinkhorn_solve"] + ["sn_sinkhorn_barycenter"] * (need_x + need_y)
        assert (xs.grad is not None) == need_x and (ys.grad is not None) == need_y
        sizes = [_scalars(c[1])[3:6] for c in stub if c[0] == "sn_sinkhorn_barycenter"]
        assert sizes == [(3, 20, 7)] * need_x + [(3, 7, 20)] * need_y

    # the divergence: ONE solve of 3b problems padded to the wider cloud, ragged
    del stub[:]
    xs, ys = torch.rand(2, 20, 3, requires_grad=True), torch.rand(2, 7, 3, requires_grad=True)
    s = sk.sinkhorn_divergence(xs, ys, 0.5, iters=2)
    assert s.shape == (2,)
    solves = [c for c in stub if c[0] == "sn_sinkhorn_solve"]
    assert len(solves) == 1 and _scalars(solves[0][1])[2:7] == (6, 20, 20, True, True)
    s.sum().backward()
    assert xs.grad.shape == xs.shape and ys.grad.shape == ys.shape


def test_schedule_arithmetic_equals_the_reference():
    from sparenet_amd.cuda import sinkhorn as sk

    cases = [(0.01, None, 3.0, 0.5), (0.01, 12, 3.0, 0.5), (0.0025, None, 3.0, 0.7), (1e-4, None, 1.0, 0.9),
             (0.05, None, None, 0.5), (0.05, 7, None, 0.5), (0.05, 3, 0.0, 0.5), (0.05, 3, -1.0, 0.5),
             (0.3, None, 0.1, 0.5), (0.1, 4, 0.1, 0.3), (1e4, None, 3.0, 0.5), (0.001, 9, 123.456, 0.61)]
    for eps, iters, eps_start, decay in cases:
        got = sk.schedule(eps, iters, eps_start, decay)
        want = ref.schedule(eps, iters, eps_start, decay)
        assert [np.float32(v).view(np.int32) for v in got] == [v.view(np.int32) for v in want], (eps, iters, eps_start)
        assert all(np.float32(v) == v for v in got) and got[-1] >= np.float32(eps)
        assert len(got) == (ref.default_iters(eps, eps_start, decay) if iters is None else iters)
    assert len(sk.schedule(0.01, None, 3.0, 0.5)) == 9 + 5      # 3 * 0.5^9 is the first value <= 0.01
    assert len(sk.schedule(0.05)) == 20
    assert sk.schedule(0.01, 3, 3.0, 0.5) == [3.0, 1.5, 0.75]
