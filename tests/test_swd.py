"""Sliced Wasserstein distance without a GPU: the NumPy reference against the textbook construction and against finite
differences, the header and its binding, and the wrapper's argument checks (tests/test_swd_gpu.py runs the kernels)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import swd_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ops", "swd.h")
NAMES = ["sn_swd_forward", "sn_swd_project_sort", "sn_swd_workspace_bytes"]


# ------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("n,m", [(1, 1), (1, 5), (5, 1), (7, 7), (6, 4), (64, 65), (257, 255)])
def test_transport_equals_replicate_and_sort(n, m, p):
    rng = np.random.default_rng(n * 1000 + m)
    sx, sy = np.sort(rng.standard_normal(n)), np.sort(rng.standard_normal(m) + 0.25)
    i, j, w = ref.plan(n, m)
    assert len(w) == ref.term_count(n, m) == n + m - math.gcd(n, m)
    assert (w > 0).all() and w.sum() == n * m
    assert (np.bincount(i, w) == m).all() and (np.bincount(j, w) == n).all()      # the plan's marginals are uniform
    # a rank's partners are the range the kernel walks: floor(i m / n) .. ceil((i + 1) m / n) - 1
    for r in range(n):
        assert j[i == r].min() == r * m // n and j[i == r].max() == -(-(r + 1) * m // n) - 1
    cost, _, _ = ref.transport_1d(sx, sy, p)
    want = ref.replicate_and_sort(sx, sy, p)
    assert abs(cost - want) <= 1e-12 * max(abs(want), 1e-300), (cost, want)


def test_overlap_formula_of_the_header():
    """w_ij = min((i+1) m, (j+1) n) - max(i m, j n), positive exactly on the plan's terms."""
    for n, m in [(6, 4), (5, 7), (1, 9), (8, 8)]:
        i, j, w = ref.plan(n, m)
        ii, jj = np.meshgrid(np.arange(n), np.arange(m), indexing="ij")
        full = np.minimum((ii + 1) * m, (jj + 1) * n) - np.maximum(ii * m, jj * n)
        dense = np.zeros((n, m), np.int64)
        dense[i, j] = w
        assert np.array_equal(np.maximum(full, 0), dense)


@pytest.mark.parametrize("n,m", [(9, 9), (12, 7), (5, 16)])
def test_gradient_equals_finite_differences(n, m):
    """p = 2, float64 throughout (the projections too), tie-free: central differences of the mean over the slices."""
    rng = np.random.default_rng(n + m)
    x, y = rng.standard_normal((n, 3)), rng.standard_normal((m, 3)) + 0.5
    dirs = rng.standard_normal((4, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)

    def value(x, y):
        proj = (np.stack([x @ t for t in dirs]), np.stack([y @ t for t in dirs]))
        return ref.swd(x, y, dirs, 2, projections=proj)

    _, gx, gy = value(x, y)
    h = 1e-6      # far below the smallest gap of the projections: the order does not change
    for pts, grad, side in ((x, gx, 0), (y, gy, 1)):
        for i in range(len(pts)):
            for c in range(3):
                hi, lo = pts.copy(), pts.copy()
                hi[i, c] += h
                lo[i, c] -= h
                fd = (value(*((hi, y) if side == 0 else (x, hi)))[0].mean()
                      - value(*((lo, y) if side == 0 else (x, lo)))[0].mean()) / (2 * h)
                assert abs(fd - grad[i, c]) <= 1e-7 * max(1.0, abs(fd)), (side, i, c, fd, grad[i, c])


def test_order_is_stable_and_treats_signed_zeros_as_equal():
    proj = np.array([0.0, -0.0, 1.0, -0.0, 0.0, -1.0], np.float32)
    assert ref.order(proj).tolist() == [5, 0, 1, 3, 4, 2]


def test_fp32_restatement_is_close_and_not_identical():
    rng = np.random.default_rng(3)
    x, y = rng.random((300, 3), np.float32), rng.random((200, 3), np.float32)
    dirs = rng.standard_normal((3, 3)).astype(np.float32)
    c64, gx64, gy64 = ref.swd(x, y, dirs, 2)
    c32, gx32, gy32 = ref.swd(x, y, dirs, 2, dtype=np.float32)
    assert c32.dtype == gx32.dtype == np.float32 and c64.dtype == np.float64
    assert np.allclose(c32, c64, rtol=1e-4) and np.allclose(gx32, gx64, atol=1e-6) and np.allclose(gy32, gy64, atol=1e-6)
    assert np.abs(gx32 - gx64).max() > 0


# ------------------------------------------------------------------------------------------ header and binding
def test_header_declares_the_three_functions():
    from sparenet_amd import _lib

    protos = _lib.prototypes(HEADER)
    assert sorted(protos) == NAMES
    ret, params = protos["sn_swd_forward"]
    assert ret == "int" and params[-1] == _lib.Param("stream", "void", True, False)
    assert _lib.Param("cost", "double", True, False) in params
    assert [p.name for p in params] == ["x", "y", "dirs", "b", "n", "m", "slices", "dirs_per_cloud", "x_lengths",
                                        "y_lengths", "p", "cost", "gradx", "grady", "workspace", "workspace_bytes",
                                        "stream"]
    ret, params = protos["sn_swd_project_sort"]
    assert ret == "int" and params[-1] == _lib.Param("stream", "void", True, False)
    assert [p.name for p in params] == ["x", "dirs", "b", "n", "slices", "dirs_per_cloud", "lengths", "sorted", "perm",
                                        "stream"]
    assert protos["sn_swd_workspace_bytes"][0] == "size_t"
    assert [p.name for p in protos["sn_swd_workspace_bytes"][1]] == ["b", "n", "m", "slices"]


def test_header_functions_are_exported_and_registered(monkeypatch):
    from sparenet_amd import _lib

    L = _lib.lib()
    for n in NAMES:
        assert hasattr(L, n), f"{n} declared in include/ops/swd.h but not exported"
    assert _lib.op_headers()["swd"] == HEADER
    assert sorted(_lib._op_calls["swd"]) == NAMES
    assert _lib.signature("sn_swd_forward") == ["x", "y", "dirs", "b", "n", "m", "slices", "dirs_per_cloud",
                                                "x_lengths", "y_lengths", "p", "cost", "gradx", "grady", "workspace"]
    assert L.sn_abi_version() == 4
    # the workspace does not grow with the slices beyond a chunk, and SN_SWD_CHUNK sets the chunk
    monkeypatch.delenv("SN_SWD_CHUNK", raising=False)
    size = lambda *shape: _lib.op_call("swd", "sn_swd_workspace_bytes", *shape)      # noqa: E731
    assert size(32, 16384, 16384, 16) == size(32, 16384, 16384, 128) == 32 * 16 * 32768 * 12
    assert size(32, 16384, 16384, 8) == size(32, 16384, 16384, 16) // 2
    assert size(0, 1, 1, 1) == 0
    monkeypatch.setenv("SN_SWD_CHUNK", "1")
    assert size(32, 16384, 16384, 128) == 32 * 32768 * 12
    monkeypatch.setenv("SN_SWD_CHUNK", "1000")
    assert size(2, 1024, 512, 7) == 2 * 7 * 1536 * 12


def test_library_refuses_bad_arguments_without_gpu():
    import sparenet_amd

    L = sparenet_amd.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(8)      # `one` is never dereferenced: validation fails first

    def refused(fn, text, *args):
        assert fn(*args) == -22
        assert text in L.sn_last_error(), L.sn_last_error()

    def forward(x=one, y=one, dirs=one, b=2, n=8, m=4, slices=3, p=2, cost=one, ws=one, nbytes=1 << 30):
        return (x, y, dirs, b, n, m, slices, 0, null, null, p, cost, null, null, ws, ctypes.c_size_t(nbytes), null)

    for missing in ("x", "y", "dirs", "cost"):
        refused(L.sn_swd_forward, b"null pointer", *forward(**{missing: null}))
    for size in ("b", "n", "m", "slices"):
        refused(L.sn_swd_forward, b">= 1", *forward(**{size: 0}))
    for size in ("n", "m"):
        refused(L.sn_swd_forward, b"at most 16384 points", *forward(**{size: 16385}))
    for p in (0, 3, -1):
        refused(L.sn_swd_forward, b"p must be 1 or 2", *forward(p=p))
    refused(L.sn_swd_forward, b"workspace too small", *forward(nbytes=16))
    refused(L.sn_swd_forward, b"workspace too small", *forward(ws=null))
    refused(L.sn_swd_project_sort, b"null pointer", null, one, 1, 8, 1, 0, null, one, one, null)
    refused(L.sn_swd_project_sort, b"at most 16384 points", one, one, 1, 16385, 1, 0, null, one, one, null)


# ------------------------------------------------------------------------------------------ the wrapper's checks
def test_wrapper_refuses_bad_arguments_before_anything_is_allocated(monkeypatch):
    import sparenet_amd
    from sparenet_amd import _lib
    from sparenet_amd.cuda import swd
    from sparenet_amd.utils import metrics

    def no_call(*a, **k):
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "op_call", no_call)
    monkeypatch.setattr(_lib, "op_workspace", no_call)
    monkeypatch.setattr(swd, "random_directions", no_call)      # nothing is drawn for a refused call either
    x, y = torch.zeros(2, 8, 3), torch.zeros(2, 4, 3)
    for p in (0, 3, 1.5, "2", True):
        with pytest.raises(ValueError, match="p must be 1 or 2"):
            swd.sliced_wasserstein(x, y, p=p)
    with pytest.raises(ValueError, match="reduction"):
        swd.sliced_wasserstein(x, y, reduction="sum")
    for bad in (torch.zeros(2, 8, 2), torch.zeros(8, 3), torch.zeros(2, 0, 3), torch.zeros(0, 8, 3)):
        with pytest.raises(ValueError, match=r"\[B, N, 3\]"):
            swd.sliced_wasserstein(bad, y)
        with pytest.raises(ValueError, match=r"\[B, N, 3\]"):
            swd.sliced_wasserstein(x, bad)
    with pytest.raises(TypeError, match="floating-point"):
        swd.sliced_wasserstein(x.int(), y)
    with pytest.raises(ValueError, match="at most 16384"):
        swd.sliced_wasserstein(torch.zeros(1, 16385, 3), torch.zeros(1, 4, 3))
    # CPU tensors: the message of a device entry point
    with pytest.raises(sparenet_amd.SparenetHipError, match="x: expected a CUDA"):
        swd.sliced_wasserstein(x, y)
    with pytest.raises(sparenet_amd.SparenetHipError, match="x: expected a CUDA"):
        swd.sorted_projections(x, torch.zeros(3, 3))
    with pytest.raises(sparenet_amd.SparenetHipError, match="x: expected a CUDA"):
        swd.SlicedWassersteinDistance(4)(x, y)
    with pytest.raises(sparenet_amd.SparenetHipError, match="x: expected a CUDA"):
        metrics.swd(x, y)
    with pytest.raises(ValueError):
        swd.SlicedWassersteinDistance(0)
    with pytest.raises(ValueError, match="p must be 1 or 2"):
        swd.SlicedWassersteinDistance(4, p=3)


def test_random_directions_are_unit_vectors_from_the_generator():
    from sparenet_amd.cuda.swd import random_directions

    a = random_directions(64, torch.device("cpu"), torch.Generator().manual_seed(5))
    b = random_directions(64, torch.device("cpu"), torch.Generator().manual_seed(5))
    assert a.shape == (64, 3) and a.dtype == torch.float32 and torch.equal(a, b)
    assert torch.allclose(a.norm(dim=1), torch.ones(64), atol=1e-6)
    with pytest.raises(ValueError):
        random_directions(0, torch.device("cpu"))


def test_exported_from_the_package():
    import sparenet_amd
    from sparenet_amd.cuda import swd

    for name in ("sliced_wasserstein", "sorted_projections", "random_directions", "SlicedWassersteinDistance"):
        assert getattr(sparenet_amd, name) is getattr(swd, name)
