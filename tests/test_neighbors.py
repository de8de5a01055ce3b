"""Neighbourhood queries without a GPU: the operator header (include/ops/neighbors.h) and its call path in
sparenet_amd._lib, every SN_EINVAL case through direct ctypes with nothing dereferenced, the workspace size exports,
the Python wrappers' refusals and the arguments they pass (against a converting stub), and self-tests of the NumPy
reference (tests/neighbors_ref.py) on hand-computed cases."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from lib_stub import _scalars, install
from neighbors_ref import (ball_ref, ball_ref_batch, dist_matrix, group_backward_ref, group_ref, interpolate_ref,
                           knn_ref, knn_ref_batch, lattice_points, same_bits, sum_bound)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ops", "neighbors.h")
NAMES = sorted(["sn_neighbors_workspace_bytes", "sn_knn_query", "sn_ball_query", "sn_group_forward",
                "sn_interpolate_forward", "sn_group_backward_workspace_bytes", "sn_group_backward"])


def _declared(path):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"^(?:int|size_t|void|long long|const char \*)\s*(sn_[a-z0-9_]+)\s*\(", txt, re.M)))


# ------------------------------------------------------------------------------------------ header and binding
def test_header_functions_are_exported_and_registered():
    from sparenet_amd import _lib

    assert _declared(HEADER) == NAMES
    L = _lib.lib()
    for n in NAMES:
        assert hasattr(L, n), f"{n} declared in include/ops/neighbors.h but not exported"
    assert _lib.op_headers()["neighbors"] == HEADER
    assert sorted(_lib._op_calls["neighbors"]) == NAMES == sorted(_lib.prototypes(HEADER))
    assert _lib.signature("sn_neighbors_workspace_bytes") == ["b", "n", "m", "k"]
    assert _lib.signature("sn_knn_query") == ["xyz", "new_xyz", "b", "n", "m", "k", "lengths", "new_lengths", "idx",
                                              "dist2", "workspace"]
    assert _lib.signature("sn_ball_query") == ["xyz", "new_xyz", "b", "n", "m", "radius", "nsample", "pad_first",
                                               "lengths", "new_lengths", "idx", "cnt", "workspace"]
    assert _lib.signature("sn_group_forward") == ["features", "idx", "b", "c", "n", "m", "s", "out"]
    assert _lib.signature("sn_interpolate_forward") == ["features", "idx", "weight", "b", "c", "n", "m", "s", "out"]
    assert _lib.signature("sn_group_backward_workspace_bytes") == ["b", "n", "m", "s"]
    assert _lib.signature("sn_group_backward") == ["grad_out", "idx", "weight", "b", "c", "n", "m", "s",
                                                   "grad_features", "workspace"]
    assert L.sn_abi_version() == 4


def test_op_call_serves_its_own_header_only():
    from sparenet_amd import SparenetHipError, _lib

    assert _lib.op_call("neighbors", "sn_group_backward_workspace_bytes", 1, 1, 1, 1) > 0
    with pytest.raises(SparenetHipError, match="ops/neighbors.h"):
        _lib.op_call("neighbors", "sn_fps_workspace_bytes", 1, 1)                   # another operator's
    with pytest.raises(SparenetHipError, match="ops/neighbors.h"):
        _lib.op_call("neighbors", "sn_mds_workspace_bytes", 2, 4096)                # the main header's
    with pytest.raises(SparenetHipError, match="ops/fps.h"):
        _lib.op_call("fps", "sn_neighbors_workspace_bytes", 1, 1, 1, 1)
    with pytest.raises(SparenetHipError, match="sparenet_hip.h"):
        _lib.call("sn_knn_query")
    with pytest.raises(TypeError, match="takes 4 arguments"):
        _lib.op_call("neighbors", "sn_neighbors_workspace_bytes", 1, 1)
    x = torch.rand(2, 8, 3)
    with pytest.raises(SparenetHipError, match="xyz: .*no CPU path"):
        _lib.op_call("neighbors", "sn_knn_query", x, x, 2, 8, 8, 3, None, None,
                     torch.empty(2, 8, 3, dtype=torch.int32), None, None)


# ------------------------------------------------------------------------------------------ argument validation
def test_argument_validation_without_gpu():
    import sparenet_amd

    L = sparenet_amd.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(8)      # `one` is never dereferenced: validation fails first
    f = ctypes.c_float

    def refused(fn, text, *args):
        assert fn(*args) == -22
        assert text in L.sn_last_error(), L.sn_last_error()

    # sn_knn_query(xyz, new_xyz, b, n, m, k, lengths, new_lengths, idx, dist2, workspace, workspace_bytes, stream)
    def knn(xyz=one, new_xyz=one, b=2, n=8, m=4, k=3, idx=one):
        return (xyz, new_xyz, b, n, m, k, null, null, idx, null, null, 0, null)

    for missing in ("xyz", "new_xyz", "idx"):
        refused(L.sn_knn_query, b"null pointer", *knn(**{missing: null}))
    for size in ("b", "n", "m"):
        for v in (0, -3):
            refused(L.sn_knn_query, b">= 1", *knn(**{size: v}))
    for k in (0, -1, 33, 1000):
        refused(L.sn_knn_query, b"1 <= k <= 32", *knn(k=k))

    # sn_ball_query(xyz, new_xyz, b, n, m, radius, nsample, pad_first, lengths, new_lengths, idx, cnt, ws, bytes, stream)
    def ball(xyz=one, new_xyz=one, b=2, n=8, m=4, radius=0.1, nsample=4, idx=one):
        return (xyz, new_xyz, b, n, m, f(radius), nsample, 1, null, null, idx, null, null, 0, null)

    for missing in ("xyz", "new_xyz", "idx"):
        refused(L.sn_ball_query, b"null pointer", *ball(**{missing: null}))
    for size in ("b", "n", "m"):
        for v in (0, -3):
            refused(L.sn_ball_query, b">= 1", *ball(**{size: v}))
    for nsample in (0, -2):
        refused(L.sn_ball_query, b"nsample >= 1", *ball(nsample=nsample))
    for radius in (-1e-30, -1.0, float("inf"), float("-inf"), float("nan")):
        refused(L.sn_ball_query, b"radius must be finite and >= 0", *ball(radius=radius))

    # sn_group_forward(features, idx, b, c, n, m, s, out, stream)
    def group(features=one, idx=one, b=2, c=3, n=8, m=4, s=2, out=one):
        return (features, idx, b, c, n, m, s, out, null)

    for missing in ("features", "idx", "out"):
        refused(L.sn_group_forward, b"null pointer", *group(**{missing: null}))
    for size in ("b", "c", "n", "m", "s"):
        for v in (0, -3):
            refused(L.sn_group_forward, b">= 1", *group(**{size: v}))

    # sn_interpolate_forward(features, idx, weight, b, c, n, m, s, out, stream)
    def interpolate(features=one, idx=one, weight=one, b=2, c=3, n=8, m=4, s=2, out=one):
        return (features, idx, weight, b, c, n, m, s, out, null)

    for missing in ("features", "idx", "weight", "out"):
        refused(L.sn_interpolate_forward, b"null pointer", *interpolate(**{missing: null}))
    for size in ("b", "c", "n", "m", "s"):
        for v in (0, -3):
            refused(L.sn_interpolate_forward, b">= 1", *interpolate(**{size: v}))

    # sn_group_backward(grad_out, idx, weight, b, c, n, m, s, grad_features, workspace, workspace_bytes, stream)
    need = L.sn_group_backward_workspace_bytes(2, 8, 4, 2)

    def backward(grad_out=one, idx=one, weight=null, b=2, c=3, n=8, m=4, s=2, grad_features=one, ws=one, nbytes=need):
        return (grad_out, idx, weight, b, c, n, m, s, grad_features, ws, nbytes, null)

    for missing in ("grad_out", "idx", "grad_features", "ws"):
        refused(L.sn_group_backward, b"null pointer", *backward(**{missing: null}))
    for size in ("b", "c", "n", "m", "s"):
        for v in (0, -3):
            refused(L.sn_group_backward, b">= 1", *backward(**{size: v}))
    for weight in (null, one):
        refused(L.sn_group_backward, b"workspace too small", *backward(weight=weight, nbytes=need - 1))
        refused(L.sn_group_backward, b"workspace too small", *backward(weight=weight, nbytes=0))


def test_workspace_bytes():
    from sparenet_amd import _lib

    def search(b, n, m, k):
        return _lib.op_call("neighbors", "sn_neighbors_workspace_bytes", b, n, m, k)

    def backward(b, n, m, s):
        return _lib.op_call("neighbors", "sn_group_backward_workspace_bytes", b, n, m, s)

    for bad in ((0, 8, 4, 2), (2, 0, 4, 2), (2, 8, 0, 2), (2, 8, 4, 0), (-1, -1, -1, -1)):
        assert search(*bad) == 0 and backward(*bad) == 0
    # the searches need none at any shape; the backward's lists: one int per target and one per slot
    for shape in ((1, 1, 1, 1), (3, 2048, 512, 32), (32, 16384, 2048, 16)):
        assert search(*shape) == 0
        b, n, m, s = shape
        assert backward(*shape) >= 4 * b * (n + m * s)
    base = (2, 100, 50, 3)
    for axis in range(4):
        sizes = []
        for grow in (0, 1, 7, 1000):
            shape = list(base)
            shape[axis] += grow
            sizes.append((search(*shape), backward(*shape)))
        assert sizes == sorted(sizes) and sizes[0][1] < sizes[-1][1], (axis, sizes)


# ------------------------------------------------------------------------------------------------ the wrappers
def test_wrapper_refusals():
    from sparenet_amd import SparenetHipError
    from sparenet_amd.cuda import neighbors as nb

    x, q = torch.rand(2, 16, 3), torch.rand(2, 5, 3)
    feats, idx, w = torch.rand(2, 4, 16), torch.zeros(2, 5, 3, dtype=torch.int32), torch.rand(2, 5, 3)
    for call in (lambda: nb.ball_query(0.1, 4, x, q), lambda: nb.knn_query(3, x, q), lambda: nb.three_nn(q, x),
                 lambda: nb.grouping_operation(feats, idx), lambda: nb.three_interpolate(feats, idx, w),
                 lambda: nb.interpolate_features(q, x, feats)):
        with pytest.raises(SparenetHipError, match="no CPU path"):
            call()
    for bad in (torch.rand(16, 3), torch.rand(2, 16, 2), torch.rand(0, 16, 3), torch.rand(2, 0, 3)):
        with pytest.raises(ValueError, match=r"\[B, N, 3\]"):
            nb.knn_query(3, bad, q)
        with pytest.raises(ValueError, match=r"\[B, N, 3\]"):
            nb.ball_query(0.1, 4, x, bad)
    with pytest.raises(ValueError, match="batch sizes differ"):
        nb.knn_query(3, x, torch.rand(3, 5, 3))
    with pytest.raises(TypeError, match="floating-point"):
        nb.knn_query(3, torch.zeros(2, 16, 3, dtype=torch.int32), q)
    with pytest.raises(TypeError, match="floating-point"):
        nb.ball_query(0.1, 4, x, torch.zeros(2, 5, 3, dtype=torch.int64))
    for k in (0, -1, 33, 2.5):
        with pytest.raises(ValueError, match="k must be an integer >= 1 and <= 32"):
            nb.knn_query(k, x, q)
    for nsample in (0, -1, 2.5):
        with pytest.raises(ValueError, match="nsample must be an integer >= 1"):
            nb.ball_query(0.1, nsample, x, q)
    for radius in (-0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="radius"):
            nb.ball_query(radius, 4, x, q)
    for pad in ("zero", None, 1):
        with pytest.raises(ValueError, match="pad must be 'first' or 'none'"):
            nb.ball_query(0.1, 4, x, q, pad=pad)
    with pytest.raises(ValueError, match=r"\[B, C, N\]"):
        nb.grouping_operation(torch.rand(16, 3), idx)
    with pytest.raises(TypeError, match="floating-point"):
        nb.grouping_operation(torch.zeros(2, 4, 16, dtype=torch.int32), idx)
    with pytest.raises(TypeError, match="int32 / int64"):
        nb.grouping_operation(feats, idx.float())
    for bad in (torch.zeros(2, 5, dtype=torch.int32), torch.zeros(3, 5, 3, dtype=torch.int32)):
        with pytest.raises(ValueError, match=r"\[B, M, S\]"):
            nb.grouping_operation(feats, bad)
    with pytest.raises(ValueError, match="weight must have idx's shape"):
        nb.three_interpolate(feats, idx, torch.rand(2, 5, 2))
    with pytest.raises(TypeError, match="weight"):
        nb.three_interpolate(feats, idx, idx)


@pytest.fixture()
def stub(monkeypatch):
    """The converting, recording stub of tests/lib_stub.py in place of the library."""
    return install(monkeypatch, ("_op_calls",))


def test_search_wrappers_pass_what_they_were_given(stub):
    from sparenet_amd.cuda import neighbors as nb

    x = torch.rand(3, 40, 3, dtype=torch.float64)[:, ::2]      # neither fp32 nor contiguous: the wrapper converts
    q = torch.rand(3, 7, 3)
    dist2, idx = nb.knn_query(5, x, q)
    assert dist2.shape == idx.shape == (3, 7, 5) and dist2.dtype == torch.float32 and idx.dtype == torch.int32
    assert stub[0] == ("sn_neighbors_workspace_bytes", (3, 20, 7, 5))
    name, a = stub[1]
    #                              xyz  new_xyz b  n   m  k  lengths new_lengths idx  dist2  ws  bytes
    assert name == "sn_knn_query" and _scalars(a) == (True, True, 3, 20, 7, 5, False, False, True, True, True, 4096)
    del stub[:]
    nb.knn_query(32, x, q, lengths=[0, 5, 20], new_lengths=torch.tensor([7, 0, 1]))
    assert _scalars(stub[1][1]) == (True, True, 3, 20, 7, 32, True, True, True, True, True, 4096)

    del stub[:]
    dist, idx = nb.three_nn(q, x)                              # (unknown, known): the queries come first
    assert dist.shape == idx.shape == (3, 7, 3)
    assert _scalars(stub[1][1])[2:6] == (3, 20, 7, 3)

    del stub[:]
    idx = nb.ball_query(0.25, 9, x, q)
    assert isinstance(idx, torch.Tensor) and idx.shape == (3, 7, 9) and idx.dtype == torch.int32
    assert stub[0] == ("sn_neighbors_workspace_bytes", (3, 20, 7, 9))
    name, a = stub[1]
    #                               xyz  new_xyz b  n   m  radius nsample pad lengths new_lengths idx cnt ws bytes
    assert name == "sn_ball_query" and _scalars(a) == (True, True, 3, 20, 7, 0.25, 9, 1, False, False, True, False,
                                                       True, 4096)
    del stub[:]
    idx, cnt = nb.ball_query(0.25, 9, x, q, lengths=[1, 2, 3], pad="none", return_count=True)
    assert cnt.shape == (3, 7) and cnt.dtype == torch.int32
    assert _scalars(stub[1][1]) == (True, True, 3, 20, 7, 0.25, 9, 0, True, False, True, True, True, 4096)

    with pytest.raises(ValueError, match="expected 3 lengths"):
        nb.knn_query(3, x, q, lengths=[1, 2])
    with pytest.raises(ValueError, match=r"lengths must be in \[0, 20\]"):
        nb.ball_query(0.1, 4, x, q, lengths=[1, 21, 3])
    with pytest.raises(ValueError, match="expected 3 lengths"):
        nb.ball_query(0.1, 4, x, q, new_lengths=[1, 2, 3, 4])
    with pytest.raises(ValueError, match=r"new_lengths: lengths must be in \[0, 7\]"):
        nb.knn_query(3, x, q, new_lengths=[1, 8, 3])


def test_gather_wrappers_pass_what_they_were_given(stub):
    from sparenet_amd.cuda import neighbors as nb

    feats = torch.rand(2, 4, 16, dtype=torch.float64, requires_grad=True)
    idx = torch.randint(-1, 16, (2, 5, 3))                     # int64: converted
    out = nb.grouping_operation(feats, idx)
    assert out.shape == (2, 4, 5, 3) and out.dtype == torch.float32
    name, a = stub[0]
    assert name == "sn_group_forward" and _scalars(a) == (True, True, 2, 4, 16, 5, 3, True)
    del stub[:]
    out.backward(torch.ones_like(out))
    assert feats.grad.shape == feats.shape
    assert stub[0] == ("sn_group_backward_workspace_bytes", (2, 16, 5, 3))
    name, a = stub[1]
    #                                   grad_out idx weight b  c  n   m  s  grad_features ws  bytes stream
    assert name == "sn_group_backward" and _scalars(a) == (True, True, False, 2, 4, 16, 5, 3, True, True, 4096)

    del stub[:]
    feats = torch.rand(2, 4, 16, requires_grad=True)
    w = torch.rand(2, 5, 3, requires_grad=True)
    out = nb.three_interpolate(feats, idx, w)
    assert out.shape == (2, 4, 5)
    name, a = stub[0]
    assert name == "sn_interpolate_forward" and _scalars(a) == (True, True, True, 2, 4, 16, 5, 3, True)
    del stub[:]
    out.backward(torch.ones_like(out))
    assert w.grad is None                                      # the weights are constants
    assert _scalars(stub[1][1]) == (True, True, True, 2, 4, 16, 5, 3, True, True, 4096)


# ------------------------------------------------------------------------------------------ the reference itself
def _cube():
    """The 2 x 2 x 2 lattice, index = 4 x + 2 y + z."""
    return np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)


def test_reference_knn_on_the_unit_lattice():
    cube = _cube()
    idx, d = knn_ref(cube, cube[:1], 8)
    # from the corner: itself, three edge neighbours (index order 1, 2, 4), three face diagonals, the far corner
    assert idx[0].tolist() == [0, 1, 2, 4, 3, 5, 6, 7] and d[0].tolist() == [0, 1, 1, 1, 2, 2, 2, 3]
    idx, d = knn_ref(cube, np.array([[0.5, 0.5, 0.5]], np.float32), 3)
    assert idx[0].tolist() == [0, 1, 2] and d[0].tolist() == [0.75] * 3      # eight ties: the lowest indices
    idx, d = knn_ref(cube, cube[7:], 10, length=3)                           # k beyond the cloud
    assert idx[0].tolist() == [1, 2, 0] + [-1] * 7 and d[0, :3].tolist() == [2, 2, 3] and np.isinf(d[0, 3:]).all()
    idx, d = knn_ref(cube, cube, 2, new_length=1)                            # padding queries
    assert idx[0].tolist() == [0, 1] and (idx[1:] == -1).all() and np.isinf(d[1:]).all()
    idx, d = knn_ref(cube, cube, 2, length=0)                                # an empty cloud
    assert (idx == -1).all() and np.isinf(d).all()


def test_reference_preselection_is_the_stable_argsort():
    rng = np.random.default_rng(9)
    x = (rng.integers(0, 12, (5000, 3)) / 8).astype(np.float32)      # a few hundred distinct distances: ties everywhere
    q = (rng.integers(0, 12, (40, 3)) / 8).astype(np.float32)
    for k in (1, 16, 32):
        fast, plain = knn_ref(x, q, k), knn_ref(x, q, k, preselect=False)
        assert np.array_equal(fast[0], plain[0]) and same_bits(fast[1], plain[1])
        assert (np.diff(plain[1], axis=1) == 0).any() or k == 1


def test_reference_ball_query_conventions():
    cube = _cube()
    q = cube[:1]
    # radius exactly 1: the three edge neighbours lie AT the radius and are excluded
    idx, cnt = ball_ref(cube, q, 1.0, 4)
    assert idx[0].tolist() == [0, 0, 0, 0] and cnt[0] == 1
    idx, cnt = ball_ref(cube, q, 1.0, 4, pad_first=False)
    assert idx[0].tolist() == [0, -1, -1, -1] and cnt[0] == 1
    idx, cnt = ball_ref(cube, q, 1.0001, 6)
    assert idx[0].tolist() == [0, 1, 2, 4, 0, 0] and cnt[0] == 4
    idx, cnt = ball_ref(cube, q, 1.5, 3)                                     # more hits than slots: the first ones
    assert idx[0].tolist() == [0, 1, 2] and cnt[0] == 3
    far = np.array([[5, 5, 5]], np.float32)                                  # no hit: -1 under both conventions
    for pad_first in (True, False):
        idx, cnt = ball_ref(cube, far, 1.0, 3, pad_first=pad_first)
        assert idx[0].tolist() == [-1] * 3 and cnt[0] == 0
        idx, cnt = ball_ref(cube, q, 0.0, 3, pad_first=pad_first)            # radius 0: d < 0 never holds
        assert idx[0].tolist() == [-1] * 3 and cnt[0] == 0
        idx, cnt = ball_ref(cube, cube, 2.0, 3, pad_first=pad_first, length=0)
        assert (idx == -1).all() and not cnt.any()
        idx, cnt = ball_ref(cube, cube, 2.0, 3, pad_first=pad_first, new_length=2)
        assert (idx[2:] == -1).all() and not cnt[2:].any() and cnt[:2].tolist() == [3, 3]
    bi, bc = ball_ref_batch(np.stack([cube, cube]), np.stack([q, q]), 1.0001, 6, lengths=[8, 2])
    assert bi[0, 0].tolist() == [0, 1, 2, 4, 0, 0] and bi[1, 0].tolist() == [0, 1, 0, 0, 0, 0] and bc[:, 0].tolist() == [4, 2]
    ki, _ = knn_ref_batch(np.stack([cube, cube]), np.stack([q, q]), 3, lengths=[8, 2])
    assert ki[1, 0].tolist() == [0, 1, -1]


def test_reference_lattice_has_ties_at_the_radius():
    pts = lattice_points()
    d = dist_matrix(pts[:10], pts)
    assert (d == np.float32(0.0625)).sum() >= 20 and len(np.unique(d)) < 40


def test_reference_gathers_and_backward():
    feats = np.arange(2 * 3 * 4, dtype=np.float32).reshape(2, 3, 4)
    idx = np.array([[[0, 3], [-1, 2]], [[1, 1], [-1, -1]]], np.int32)
    out = group_ref(feats, idx)
    assert out.shape == (2, 3, 2, 2)
    assert out[0, 1].tolist() == [[4, 7], [0, 6]] and out[1, 2].tolist() == [[21, 21], [0, 0]]
    w = np.array([[[0.5, 0.25], [9, 2]], [[1, 3], [1, 1]]], np.float32)
    got = interpolate_ref(feats, idx, w)
    assert got[0, 1].tolist() == [0.5 * 4 + 0.25 * 7, 2 * 6.0] and got[1, 2].tolist() == [4 * 21.0, 0.0]
    # the order is left to right: 1e8 + 1 - 1e8 in fp32 is 0, not 1
    f = np.array([[[1e8, 1.0, -1e8]]], np.float32)
    assert interpolate_ref(f, np.array([[[0, 1, 2]]], np.int32), np.ones((1, 1, 3), np.float32))[0, 0, 0] == 0.0
    assert interpolate_ref(f, np.array([[[0, 2, 1]]], np.int32), np.ones((1, 1, 3), np.float32))[0, 0, 0] == 1.0
    assert same_bits(interpolate_ref(-f * 0, np.array([[[-1, 1, -1]]], np.int32), np.ones((1, 1, 3), np.float32)),
                     np.array([[[-0.0]]], np.float32))          # a lone product keeps its sign of zero

    g = np.ones((2, 3, 2, 2))
    grad, mag, length = group_backward_ref(g, idx, 4)
    assert grad[0, 0].tolist() == [1, 0, 1, 1] and grad[1, 2].tolist() == [0, 2, 0, 0]
    assert length.tolist() == [[1, 0, 1, 1], [0, 2, 0, 0]] and np.array_equal(grad, mag)
    grad, mag, _ = group_backward_ref(np.full((2, 3, 2), -2.0), idx, 4, weight=w)
    assert grad[0, 0].tolist() == [-1, 0, -4, -0.5] and grad[1, 1].tolist() == [0, -8, 0, 0]
    assert mag[1, 1].tolist() == [0, 8, 0, 0]
    assert sum_bound(0) < 1.2e-7 and 8190 * 2.0 ** -24 < sum_bound(8192) < 8200 * 2.0 ** -24
