"""Farthest point sampling without a GPU: the operator header (include/ops/fps.h) and its call path in sparenet_amd._lib
(op_call / op_workspace), the argument validation of sn_fps through direct ctypes with nothing dereferenced, the
workspace size export, the Python wrapper's refusals and the arguments it passes (against a converting stub), and
self-tests of the NumPy reference (tests/fps_ref.py) that the GPU tests compare against."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from fps_ref import fps_ref, fps_ref_batch, lattice_cloud, overflow_cloud, same_bits
from lib_stub import install

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
FPS_HEADER = os.path.join(INCLUDE, "ops", "fps.h")
NAMES = ["sn_fps", "sn_fps_workspace_bytes"]


def _declared(path):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"^(?:int|size_t|void|long long|const char \*)\s*(sn_[a-z0-9_]+)\s*\(", txt, re.M)))


# ------------------------------------------------------------------------------------------ header and binding
def test_fps_header_functions_are_exported_and_registered():
    from sparenet_amd import _lib

    assert os.path.isfile(FPS_HEADER)
    assert _declared(FPS_HEADER) == NAMES
    L = _lib.lib()
    for n in NAMES:
        assert hasattr(L, n), f"{n} declared in include/ops/fps.h but not exported"
    # only this operator's own header: the next one adds include/ops/<name>.h without touching this test
    assert "fps" in _lib.op_headers() and _lib.op_headers()["fps"] == FPS_HEADER
    assert sorted(_lib._op_calls["fps"]) == NAMES == sorted(_lib.prototypes(FPS_HEADER))
    assert _lib.signature("sn_fps") == ["xyz", "b", "n", "m", "lengths", "start", "idx", "min_dist", "workspace"]
    assert _lib.signature("sn_fps_workspace_bytes") == ["b", "n"]
    assert L.sn_abi_version() == 4


def test_the_other_registries_are_unchanged():
    from sparenet_amd import _lib

    _lib.lib()
    main = _declared(os.path.join(INCLUDE, "sparenet_hip.h"))
    ext = _declared(os.path.join(INCLUDE, "sparenet_hip_ext.h"))
    set_emd = os.path.join(INCLUDE, "sparenet_hip_ext_set_emd.h")
    assert sorted(_lib._calls) == main
    assert sorted(_lib._ext_calls) == ext
    assert _lib.topic_headers() == {"set_emd": set_emd}
    assert sorted(_lib._topic_calls) == ["set_emd"]
    assert sorted(_lib._topic_calls["set_emd"]) == _declared(set_emd)
    assert not set(NAMES) & (set(main) | set(ext) | set(_declared(set_emd)))


def test_op_call_serves_its_own_header_only():
    from sparenet_amd import SparenetHipError, _lib

    assert _lib.op_call("fps", "sn_fps_workspace_bytes", 1, 1) == 0
    with pytest.raises(SparenetHipError, match="ops/fps.h"):
        _lib.op_call("fps", "sn_mds_workspace_bytes", 2, 4096)                # the main header's
    with pytest.raises(SparenetHipError, match="ops/fps.h"):
        _lib.op_call("fps", "sn_set_emd_lds_bytes", 1, 1)                     # a topic header's
    with pytest.raises(SparenetHipError, match="sparenet_hip.h"):
        _lib.call("sn_fps_workspace_bytes", 1, 1)
    with pytest.raises(SparenetHipError, match="sparenet_hip_ext.h"):
        _lib.ext_call("sn_fps_workspace_bytes", 1, 1)
    with pytest.raises(SparenetHipError, match="sparenet_hip_ext_set_emd.h"):
        _lib.topic_call("set_emd", "sn_fps_workspace_bytes", 1, 1)
    with pytest.raises(SparenetHipError, match="ops/nothing.h"):
        _lib.op_call("nothing", "sn_fps_workspace_bytes", 1, 1)
    with pytest.raises(SparenetHipError, match="ops/nothing.h"):
        _lib.op_workspace("nothing", "sn_fps_workspace_bytes", torch.zeros(1), 1, 1)
    with pytest.raises(TypeError, match="takes 2 arguments"):
        _lib.op_call("fps", "sn_fps_workspace_bytes", 1)
    x = torch.rand(2, 8, 3)
    with pytest.raises(SparenetHipError, match="xyz: .*no CPU path"):
        _lib.op_call("fps", "sn_fps", x, 2, 8, 4, None, None, torch.empty(2, 4, dtype=torch.int32), None, None)


# ------------------------------------------------------------------------------------------ argument validation
def test_argument_validation_without_gpu():
    import sparenet_amd

    L = sparenet_amd.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(8)      # `one` is never dereferenced: validation fails first

    def refused(text, *args):
        assert L.sn_fps(*args) == -22
        assert text in L.sn_last_error(), L.sn_last_error()

    refused(b"null pointer", null, 2, 8, 4, null, null, one, null, null, 0, null)
    refused(b"null pointer", one, 2, 8, 4, null, null, null, null, null, 0, null)
    for b, n, m in ((0, 8, 4), (2, 0, 4), (2, 8, 0), (-1, 8, 4), (2, -8, 4), (2, 8, -4)):
        refused(b">= 1", one, b, n, m, null, null, one, null, null, 0, null)
    # beyond the resident size the workspace is needed: missing, then one byte short
    refused(b"workspace too small", one, 2, 24577, 4, null, null, one, null, null, 0, null)
    refused(b"workspace too small", one, 2, 24577, 4, null, null, one, null, one, 4 * 2 * 24577 - 1, null)


def test_workspace_bytes(monkeypatch):
    from sparenet_amd import _lib

    monkeypatch.delenv("SN_FPS_RESIDENT_MAX", raising=False)

    def size(b, n):
        return _lib.op_call("fps", "sn_fps_workspace_bytes", b, n)

    for n in (1, 64, 65, 1024, 16384, 24576):
        assert size(1, n) == 0 and size(32, n) == 0
    for b, n in ((1, 24577), (3, 24577), (2, 100000)):
        assert size(b, n) >= 4 * b * n
    assert size(0, 100000) == 0 and size(2, 0) == 0 and size(-1, -1) == 0
    # the knob lowers the limit (the tests reach the workspace path at small n), never raises it
    monkeypatch.setenv("SN_FPS_RESIDENT_MAX", "1000")
    assert size(2, 1000) == 0 and size(2, 1001) >= 4 * 2 * 1001
    monkeypatch.setenv("SN_FPS_RESIDENT_MAX", "100000")
    assert size(2, 24576) == 0 and size(2, 24577) >= 4 * 2 * 24577


# ------------------------------------------------------------------------------------------------ the wrapper
def test_wrapper_refusals():
    from sparenet_amd import SparenetHipError
    from sparenet_amd.cuda.fps import farthest_point_sample, furthest_point_sample, sample_points

    assert furthest_point_sample is farthest_point_sample
    x = torch.rand(2, 16, 3)
    with pytest.raises(SparenetHipError, match="no CPU path"):
        farthest_point_sample(x, 4)
    with pytest.raises(SparenetHipError, match="no CPU path"):
        sample_points(x, 4)
    for bad in (torch.rand(16, 3), torch.rand(2, 16, 2), torch.rand(0, 16, 3), torch.rand(2, 0, 3)):
        with pytest.raises(ValueError, match=r"\[B, N, 3\]"):
            farthest_point_sample(bad, 4)
    with pytest.raises(TypeError, match="floating-point"):
        farthest_point_sample(torch.zeros(2, 16, 3, dtype=torch.int32), 4)
    for npoint in (0, -1, 2.5):
        with pytest.raises(ValueError, match="npoint"):
            farthest_point_sample(x, npoint)


@pytest.fixture()
def stub(monkeypatch):
    """The converting, recording stub of tests/lib_stub.py in place of the library."""
    return install(monkeypatch, ("_op_calls",))


def _fps_args(calls):
    """(b, n, m, lengths is given, start is given, min_dist is given, workspace bytes) of each sn_fps call."""
    out = []
    for name, a in calls:
        if name == "sn_fps":
            xyz, b, n, m, lengths, start, idx, min_dist, ws, ws_bytes, stream = a
            assert xyz and idx and ws
            out.append((b, n, m, lengths is not None, start is not None, min_dist is not None, ws_bytes))
    return out


def test_wrapper_passes_what_it_was_given(stub):
    from sparenet_amd.cuda.fps import farthest_point_sample

    x = torch.rand(3, 40, 3, dtype=torch.float64)[:, ::2]      # neither fp32 nor contiguous: the wrapper converts
    idx = farthest_point_sample(x, 7)
    assert isinstance(idx, torch.Tensor) and idx.shape == (3, 7) and idx.dtype == torch.int32
    assert stub[0] == ("sn_fps_workspace_bytes", (3, 20))
    assert _fps_args(stub) == [(3, 20, 7, False, False, False, 4096)]

    del stub[:]
    idx, md = farthest_point_sample(x, 25, lengths=[0, 5, 20], start=[0, 4, 19], return_min_dist=True)
    assert idx.shape == md.shape == (3, 25) and md.dtype == torch.float32      # npoint may exceed the cloud
    assert _fps_args(stub) == [(3, 20, 25, True, True, True, 4096)]

    del stub[:]
    farthest_point_sample(x, 2, lengths=torch.tensor([20, 20, 1]), start=torch.tensor([0, 0, 0]))
    farthest_point_sample(x, 2, start=3)
    farthest_point_sample(x, 2, start=0, return_min_dist=True)
    assert _fps_args(stub) == [(3, 20, 2, True, False, False, 4096),      # an all-zero start is the default: null
                               (3, 20, 2, False, True, False, 4096),
                               (3, 20, 2, False, False, True, 4096)]


def test_wrapper_checks_host_lengths_and_start(stub):
    from sparenet_amd.cuda.fps import farthest_point_sample

    x = torch.rand(3, 20, 3)
    with pytest.raises(ValueError, match=r"lengths must be in \[0, 20\]"):
        farthest_point_sample(x, 4, lengths=[1, 21, 3])
    with pytest.raises(ValueError, match="expected 3 lengths"):
        farthest_point_sample(x, 4, lengths=[1, 2])
    with pytest.raises(TypeError, match="lengths"):
        farthest_point_sample(x, 4, lengths=torch.tensor([1.0, 2.0, 3.0]))
    for start in (20, -1, [0, 0, 20]):
        with pytest.raises(ValueError, match=r"start: must be in \[0, 20\)"):
            farthest_point_sample(x, 4, start=start)
    with pytest.raises(ValueError, match=r"start: must be in \[0, 5\) for cloud 1"):
        farthest_point_sample(x, 4, lengths=[20, 5, 20], start=[0, 5, 0])
    with pytest.raises(ValueError, match=r"start: must be in \[0, 1\) for cloud 0"):
        farthest_point_sample(x, 4, lengths=[0, 5, 20], start=[1, 0, 0])      # an empty cloud takes start 0 only
    with pytest.raises(ValueError, match="expected 3 values"):
        farthest_point_sample(x, 4, start=[0, 0])
    with pytest.raises(TypeError, match="start"):
        farthest_point_sample(x, 4, start=1.5)
    with pytest.raises(TypeError, match="start"):
        farthest_point_sample(x, 4, start=torch.tensor([0.0, 1.0, 2.0]))
    assert not _fps_args(stub)


# ------------------------------------------------------------------------------------------ the reference itself
def test_reference_against_float64_brute_force():
    """Points whose candidate distances are far apart in every step, so fp32 rounding cannot change a pick: the
    reference's picks are those of a float64 search, and its min_dist is the float64 one rounded."""
    rng = np.random.default_rng(5)
    x = rng.random((200, 3)).astype(np.float32)
    m = 40
    idx, md = fps_ref(x, m, start=3)
    x64 = x.astype(np.float64)
    mind = np.full(200, np.inf)
    c = 3
    for k in range(m):
        assert idx[k] == c
        assert md[k] == np.float32(mind[c]) or abs(md[k] - mind[c]) <= 4e-7 * mind[c]
        mind = np.minimum(mind, ((x64 - x64[c]) ** 2).sum(axis=1))
        top = np.sort(mind)[-2:]
        assert top[1] - top[0] > 1e-5 * top[1], "the test's points are not well separated"
        c = int(np.argmax(mind))
    assert len(set(idx.tolist())) == m


def test_reference_on_a_lattice_of_ties():
    idx, md = fps_ref(lattice_cloud(), 512)
    assert sorted(idx.tolist()) == list(range(512))
    assert md[0] == np.inf and np.all(md[1:] >= 1) and np.all(np.diff(md[1:]) <= 0)
    # 512 picks share a handful of distance values: ties everywhere, all broken towards the lowest index
    assert len(np.unique(md)) < 64, len(np.unique(md))


def test_reference_degenerate_clouds():
    same = np.full((20, 3), 0.25, np.float32)
    idx, md = fps_ref(same, 6, start=7)
    assert idx.tolist() == [7, 0, 0, 0, 0, 0]
    assert md[0] == np.inf and not md[1:].any() and not np.signbit(md[1:]).any()

    x = np.random.default_rng(2).random((10, 3)).astype(np.float32)
    x[3:] = 1e30                                                     # padding rows: never read into a result
    idx, md = fps_ref(x, 6, length=3)
    alone = fps_ref(x[:3], 6)
    assert np.array_equal(idx, alone[0]) and same_bits(md, alone[1])
    assert sorted(idx[:3].tolist()) == [0, 1, 2] and idx[3:].tolist() == [0, 0, 0] and not md[3:].any()
    line = np.array([[0, 0, 0], [3, 0, 0], [1, 0, 0]], np.float32)   # 1 is the farthest from 0, then 2, then all 0
    assert fps_ref(np.concatenate([line, x[3:]]), 6, length=3)[0].tolist() == [0, 1, 2, 0, 0, 0]

    idx, md = fps_ref(x, 4, length=0)
    assert idx.tolist() == [-1] * 4 and np.isnan(md).all()

    idx, md = fps_ref(overflow_cloud(), 70)                           # every distance overflows: all-inf ties
    assert idx.tolist() == list(range(64)) + [0] * 6 and np.isinf(md[:64]).all() and not md[64:].any()

    bi, bm = fps_ref_batch(np.stack([x, x]), 5, lengths=[3, 10], start=[2, 9])
    assert np.array_equal(bi[0], fps_ref(x, 5, length=3, start=2)[0]) and same_bits(bm[1], fps_ref(x, 5, start=9)[1])
