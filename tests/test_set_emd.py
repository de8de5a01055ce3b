"""The set-level EMD without a GPU: the third header (include/sparenet_hip_ext_set_emd.h) and its call path in
sparenet_amd._lib (topic_call), the argument validation of sn_set_emd_sums through direct ctypes with nothing
dereferenced, the LDS size export, the call sites of emd_direction_sums / emd_matrix against a converting stub (the
swap for n > m, the emd_general loop beyond 2048 points), and set_metrics' unchanged default."""
import ctypes
import os
import re

import pytest
import torch

from lib_stub import install

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
SET_EMD_HEADER = os.path.join(INCLUDE, "sparenet_hip_ext_set_emd.h")
NAMES = ["sn_set_emd_lds_bytes", "sn_set_emd_sums"]


def _declared(path):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"^(?:int|size_t|void|long long|const char \*)\s*(sn_[a-z0-9_]+)\s*\(", txt, re.M)))


# ------------------------------------------------------------------------------------------ header and binding
def test_set_emd_header_functions_are_exported_and_registered():
    from sparenet_amd import _lib

    assert _declared(SET_EMD_HEADER) == NAMES
    L = _lib.lib()
    for n in NAMES:
        assert hasattr(L, n), f"{n} declared in include/sparenet_hip_ext_set_emd.h but not exported"
    assert _lib.topic_headers() == {"set_emd": SET_EMD_HEADER}
    assert sorted(_lib._topic_calls) == ["set_emd"]
    assert sorted(_lib._topic_calls["set_emd"]) == NAMES == sorted(_lib.prototypes(SET_EMD_HEADER))
    assert _lib.signature("sn_set_emd_sums") == ["x", "y", "nx", "n", "ny", "m", "eps", "iters", "sums", "assignment"]
    assert _lib.signature("sn_set_emd_lds_bytes") == ["n", "m"]
    assert L.sn_abi_version() == 4


def test_the_other_two_registries_are_what_their_headers_declare():
    from sparenet_amd import _lib

    _lib.lib()
    main = _declared(os.path.join(INCLUDE, "sparenet_hip.h"))
    ext = _declared(os.path.join(INCLUDE, "sparenet_hip_ext.h"))
    assert sorted(_lib._calls) == main
    assert sorted(_lib._ext_calls) == ext
    assert not set(NAMES) & (set(main) | set(ext))


def test_topic_call_serves_its_own_header_only():
    from sparenet_amd import SparenetHipError, _lib

    assert _lib.topic_call("set_emd", "sn_set_emd_lds_bytes", 1, 1) > 0
    with pytest.raises(SparenetHipError, match="sparenet_hip_ext_set_emd.h"):
        _lib.topic_call("set_emd", "sn_set_chamfer_workspace_bytes", 2, 3, 4096)      # the second header's
    with pytest.raises(SparenetHipError, match="sparenet_hip_ext_set_emd.h"):
        _lib.topic_call("set_emd", "sn_abi_version")                                  # the main header's
    with pytest.raises(SparenetHipError, match="sparenet_hip.h"):
        _lib.call("sn_set_emd_lds_bytes", 1, 1)
    with pytest.raises(SparenetHipError, match="sparenet_hip_ext.h"):
        _lib.ext_call("sn_set_emd_lds_bytes", 1, 1)
    with pytest.raises(SparenetHipError, match="sparenet_hip_ext_nothing.h"):
        _lib.topic_call("nothing", "sn_set_emd_lds_bytes", 1, 1)
    with pytest.raises(TypeError, match="takes 2 arguments"):
        _lib.topic_call("set_emd", "sn_set_emd_lds_bytes", 1)
    x = torch.rand(2, 8, 3)
    with pytest.raises(SparenetHipError, match="x: .*no CPU path"):
        _lib.topic_call("set_emd", "sn_set_emd_sums", x, x, 2, 8, 2, 8, 0.005, 5,
                        torch.empty(2, 2, dtype=torch.float64), None)


# ------------------------------------------------------------------------------------------ argument validation
def test_argument_validation_without_gpu():
    import sparenet_amd

    L = sparenet_amd.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(8)      # `one` is never dereferenced: validation fails first
    eps = ctypes.c_float(0.005)

    def refused(text, *args):
        assert L.sn_set_emd_sums(*args) == -22
        assert text in L.sn_last_error(), L.sn_last_error()

    for x, y, sums in ((null, one, one), (one, null, one), (one, one, null)):
        refused(b"null pointer", x, y, 2, 8, 3, 8, eps, 5, sums, null, null)
    for nx, n, ny, m in ((0, 8, 3, 8), (2, 0, 3, 8), (2, 8, 0, 8), (2, 8, 3, 0), (-1, 8, 3, 8), (2, 8, 3, -1)):
        refused(b">= 1", one, one, nx, n, ny, m, eps, 5, one, null, null)
    refused(b"pass the smaller clouds first", one, one, 2, 9, 3, 8, eps, 5, one, null, null)
    refused(b"points per cloud", one, one, 2, 8, 3, 2049, eps, 5, one, null, null)
    refused(b"points per cloud", one, one, 2, 2049, 3, 2049, eps, 5, one, null, null)
    refused(b"iters", one, one, 2, 8, 3, 8, eps, -1, one, null, null)
    refused(b"nx * ny must not exceed 2^31 - 1", one, one, 1 << 16, 8, 1 << 15, 8, eps, 5, one, null, null)
    # 2^20 pairs of 2048 bidders: fine for the sums, one entry too many for an int-indexed assignment
    refused(b"nx * ny * n must not exceed 2^31 - 1", one, one, 1 << 10, 2048, 1 << 10, 2048, eps, 5, one, one, null)
    # more pairs than one launch takes
    refused(b"too large", one, one, 1 << 11, 8, 1 << 11, 8, eps, 5, one, null, null)


def test_lds_bytes():
    import sparenet_amd

    L = sparenet_amd.lib()
    L.sn_set_emd_lds_bytes.restype = ctypes.c_size_t
    assert 0 < L.sn_set_emd_lds_bytes(2048, 2048) <= 160 * 1024
    assert L.sn_set_emd_lds_bytes(1, 1) > 0
    assert L.sn_set_emd_lds_bytes(5, 4) == 0
    assert L.sn_set_emd_lds_bytes(1, 2049) == 0
    assert L.sn_set_emd_lds_bytes(0, 4) == 0
    # the arrays the kernel's header names: a 16-byte record, 8-byte window word and three words per target; three
    # coordinates and five words per bidder
    assert L.sn_set_emd_lds_bytes(2048, 2048) >= 2048 * (16 + 8 + 12) + 2048 * (12 + 20)
    # two workgroups per CU at 1024 points
    assert 2 * L.sn_set_emd_lds_bytes(1024, 1024) <= 160 * 1024


# ------------------------------------------------------------------------------------------------- call sites
@pytest.fixture()
def stub(monkeypatch):
    """The converting, recording stub of tests/lib_stub.py in place of the library."""
    return install(monkeypatch, ("_calls", "_topic_calls"))


def _named(calls, name):
    return [args for n, args in calls if n == name]


def test_wrappers_pass_convertible_arguments(stub):
    from sparenet_amd.cuda.set_distance import emd_direction_sums, emd_matrix

    x, y = torch.rand(3, 5, 3), torch.rand(2, 8, 3)
    out = emd_direction_sums(x, y)
    assert out.shape == (3, 2) and out.dtype == torch.float64
    (args,) = _named(stub, "sn_set_emd_sums")
    assert len(args) == 11                                          # ten declared parameters and the stream
    assert args[2:6] == (3, 5, 2, 8) and args[7] == 50 and abs(args[6] - 0.005) < 1e-9
    assert args[9] is None                                          # metrics pass no assignment
    del stub[:]
    sums, assignment = emd_direction_sums(x, y, eps=-0.001, iters=0, return_assignment=True)
    assert sums.shape == (3, 2) and assignment.shape == (3, 2, 5) and assignment.dtype == torch.int32
    (args,) = _named(stub, "sn_set_emd_sums")
    assert args[7] == 0 and args[6] < 0 and args[9] == assignment.data_ptr()
    with pytest.raises(ValueError, match="pass the smaller clouds first"):
        emd_direction_sums(y, x)
    with pytest.raises(ValueError, match="iters"):
        emd_direction_sums(x, y, iters=-1)
    with pytest.raises(ValueError, match="iters"):
        emd_direction_sums(x, y, iters=2.5)
    del stub[:]
    assert emd_matrix(x, y, 0.01, 7).shape == (3, 2)
    (args,) = _named(stub, "sn_set_emd_sums")
    assert args[2:6] == (3, 5, 2, 8) and args[7] == 7


def test_emd_matrix_swaps_the_sets_when_the_first_has_the_larger_clouds(stub):
    from sparenet_amd.cuda.set_distance import emd_matrix

    x, y = torch.rand(3, 9, 3), torch.rand(2, 4, 3)
    out = emd_matrix(x, y)
    assert out.shape == (3, 2) and out.dtype == torch.float64        # the swapped call's [2, 3], transposed
    (args,) = _named(stub, "sn_set_emd_sums")
    assert args[0] == y.data_ptr() and args[1] == x.data_ptr()
    assert args[2:6] == (2, 4, 3, 9)


def test_clouds_beyond_the_kernel_take_the_emd_general_loop(stub, monkeypatch):
    from sparenet_amd.cuda import set_distance as SD

    x, y = torch.rand(3, 7, 3), torch.rand(2, 2049, 3)
    out, assignment = SD.emd_direction_sums(x, y, return_assignment=True)
    assert out.shape == (3, 2) and out.dtype == torch.float64 and assignment.shape == (3, 2, 7)
    assert not _named(stub, "sn_set_emd_sums")
    loop = _named(stub, "sn_emd_forward_general")
    assert len(loop) == 1 and loop[0][2:5] == (6, 7, 2049)           # all six pairs in one chunk
    # the bound on expanded memory decides the chunks: room for two pairs -> three calls of two pairs
    del stub[:]
    monkeypatch.setattr(SD, "_EMD_LOOP_EXPANDED_BYTES", 2 * 12 * (7 + 2049))
    assert SD.emd_matrix(x, y).shape == (3, 2)
    assert [a[2:5] for a in _named(stub, "sn_emd_forward_general")] == [(2, 7, 2049)] * 3
    # ... and never fewer than one pair
    del stub[:]
    monkeypatch.setattr(SD, "_EMD_LOOP_EXPANDED_BYTES", 1)
    SD.emd_matrix(x, y)
    assert [a[2] for a in _named(stub, "sn_emd_forward_general")] == [1] * 6
    # the larger clouds first: swapped, and still the loop
    del stub[:]
    assert SD.emd_matrix(y, x).shape == (2, 3)
    assert not _named(stub, "sn_set_emd_sums") and len(_named(stub, "sn_emd_forward_general")) == 6
    # 2048 points are the kernel's
    del stub[:]
    SD.emd_matrix(x, torch.rand(2, 2048, 3))
    assert len(_named(stub, "sn_set_emd_sums")) == 1 and not _named(stub, "sn_emd_forward_general")


def test_set_metrics_default_is_the_three_chamfer_keys(monkeypatch):
    """set_metrics builds its dict from the matrix functions; here they are stand-ins that return a fixed random
    matrix of the right shape and record the call."""
    from sparenet_amd.cuda import set_distance as SD
    from sparenet_amd.utils import set_metrics as M

    calls = []

    def matrix(kind):
        def fn(a, b, *args):
            calls.append((kind, a.size(0), b.size(0)) + args)
            g = torch.Generator().manual_seed(a.size(0) * 7 + b.size(0))
            return torch.rand(a.size(0), b.size(0), dtype=torch.float64, generator=g)
        return fn

    monkeypatch.setattr(SD, "chamfer_matrix", matrix("cd"))
    monkeypatch.setattr(SD, "emd_matrix", matrix("emd"))
    gen, ref = torch.rand(3, 8, 3), torch.rand(2, 8, 3)
    out = M.set_metrics(gen, ref)
    assert list(out) == ["MMD-CD", "COV-CD", "1-NNA-CD"]
    assert calls == [("cd", 3, 2), ("cd", 3, 3), ("cd", 2, 2)]
    del calls[:]
    both = M.set_metrics(gen, ref, with_emd=True, emd_iters=3)
    assert list(both) == ["MMD-CD", "COV-CD", "1-NNA-CD", "MMD-EMD", "COV-EMD", "1-NNA-EMD"]
    assert all(v.dtype == torch.float64 and v.dim() == 0 for v in both.values())
    assert all(both[k].item() == out[k].item() for k in out)
    assert calls[3:] == [("emd", 3, 2, 0.005, 3), ("emd", 3, 3, 0.005, 3), ("emd", 2, 2, 0.005, 3)]
    # the EMD keys are the metric functions on the EMD matrices, the lower-left block being emd_gr transposed
    gr, gg, rr = (matrix("emd")(a, b) for a, b in ((gen, ref), (gen, gen), (ref, ref)))
    assert both["MMD-EMD"].item() == M.minimum_matching_distance(gr).item()
    assert both["COV-EMD"].item() == M.coverage(gr).item()
    assert both["1-NNA-EMD"].item() == M.one_nn_accuracy(gg, gr, rr).item()
    del calls[:]
    M.set_metrics(gen, ref, with_emd=True, emd_rr=rr, cd_rr=rr)
    assert [c[:3] for c in calls] == [("cd", 3, 2), ("cd", 3, 3), ("emd", 3, 2), ("emd", 3, 3)]


# --------------------------------------------------------------------------------------------------- refusals
def test_wrappers_refuse_what_the_kernel_cannot_take(stub, monkeypatch):
    from sparenet_amd import SparenetHipError, _lib
    from sparenet_amd.cuda.set_distance import emd_direction_sums, emd_matrix

    y = torch.rand(2, 9, 3)
    for bad in (torch.rand(3, 8, 2), torch.rand(3, 8, 3).double(), torch.rand(8, 3),
                torch.rand(3, 3, 8).transpose(1, 2), torch.rand(0, 8, 3)):
        for fn in (emd_direction_sums, emd_matrix):
            with pytest.raises((ValueError, TypeError), match="^x: "):
                fn(bad, y)
            with pytest.raises((ValueError, TypeError), match="^y: "):
                fn(torch.rand(2, 4, 3), bad)
    # emd_matrix names the caller's tensor also where it would swap the sets
    with pytest.raises(ValueError, match="^y: "):
        emd_matrix(torch.rand(2, 100, 3), torch.rand(3, 8, 2))
    monkeypatch.undo()      # the real device check: CPU tensors are refused
    x = torch.rand(2, 8, 3)
    for fn in (emd_direction_sums, emd_matrix):
        with pytest.raises(SparenetHipError, match="^x: .*no CPU path"):
            fn(x, x)
