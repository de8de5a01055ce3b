"""Set-level metrics without a GPU: MMD-CD / COV-CD / 1-NNA-CD (sparenet_amd/utils/set_metrics.py) on hand-built
distance matrices with known answers and against the loop restatement (tests/set_metrics_ref.py); the extension header
(include/sparenet_hip_ext.h) and its call path in sparenet_amd._lib; the argument validation of sn_set_chamfer_sums
through direct ctypes, with nothing dereferenced."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import set_metrics_ref as R
from lib_stub import install

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT_HEADER = os.path.join(ROOT, "include", "sparenet_hip_ext.h")


def _metrics():
    from sparenet_amd.utils import set_metrics as M
    return M


def _t(a):
    return torch.tensor(a, dtype=torch.float64)


def _distinct_symmetric(k, seed, lo=1.0, hi=2.0):
    """[k, k] symmetric, zero diagonal, pairwise distinct off-diagonal values in [lo, hi)."""
    r = np.random.default_rng(seed)
    vals = lo + (hi - lo) * (r.permutation(k * k) + 0.5) / (k * k)
    a = np.triu(vals.reshape(k, k), 1)
    return a + a.T


# ------------------------------------------------------------------------------------------- known answers
def test_two_well_separated_groups_are_told_apart():
    M = _metrics()
    gg, rr = _distinct_symmetric(4, 0, 0.1, 0.2), _distinct_symmetric(3, 1, 0.1, 0.2)     # G != R
    gr = 10.0 + np.random.default_rng(2).random((4, 3))
    assert M.one_nn_accuracy(_t(gg), _t(gr), _t(rr)).item() == 1.0
    assert R.one_nna(gg, gr, rr) == 1.0


def test_a_set_against_itself():
    """gen identical to ref, clouds pairwise distinct: every cloud's nearest neighbour is its twin in the other set."""
    M = _metrics()
    d = _distinct_symmetric(5, 3)
    acc = M.one_nn_accuracy(_t(d), _t(d), _t(d))
    assert acc.dtype == torch.float64 and acc.dim() == 0 and acc.item() == 0.0
    assert M.coverage(_t(d)).item() == 1.0
    assert M.minimum_matching_distance(_t(d)).item() == 0.0
    assert (R.one_nna(d, d, d), R.cov(d), R.mmd(d)) == (0.0, 1.0, 0.0)


def test_every_generated_cloud_nearest_to_one_reference_cloud():
    M = _metrics()
    gr = 1.0 + np.random.default_rng(4).random((6, 4))
    gr[:, 2] = 0.25
    cov = M.coverage(_t(gr))
    assert cov.dtype == torch.float64 and cov.item() == 0.25 == R.cov(gr)
    assert M.minimum_matching_distance(_t(gr)).item() == R.mmd(gr)


def test_an_exact_tie_goes_to_the_lower_index():
    M = _metrics()
    # COV: both generated clouds are exactly as near to reference 1 as to reference 3 -> both count for 1
    gr = np.array([[5.0, 0.5, 4.0, 0.5], [6.0, 0.75, 7.0, 0.75]])
    assert M.coverage(_t(gr)).item() == 0.25 == R.cov(gr)
    # 1-NNA: a reference cloud exactly as near to generated 0 (concatenated index 0) as to reference 1 (index 3):
    # the generated cloud decides and the reference cloud is misclassified; with the tie broken upwards it would not be
    gg = np.array([[0.0, 1.0], [1.0, 0.0]])
    rr = np.array([[0.0, 2.0], [2.0, 0.0]])
    gr = np.array([[2.0, 3.0], [9.0, 9.0]])       # reference 0: generated 0 at 2.0, reference 1 at 2.0
    want = R.one_nna(gg, gr, rr)
    assert want == 0.75       # generated 0, 1 right (each other); reference 0 wrong (tie -> generated 0); reference 1 right
    assert M.one_nn_accuracy(_t(gg), _t(gr), _t(rr)).item() == want


def test_metric_functions_refuse_misshapen_matrices():
    M = _metrics()
    with pytest.raises(ValueError, match="cd_gg"):
        M.one_nn_accuracy(torch.zeros(3, 3), torch.zeros(2, 4), torch.zeros(4, 4))
    with pytest.raises(ValueError, match="cd_rr"):
        M.one_nn_accuracy(torch.zeros(2, 2), torch.zeros(2, 4), torch.zeros(3, 3))
    with pytest.raises(ValueError, match="cd_gr"):
        M.coverage(torch.zeros(4))
    with pytest.raises(ValueError, match="NaN"):
        M.coverage(torch.full((2, 2), float("nan")))


@pytest.mark.parametrize("g,r,seed", [(7, 7, 0), (5, 9, 1), (12, 3, 2), (1, 4, 3), (4, 1, 4)])
def test_random_matrices_agree_with_the_restatement(g, r, seed):
    M = _metrics()
    rng = np.random.default_rng(seed)
    gg, rr = rng.random((g, g)), rng.random((r, r))
    gg, rr = gg + gg.T, rr + rr.T
    np.fill_diagonal(gg, 0.0)
    np.fill_diagonal(rr, 0.0)
    gr = 2 * rng.random((g, r))
    gr[rng.integers(g), :] = gr[rng.integers(g), :]                  # a duplicated generated cloud: exact ties
    assert M.coverage(_t(gr)).item() == R.cov(gr)                    # ratios of integers: equal
    assert M.one_nn_accuracy(_t(gg), _t(gr), _t(rr)).item() == R.one_nna(gg, gr, rr)
    want = R.mmd(gr)
    assert abs(M.minimum_matching_distance(_t(gr)).item() - want) <= 1e-15 * want
    assert R.argmin_gaps(gg, gr, rr).shape == (g + g + r,)


def test_set_metrics_is_reexported_beside_the_other_metrics():
    from sparenet_amd.utils import metrics, set_metrics
    assert metrics.set_metrics is set_metrics.set_metrics


# ----------------------------------------------------------------------------------- the extension header
def _declared(path):
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"^(?:int|size_t|void|long long|const char \*)\s*(sn_[a-z0-9_]+)\s*\(", txt, re.M)))


def test_extension_header_functions_are_exported_and_registered():
    from sparenet_amd import _lib

    names = _declared(EXT_HEADER)
    assert names == ["sn_set_chamfer_sums", "sn_set_chamfer_workspace_bytes"]
    L = _lib.lib()
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/sparenet_hip_ext.h but not exported"
    assert sorted(_lib._ext_calls) == names == sorted(_lib.prototypes(EXT_HEADER))
    assert _lib.signature("sn_set_chamfer_sums") == ["x", "y", "nx", "n", "ny", "m", "sums", "workspace"]
    assert _lib.signature("sn_set_chamfer_workspace_bytes") == ["nx", "ny", "n"]
    # the main header's registry is what it was: the two lists do not mix
    main = _declared(os.path.join(ROOT, "include", "sparenet_hip.h"))
    assert sorted(_lib._calls) == main and not set(main) & set(names)
    assert L.sn_abi_version() == 4


def test_each_call_path_serves_its_own_header_only():
    from sparenet_amd import SparenetHipError, _lib

    assert _lib.ext_call("sn_set_chamfer_workspace_bytes", 2, 3, 4096) > 0
    with pytest.raises(SparenetHipError, match="sparenet_hip.h"):
        _lib.call("sn_set_chamfer_workspace_bytes", 2, 3, 4096)
    with pytest.raises(SparenetHipError, match="sparenet_hip_ext.h"):
        _lib.ext_call("sn_abi_version")
    with pytest.raises(TypeError, match="takes 3 arguments"):
        _lib.ext_call("sn_set_chamfer_workspace_bytes", 2, 3)
    x = torch.rand(2, 8, 3)
    with pytest.raises(SparenetHipError, match="x: .*no CPU path"):
        _lib.ext_call("sn_set_chamfer_sums", x, x, 2, 8, 2, 8, torch.empty(2, 2, dtype=torch.float64), None)


def test_lib_refuses_to_load_without_the_extension_header(monkeypatch, tmp_path):
    from sparenet_amd import SparenetHipError, _lib

    _lib.lib()
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "EXT_HEADER_PATH", str(tmp_path / "sparenet_hip_ext.h"))
    with pytest.raises(SparenetHipError, match="sparenet_hip_ext.h not found"):
        _lib.lib()


# ------------------------------------------------------------------------------------ argument validation
def test_argument_validation_without_gpu():
    import sparenet_amd

    L = sparenet_amd.lib()
    L.sn_set_chamfer_workspace_bytes.restype = ctypes.c_size_t
    null, one, big = ctypes.c_void_p(0), ctypes.c_void_p(8), ctypes.c_size_t(1 << 30)   # `one` is never dereferenced

    def refused(text, *args):
        assert L.sn_set_chamfer_sums(*args) == -22
        assert text in L.sn_last_error(), L.sn_last_error()

    for x, y, sums in ((null, one, one), (one, null, one), (one, one, null)):
        refused(b"null pointer", x, y, 2, 8, 3, 8, sums, one, big, null)
    refused(b">= 1", one, one, 2, 0, 3, 8, one, one, big, null)          # n = 0
    refused(b">= 1", one, one, 0, 8, 3, 8, one, one, big, null)
    refused(b">= 1", one, one, 2, 8, 3, -1, one, one, big, null)
    refused(b"points per cloud", one, one, 2, (1 << 20) + 1, 3, 8, one, one, big, null)
    refused(b"points per cloud", one, one, 2, 8, 3, (1 << 20) + 1, one, one, big, null)
    refused(b"2^31 - 1", one, one, 1 << 16, 8, 1 << 15, 8, one, one, big, null)
    refused(b"too large", one, one, 1 << 15, 8, 1 << 15, 8, one, one, big, null)
    need = L.sn_set_chamfer_workspace_bytes(2, 3, 2049)
    assert need >= 2 * 3 * 2 * 8        # two query blocks per cloud, one double each
    refused(b"workspace too small", one, one, 2, 2049, 3, 8, one, one, ctypes.c_size_t(need - 1), null)
    refused(b"workspace too small", one, one, 2, 2049, 3, 8, one, null, big, null)
    assert L.sn_set_chamfer_workspace_bytes(2, 3, 2048) == 0            # one block per cloud: nothing to carve
    for bad in ((0, 3, 4096), (2, 0, 4096), (2, 3, 0), (2, 3, (1 << 20) + 1), (1 << 16, 1 << 15, 4096)):
        assert L.sn_set_chamfer_workspace_bytes(*bad) == 0, bad


# ------------------------------------------------------------------------------------------- the wrappers
def test_wrappers_refuse_what_the_kernel_cannot_take():
    from sparenet_amd import SparenetHipError
    from sparenet_amd.cuda.set_distance import chamfer_direction_sums, chamfer_matrix

    x = torch.rand(2, 8, 3)
    with pytest.raises(SparenetHipError, match="x: .*no CPU path"):
        chamfer_direction_sums(x, x)
    with pytest.raises(SparenetHipError, match="x: .*no CPU path"):
        chamfer_matrix(x, x)


def test_wrappers_pass_convertible_arguments_and_a_set_against_itself_is_one_call(monkeypatch):
    """The call sites of the extension path, exercised as tests/test_callsites.py does for the main header: a stub in
    place of the library that only converts what ext_call hands it with the argtypes parsed from the header."""
    from sparenet_amd.cuda.set_distance import chamfer_matrix

    calls = install(monkeypatch, ("_ext_calls",), record=lambda name, args: name)
    x, y = torch.rand(3, 8, 3), torch.rand(2, 5, 3)
    assert chamfer_matrix(x, y).shape == (3, 2)
    assert calls.count("sn_set_chamfer_sums") == 2
    del calls[:]
    out = chamfer_matrix(x, x)
    assert out.shape == (3, 3) and out.dtype == torch.float64
    assert calls.count("sn_set_chamfer_sums") == 1
    del calls[:]
    chamfer_matrix(x, x.view(3, 8, 3))      # the same storage and shape under another tensor object
    assert calls.count("sn_set_chamfer_sums") == 1
    for bad, name in ((torch.rand(3, 8, 2), "x"), (torch.rand(3, 8, 3).double(), "x"), (torch.rand(8, 3), "x"),
                      (torch.rand(3, 3, 8).transpose(1, 2), "x")):
        with pytest.raises((ValueError, TypeError), match=f"^{name}: "):
            chamfer_matrix(bad, y)
        with pytest.raises((ValueError, TypeError), match="^y: "):
            chamfer_matrix(y, bad)
