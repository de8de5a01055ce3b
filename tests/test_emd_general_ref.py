"""The NumPy restatement of the general-size auction (tests/emd_general_ref.py) against the oracle's C restatement of
the reference auction and against the emulated-reference goldens, on the sizes both cover (n == m, n % 1024 == 0).
CPU only: the GPU tests of the general path (test_emd_general.py) trust the restatement because of these."""
import glob
import os

import numpy as np
import pytest

import oracle
from emd_general_ref import emd_general, emd_general_backward


def _clouds(b, n, m, seed, kind="uniform"):
    r = np.random.default_rng(seed)
    x = r.random((b, n, 3), dtype=np.float32)
    y = r.random((b, m, 3), dtype=np.float32)
    if kind == "contested":   # duplicate points on both sides: exact ties in the bid values
        x = x[:, r.integers(0, max(1, n // 8), n)]
        y = y[:, r.integers(0, max(1, m // 4), m)]
    return np.ascontiguousarray(x), np.ascontiguousarray(y)


@pytest.mark.parametrize("b,n,kind,eps,iters", [
    (2, 1024, "uniform", 0.005, [1, 3, 10]),
    (1, 2048, "contested", 0.005, [1, 4, 12]),
    (1, 1024, "uniform", -0.001, [1, 2, 6]),
    (1, 1024, "contested", -0.002, [3, 5]),
    (1, 3072, "uniform", 0.002, [2, 5]),
])
def test_restatement_equals_oracle(b, n, kind, eps, iters):
    x, y = _clouds(b, n, n, 100 + n + b, kind)
    got = emd_general(x, y, eps, iters)
    for k in iters:
        d0, a0, aux = oracle.emd_forward(x, y, eps, k, mt=True, return_aux=True)
        d, a, pairs = got[k]
        assert np.array_equal(a, a0), (kind, eps, k)
        assert np.array_equal(d, d0), (kind, eps, k)
        assert pairs == aux["pairs_eff"], (kind, eps, k)


def test_restatement_equals_every_emulated_golden(golden_dir):
    files = sorted(glob.glob(os.path.join(golden_dir, "emd_*.npz")))
    assert len(files) >= 10
    for f in files:
        z = np.load(f)
        d, a, pairs = emd_general(z["xyz1"], z["xyz2"], float(z["eps"]), int(z["iters"]))
        assert np.array_equal(a, z["assignment"]), f
        assert np.array_equal(d, z["dist"]), f
        assert pairs == int(z["unass"].astype(np.int64).sum()) * z["xyz1"].shape[1], f


def test_restatement_zero_iterations_and_single_point():
    x, y = _clouds(2, 5, 9, 3)
    d, a, pairs = emd_general(x, y, 0.005, 0)
    assert (a == -1).all() and (d == 0).all() and pairs == 0
    x, y = _clouds(1, 1, 1, 4)
    d, a, pairs = emd_general(x, y, 0.005, 3)
    assert a.tolist() == [[0]] and pairs == 1
    assert d[0, 0] == np.float32(((x - y) ** 2).sum())


def test_restatement_backward_matches_oracle_and_sums_shared_targets():
    x, y = _clouds(2, 1024, 1024, 7)
    d, a = oracle.emd_forward(x, y, 0.005, 3)
    gd = np.random.default_rng(1).random((2, 1024), dtype=np.float32)
    g1, g2 = emd_general_backward(x, y, gd, a)
    assert np.array_equal(g1, oracle.emd_backward(x, y, gd, a))
    # one iteration: every bidder is forced onto its first choice, several share a target
    x, y = _clouds(1, 300, 700, 8, "contested")
    d, a, _ = emd_general(x, y, 0.005, 1)
    assert len(np.unique(a[0])) < 300
    gd = np.random.default_rng(2).random((1, 300), dtype=np.float32)
    g1, g2 = emd_general_backward(x, y, gd, a)
    ref = np.zeros((700, 3), np.float32)
    for j in range(300):
        ref[a[0, j]] = ref[a[0, j]] - g1[0, j]
    assert np.array_equal(g2[0], ref)
    np.testing.assert_allclose(g2.sum((0, 1)), -g1.sum((0, 1)), rtol=1e-4, atol=1e-5)
