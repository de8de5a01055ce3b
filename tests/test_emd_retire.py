"""The auction's wave retirement (emd.hip: once a cloud is sparse, a workgroup lets waves 8-15 end and goes on with
waves 0-7): every setting of SN_EMD_RETIRE must give the bits of oracle/emd.c -- assignment, distances and the
device's pair counter (unassigned bidders x n, summed over the iterations).

SN_EMD_RETIRE: "0" never, "-1" from iteration 0 (the whole call at 8 waves: seeds, matrix-core search, scan),
"-2" / "-4" a switch while the matrix-core search is still in use, "1000000" at the first iteration that is neither
contested nor far, unset = the tuned default.  A team retires in its LAST cloud only."""
import functools
import os

import numpy as np
import pytest

import oracle
from test_emd import _clouds, _contested, _golden, _hip

RETIRE = ["0", "-1", "-2", "-4", "1000000", None]

# (kind, b, n, iters, eps, seed)
CASES = [
    ("uniform", 3, 1024, 7, 0.005, 1),
    ("uniform", 9, 1024, 20, 0.005, 9),      # batch not a multiple of 8
    ("uniform", 2, 2048, 10, -0.001, 10),    # prices may fall
    ("lattice", 2, 1024, 6, 0.005, 5),       # massive exact ties
    ("clustered", 1, 8192, 6, 0.005, 11),    # long hit queues on 8 waves
    ("far", 2, 1024, 8, 0.005, 12),
    ("uniform", 1, 16384, 9, 0.005, 13),     # the boxes fill the LDS copy
    ("uniform", 1, 32768, 3, 0.005, 14),     # no scan: retired waves use the matrix-core search only
    ("contested", 40, 1024, 6, 0.002, 23),   # the smallest teams
    ("contested", 2, 2048, 12, 0.005, 21),   # a retired workgroup in contested iterations (forced retirement only)
    ("uniform", 70, 1024, 10, 0.005, 31),    # teams of two workgroups (256 CUs: 128 teams, one cloud each)
    ("uniform", 260, 1024, 5, 0.005, 33),    # 256 CUs: more clouds than teams -- a team's first cloud runs at full
                                             # width, its second may retire; the scan's boxes change hands in LDS
    ("uniform", 3, 1024, 1, 0.005, 32),      # only the forced last iteration
    ("uniform", 1, 1024, 0, 0.005, 8),       # no iteration at all
]


@functools.lru_cache(maxsize=None)
def _case(kind, b, n, iters, eps, seed):
    """The clouds and the oracle's answer, computed once and shared by every setting."""
    x, y = _contested(b, n, seed) if kind == "contested" else _clouds(b, n, seed, kind)
    d, a, aux = oracle.emd_forward(x, y, eps, iters, mt=True, return_aux=True)
    return x, y, d, a, int(aux["pairs_eff"])


def _set(monkeypatch, retire):
    if retire is None:
        monkeypatch.delenv("SN_EMD_RETIRE", raising=False)
    else:
        monkeypatch.setenv("SN_EMD_RETIRE", retire)


def _check(case, dev, tag):
    kind, b, n, iters, eps, seed = case
    x, y, d0, a0, pairs = _case(*case)
    d1, a1, st = _hip(x, y, eps, iters, dev, stats=True)
    if iters == 0:
        assert (a1 == -1).all() and (d1 == 0).all() and int(st[0]) == 0, (tag, case)
        return
    assert np.array_equal(a0, a1), (tag, case)
    assert np.array_equal(d0, d1), (tag, case)
    assert int(st[0]) == pairs, (tag, case)


@pytest.mark.gpu
@pytest.mark.parametrize("retire", RETIRE)
def test_retire_matches_emulated_reference_golden(retire, golden_dir, dev, monkeypatch):
    _set(monkeypatch, retire)
    seen_contested = seen_negeps = 0
    for f in _golden(golden_dir):
        z = np.load(f)
        seen_contested += "contested" in os.path.basename(f)
        seen_negeps += float(z["eps"]) < 0
        d, a, st = _hip(z["xyz1"], z["xyz2"], float(z["eps"]), int(z["iters"]), dev, stats=True)
        assert np.array_equal(a, z["assignment"]), (f, retire)
        assert np.array_equal(d, z["dist"]), (f, retire)
        assert st[0] == int(z["unass"].astype(np.int64).sum()) * z["xyz1"].shape[1], (f, retire)
    assert seen_contested >= 4 and seen_negeps >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("retire", RETIRE)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%dx%d-it%d" % c[:4])
def test_retire_matches_oracle(case, retire, dev, monkeypatch):
    _set(monkeypatch, retire)
    _check(case, dev, retire)


@pytest.mark.gpu
@pytest.mark.parametrize("retire", RETIRE)
def test_retire_with_outbid_skip_in_every_iteration(retire, dev, monkeypatch):
    """SN_EMD_SKIP=2: every iteration is a contested one -- only a forced retirement happens, and the retired
    workgroup then bids with the outbid-skip and the transposed split."""
    _set(monkeypatch, retire)
    monkeypatch.setenv("SN_EMD_SKIP", "2")
    _check(("contested", 2, 2048, 12, 0.005, 21), dev, retire)


@pytest.mark.gpu
@pytest.mark.parametrize("scan", ["0", "1000000"])
def test_retire_with_either_bid_form(scan, dev, monkeypatch):
    """Retirement at iteration 1 with the matrix-core search only, and with the scan from the first iteration on."""
    monkeypatch.setenv("SN_EMD_RETIRE", "-2")
    monkeypatch.setenv("SN_EMD_SCAN", scan)
    _check(("near", 2, 1024, 15, 0.005, 4), dev, "-2/scan=" + scan)


@pytest.mark.gpu
def test_retired_workgroup_leaves_a_nan_bidder_unassigned(dev, monkeypatch):
    """A bidder with a NaN coordinate never bids: at 8 waves, too, it ends unassigned with distance 0 and the rest of
    the cloud is what the full-width call gives."""
    x, y = (v.copy() for v in _clouds(2, 1024, 41))
    x[1, 333, 1] = np.nan
    monkeypatch.setenv("SN_EMD_RETIRE", "0")
    d0, a0 = _hip(x, y, 0.005, 10, dev)
    monkeypatch.setenv("SN_EMD_RETIRE", "-1")
    d1, a1 = _hip(x, y, 0.005, 10, dev)
    assert a1[1, 333] == -1 and d1[1, 333] == 0
    assert np.array_equal(a0, a1) and np.array_equal(d0, d1)
    xo, yo = _clouds(2, 1024, 41)
    do, ao = oracle.emd_forward(xo[:1], yo[:1], 0.005, 10, mt=True)  # the cloud without the NaN: the oracle's bits
    assert np.array_equal(ao, a1[:1]) and np.array_equal(do, d1[:1])
