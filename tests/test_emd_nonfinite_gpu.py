"""Non-finite rows in the two auctions that share sparenet_amd/csrc/emd_auction.hpp: sn_emd_forward_general (the
stream-ordered launches) and sn_set_emd_sums (one workgroup per pair).

A bidder with a NaN or infinite coordinate passes no filter, so it posts no bid and touches no target word; it is
re-queued every iteration and skipped by the forced assignment of the last one.  All it changes is the unassigned
count, which enters the tie key (k / delta, k) alone -- and for m <= 2048 that key orders the targets by index whatever
delta is.  So every other bidder must come out, bit for bit, as tests/emd_general_ref.py computes it for the same
clouds with the non-finite bidder rows deleted (compared through the row map), and the non-finite rows come back
unassigned with dist 0.  A non-finite target (the last row, so no index shifts) is never bid for, and the auction
equals the restatement on the cloud without it.  The stats words are not asserted: they count the non-finite bidders'
scans."""
import numpy as np
import pytest
import torch

import emd_general_ref as E

pytestmark = pytest.mark.gpu

N, M, EPS, ITERS = 70, 200, 0.005, [1, 3, 50]
BAD = {0: (np.nan, 0.5, 0.5), 33: (np.inf, 0.0, 0.0), 69: (0.1, -np.inf, 0.2)}
KEEP = np.array([j for j in range(N) if j not in BAD])


def _oracle(x, y):
    """{k: (dist [2, 2, n'], assignment [2, 2, n'])} of every pair (x_i, y_j), from one pass of the restatement."""
    n = x.shape[1]
    res = E.emd_general(np.repeat(x, 2, axis=0), np.tile(y, (2, 1, 1)), EPS, ITERS)
    return {k: (d.reshape(2, 2, n), a.reshape(2, 2, n)) for k, (d, a, _) in res.items()}


@pytest.fixture(scope="module")
def bad_bidders():
    """(x [2, N, 3] with the rows of BAD replaced, y [2, M, 3], the oracle of x without those rows)."""
    r = np.random.default_rng(2026)
    x = r.random((2, N, 3), dtype=np.float32)
    y = r.random((2, M, 3), dtype=np.float32)
    for j, row in BAD.items():
        x[:, j] = row
    return x, y, _oracle(np.ascontiguousarray(x[:, KEEP]), y)


@pytest.fixture(scope="module")
def bad_target():
    """(x [2, N, 3] finite, y [2, M, 3] whose last row is NaN, the oracle of y without that row)."""
    r = np.random.default_rng(2027)
    x = r.random((2, N, 3), dtype=np.float32)
    y = r.random((2, M, 3), dtype=np.float32)
    y[:, M - 1] = np.nan
    return x, y, _oracle(x, np.ascontiguousarray(y[:, :M - 1]))


def _general(x, y, iters, dev):
    from sparenet_amd.cuda.emd.emd_general import emd_general

    d, a = emd_general(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), EPS, iters)
    return d.cpu().numpy(), a.cpu().numpy()


def _set_level(x, y, iters, dev):
    from sparenet_amd.cuda.set_distance import emd_direction_sums

    sums, a = emd_direction_sums(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), EPS, iters,
                                 return_assignment=True)
    return sums.cpu().numpy(), a.cpu().numpy()


def _assert_sums(got, want_dist, n, what):
    """the bound of tests/test_set_emd_gpu.py: both sides add the same n non-negative doubles, each in some order"""
    want = np.sqrt(want_dist).astype(np.float64).sum(axis=2)
    err = np.abs(got - want)
    print(f"{what}: max |got - want| / want = {np.max(err / want):.3e}, bound {n * 2.0 ** -52:.3e}")
    assert got.dtype == np.float64 and (err <= n * 2.0 ** -52 * want).all(), (what, got, want)


@pytest.mark.parametrize("iters", ITERS)
def test_general_skips_non_finite_bidders(bad_bidders, iters, dev):
    x, y, oracle = bad_bidders
    want_d, want_a = oracle[iters]
    d, a = _general(x, y, iters, dev)
    assert (a[:, list(BAD)] == -1).all(), a[:, list(BAD)]
    assert (d[:, list(BAD)] == 0).all(), d[:, list(BAD)]
    for i in range(2):   # the batch holds the pairs (x_i, y_i)
        assert np.array_equal(a[i, KEEP], want_a[i, i]), (i, np.argwhere(a[i, KEEP] != want_a[i, i])[:5])
        assert np.array_equal(d[i, KEEP], want_d[i, i]), i
    assert (a[:, KEEP] >= 0).all()


@pytest.mark.parametrize("iters", ITERS)
def test_set_level_skips_non_finite_bidders(bad_bidders, iters, dev):
    x, y, oracle = bad_bidders
    want_d, want_a = oracle[iters]
    sums, a = _set_level(x, y, iters, dev)
    assert a.shape == (2, 2, N) and (a[:, :, list(BAD)] == -1).all(), a[:, :, list(BAD)]
    assert np.array_equal(a[:, :, KEEP], want_a), np.argwhere(a[:, :, KEEP] != want_a)[:5]
    # the three rows add sqrt(0) = 0.0: the sum is the remaining rows' sum
    _assert_sums(sums, want_d, N, f"non-finite bidders, {iters} iterations")


@pytest.mark.parametrize("iters", ITERS)
def test_general_never_bids_for_a_non_finite_target(bad_target, iters, dev):
    x, y, oracle = bad_target
    want_d, want_a = oracle[iters]
    d, a = _general(x, y, iters, dev)
    assert (a != M - 1).all()
    for i in range(2):
        assert np.array_equal(a[i], want_a[i, i]), (i, np.argwhere(a[i] != want_a[i, i])[:5])
        assert np.array_equal(d[i], want_d[i, i]), i


@pytest.mark.parametrize("iters", ITERS)
def test_set_level_never_bids_for_a_non_finite_target(bad_target, iters, dev):
    x, y, oracle = bad_target
    want_d, want_a = oracle[iters]
    sums, a = _set_level(x, y, iters, dev)
    assert (a != M - 1).all()
    assert np.array_equal(a, want_a), np.argwhere(a != want_a)[:5]
    _assert_sums(sums, want_d, N, f"non-finite target, {iters} iterations")
