"""Neighbourhood queries on the GPU against the NumPy reference (tests/neighbors_ref.py).  Every search comparison is
idx exact, cnt exact and dist2 bit-equal (int32 views): the rule decides every tie, so nothing is tolerated.  Sizes sit
at the edges of lanes (64), waves, workgroups (256 queries) and the LDS tiles of sparenet_amd/csrc/neighbors.hip (1024
targets on the wide path, 256 per segment on the split path); SN_NEIGHBORS_SPLIT forces the split width so that every
path is reached at small sizes and compared with the others.  The gathers are bit-equal to the reference, the backward
is held to the bound of a recursive fp32 sum."""
import functools

import numpy as np
import pytest
import torch

from neighbors_ref import (ball_ref_batch, group_backward_ref, group_ref, interpolate_ref, knn_ref_batch,
                           lattice_points, same_bits, sum_bound)

pytestmark = pytest.mark.gpu

SPLITS = ("1", "3", "16", None)      # the wide path, two split widths (16 is held to the bucket's cap), the dispatch


def _cloud(seed, b, n):
    return np.random.default_rng(seed).random((b, n, 3)).astype(np.float32)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _set_split(monkeypatch, split):
    if split is None:
        monkeypatch.delenv("SN_NEIGHBORS_SPLIT", raising=False)
    else:
        monkeypatch.setenv("SN_NEIGHBORS_SPLIT", split)


def _knn(dev, x, q, k, lengths=None, new_lengths=None):
    from sparenet_amd.cuda.neighbors import knn_query

    d, idx = knn_query(k, _t(x, dev), _t(q, dev), lengths, new_lengths)
    assert idx.dtype == torch.int32 and d.dtype == torch.float32 and idx.shape == d.shape == q.shape[:2] + (k,)
    return idx.cpu().numpy(), d.cpu().numpy()


def _ball(dev, x, q, radius, nsample, pad="first", lengths=None, new_lengths=None):
    from sparenet_amd.cuda.neighbors import ball_query

    idx, cnt = ball_query(radius, nsample, _t(x, dev), _t(q, dev), lengths, new_lengths, pad=pad, return_count=True)
    assert idx.dtype == cnt.dtype == torch.int32 and idx.shape == q.shape[:2] + (nsample,) and cnt.shape == q.shape[:2]
    return idx.cpu().numpy(), cnt.cpu().numpy()


def _first_diff(got, want):
    bad = np.argwhere(got != want)
    return f"at {tuple(bad[0])}: {got[tuple(bad[0])]!r}, reference {want[tuple(bad[0])]!r} ({len(bad)} differ)"


def _assert_knn(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: idx {_first_diff(got[0], want[0])}"
    assert same_bits(got[1], want[1]), f"{what}: dist2 {_first_diff(got[1].view(np.int32), want[1].view(np.int32))}"


def _assert_ball(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: idx {_first_diff(got[0], want[0])}"
    assert np.array_equal(got[1], want[1]), f"{what}: cnt {_first_diff(got[1], want[1])}"


def _check_knn(dev, monkeypatch, x, q, k, lengths=None, new_lengths=None, what="", splits=SPLITS):
    want = knn_ref_batch(x, q, k, lengths, new_lengths)
    for split in splits:
        _set_split(monkeypatch, split)
        _assert_knn(_knn(dev, x, q, k, lengths, new_lengths), want, f"{what} k={k} split={split}")
    return want


def _check_ball(dev, monkeypatch, x, q, radius, nsample, lengths=None, new_lengths=None, what="", splits=SPLITS):
    for pad in ("first", "none"):
        want = ball_ref_batch(x, q, radius, nsample, pad == "first", lengths, new_lengths)
        for split in splits:
            _set_split(monkeypatch, split)
            _assert_ball(_ball(dev, x, q, radius, nsample, pad, lengths, new_lengths), want,
                         f"{what} r={radius} nsample={nsample} pad={pad} split={split}")
    return want


# ------------------------------------------------------------------ edges of lanes, waves, workgroups and tiles
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_lane_wave_workgroup_and_tile_edges(dev, monkeypatch, n):
    x = _cloud(n, 3, n)
    for m in (1, 63, 64, 65, 257):
        q = _cloud(1000 + n + m, 3, m)
        _check_knn(dev, monkeypatch, x, q, 3, what=f"n={n} m={m}")
        _check_ball(dev, monkeypatch, x, q, 0.15, 16, what=f"n={n} m={m}")


# every list bucket's last k and the first of the next; the small cloud has k > n
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8, 9, 16, 17, 32])
def test_k_buckets(dev, monkeypatch, k):
    for n in (20, 700):
        idx, d = _check_knn(dev, monkeypatch, _cloud(k, 2, n), _cloud(50 + k, 2, 130), k, what=f"n={n}")
        assert (idx[:, :, n:] == -1).all() and np.isinf(d[:, :, n:]).all() and (idx[:, :, :min(k, n)] >= 0).all()


@pytest.mark.parametrize("nsample", [1, 16, 33, 64])
def test_nsample_and_radii(dev, monkeypatch, nsample):
    x, q = _cloud(3, 2, 1500), _cloud(4, 2, 200)
    none = _check_ball(dev, monkeypatch, x, q, 1e-4, nsample, what="no hit")
    assert not none[1].any() and (none[0] == -1).all()
    few = _check_ball(dev, monkeypatch, x, q, 0.08, nsample, what="a few hits")      # about 3 hits a query
    assert 0 < few[1].mean() < 8 and (few[1] == 0).any()
    many = _check_ball(dev, monkeypatch, x, q, 0.6, nsample, what="many hits")       # hundreds of hits a query
    assert (many[1] == nsample).all()
    zero = _check_ball(dev, monkeypatch, x, x[:, :200], 0.0, nsample, what="radius 0")   # d = 0 < 0 never holds
    assert not zero[1].any()


# --------------------------------------------------------------------------------------------- the split paths
def test_hits_straddle_a_segment_boundary_and_segments_are_empty(dev, monkeypatch):
    x = np.full((1, 41, 3), 5.0, np.float32) + _cloud(1, 1, 41)
    near = [8, 9, 10, 11, 12, 30]              # split 4: segments of 11 -- the first four hits are 8, 9, 10 | 11
    x[0, near] = _cloud(2, 1, len(near))[0] * 0.01
    q = np.zeros((1, 70, 3), np.float32)
    q[0, 1:] = _cloud(3, 1, 69)[0] * 0.01
    for split in ("4", "3", "16", "1"):
        _set_split(monkeypatch, split)
        idx, cnt = _ball(dev, x, q, 0.5, 4, "first")
        assert idx[0].tolist() == [near[:4]] * 70 and (cnt == 4).all(), split
        idx, cnt = _ball(dev, x, q, 0.5, 8, "none")
        assert idx[0].tolist() == [near + [-1, -1]] * 70 and (cnt == 6).all(), split
    _check_ball(dev, monkeypatch, x, q, 0.5, 4, what="straddle", splits=("1", "3", "4", "16"))
    _check_knn(dev, monkeypatch, x, q, 8, what="straddle", splits=("1", "3", "4", "16"))
    # 5 points under split 4 are segments of 2, 2, 1 and none; 9 points under split 16 leave seven segments empty
    for n in (5, 9):
        _check_knn(dev, monkeypatch, x[:, :n], q, 4, what=f"{n} points", splits=("4", "16"))
        _check_ball(dev, monkeypatch, x[:, 6:6 + n], q, 0.5, 3, what=f"{n} points", splits=("4", "16"))


def test_every_path_gives_the_same_bits(dev, monkeypatch):
    x, q = _cloud(5, 3, 1501), _cloud(6, 3, 333)      # 1501 is no multiple of any split width
    knn, ball = {}, {}
    for split in ("1", "2", "3", "4", "7", "16"):
        _set_split(monkeypatch, split)
        knn[split] = [_knn(dev, x, q, k) for k in (3, 16, 32)]
        ball[split] = _ball(dev, x, q, 0.2, 32)
    want = [knn_ref_batch(x, q, k) for k in (3, 16, 32)]
    for split in knn:
        for got, ref, first in zip(knn[split], want, knn["1"]):
            _assert_knn(got, ref, f"split {split}")
            assert np.array_equal(got[0], first[0]) and same_bits(got[1], first[1])
        _assert_ball(ball[split], ball_ref_batch(x, q, 0.2, 32), f"split {split}")


# ---------------------------------------------------------------------------------------------------------- ties
def test_lattice_of_ties(dev, monkeypatch):
    pts = lattice_points()                       # 125 points, coordinates in multiples of 1/8
    x = pts[None]
    q = np.concatenate([pts, pts + np.float32(1 / 16)])[None]
    for k in (3, 16, 32):
        _check_knn(dev, monkeypatch, x, q, k, what="lattice")
    _check_ball(dev, monkeypatch, x, q, 0.25, 8, what="lattice")
    at = _check_ball(dev, monkeypatch, x, q, 0.25, 64, what="lattice")                       # d == r2 is no hit
    beyond = _check_ball(dev, monkeypatch, x, q, 0.2500001, 64, what="lattice, just beyond")
    assert (beyond[1][0, :125] > at[1][0, :125]).all() and at[1].max() < 64      # every point has neighbours AT 0.25


def test_duplicated_points_and_a_collapsed_cloud(dev, monkeypatch):
    half = _cloud(21, 2, 300)
    x = np.concatenate([half, half], axis=1)
    q = _cloud(22, 2, 100)
    idx, d = _check_knn(dev, monkeypatch, x, q, 16, what="doubled")
    assert np.array_equal(idx[:, :, 0::2] + 300, idx[:, :, 1::2]) and same_bits(d[:, :, 0::2], d[:, :, 1::2])
    _check_ball(dev, monkeypatch, x, q, 0.2, 16, what="doubled")
    same = np.full((2, 300, 3), 0.25, np.float32)
    idx, d = _check_knn(dev, monkeypatch, same, q, 32, what="collapsed")
    assert (idx == np.arange(32)).all()
    idx, cnt = _check_ball(dev, monkeypatch, same, same[:, :70], 0.01, 33, what="collapsed")
    assert (idx == np.arange(33)).all() and (cnt == 33).all()


# -------------------------------------------------------------------------------------------------------- ragged
RAGGED_LENGTHS = [0, 1, 256, 1024, 1500]
RAGGED_QUERIES = [300, 0, 1, 64, 257]


def test_ragged_batch(dev, monkeypatch):
    x, q = _cloud(31, 5, 1500), _cloud(32, 5, 300)
    for i, (n, m) in enumerate(zip(RAGGED_LENGTHS, RAGGED_QUERIES)):
        x[i, n:] = 1e30                             # padding rows: never read into a result
        q[i, m:] = -1e30
    knn = _check_knn(dev, monkeypatch, x, q, 5, RAGGED_LENGTHS, RAGGED_QUERIES, what="ragged")
    ball = _check_ball(dev, monkeypatch, x, q, 0.15, 16, RAGGED_LENGTHS, RAGGED_QUERIES, what="ragged")
    assert (knn[0][0] == -1).all() and np.isinf(knn[1][0]).all() and (knn[0][1] == -1).all()      # no points; no queries
    assert (ball[0][:2] == -1).all() and not ball[1][:2].any()
    assert (knn[0][2, 1:] == -1).all() and (ball[0][2, 1:] == -1).all() and not ball[1][2, 1:].any()
    monkeypatch.delenv("SN_NEIGHBORS_SPLIT", raising=False)
    lengths = torch.tensor(RAGGED_LENGTHS, device=dev)
    new_lengths = torch.tensor(RAGGED_QUERIES, device=dev, dtype=torch.int32)
    _assert_knn(_knn(dev, x, q, 5, lengths, new_lengths), knn, "device lengths")
    _assert_ball(_ball(dev, x, q, 0.15, 16, "none", lengths, new_lengths), ball, "device lengths")
    for i, (n, m) in enumerate(zip(RAGGED_LENGTHS, RAGGED_QUERIES)):
        if n and m:                                 # each row equals the one-cloud call
            alone = _knn(dev, x[i:i + 1, :n], q[i:i + 1, :m], 5)
            assert np.array_equal(alone[0][0], knn[0][i, :m]) and same_bits(alone[1][0], knn[1][i, :m]), f"cloud {i}"
            alone = _ball(dev, x[i:i + 1, :n], q[i:i + 1, :m], 0.15, 16, "none")
            assert np.array_equal(alone[0][0], ball[0][i, :m]) and np.array_equal(alone[1][0], ball[1][i, :m])
    # device values outside their range are held to it, not trusted
    wild = _knn(dev, x[4:5], q[4:5], 5, torch.tensor([5000], device=dev), torch.tensor([-3], device=dev))
    assert (wild[0] == -1).all()
    wild = _knn(dev, x[4:5], q[4:5, :257], 5, torch.tensor([5000], device=dev), torch.tensor([9999], device=dev))
    assert np.array_equal(wild[0][0], knn[0][4, :257])


# --------------------------------------------------------------------------------------------------------- scale
def test_subnormal_and_overflowing_distances(dev, monkeypatch):
    x, q = _cloud(41, 2, 1100), _cloud(42, 2, 130)
    tiny = knn_ref_batch(x * np.float32(1e-20), q * np.float32(1e-20), 8)
    assert 0 < tiny[1].max() < np.float32(1.17e-38)              # every distance is subnormal: flushing gives zeros
    _check_knn(dev, monkeypatch, x * np.float32(1e-20), q * np.float32(1e-20), 8, what="1e-20")
    hits = _check_ball(dev, monkeypatch, x * np.float32(1e-20), q * np.float32(1e-20), 1.5e-21, 16, what="1e-20")
    assert 0 < hits[1].mean() < 16
    big_x, big_q = (x * 2 - 1) * np.float32(1e19), (q * 2 - 1) * np.float32(1e19)      # negative coordinates too
    far = _check_knn(dev, monkeypatch, big_x, big_q, 32, what="1e19")
    assert np.isfinite(far[1][:, :, 0]).all()
    idx, d = _check_knn(dev, monkeypatch, big_x[:, :40], big_q, 32, what="1e19, 40 points")
    assert np.isinf(d[:, :, :32]).any() and (idx[:, :, :32] >= 0).all()      # +inf is a value: the slot holds a point
    _check_ball(dev, monkeypatch, big_x, big_q, 3e18, 16, what="1e19")
    _check_knn(dev, monkeypatch, x * 40 - 70, q * 40 - 70, 8, what="[-70, -30]")
    _check_ball(dev, monkeypatch, x * 40 - 70, q * 40 - 70, 4.0, 16, what="[-70, -30]")


# ----------------------------------------------------------------------------------------------------- full size
@functools.lru_cache(maxsize=None)
def _full_size():
    x, q = _cloud(51, 2, 16384), _cloud(52, 2, 2048)
    return x, q, knn_ref_batch(x, q, 16), ball_ref_batch(x, q, 0.08, 32)


def test_full_size(dev, monkeypatch):
    x, q, knn, ball = _full_size()
    monkeypatch.delenv("SN_NEIGHBORS_SPLIT", raising=False)
    _assert_knn(_knn(dev, x, q, 16), knn, "16384 x 2048")
    _assert_ball(_ball(dev, x, q, 0.08, 32), ball, "16384 x 2048")
    assert (ball[1] == 32).any() and (ball[1] < 32).any()


def test_two_calls_and_batch_rows_give_the_same_bits(dev, monkeypatch):
    x, q, knn, ball = _full_size()
    for split in ("1", "4"):
        _set_split(monkeypatch, split)
        for _ in range(2):
            _assert_knn(_knn(dev, x[:, :4000], q[:, :512], 16), _knn(dev, x[:, :4000], q[:, :512], 16), "twice")
            _assert_ball(_ball(dev, x[:, :4000], q[:, :512], 0.08, 32), _ball(dev, x[:, :4000], q[:, :512], 0.08, 32),
                         "twice")
    monkeypatch.delenv("SN_NEIGHBORS_SPLIT", raising=False)
    alone = _knn(dev, x[1:], q[1:], 16)             # another batch size may take another path: the same bits
    assert np.array_equal(alone[0][0], knn[0][1]) and same_bits(alone[1][0], knn[1][1])
    alone = _ball(dev, x[1:], q[1:, :512], 0.08, 32)
    assert np.array_equal(alone[0][0], ball[0][1, :512]) and np.array_equal(alone[1][0], ball[1][1, :512])


def test_three_nn_is_the_root_of_knn_query(dev):
    from sparenet_amd.cuda.neighbors import knn_query, three_nn

    known, unknown = _t(_cloud(61, 2, 500), dev), _t(_cloud(62, 2, 90), dev)
    dist, idx = three_nn(unknown, known)
    d2, want = knn_query(3, known, unknown)
    assert dist.shape == (2, 90, 3) and torch.equal(idx, want) and torch.equal(dist, torch.sqrt(d2))
    assert not dist.requires_grad and not idx.requires_grad


# ------------------------------------------------------------------------------------------- gathers, forward
def _search_idx(dev, s):
    """idx [2, 70, s] from the searches: a k-NN with slots beyond a short cloud (-1) and a ball query padded with -1."""
    x, q = _cloud(71, 2, 200), _cloud(72, 2, 70)
    knn = _knn(dev, x, q, s, [200, s // 2])[0]
    ball = _ball(dev, x, q, 0.2, s, "none")[0]
    return [knn, ball]


@pytest.mark.parametrize("s", [1, 3, 32])
def test_grouping_and_interpolation_forward(dev, s):
    from sparenet_amd.cuda.neighbors import grouping_operation, three_interpolate

    rng = np.random.default_rng(s)
    hand = rng.integers(-1, 200, (2, 70, s)).astype(np.int32)
    hand[0, 0] = -1                                  # a row without a slot
    hand[1, 1] = 199
    cases = _search_idx(dev, s) + [hand]
    assert any((i == -1).any() for i in cases[:2])
    for c in (1, 3, 64, 65):
        feats = rng.standard_normal((2, c, 200)).astype(np.float32)
        w = (rng.standard_normal((2, 70, s)) * 10.0 ** rng.uniform(-3, 3, (2, 70, s))).astype(np.float32)
        for idx in cases:
            got = grouping_operation(_t(feats, dev), _t(idx, dev))
            assert got.shape == (2, c, 70, s) and same_bits(got.cpu().numpy(), group_ref(feats, idx)), (c, s)
            got = three_interpolate(_t(feats, dev), _t(idx, dev).long(), _t(w, dev))      # int64 is converted
            assert got.shape == (2, c, 70) and same_bits(got.cpu().numpy(), interpolate_ref(feats, idx, w)), (c, s)


# ------------------------------------------------------------------------------------------ gathers, backward
def _upstream(rng, shape):
    """Mixed sign, magnitudes across 1e-3 .. 1e3 (the `wide` regime of tests/test_backward_regimes.py)."""
    return (np.where(rng.random(shape) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-3, 3, shape)).astype(np.float32)


def _backward_idx(dev, case):
    x, q = _cloud(81, 2, 512), _cloud(82, 2, 256)
    if case == "ball, pad first":                    # heavy repeats: every row's tail is its first hit
        return _ball(dev, x, q, 0.2, 32, "first")[0]
    if case == "ball, pad none":                     # -1 slots
        return _ball(dev, x, q, 0.2, 32, "none")[0]
    return np.zeros((2, 256, 32), np.int32)          # all m * s = 8192 slots of a cloud on target 0


def _check_backward(dev, idx, c, n, rng, what):
    """grouping_operation and three_interpolate backward against float64; returns the list lengths [b, n]."""
    from sparenet_amd.cuda.neighbors import grouping_operation, three_interpolate

    feats = rng.standard_normal((idx.shape[0], c, n)).astype(np.float32)
    w = _upstream(rng, idx.shape)
    for weight in (None, w):
        f = _t(feats, dev).requires_grad_(True)
        wt = None if weight is None else _t(weight, dev).requires_grad_(True)
        out = grouping_operation(f, _t(idx, dev)) if weight is None else three_interpolate(f, _t(idx, dev), wt)
        g = _upstream(rng, tuple(out.shape))
        out.backward(_t(g, dev))
        assert wt is None or wt.grad is None
        got = f.grad.cpu().numpy().astype(np.float64)
        want, mag, length = group_backward_ref(g, idx, n, weight)
        bound = sum_bound(length)[:, None, :] * mag
        err = np.abs(got - want)
        worst = np.unravel_index(np.argmax(err - bound), err.shape)
        print(f"{what}, weight {weight is not None}: longest list {length.max()}, largest error / bound "
              f"{(err[bound > 0] / bound[bound > 0]).max():.3f}")
        assert (err <= bound).all(), f"{what}: at {worst} error {err[worst]:.3e}, bound {bound[worst]:.3e}"
        empty = np.broadcast_to((length == 0)[:, None, :], got.shape)
        assert not got[empty].any()                      # targets without a slot are exactly 0
        yield got, length


@pytest.mark.parametrize("case", ["ball, pad first", "ball, pad none", "one target"])
def test_backward_against_float64(dev, monkeypatch, case):
    monkeypatch.delenv("SN_NEIGHBORS_SPLIT", raising=False)
    idx = _backward_idx(dev, case)
    if case == "ball, pad first":
        assert (idx[:, :, -1] == idx[:, :, 0]).mean() > 0.5
    elif case == "ball, pad none":
        assert (idx == -1).mean() > 0.2
    for got, length in _check_backward(dev, idx, 5, 512, np.random.default_rng(len(case)), case):
        if case == "one target":
            assert length[0, 0] == 8192 and not got[:, :, 1:].any()


@pytest.mark.parametrize("n", [1024, 1025, 2049])
def test_backward_lists_past_one_scan_chunk(dev, n):
    """The inverted lists' scan hands a carry from one chunk of 1024 targets to the next: n at and just past one and two
    chunks, a long list in the last chunk behind mostly empty ones."""
    b, m, s = 2, 64, 8
    rng = np.random.default_rng(n)
    idx = rng.integers(0, n, (b, m, s)).astype(np.int32)
    idx[rng.random(idx.shape) < 0.2] = -1
    idx[:, :, 3] = n - 1
    for got, length in _check_backward(dev, idx, 3, n, rng, f"n = {n}"):
        assert (length[:, n - 1] >= m).all() and (length == 0).mean() > 0.5


def test_interpolate_features_against_its_float64_composite(dev):
    from sparenet_amd.cuda.neighbors import interpolate_features, knn_query

    known, unknown = _t(_cloud(91, 2, 400), dev), _t(_cloud(92, 2, 150), dev)
    feats = torch.rand(2, 6, 400, device=dev) + 0.5      # positive: the bound below is a relative error
    for k in (3, 5):
        got = interpolate_features(unknown, known, feats, k=k)
        dist2, idx = knn_query(k, known, unknown)
        w = 1.0 / (torch.sqrt(dist2.double()) + 1e-8)
        w = w / w.sum(dim=2, keepdim=True)
        picked = torch.gather(feats.double()[:, :, None, :].expand(-1, -1, 150, -1), 3,
                              idx.long()[:, None].expand(-1, 6, -1, -1))
        want = (picked * w[:, None]).sum(dim=3)
        assert got.shape == (2, 6, 150) and got.dtype == torch.float32
        assert ((got.double() - want).abs() <= 1e-5 * want.abs()).all()
    f = feats.clone().requires_grad_(True)
    u = unknown.clone().requires_grad_(True)
    interpolate_features(u, known, f).sum().backward()
    assert u.grad is None and f.grad is not None and torch.isfinite(f.grad).all()
