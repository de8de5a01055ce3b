"""Farthest point sampling on the GPU against the NumPy reference (tests/fps_ref.py): every comparison is idx exact AND
min_dist bit-equal (int32 views) -- a contracted product would keep most index sequences and change min_dist bits.
Sizes sit at the edges of lanes (64), waves, workgroups (64 / 256 / 1024 threads) and of every register bucket of
sparenet_amd/csrc/fps.hip, on both sides; the workspace path is reached at small n through SN_FPS_RESIDENT_MAX."""
import functools

import numpy as np
import pytest
import torch

from fps_ref import fps_ref, fps_ref_batch, lattice_cloud, overflow_cloud, same_bits

pytestmark = pytest.mark.gpu


def _cloud(seed, b, n):
    return np.random.default_rng(seed).random((b, n, 3)).astype(np.float32)


def _run(dev, x, m, lengths=None, start=0):
    from sparenet_amd.cuda.fps import farthest_point_sample

    idx, md = farthest_point_sample(torch.from_numpy(np.ascontiguousarray(x)).to(dev), m, lengths, start,
                                    return_min_dist=True)
    assert idx.dtype == torch.int32 and md.dtype == torch.float32 and idx.shape == md.shape == (x.shape[0], m)
    return idx.cpu().numpy(), md.cpu().numpy()


def _check(dev, x, m, lengths=None, start=None, what=""):
    idx, md = _run(dev, x, m, lengths, 0 if start is None else start)
    ri, rm = fps_ref_batch(x, m, lengths, start)
    for i in range(x.shape[0]):
        bad = np.flatnonzero(idx[i] != ri[i])
        assert not bad.size, f"{what} cloud {i}: pick {bad[0]} is {idx[i][bad[0]]}, reference {ri[i][bad[0]]}"
        bad = np.flatnonzero(md[i].view(np.int32) != rm[i].view(np.int32))
        assert not bad.size, f"{what} cloud {i}: min_dist[{bad[0]}] is {md[i][bad[0]]!r}, reference {rm[i][bad[0]]!r}"
    return idx, md


# ------------------------------------------------------------------------- edges of lanes, waves and workgroups
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_lane_wave_and_workgroup_edges(dev, n):
    x = _cloud(n, 3, n)
    for m in sorted({1, n // 2 or 1, n}):
        _check(dev, x, m, what=f"n={n} m={m}")


# the last size of every register bucket of sn_fps's dispatch and the first of the next; 24577 is the workspace path
@pytest.mark.parametrize("n", [64, 65, 256, 257, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385, 24576,
                               24577])
def test_register_bucket_edges(dev, n):
    x = _cloud(100 + n, 2, n)
    x[1, -1] = 3.0      # the last point of a full bucket is the farthest: pick 1 of cloud 1
    idx, _ = _check(dev, x, 64, start=[0, 1], what=f"n={n}")
    assert idx[1, 1] == n - 1


def test_workspace_path_gives_the_resident_bits(dev, monkeypatch):
    x = _cloud(7, 3, 1500)
    lengths, start = [1500, 1025, 1], [5, 1024, 0]
    monkeypatch.delenv("SN_FPS_RESIDENT_MAX", raising=False)
    resident = _check(dev, x, 200, lengths, start, what="resident")
    monkeypatch.setenv("SN_FPS_RESIDENT_MAX", "1000")
    from sparenet_amd import _lib
    assert _lib.op_call("fps", "sn_fps_workspace_bytes", 3, 1500) >= 4 * 3 * 1500
    workspace = _check(dev, x, 200, lengths, start, what="workspace")
    assert np.array_equal(resident[0], workspace[0]) and same_bits(resident[1], workspace[1])


# ------------------------------------------------------------------------------------ ties and degenerate clouds
def test_lattice_of_ties(dev):
    x = lattice_cloud()[None]
    idx, md = _check(dev, x, 600, what="lattice")       # 512 distinct points: a permutation, then index 0 repeats
    assert sorted(idx[0, :512].tolist()) == list(range(512)) and not idx[0, 512:].any() and not md[0, 512:].any()


def test_all_equal_cloud(dev):
    x = np.full((2, 300, 3), 0.25, np.float32)
    idx, md = _check(dev, x, 40, start=[7, 299], what="all equal")
    assert idx[0].tolist() == [7] + [0] * 39 and idx[1].tolist() == [299] + [0] * 39
    assert np.isinf(md[:, 0]).all() and not md[:, 1:].any()


def test_every_point_stored_twice(dev):
    half = _cloud(21, 1, 300)
    x = np.concatenate([half, half], axis=1)
    idx, md = _check(dev, x, 600, what="doubled")
    # the first copy wins every tie; once the 300 distinct points are taken every distance is 0
    assert sorted(idx[0, :300].tolist()) == list(range(300)) and not idx[0, 300:].any() and not md[0, 300:].any()
    inter = np.stack([half[0], half[0]], axis=1).reshape(1, 600, 3)      # the copies next to each other
    idx, _ = _check(dev, inter, 600, what="interleaved")
    assert not (idx[0, :300] % 2).any()


# -------------------------------------------------------------------------------------------------------- ragged
RAGGED_LENGTHS = [0, 1, 64, 1025, 1500]
RAGGED_START = [0, 0, 63, 1024, 7]


def _ragged_batch():
    x = _cloud(31, 5, 1500)
    for i, n in enumerate(RAGGED_LENGTHS):
        x[i, n:] = 1e30                             # padding rows: never read into a result
    return x


def test_ragged_batch(dev):
    x = _ragged_batch()
    idx, md = _check(dev, x, 64, RAGGED_LENGTHS, what="ragged")
    assert (idx[0] == -1).all() and same_bits(md[0], np.full(64, np.nan, np.float32))
    assert idx[1].tolist() == [0] * 64
    for i, n in enumerate(RAGGED_LENGTHS):
        assert idx[i].max() < max(n, 1)
        if n:
            alone = _run(dev, x[i:i + 1, :n], 64)
            assert np.array_equal(alone[0][0], idx[i]) and same_bits(alone[1][0], md[i]), f"cloud {i}"


def test_ragged_batch_with_starts_and_device_lengths(dev):
    x = _ragged_batch()
    idx, md = _check(dev, x, 64, RAGGED_LENGTHS, RAGGED_START, what="ragged + start")
    assert idx[:, 0].tolist() == [-1] + RAGGED_START[1:]
    lengths = torch.tensor(RAGGED_LENGTHS, device=dev)
    start = torch.tensor(RAGGED_START, device=dev, dtype=torch.int32)
    again = _run(dev, x, 64, lengths, start)
    assert np.array_equal(again[0], idx) and same_bits(again[1], md)
    # device values outside their range are held to it, not trusted: length 5000 -> 1500, start 99999 -> the last point
    wild = _run(dev, x[4:5], 8, torch.tensor([5000], device=dev), torch.tensor([99999], device=dev))
    want = fps_ref(x[4], 8, start=1499)
    assert np.array_equal(wild[0][0], want[0]) and same_bits(wild[1][0], want[1])


# --------------------------------------------------------------------------------------------------------- range
def test_offset_4096_cancellation(dev):
    x = _cloud(41, 1, 1500) + np.float32(4096)
    idx, md = _check(dev, x, 300, what="+4096")
    assert len(set(idx[0].tolist())) == 300


def test_subnormal_squares(dev):
    """Coordinates scaled by 1e-20: every squared distance is below 3e-40, subnormal in fp32 (normal from 1.18e-38).
    The reference makes 300 distinct picks at this scale (checked here, on the CPU side); a kernel that flushes
    subnormals sees only zeros."""
    x = _cloud(7, 1, 1500) * np.float32(1e-20)
    ri, rm = fps_ref(x[0], 300)
    assert len(set(ri.tolist())) > 16 and 0 < rm[1:].max() < np.float32(1.17e-38)
    _check(dev, x, 300, what="1e-20")


def test_overflowing_squares(dev):
    idx, md = _check(dev, overflow_cloud()[None], 70, what="all inf")
    assert idx[0].tolist() == list(range(64)) + [0] * 6 and np.isinf(md[0, :64]).all()
    # a unit cube scaled by 1e20: +inf between distant points, finite values (above 1e36) between near ones
    x = (_cloud(43, 1, 1500) - np.float32(0.5)) * np.float32(1e20)
    idx, md = _check(dev, x, 300, what="1e20")
    assert np.isinf(md[0, 1]) and np.isfinite(md[0, -1])


# ----------------------------------------------------------------------------------------------------- full size
@functools.lru_cache(maxsize=None)
def _full_size(b, n):
    x = _cloud(50 + b, b, n)
    return x, fps_ref_batch(x, 2048)


@pytest.mark.parametrize("b,n", [(2, 16384), (1, 19384)])
def test_full_size(dev, b, n):
    x, (ri, rm) = _full_size(b, n)
    idx, md = _run(dev, x, 2048)
    assert np.array_equal(idx, ri) and same_bits(md, rm)


# ------------------------------------------------------------------------------------------------------ identity
def test_two_calls_and_batch_rows_give_the_same_bits(dev):
    x, (ri, rm) = _full_size(2, 16384)
    first, second = _run(dev, x, 512), _run(dev, x, 512)
    assert np.array_equal(first[0], second[0]) and same_bits(first[1], second[1])
    assert np.array_equal(first[0], ri[:, :512]) and same_bits(first[1], rm[:, :512])      # a prefix of the longer run
    for i in range(2):
        alone = _run(dev, x[i:i + 1], 512)
        assert np.array_equal(alone[0][0], first[0][i]) and same_bits(alone[1][0], first[1][i])
    from sparenet_amd.cuda.fps import farthest_point_sample
    only = farthest_point_sample(torch.from_numpy(x).to(dev), 512)
    assert isinstance(only, torch.Tensor) and np.array_equal(only.cpu().numpy(), first[0])


# -------------------------------------------------------------------------------------------------------- gather
def test_sample_points_and_its_gradient(dev):
    from sparenet_amd.cuda.fps import farthest_point_sample, sample_points

    x = torch.from_numpy(_cloud(61, 3, 200)).to(dev)
    lengths, m = [200, 50, 200], 80           # cloud 1 has 50 points: picks 50.. repeat index 0, gradients accumulate
    idx = farthest_point_sample(x, m, lengths).long()
    assert (idx[1, 50:] == 0).all()
    a = x.clone().requires_grad_(True)
    out = sample_points(a, m, lengths)
    b = x.clone().requires_grad_(True)
    want = torch.gather(b, 1, idx[:, :, None].expand(-1, -1, 3))
    assert out.shape == (3, m, 3) and torch.equal(out, want)
    # small integers: every sum of them is exact, whatever order the duplicates are added in
    g = torch.randint(-8, 9, (3, m, 3), generator=torch.Generator().manual_seed(5)).float().to(dev)
    out.backward(g)
    want.backward(g)
    assert torch.equal(a.grad, b.grad)
    picked = torch.zeros(3, 200, dtype=torch.bool, device=dev).scatter_(1, idx, True)
    assert not a.grad[~picked].any()
    assert torch.equal(a.grad[1, 0], g[1][idx[1] == 0].sum(dim=0))      # every copy of a repeated pick adds up
