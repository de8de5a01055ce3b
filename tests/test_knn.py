"""EdgeConv k-NN graph and edge features (models/sparenet_generator.py:852-906).

Golden vectors come from the reference's own functions run on the CPU (tests/golden/gen_knn.py).  The
neighbour ORDER of a row is only defined up to fp32 rounding of nearly equal distances (the reference's
two branches -- KNN_CUDA and the matmul fallback -- disagree there themselves), so indices are compared
as sets after checking that the k-th and (k+1)-th distances are separated."""
import glob
import os

import numpy as np
import pytest
import torch

import grnet_ref as R
import oracle


def _tau(x):
    """The one tolerance of this file, per cloud [B]: the fp32 rounding of the ranking expression |x_j|^2 - 2 x_i.x_j,
    2e-5 * 3 * max |x|^2."""
    return R.knn_tau(x)


def _rows_valid(idx, x, k, tau):
    """EVERY row, none skipped (grnet_ref.rows_valid): no duplicates, the point itself first, every returned j has
    d_j <= d_k + tau, every j with d_j < d_k - tau is returned, consecutive neighbours ascend within tau -- against exact
    float64 distances.  Returns {failure: rows}; empty = valid."""
    return R.rows_valid(idx, x, k, tau)


def _rows_match(idx_a, idx_b, x, k):
    """Same neighbour set in every row whose k-th / (k+1)-th distances are separated by more than the
    fp32 rounding of the ranking expression |x_j|^2 - 2 x_i.x_j (terms of size |x|^2, they cancel)."""
    x64 = x.astype(np.float64)
    bad = 0
    tau = _tau(x)
    for b in range(x.shape[0]):
        xx = (x64[b] ** 2).sum(0)
        d = xx[:, None] + xx[None, :] - 2.0 * x64[b].T @ x64[b]
        srt = np.sort(d, axis=1)
        clear = (srt[:, k] - srt[:, k - 1]) > tau[b]
        for i in np.nonzero(clear)[0]:
            bad += set(idx_a[b, i]) != set(idx_b[b, i])
    return bad


def test_oracle_matches_reference_golden(golden_dir):
    files = sorted(glob.glob(os.path.join(golden_dir, "knn_*.npz")))
    assert files
    for f in files:
        z = np.load(f)
        k = int(z["k"])
        idx = oracle.knn(z["x"], k)
        assert _rows_match(idx, z["idx"], z["x"], k) == 0, f
        assert (idx[:, :, 0] == np.arange(idx.shape[1])[None]).all()       # the point itself first
        np.testing.assert_array_equal(oracle.graph_feature(z["x"], z["idx"]), z["feature"])


@pytest.mark.gpu
def test_hip_knn_and_graph_feature(golden_dir, dev):
    from sparenet_amd.cuda.knn import get_graph_feature, knn

    for f in sorted(glob.glob(os.path.join(golden_dir, "knn_*.npz"))):
        z = np.load(f)
        k = int(z["k"])
        x = torch.from_numpy(z["x"]).to(dev)
        idx = knn(x, k)
        assert idx.dtype == torch.int64 and tuple(idx.shape) == z["idx"].shape
        assert _rows_match(idx.cpu().numpy(), z["idx"], z["x"], k) == 0, f
        feat = get_graph_feature(x, k=k, idx=torch.from_numpy(z["idx"]).to(dev))
        np.testing.assert_array_equal(feat.cpu().numpy(), z["feature"])


@pytest.mark.gpu
def test_hip_knn_sparenet_sizes_and_autograd(dev):
    """The generator's EdgeConv sizes (3000 points, C = 3 and 256, k = 8) against the oracle, and the
    gradient of the edge features against torch's own gather formulation."""
    from sparenet_amd.cuda.knn import get_graph_feature, knn, knn_fused, knn_unfused

    g = torch.Generator().manual_seed(5)
    for c in (3, 256):
        x = torch.rand(2, c, 3000, generator=g)
        ref = oracle.knn(x.numpy(), 8)
        for fn in (knn_fused, knn_unfused):   # the fused MFMA kernel and the GEMM + ranking pair
            idx = fn(x.to(dev), 8)
            assert _rows_match(idx.cpu().numpy(), ref, x.numpy(), 8) == 0, fn.__name__
            assert (idx[:, :, 0].cpu() == torch.arange(3000)[None]).all()
    x = torch.rand(2, 5, 300, generator=g).to(dev).requires_grad_(True)
    w = torch.rand(2, 10, 300, 4, generator=g).to(dev)
    idx = knn(x.detach(), 4)
    (get_graph_feature(x, k=4, idx=idx) * w).sum().backward()
    x2 = x.detach().clone().requires_grad_(True)
    nb = torch.gather(x2.unsqueeze(2).expand(-1, -1, 300, -1), 3, idx.unsqueeze(1).expand(-1, 5, -1, -1))
    ref = torch.cat([nb - x2.unsqueeze(3), x2.unsqueeze(3).expand(-1, -1, -1, 4)], dim=1)
    (ref * w).sum().backward()
    np.testing.assert_allclose(x.grad.cpu().numpy(), x2.grad.cpu().numpy(), rtol=1e-5, atol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("b,c,n,k", [(1, 3, 130, 4), (2, 17, 257, 8), (3, 64, 1000, 20), (2, 5, 64, 16),
                                     (1, 512, 515, 8), (2, 33, 129, 1), (1, 7, 24, 20)])
def test_hip_fused_knn_shapes(b, c, n, k, dev):
    """Ragged sizes of the fused kernel: n not a multiple of the 128-point tile or of 4 (scalar loads),
    channel counts that do not fill a 16-channel stage, k at both list sizes, k close to n."""
    from sparenet_amd.cuda.knn import knn_fused

    g = torch.Generator().manual_seed(b * 1000 + c * 10 + k)
    x = torch.randn(b, c, n, generator=g)
    idx = knn_fused(x.to(dev), k).cpu().numpy()
    assert idx.shape == (b, n, k) and idx.min() >= 0 and idx.max() < n
    assert (idx[:, :, 0] == np.arange(n)[None]).all()
    for row in idx.reshape(-1, k):
        assert len(set(row.tolist())) == k
    assert _rows_match(idx, oracle.knn(x.numpy(), k), x.numpy(), k) == 0


@pytest.mark.gpu
def test_hip_fused_knn_ties(dev):
    """Duplicate points: equal scores resolve to the lower index, the point itself stays first."""
    from sparenet_amd.cuda.knn import knn_fused as knn

    base = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [5.0, 5.0, 5.0]]).t()   # [3, 4]
    x = base.repeat(1, 40).unsqueeze(0).contiguous()                       # [1, 3, 160]: every point 40 times
    idx = knn(x.to(dev), 8).cpu().numpy()[0]
    for i in range(160):
        same = [j for j in range(160) if j % 4 == i % 4 and j != i]
        assert idx[i, 0] == i and list(idx[i, 1:]) == same[:7], (i, idx[i])


# ------------------------------------------------------------------ every row, order and tie rule
SHAPES = [(1, 3, 130, 4), (2, 17, 257, 8), (3, 64, 1000, 20), (2, 5, 64, 16), (1, 512, 515, 8), (2, 33, 129, 1),
          (1, 7, 24, 20)]                      # test_hip_fused_knn_shapes' list
# Shifting a cloud by +s on every channel makes |x|^2 - 2 x.y cancel terms of size c s^2.  At +50 the tolerance band
# [d_k - tau, d_k + tau] holds a non-returned point in 46 % - 100 % of the rows of every shape but (2, 33, 129, 1), so the
# check would accept almost anything; the shift is shrunk per shape (50, 10, 5, 2, 1) to the largest for which the float64
# reference alone keeps that share at or below 5 %.
SHIFTS = {(1, 3, 130, 4): 2, (2, 17, 257, 8): 2, (3, 64, 1000, 20): 1, (2, 5, 64, 16): 5, (1, 512, 515, 8): 1,
          (2, 33, 129, 1): 50, (1, 7, 24, 20): 5}
CLUSTERS = [(2, 3, 8), (2, 3, 20)]             # b, c, k: two clusters of k points each, n = 2 k
MAX_BAND_SHARE = 0.05


def _random_case(kind, shape):
    """x fp32 [b, c, n] and k of one random case (the seeds of test_hip_fused_knn_shapes)."""
    if kind == "clusters":
        b, c, k = shape
        r = np.random.default_rng(40 + k)
        x = (r.random((b, c, 2 * k)) * 1e-3).astype(np.float32)        # two clusters 1e-3 wide ...
        x[:, 0, 1::2] += np.float32(10)                                # ... 10 apart (odd points)
        return x, k
    b, c, n, k = shape
    g = torch.Generator().manual_seed(b * 1000 + c * 10 + k)
    x = torch.randn(b, c, n, generator=g).numpy()
    return ((x + np.float32(SHIFTS[shape])).astype(np.float32) if kind == "shifted" else x), k


RANDOM_CASES = ([("plain", s) for s in SHAPES] + [("shifted", s) for s in SHAPES] + [("clusters", s) for s in CLUSTERS])


@pytest.mark.parametrize("kind,shape", RANDOM_CASES)
def test_tolerance_band_stays_narrow(kind, shape):
    """The tolerance must not make the per-row check soft: the share of rows in which a point the exact search does not
    return lies inside [d_k - tau, d_k + tau] is at most 5 % for every random case, from the float64 reference alone.
    Shares: plain 0.8 %, 0.6 %, 1.6 %, 0, 1.0 %, 0, 0; shifted (by SHIFTS) 2.3 %, 1.6 %, 3.1 %, 1.6 %, 2.5 %, 0, 0;
    clusters 0, 0 (k is the cluster size: the next candidate is 10 away)."""
    x, k = _random_case(kind, shape)
    share = R.band_share(x, k, _tau(x))
    print(f"{kind} {shape}: band share {share:.4f}")
    assert share <= MAX_BAND_SHARE


def _integer_cloud(b, c, n):
    """Coordinates in {0, 1, 2, 3}: every product and sum of the ranking expression is exact in fp32 -- on the matrix cores
    and in the GEMM alike -- and most distances tie."""
    return np.random.default_rng(b * 100 + c * 10 + n).integers(0, 4, (b, c, n)).astype(np.float32)


EXACT_FUSED = [(1, 3, 129, 8), (2, 16, 257, 8), (1, 17, 515, 20), (2, 1, 64, 4), (1, 5, 24, 20)]
EXACT_UNFUSED = [(2, 3, 130, k) for k in (1, 2, 4, 8, 16, 20, 32)] + [(2, 3, 32, 32)]


def test_oracle_knn_order_and_ties():
    """oracle.knn against the exact search on the integer clouds: the point itself first (also among its duplicates), then
    ascending distance, equal distances by lower index."""
    for b, c, n, k in EXACT_FUSED + EXACT_UNFUSED:
        x = _integer_cloud(b, c, n)
        d, ref = R.knn_exact(x, k)
        srt = np.sort(d, 2)
        assert (srt[:, :, 1:] == srt[:, :, :-1]).any() and (c > 3 or (srt[:, :, 1] == 0).any())   # ties; duplicates
        assert np.array_equal(oracle.knn(x, k), ref), (b, c, n, k)
        assert _rows_valid(ref, x, k, 0.0) == {}


@pytest.mark.gpu
@pytest.mark.parametrize("b,c,n,k", EXACT_FUSED)
def test_hip_fused_knn_exact_order(b, c, n, k, dev):
    """tau = 0: order and tie rule of the one-kernel search, bit for bit."""
    from sparenet_amd.cuda.knn import knn_fused

    x = _integer_cloud(b, c, n)
    idx = knn_fused(torch.from_numpy(x).to(dev), k).cpu().numpy()
    assert _rows_valid(idx, x, k, 0.0) == {}
    assert np.array_equal(idx, R.knn_exact(x, k)[1])


@pytest.mark.gpu
@pytest.mark.parametrize("b,c,n,k", EXACT_UNFUSED)
def test_hip_unfused_knn_exact_order(b, c, n, k, dev):
    """tau = 0: every template instance of knn_topk_kernel at a ragged size (130 = 2 x 64 + 2 lanes' worth), and k = n."""
    from sparenet_amd.cuda.knn import knn_unfused

    x = _integer_cloud(b, c, n)
    idx = knn_unfused(torch.from_numpy(x).to(dev), k).cpu().numpy()
    assert _rows_valid(idx, x, k, 0.0) == {}
    assert np.array_equal(idx, R.knn_exact(x, k)[1])


@pytest.mark.gpu
@pytest.mark.parametrize("kind,shape", RANDOM_CASES)
def test_hip_knn_every_row(kind, shape, dev):
    """Both paths on random clouds, clouds shifted off the origin (cancellation in |x|^2 - 2 x.y) and two tight clusters far
    apart: every row valid within tau, the band share (test_tolerance_band_stays_narrow) printed and capped."""
    from sparenet_amd.cuda.knn import knn_fused, knn_unfused

    x, k = _random_case(kind, shape)
    tau = _tau(x)
    share = R.band_share(x, k, tau)
    print(f"{kind} {shape}: band share {share:.4f}")
    assert share <= MAX_BAND_SHARE
    for fn in (knn_fused, knn_unfused):
        idx = fn(torch.from_numpy(x).to(dev), k).cpu().numpy()
        assert _rows_valid(idx, x, k, tau) == {}, fn.__name__


# ------------------------------------------------------------------ edge features
def _edge_features(x, idx, dev, what):
    """Forward and backward against the float64 reference inside the derived bound (grnet_ref): the forward is one
    subtraction, a backward sum has k own terms and one term per entry of the point's inverse list, in any order."""
    from sparenet_amd.cuda.knn import get_graph_feature

    xt = torch.from_numpy(x).to(dev).requires_grad_(True)
    out = get_graph_feature(xt, k=idx.shape[2], idx=torch.from_numpy(idx).to(dev))
    ref = R.graph_feature(x, idx)
    R.assert_within(out.detach().cpu().numpy(), ref, R.sum_bound(1, 1, np.abs(ref)), what + ": forward")
    go = (np.random.default_rng(3).random(ref.shape) * 2 - 1).astype(np.float32)
    out.backward(torch.from_numpy(go).to(dev))
    g, terms, a = R.graph_feature_backward(go, idx)
    R.assert_within(xt.grad.cpu().numpy(), g, R.sum_bound(terms[:, None], 1, a), what + ": backward")
    return terms


@pytest.mark.gpu
def test_hip_edge_features_inverse_lists(dev):
    """The inverse-list build (count, scan, fill) past one 1024-entry scan chunk: n = 3000 with the kernel's own graph
    (three chunks, a carry twice), a star graph (one list of 3,000 entries or more, many empty lists), a hand-made graph
    whose rows repeat a neighbour, and n = 1024 / 1025 on either side of the chunk size."""
    from sparenet_amd.cuda.knn import knn

    r = np.random.default_rng(12)
    x = r.standard_normal((2, 5, 3000)).astype(np.float32)
    own = knn(torch.from_numpy(x).to(dev), 8).cpu().numpy()
    assert _rows_valid(own, x, 8, _tau(x)) == {}
    _edge_features(x, own, dev, "own graph")
    star = own.copy()
    star[:, :, 0] = 7
    terms = _edge_features(x, star, dev, "star graph")
    assert terms[:, 7].min() >= 8 + 3000 and (terms == 8).any()       # the hub's list, and empty lists
    p = np.arange(3000)
    q, s = r.integers(0, 3000, 3000), r.integers(0, 3000, 3000)
    repeats = np.stack([p, q, q, q, s, s, p, p], 1)[None].repeat(2, 0)
    repeats[1] = repeats[1, ::-1]
    _edge_features(x, np.ascontiguousarray(repeats), dev, "repeated neighbours")
    for n in (1024, 1025):
        xs = np.ascontiguousarray(x[:, :, :n])
        _edge_features(xs, R.knn_exact(xs, 4)[1], dev, f"n={n}")
