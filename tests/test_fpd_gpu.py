"""The fused PointNet feature kernel (sn_pointnet_pool_forward) and the FPD built on it, on the GPU: exact properties of
the op, the op against float64 with the derived error bound of its fp32 fma chains, activations and FPD end to end
against the reference's float64 run (fixtures of tests/golden/gen_fpd.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fpd_ref  # noqa: E402

pytestmark = pytest.mark.gpu

BLOCKS = (("x1", 0, 1024), ("x2", 1024, 1536), ("x3", 1536, 1792), ("x4", 1792, 1808))


def _pool(dev, xyz, trans, w, relu_last):
    """numpy in, numpy out: xyz [b,n,3], trans [b,3,3] or None, w = (w1, b1, w2, b2, w3, b3)"""
    from sparenet_amd.Frechet.pointnet import pool_mlp_fused

    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in w]
    x = torch.from_numpy(np.ascontiguousarray(xyz)).to(dev).transpose(1, 2)
    tr = None if trans is None else torch.from_numpy(np.ascontiguousarray(trans)).to(dev)
    out = pool_mlp_fused(x, tr, ((t[0], t[1]), (t[2], t[3]), (t[4], t[5])), relu_last)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def model(dev):
    from sparenet_amd.Frechet.pointnet import PointNetCls

    return fpd_ref.load_recipe(PointNetCls(k=16)).to(dev)


def _golden(golden_dir, case, i):
    return np.load(os.path.join(golden_dir, f"fpd_{case}_set{i}.npz"))


# ------------------------------------------------------------------ exact properties, no tolerance
@pytest.mark.parametrize("with_trans", [False, True])
def test_exact_properties(dev, with_trans):
    xyz, trans, w = fpd_ref.op_inputs(3, 1000, 1, with_trans)
    out = _pool(dev, xyz, trans, w, 0)
    assert out.shape == (3, 1024) and np.isfinite(out).all()
    # two runs
    assert np.array_equal(out, _pool(dev, xyz, trans, w, 0))
    # permuting the points of a cloud
    perm = np.random.RandomState(2).permutation(1000)
    assert np.array_equal(out, _pool(dev, xyz[:, perm], trans, w, 0))
    # n = 1000 against the same clouds padded to 1024 with copies of one of their points
    padded = np.concatenate([xyz, np.repeat(xyz[:, 417:418], 24, axis=1)], axis=1)
    assert np.array_equal(out, _pool(dev, padded, trans, w, 0))
    # a cloud alone against its row in the batch
    for c in range(3):
        alone = _pool(dev, xyz[c:c + 1], None if trans is None else trans[c:c + 1], w, 0)
        assert np.array_equal(out[c], alone[0])
    # ReLU after the maximum
    assert np.array_equal(np.maximum(out, 0), _pool(dev, xyz, trans, w, 1))
    assert (out < 0).any()


def test_single_point(dev):
    xyz, trans, w = fpd_ref.op_inputs(2, 1, 3, True)
    out = _pool(dev, xyz, trans, w, 0)
    ref, err = fpd_ref.pool_ref64(xyz, trans, w, 0)
    assert np.array_equal(out, _pool(dev, np.repeat(xyz, 130, axis=1), trans, w, 0))
    assert (np.abs(out - ref) <= err).all()


# ------------------------------------------------------------------ against float64 with the derived bound
@pytest.mark.parametrize("n", [1, 1000, 2048, 16384])
@pytest.mark.parametrize("relu_last", [0, 1])
@pytest.mark.parametrize("with_trans", [False, True])
def test_op_against_float64_within_the_fma_chain_bound(dev, n, relu_last, with_trans):
    """|out - out64| <= e element by element; e is the worst-case forward error of the fp32 fma chains (fpd_ref.pool_ref64).
    Worst case and loose (a few 1e-4 of the largest output for these weights), but any indexing or layout mistake is orders of magnitude outside it."""
    xyz, trans, w = fpd_ref.op_inputs(2, n, 100 + n, with_trans)
    out = _pool(dev, xyz, trans, w, relu_last)
    ref, err = fpd_ref.pool_ref64(xyz, trans, w, relu_last)
    diff = np.abs(out.astype(np.float64) - ref)
    print(f"n {n} relu_last {relu_last} trans {with_trans}: max |out - out64| {diff.max():.3e}, max diff/bound "
          f"{(diff / err).max():.3e}, bound / |out| median {np.median(err / np.maximum(np.abs(ref), 1e-30)):.3e}")
    assert np.abs(ref).max() > 0.5 and err.max() < 1e-3 * np.abs(ref).max()    # the bound itself is tight enough to mean something
    assert (diff <= err).all()


# ------------------------------------------------------------------ end to end against the reference's float64 run
@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_activations_against_the_reference(dev, golden_dir, model, case):
    """Measured against the reference's float64 activations.  Margin: the fixture also holds the reference's own fp32 run;
    20 x its fp32-to-float64 gap, per block, as a maximum absolute error (a strictly sequential K = 128 chain against
    the CPU library's blocked sums, the dense layers on another BLAS)."""
    from sparenet_amd.Frechet.FPD import get_activations

    bs = fpd_ref.CASES[case][4]
    for i, pc in enumerate(fpd_ref.case_clouds(case), 1):
        if pc is None:
            continue
        g = _golden(golden_dir, case, i)
        want, ref32 = g["act64"], g["act32"].astype(np.float64)
        got = get_activations(torch.from_numpy(pc), model, bs, 1808, dev)
        assert got.shape == want.shape
        bad = []
        for name, lo, hi in BLOCKS:
            gap = np.abs(ref32[:, lo:hi] - want[:, lo:hi]).max()
            err = np.abs(got[:, lo:hi] - want[:, lo:hi]).max()
            print(f"case {case} set {i} block {name}: |ours - ref64| {err:.3e}, reference fp32 gap {gap:.3e}, ratio {err / gap:.2f}")
            if not err <= 20 * gap:
                bad.append((name, err, gap))
        assert not bad, bad


@pytest.mark.parametrize("case", ["a", "b"])
def test_fpd_end_to_end(dev, golden_dir, model, case):
    """calculate_fpd(..., device=cuda) against the float64 reference scalar: 20 x the reference's own fp32-to-float64
    gap, and never more than 1e-5 relative."""
    from sparenet_amd.Frechet.FPD import calculate_fpd
    from sparenet_amd.utils.metrics import fpd

    g = _golden(golden_dir, case, 1)
    ref64, ref32 = float(g["fpd_ref64"]), float(g["fpd_ref32"])
    pc1, pc2 = (torch.from_numpy(p) for p in fpd_ref.case_clouds(case))
    bs = fpd_ref.CASES[case][4]
    got = calculate_fpd(pc1, pc2, batch_size=bs, device=dev, model=model)
    tol = min(20 * abs(ref32 - ref64), 1e-5 * abs(ref64))
    print(f"case {case}: fpd {got:.12g} ref64 {ref64:.12g} ref32 {ref32:.12g} |got - ref64| {abs(got - ref64):.3e} "
          f"reference gap {abs(ref32 - ref64):.3e} allowed {tol:.3e} relative {abs(got - ref64) / ref64:.3e}")
    assert abs(got - ref64) <= tol
    # the metrics entry point on the same clouds, already on the device
    assert fpd(pc1.to(dev), pc2.to(dev), model, batch_size=bs) == got


def test_cuda_forward_uses_the_fused_kernel_only(dev, model, monkeypatch):
    """CUDA tensors never reach the torch layers: with the stock path removed the forward still runs."""
    import sparenet_amd.Frechet.pointnet as pn

    def boom(*a, **k):
        raise AssertionError("stock torch path used for a CUDA tensor")

    monkeypatch.setattr(pn, "pool_mlp_torch", boom)
    x = torch.from_numpy(fpd_ref.clouds("cube", 2, 300, 9)).to(dev).transpose(1, 2)
    logp, trans, actv = model(x)
    assert actv.shape == (2, 1808) and trans.shape == (2, 3, 3) and logp.shape == (2, 16)
    with pytest.raises(RuntimeError, match="eval mode"):
        model.train()(x)
    model.eval()
