"""Ragged batches on CPU tensors (sparenet_amd.cuda.ragged, no GPU needed): chamfer_ragged loops over the clouds
through the library's host Chamfer, so every cloud's valid range must equal the oracle on the slice bit for bit,
gradients included, and padding rows must follow the contract of include/sparenet_hip.h (distance 0, gradient 0,
never read -- NaN is planted in them).  masked_mean and the ragged validation metrics against a per-sample numpy
restatement; the lengths validation."""
import numpy as np
import pytest
import torch

import oracle


def _batch(seed=0, b=5, n=70, m=90):
    r = np.random.default_rng(seed)
    x = r.random((b, n, 3), dtype=np.float32)
    y = r.random((b, m, 3), dtype=np.float32)
    l1 = [n, 1, 0, 33, 17][:b]
    l2 = [m, m, 40, 0, 1][:b]
    for i in range(b):   # padding rows must never be read
        x[i, l1[i]:] = np.nan
        y[i, l2[i]:] = np.nan
    return x, y, l1, l2


@pytest.mark.parametrize("as_tensor", [False, True])
def test_chamfer_ragged_cpu_equals_oracle_on_every_slice(as_tensor):
    from sparenet_amd.cuda.ragged import chamfer_ragged, chamfer_ragged_forward_raw

    x, y, l1, l2 = _batch()
    a1, a2 = (torch.tensor(l1), torch.tensor(l2, dtype=torch.int32)) if as_tensor else (l1, l2)
    xt = torch.from_numpy(x).requires_grad_(True)
    yt = torch.from_numpy(y).requires_grad_(True)
    d1, d2 = chamfer_ragged(xt, yt, a1, a2)
    r = np.random.default_rng(1)
    gd1 = r.standard_normal(d1.shape).astype(np.float32)
    gd2 = r.standard_normal(d2.shape).astype(np.float32)
    for i in range(len(l1)):   # upstream gradients of padding rows are not read either
        gd1[i, l1[i]:] = np.nan
        gd2[i, l2[i]:] = np.nan
    torch.autograd.backward([d1, d2], [torch.from_numpy(gd1), torch.from_numpy(gd2)])
    _, _, i1, i2, *_ = chamfer_ragged_forward_raw(torch.from_numpy(x), torch.from_numpy(y), a1, a2)
    d1, d2, g1, g2 = d1.detach().numpy(), d2.detach().numpy(), xt.grad.numpy(), yt.grad.numpy()
    i1, i2 = i1.numpy(), i2.numpy()
    for i, (n, m) in enumerate(zip(l1, l2)):
        if n and m:
            xs, ys = np.ascontiguousarray(x[i:i + 1, :n]), np.ascontiguousarray(y[i:i + 1, :m])
            o1, o2, j1, j2 = oracle.chamfer_forward(xs, ys)
            assert np.array_equal(d1[i, :n], o1[0]) and np.array_equal(d2[i, :m], o2[0]), i
            assert np.array_equal(i1[i, :n], j1[0]) and np.array_equal(i2[i, :m], j2[0]), i
            w1, w2 = oracle.chamfer_backward(xs, ys, np.ascontiguousarray(gd1[i:i + 1, :n]),
                                             np.ascontiguousarray(gd2[i:i + 1, :m]), j1, j2)
            assert np.array_equal(g1[i, :n], w1[0]) and np.array_equal(g2[i, :m], w2[0]), i
        else:   # an empty side: the whole cloud is 0 / -1 / 0
            n = m = 0
        assert not d1[i, n:].any() and not d2[i, m:].any(), i
        assert (i1[i, n:] == -1).all() and (i2[i, m:] == -1).all(), i
        assert not g1[i, n:].any() and not g2[i, m:].any(), i


def test_chamfer_ragged_cpu_full_lengths_equal_the_dense_op():
    from sparenet_amd.cuda.chamfer_distance import ChamferDistanceFunction
    from sparenet_amd.cuda.ragged import chamfer_ragged

    r = np.random.default_rng(5)
    x = torch.from_numpy(r.random((3, 50, 3), dtype=np.float32))
    y = torch.from_numpy(r.random((3, 61, 3), dtype=np.float32))
    a = chamfer_ragged(x, y, [50] * 3, [61] * 3)
    b = ChamferDistanceFunction.apply(x, y)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _masked_mean_np(d, lengths):
    return np.array([d[i, :n].astype(np.float64).sum() / n if n else 0.0 for i, n in enumerate(lengths)])


def test_masked_mean_equals_numpy_restatement():
    from sparenet_amd.cuda.ragged import masked_mean

    r = np.random.default_rng(2)
    d = r.random((4, 300), dtype=np.float32)
    lengths = [300, 0, 1, 129]
    for i, n in enumerate(lengths):
        d[i, n:] = np.nan
    want = _masked_mean_np(d, lengths)
    for given in (lengths, torch.tensor(lengths), torch.tensor(lengths, dtype=torch.int32)):
        got = masked_mean(torch.from_numpy(d), given)
        assert got.dtype == torch.float32 and got.shape == (4,)
        # the float64 sum of <= 300 fp32 values is exact to 2^-44 relative: one rounding to fp32 remains
        assert np.array_equal(got.numpy(), want.astype(np.float32))
    # the padded width does not enter the value
    wide = np.full((4, 1000), np.nan, np.float32)
    wide[:, :300] = d
    assert torch.equal(masked_mean(torch.from_numpy(wide), lengths), masked_mean(torch.from_numpy(d), lengths))


def test_ragged_metrics_cpu_equal_per_sample_numpy_restatement():
    from sparenet_amd.utils.metrics import fused_validation_metrics

    x, y, l1, l2 = _batch(seed=3, b=5, n=200, m=260)
    x[:, :, :] = np.where(np.isnan(x), np.nan, x * 0.05)   # close clouds: a threshold that splits the distances
    y[:, :, :] = np.where(np.isnan(y), np.nan, y * 0.05)
    th = 0.004
    out = fused_validation_metrics(torch.from_numpy(x), torch.from_numpy(y), th=th, with_emd=False,
                                   pred_lengths=l1, gt_lengths=torch.tensor(l2))
    assert set(out) == {"F-Score", "ChamferDistance"}
    seen = set()
    for i, (n, m) in enumerate(zip(l1, l2)):
        if n and m:
            o1, o2, _, _ = oracle.chamfer_forward(np.ascontiguousarray(x[i:i + 1, :n]), np.ascontiguousarray(y[i:i + 1, :m]))
            th2 = float(th) * float(th)
            p, r = (o1[0] < th2).mean(), (o2[0] < th2).mean()
            f = 2 * p * r / (p + r) if p + r > 0 else 0.0
            cd = (np.float32(o1[0].astype(np.float64).mean()) + np.float32(o2[0].astype(np.float64).mean())) * np.float32(1000)
            seen.add(0 < f < 1)
        else:
            f, cd = 0.0, np.float32(0)
        assert float(out["F-Score"][i]) == f, i
        assert np.float32(out["ChamferDistance"][i].item()) == cd, i
    assert True in seen   # the threshold did split some cloud's distances


def test_lengths_validation():
    from sparenet_amd import SparenetHipError
    from sparenet_amd.cuda.ragged import chamfer_ragged, emd_ragged, pad_compact
    from sparenet_amd.utils.metrics import fused_validation_metrics

    x, y = torch.rand(2, 8, 3), torch.rand(2, 9, 3)
    for bad in ([9, 1], [-1, 1], torch.tensor([1, 100])):
        with pytest.raises(ValueError):
            chamfer_ragged(x, y, bad, [9, 9])
    with pytest.raises(ValueError):
        chamfer_ragged(x, y, [8, 8], [9, 10])
    with pytest.raises(ValueError):
        chamfer_ragged(x, y, [8], [9, 9])
    with pytest.raises(TypeError):
        chamfer_ragged(x, y, torch.tensor([1.0, 2.0]), [9, 9])
    with pytest.raises(ValueError, match="pred_lengths"):   # pred bids for gt: checked on the host for host lengths
        fused_validation_metrics(x, y, with_emd=True, emd_any_size=True, pred_lengths=[8, 5], gt_lengths=[9, 4])
    with pytest.raises(ValueError, match="emd_any_size"):
        fused_validation_metrics(x, y, with_emd=True, pred_lengths=[8, 4], gt_lengths=[9, 4])
    with pytest.raises(ValueError):
        fused_validation_metrics(x, y, with_emd=False, pred_lengths=[8, 9], gt_lengths=[9, 4])
    # no host path for the other ragged ops, as for the dense ones
    with pytest.raises((SparenetHipError, RuntimeError)):
        emd_ragged(x, y, [8, 4], [9, 4], 0.005, 2)
    with pytest.raises((SparenetHipError, RuntimeError)):
        pad_compact(x)


def test_ragged_entry_points_validate_arguments_without_gpu():
    import ctypes

    import sparenet_amd

    lib = sparenet_amd.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(8)   # never dereferenced: validation fails first
    assert lib.sn_chamfer_forward_ragged(one, one, 1, 4, 4, null, one, one, one, one, one, null) == -22
    assert b"null pointer" in lib.sn_last_error()
    assert lib.sn_chamfer_forward_ragged(one, one, 1, 0, 4, one, one, one, one, one, one, null) == -22
    assert lib.sn_emd_forward_ragged(one, one, 1, 4, 1 << 21, one, one, ctypes.c_float(0.005), 1, one, one, one,
                                     ctypes.c_size_t(1 << 40), null, null) == -22
    assert b"2^20" in lib.sn_last_error()
    assert lib.sn_emd_forward_ragged(one, one, 1, 8, 4, one, one, ctypes.c_float(0.005), 1, one, one, one,
                                     ctypes.c_size_t(0), null, null) == -22     # widths n > m are fine, the workspace is not
    assert b"workspace" in lib.sn_last_error()
    assert lib.sn_pad_compact(one, 1, 4, one, one, one, null) == -22            # packed aliases xyz
    assert lib.sn_pad_scatter_rows(one, one, 1, 4, 0, ctypes.c_void_p(16), null) == -22
    assert lib.sn_chamfer_backward_ragged_workspace_bytes(2, 100, 50) == lib.sn_chamfer_backward_workspace_bytes(2, 100, 50)
    assert lib.sn_emd_ragged_workspace_bytes(2, 100, 50) > 0 and lib.sn_emd_ragged_backward_workspace_bytes(2, 100, 50) > 0
    assert lib.sn_abi_version() == 4
