"""Density-aware Chamfer distance on the GPU: the kernels against the NumPy reference (tests/dcd_ref.py) at the derived
tolerances of tests/dcd_cases.py, and against the host entry point bit for bit -- sides, counts and both gradients.
Every comparison with the reference prints its figures (`pytest -s`).

Measured on an MI355X ("Density-aware Chamfer"): the loss is within 2.3e-8 of the reference where 2.4e-7 or
more is allowed (worst at 1/1), a gradient component within 0.28 of its bound 2^-21 S (worst at 1/20000); counts, idx
and dist are exact and the device equals the host in every bit of every case."""
import numpy as np
import pytest
import torch

import dcd_cases as cases
import dcd_ref as ref
import list_thresholds

pytestmark = pytest.mark.gpu

CPU = torch.device("cpu")


def assert_same_bits(got, want, label):
    """run()'s outputs of two calls: the value, sides, counts, the search and both gradients."""
    value, raw, g1, g2 = got
    wvalue, wraw, wg1, wg2 = want
    assert np.array_equal(value.view(np.uint32), wvalue.view(np.uint32)), f"{label}: value"
    for key in ("sides", "count1", "count2", "dist1", "dist2", "idx1", "idx2"):
        assert np.array_equal(raw[key], wraw[key]) and raw[key].dtype == wraw[key].dtype, f"{label}: {key}"
    assert np.array_equal(raw["sides"].view(np.uint64), wraw["sides"].view(np.uint64)), f"{label}: sides' bits"
    assert np.array_equal(g1.view(np.uint32), wg1.view(np.uint32)), f"{label}: gradxyz1"
    assert np.array_equal(g2.view(np.uint32), wg2.view(np.uint32)), f"{label}: gradxyz2"


@pytest.mark.parametrize("n_lambda,ratio", cases.RULES)
@pytest.mark.parametrize("n,m", cases.SHAPES)
def test_device_against_reference_and_host(dev, n, m, n_lambda, ratio):
    got = cases.check_shape_against_ref(n, m, n_lambda, ratio, dev)
    x, y, alpha, _ = cases.case(n, m)
    assert_same_bits(got, cases.run(x, y, alpha, n_lambda, ratio, CPU), f"{n}x{m} device against host")


@pytest.mark.parametrize("n,m", [(1500, 1), (20000, 1), (1, 1500), (1, 20000)])
def test_one_target_for_everyone(dev, n, m):
    """A list of 1500 is sorted by a workgroup in LDS, one of 20000 in place; on either side."""
    rng = np.random.default_rng(n + 3 * m)
    x, y = (0.1 * rng.random((1, n, 3))).astype(np.float32), (0.1 * rng.random((1, m, 3))).astype(np.float32)
    for n_lambda, ratio in ((1.0, "none"), (0.5, "size")):
        got = cases.run(x, y, 1000.0, n_lambda, ratio, dev)
        _, raw, g1, g2 = got
        assert raw["count2"].max() == n and raw["count1"].max() == m
        want = ref.dcd(x[0], y[0], 1000.0, n_lambda, ratio)
        cases.check_cloud((raw["sides"][0], raw["count1"][0], raw["count2"][0], g1[0], g2[0]), want,
                          f"{n}x{m} {n_lambda} {ratio}")
        assert_same_bits(got, cases.run(x, y, 1000.0, n_lambda, ratio, CPU), f"{n}x{m} device against host")


def test_copies_of_one_point_choose_index_zero(dev):
    rng = np.random.default_rng(5)
    x = (0.1 * rng.random((1, 700, 3))).astype(np.float32)
    y = np.repeat((0.1 * rng.random((1, 1, 3))).astype(np.float32), 1500, axis=1)
    got = cases.run(x, y, 1000.0, 1.0, "none", dev)
    _, raw, g1, g2 = got
    assert (raw["idx1"] == 0).all() and raw["count2"][0, 0] == 700 and (raw["count2"][0, 1:] == 0).all()
    assert raw["count1"].max() == 1500
    want = ref.dcd(x[0], y[0], 1000.0, 1.0, "none")
    cases.check_cloud((raw["sides"][0], raw["count1"][0], raw["count2"][0], g1[0], g2[0]), want, "700 x 1500 copies")
    assert_same_bits(got, cases.run(x, y, 1000.0, 1.0, "none", CPU), "copies, device against host")


def test_sorted_search_threshold(dev):
    """b = 2, n = m = 2048: the pair count at which cd.forward_cuda switches to the sorted search."""
    from sparenet_amd.cuda.chamfer_distance.chamfer_distance import cd

    assert 2048 * 2048 == cd.SORTED_MIN_PAIRS
    x, y = cases.clouds(2048, 2048, 1000.0, seed=2048, batch=2)
    got = cases.run(x, y, 1000.0, 1.0, "none", dev)
    _, raw, g1, g2 = got
    for i in range(2):
        found = ref.search(x[i], y[i])
        for key, t in zip(("dist1", "idx1", "dist2", "idx2"), found):
            assert np.array_equal(raw[key][i], t), key
        want = ref.dcd(x[i], y[i], 1000.0, 1.0, "none", found=found)
        cases.check_cloud((raw["sides"][i], raw["count1"][i], raw["count2"][i], g1[i], g2[i]), want, f"2048x2048 cloud {i}")
    assert_same_bits(got, cases.run(x, y, 1000.0, 1.0, "none", CPU), "2048x2048 device against host")


def test_more_points_than_one_workgroup_counts_in_lds(dev):
    """b = 1, n = 20000, m = 17000 against the host: more points than the 36864 counters of chamfer.hip's LDS list
    builder, and too many pairs for the NumPy reference."""
    rng = np.random.default_rng(20000)
    x, y = rng.random((1, 20000, 3)).astype(np.float32), rng.random((1, 17000, 3)).astype(np.float32)
    got = cases.run(x, y, 1000.0, 0.5, "size", dev)
    assert got[1]["count1"].sum() == 17000 and got[1]["count2"].sum() == 20000
    assert_same_bits(got, cases.run(x, y, 1000.0, 0.5, "size", CPU), "20000x17000")


@pytest.mark.parametrize("n_lambda,ratio", cases.RULES)
def test_exact_values(dev, n_lambda, ratio):
    rng = np.random.default_rng(2)
    x = rng.random((2, 257, 3)).astype(np.float32)
    y = np.stack([x[i][rng.permutation(257)] for i in range(2)])
    value, raw, g1, g2 = cases.run(x, y, 1000.0, n_lambda, ratio, dev)
    assert (value == 0.0).all() and (raw["sides"] == 0.0).all() and (g1 == 0.0).all() and (g2 == 0.0).all()
    y = (0.1 * rng.random((2, 40, 3)) + np.array([1.45, 0.0, 0.0])).astype(np.float32)
    value, raw, g1, g2 = cases.run(x, y, 1000.0, n_lambda, ratio, dev)
    assert raw["dist1"].min() > 0.104 and raw["dist2"].min() > 0.104
    assert (value == 1.0).all() and (raw["sides"] == 1.0).all() and (g1 == 0.0).all() and (g2 == 0.0).all()


def test_ragged_equals_dense_on_every_slice_and_the_host(dev):
    cases.check_ragged(dev)
    x, y, lengths1, lengths2 = cases.ragged_batch()
    for n_lambda, ratio in ((1.0, "none"), (0.5, "size")):
        assert_same_bits(cases.run(x, y, 1000.0, n_lambda, ratio, dev, lengths1, lengths2),
                         cases.run(x, y, 1000.0, n_lambda, ratio, CPU, lengths1, lengths2), "ragged device against host")
    # lengths already on the device are used as they are
    on_device = cases.run(x, y, 1000.0, 1.0, "none", dev, torch.tensor(lengths1, device=dev),
                          torch.tensor(lengths2, dtype=torch.int32, device=dev))
    assert_same_bits(on_device, cases.run(x, y, 1000.0, 1.0, "none", dev, lengths1, lengths2), "device lengths")


def test_second_call_and_upstream_gradient(dev):
    from sparenet_amd.cuda.dcd import DensityAwareChamferDistance

    x, y, alpha, _ = cases.case(513, 64)
    first = cases.run(x, y, alpha, 0.5, "size", dev)
    assert_same_bits(cases.run(x, y, alpha, 0.5, "size", dev), first, "second call")
    weights = torch.tensor([0.25, -3.0, 1.7], device=dev)
    xt, yt = torch.tensor(x, device=dev).requires_grad_(True), torch.tensor(y, device=dev).requires_grad_(True)
    (DensityAwareChamferDistance(alpha, 0.5, "size")(xt, yt) * weights).sum().backward()
    scale = weights[:, None, None].cpu()
    assert torch.equal(xt.grad.cpu(), scale * torch.tensor(first[2]))
    assert torch.equal(yt.grad.cpu(), scale * torch.tensor(first[3]))


def test_fused_validation_metrics_with_dcd(dev):
    from sparenet_amd.cuda.dcd import density_aware_chamfer
    from sparenet_amd.utils.metrics import fused_validation_metrics

    x, y, _, _ = cases.case(1025, 1025)
    pred, gt = torch.tensor(x, device=dev), torch.tensor(y, device=dev)
    plain = fused_validation_metrics(pred, gt, with_emd=False)
    flagged = fused_validation_metrics(pred, gt, with_emd=False, with_dcd=True, dcd_alpha=500.0, dcd_n_lambda=0.5)
    assert sorted(plain) == ["ChamferDistance", "F-Score"] and sorted(flagged) == ["ChamferDistance", "DCD", "F-Score"]
    for key in plain:
        assert torch.equal(plain[key], flagged[key]), key
    assert torch.equal(flagged["DCD"], density_aware_chamfer(pred, gt, 500.0, 0.5))
    xr, yr, lengths1, lengths2 = cases.ragged_batch()
    pred, gt = torch.tensor(xr, device=dev), torch.tensor(yr, device=dev)
    plain = fused_validation_metrics(pred, gt, with_emd=False, pred_lengths=lengths1, gt_lengths=lengths2)
    flagged = fused_validation_metrics(pred, gt, with_emd=False, pred_lengths=lengths1, gt_lengths=lengths2, with_dcd=True)
    assert sorted(flagged) == ["ChamferDistance", "DCD", "F-Score"]
    for key in plain:
        assert torch.equal(plain[key], flagged[key]), key
    assert torch.equal(flagged["DCD"], density_aware_chamfer(pred, gt, lengths1=lengths1, lengths2=lengths2))


@pytest.mark.parametrize("swap", [False, True], ids=["lists_of_cloud2", "lists_of_cloud1"])
@pytest.mark.parametrize("counts", list_thresholds.COUNTS, ids=["16_64", "16384"])
def test_list_thresholds(dev, counts, swap):
    """Lists of exactly 1, 2, 16, 17, 64, 65 and of 16384, 16385 entries (tests/list_thresholds.py), on either side: the
    device equals the host in sides, counts and both gradients."""
    x, y = list_thresholds.clouds(counts)
    if swap:
        x, y = y, x
    got = cases.run(x, y, 1000.0, 1.0, "none", dev)
    assert np.array_equal(got[1]["count1" if swap else "count2"][0], counts)
    assert_same_bits(got, cases.run(x, y, 1000.0, 1.0, "none", CPU), f"lists of {counts}, device against host")
