"""sparenet_amd.cuda.registration on the device: against the NumPy reference (tests/registration_ref.py) at the
tolerances tests/registration_cases.py derives, and against the host entry points bit for bit."""
import numpy as np
import pytest
import torch

import registration_cases as cases
from sparenet_amd.cuda.registration import icp, rigid_fit

pytestmark = pytest.mark.gpu

GPU, CPU = torch.device("cuda:0"), torch.device("cpu")


def _same_arrays(a, b):
    return all(x.tobytes() == y.tobytes() and x.dtype == y.dtype for x, y in zip(a, b))


def _same_tensors(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        x, y = x.cpu(), y.cpu()
        if x.is_floating_point():      # a NaN that passed through (an unread padding row) is a NaN on both sides
            assert torch.equal(x.isnan(), y.isnan()), "device and host differ"
            x, y = x.nan_to_num(nan=0.0), y.nan_to_num(nan=0.0)
        assert x.dtype == y.dtype and torch.equal(x, y), "device and host differ"


@pytest.mark.parametrize("name", [c["name"] for c in cases.fit_cases()])
def test_fit_against_reference_host_and_independent_of_the_batch(name):
    c = cases.fit_case(name)
    alone, among = cases.run_fit(c, GPU, 1), cases.run_fit(c, GPU, 3)
    cases.check_fit(c, alone)
    assert _same_arrays(alone, among), "a cloud's bits depend on its batch"
    assert _same_arrays(alone, cases.run_fit(c, GPU, 1)), "two calls differ"
    assert _same_arrays(alone, cases.run_fit(c, CPU, 1)), "device and host differ"
    assert _same_arrays(among, cases.run_fit(c, CPU, 3)), "device and host differ in a batch"


def test_translated_cloud_meets_the_tolerance_of_its_twin_at_the_origin():
    near = cases.fit_deviation(cases.fit_case("origin_twin"), cases.run_fit(cases.fit_case("origin_twin"), GPU, 1))
    far = cases.fit_deviation(cases.fit_case("translated"), cases.run_fit(cases.fit_case("translated"), GPU, 1))
    print(f"deviation at the origin {near:.3g}, at (1000, -2000, 500) {far:.3g}, bound {cases.K:.3g}")
    assert near <= cases.K and far <= cases.K


def test_ragged_lengths_including_zero():
    _same_tensors(cases.ragged_fit_scenario(GPU), cases.ragged_fit_scenario(CPU))


def test_transform_points_bits_and_padding():
    _same_tensors(cases.transform_scenario(GPU), cases.transform_scenario(CPU))


def test_transform_points_gradients():
    cases.gradient_scenario(GPU)      # the backward is torch's float64 arithmetic: no bit contract with the host


def test_aligned_chamfer_and_its_gradient():
    cases.aligned_chamfer_scenario(GPU)


@pytest.mark.parametrize("deg", [10, 30])
def test_icp_recovers_the_pose_of_moved_points(deg):
    _same_tensors(cases.icp_same_scenario(GPU, deg), cases.icp_same_scenario(CPU, deg))


@pytest.mark.parametrize("deg", [10, 30])
def test_icp_on_a_resampled_surface_point_and_plane(deg):
    _same_tensors(cases.icp_resampled_scenario(GPU, deg), cases.icp_resampled_scenario(CPU, deg))


def test_icp_ragged_batch_max_dist_and_init():
    _same_tensors(cases.icp_options_scenario(GPU), cases.icp_options_scenario(CPU))


def test_icp_frozen_pose_does_not_depend_on_iters():
    a = cases.run_icp(GPU, "same", 10, "point", iters=60)
    b = cases.run_icp(GPU, "same", 10, "point", iters=90)
    assert bool(a.converged[0]) and cases.same_bits(a, b)


def test_icp_estimates_normals_when_none_are_given():
    """mode="plane" without normals: estimate_normals on the target (device only), then the same loop."""
    src, dst, normals, _ = cases.icp_clouds("resampled", 10)
    s, d = torch.from_numpy(src.copy())[None].to(GPU), torch.from_numpy(dst.copy())[None].to(GPU)
    out = icp(s, d, cases.ICP_ITERS, mode="plane")
    given = cases.run_icp(GPU, "resampled", 10, "plane")
    angle, shift = cases.pose_error(out.pose[0].cpu().numpy(), given.pose[0].cpu().numpy())
    print(f"estimated against exact normals: {angle:.3g} degrees, {shift:.3g}; iterations {int(out.iterations[0])}")
    assert bool(out.converged[0]) and angle <= 0.5 and shift <= 0.01      # the same basin: edges blur estimated normals


def test_larger_icp_is_the_host_run_bit_for_bit():
    """2 x 16384 on 2 x 16384, iters = 10: the sorted search and sixteen chunks per cloud."""
    rng = np.random.default_rng(5)
    src = rng.random((2, 16384, 3)).astype(np.float32)
    dst = np.stack([cases.moved_copy(rng.random((16384, 3)).astype(np.float32), cases.pose_of(5.0, cases.SHIFT))
                    for _ in range(2)])
    on_gpu = icp(torch.from_numpy(src).to(GPU), torch.from_numpy(dst).to(GPU), iters=10)
    on_cpu = icp(torch.from_numpy(src), torch.from_numpy(dst), iters=10)
    print(f"rmse {on_gpu.rmse.tolist()}, host {on_cpu.rmse.tolist()}")
    _same_tensors(list(on_gpu), list(on_cpu))


def test_negative_weights_are_no_inliers_on_the_device():
    """The device entry point cannot refuse what it cannot read: such rows are no inliers (the wrapper refuses them)."""
    from sparenet_amd import _lib

    c = cases.fit_case("weights")
    b, n = 1, c["src"].shape[0]
    src, dst = torch.from_numpy(c["src"].copy())[None].to(GPU), torch.from_numpy(c["dst"].copy())[None].to(GPU)
    w = torch.from_numpy(c["weight"].copy())[None].to(GPU)
    results = []
    for weights in (w, torch.where(w == 0, torch.full_like(w, -1.0), w)):
        pose = torch.eye(4, dtype=torch.float64, device=GPU)[None].clone()
        scale, state = torch.ones(1, dtype=torch.float64, device=GPU), torch.zeros(1, 4, dtype=torch.float64, device=GPU)
        stats = torch.empty(1, 4, dtype=torch.float64, device=GPU)
        ws = _lib.op_workspace("rigid_fit", "sn_rigid_step_workspace_bytes", src, b, n)
        _lib.op_call("rigid_fit", "sn_rigid_step", src, dst, None, weights, None, None, None, b, n, n, 0, 0, 0.0, 0.0, 0.0,
                     0, pose, scale, state, stats, ws)
        results.append((pose.cpu(), stats.cpu()))
    (pose0, stats0), (pose1, stats1) = results
    assert torch.equal(stats0[:, 2], stats1[:, 2]) and float(stats1[0, 1]) < float(stats0[0, 1]) == 1.0
    assert torch.equal(pose0, pose1)      # the zero-weight rows added exact zeros
