"""sparenet_amd.cuda.registration on CPU tensors -- the library's host entry points, the same routines as the kernels --
against the NumPy reference (tests/registration_ref.py) at the tolerances tests/registration_cases.py derives.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import registration_cases as cases
import registration_ref as ref
from sparenet_amd.cuda.registration import aligned_chamfer, icp, rigid_fit, transform_points

CPU = torch.device("cpu")


@pytest.mark.parametrize("name", [c["name"] for c in cases.fit_cases()])
def test_fit_against_reference_and_independent_of_the_batch(name):
    c = cases.fit_case(name)
    alone, among = cases.run_fit(c, CPU, 1), cases.run_fit(c, CPU, 3)
    cases.check_fit(c, alone)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(alone, among)), "a cloud's bits depend on its batch"
    again = cases.run_fit(c, CPU, 1)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(alone, again)), "two calls differ"


def test_translated_cloud_meets_the_tolerance_of_its_twin_at_the_origin():
    """The pivot's test: the deviation is in units of u T / gap, and T and the gap are those of the cloud at the origin."""
    near = cases.fit_deviation(cases.fit_case("origin_twin"), cases.run_fit(cases.fit_case("origin_twin"), CPU, 1))
    far = cases.fit_deviation(cases.fit_case("translated"), cases.run_fit(cases.fit_case("translated"), CPU, 1))
    print(f"deviation at the origin {near:.3g}, at (1000, -2000, 500) {far:.3g}, bound {cases.K:.3g}")
    assert near <= cases.K and far <= cases.K


def test_ragged_lengths_including_zero():
    cases.ragged_fit_scenario(CPU)


def test_transform_points_bits_and_padding():
    cases.transform_scenario(CPU)


def test_transform_points_gradients():
    cases.gradient_scenario(CPU)


@pytest.mark.parametrize("deg", [10, 30])
def test_icp_recovers_the_pose_of_moved_points(deg):
    cases.icp_same_scenario(CPU, deg)


@pytest.mark.parametrize("deg", [10, 30])
def test_icp_on_a_resampled_surface_point_and_plane(deg):
    cases.icp_resampled_scenario(CPU, deg)


def test_icp_ragged_batch_max_dist_and_init():
    cases.icp_options_scenario(CPU)


def test_icp_frozen_pose_does_not_depend_on_iters():
    a = cases.run_icp(CPU, "same", 10, "point", iters=60)
    b = cases.run_icp(CPU, "same", 10, "point", iters=90)
    assert bool(a.converged[0]) and cases.same_bits(a, b)


def test_icp_zero_iterations_measures_the_start():
    src, dst, _, _ = cases.icp_clouds("same", 10)
    out = icp(torch.from_numpy(src.copy())[None], torch.from_numpy(dst.copy())[None], iters=0)
    want = ref.icp(src, dst, 0)
    assert torch.equal(out.pose[0], torch.eye(4, dtype=torch.float64)) and int(out.iterations[0]) == 0
    assert not bool(out.converged[0]) and float(out.fitness[0]) == 1.0
    assert abs(float(out.rmse[0]) - want.rmse) <= cases.K * cases.U * want.rmse


def test_aligned_chamfer_and_its_gradient():
    cases.aligned_chamfer_scenario(CPU)


# ------------------------------------------------------------------------------------------------------ refusals
def _lib():
    import sparenet_amd

    return sparenet_amd.lib()


def _step_host(lib, **change):
    one = ctypes.c_void_p(8)      # never dereferenced: validation fails first
    null = ctypes.c_void_p(0)
    a = dict(moved=one, dst=one, idx=one, weight=null, dst_normals=null, src_lengths=null, dst_lengths=null, b=1, n=4,
             m=4, mode=0, with_scale=0, max_dist=0.0, rtol=0.0, atol=0.0, freeze=0, pose=one, scale=one, state=one,
             stats=one)
    a.update(change)
    f = lambda v: ctypes.c_double(v)      # noqa: E731
    rc = lib.sn_rigid_step_host(a["moved"], a["dst"], a["idx"], a["weight"], a["dst_normals"], a["src_lengths"],
                                a["dst_lengths"], a["b"], a["n"], a["m"], a["mode"], a["with_scale"], f(a["max_dist"]),
                                f(a["rtol"]), f(a["atol"]), a["freeze"], a["pose"], a["scale"], a["state"], a["stats"], 0)
    return rc, lib.sn_last_error().decode()


@pytest.mark.parametrize("change, text", [
    (dict(b=0), "need b,n,m >= 1"),
    (dict(n=0), "need b,n,m >= 1"),
    (dict(m=0), "need b,n,m >= 1"),
    (dict(moved=ctypes.c_void_p(0)), "null pointer (moved, dst and stats are required)"),
    (dict(stats=ctypes.c_void_p(0)), "null pointer (moved, dst and stats are required)"),
    (dict(state=ctypes.c_void_p(0)), "a pose needs scale and state"),
    (dict(pose=ctypes.c_void_p(0), freeze=1), "freeze needs a pose"),
    (dict(mode=2), "mode must be 0 (point) or 1 (plane)"),
    (dict(mode=1), "mode 1 (plane) needs dst_normals"),
    (dict(mode=1, dst_normals=ctypes.c_void_p(8), with_scale=1), "with_scale is for mode 0 (point) only"),
    (dict(idx=ctypes.c_void_p(0), m=5), "a null idx matches row i to row i and needs n == m"),
    (dict(rtol=-1.0), "rtol and atol must not be negative"),
    (dict(atol=-1.0), "rtol and atol must not be negative"),
])
def test_step_refusals_by_message(change, text):
    rc, message = _step_host(_lib(), **change)
    assert rc == -22 and text in message, message


def test_device_entry_points_refuse_before_touching_the_gpu():
    lib = _lib()
    one, null = ctypes.c_void_p(8), ctypes.c_void_p(0)
    f = ctypes.c_double
    assert lib.sn_rigid_step_workspace_bytes(2, 1025) == 2 * 2 * 32 * 8
    assert lib.sn_rigid_step_workspace_bytes(1, 1024) == 32 * 8
    rc = lib.sn_rigid_step(one, one, one, null, null, null, null, 2, 1025, 7, 0, 0, f(0), f(0), f(0), 0, one, one, one, one,
                           one, ctypes.c_size_t(2 * 2 * 32 * 8 - 1), null)
    assert rc == -22 and "workspace too small" in lib.sn_last_error().decode()
    rc = lib.sn_rigid_step(one, one, one, null, null, null, null, 2, 1025, 7, 3, 0, f(0), f(0), f(0), 0, one, one, one, one,
                           one, ctypes.c_size_t(1 << 20), null)
    assert rc == -22 and "mode must be 0 (point) or 1 (plane)" in lib.sn_last_error().decode()
    assert lib.sn_rigid_apply(null, one, null, null, 1, 4, one, null) == -22
    assert "null pointer (xyz, pose and out are required)" in lib.sn_last_error().decode()
    assert lib.sn_rigid_apply_host(one, one, null, null, 0, 4, one, 0) == -22
    assert "need b,n >= 1" in lib.sn_last_error().decode()


def test_host_step_refuses_negative_weights():
    x = torch.rand(1, 8, 3)
    w = torch.ones(1, 8)
    w[0, 3] = -1.0
    with pytest.raises(ValueError, match="rigid_fit: weights must be finite and not negative"):
        rigid_fit(x, x, weights=w)
    lib = _lib()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    rc, message = _step_host(lib, moved=ptr(x), dst=ptr(x), idx=ctypes.c_void_p(0), weight=ptr(w), n=8, m=8)
    assert rc == -22 and "weight must not be negative (cloud 0, row 3)" in message, message


X, Y = torch.rand(2, 8, 3), torch.rand(2, 9, 3)
POSE = torch.eye(4, dtype=torch.float64)


@pytest.mark.parametrize("call, error, text", [
    (lambda: transform_points(X[0], POSE), ValueError, "transform_points: xyz must be a non-empty [B, N, 3] tensor"),
    (lambda: transform_points(X.int(), POSE), TypeError, "transform_points: xyz must be a floating-point tensor"),
    (lambda: transform_points(X, POSE[:3]), ValueError, "transform_points: pose must be a floating-point [4, 4] or [2, 4, 4]"),
    (lambda: transform_points(X, POSE, scale=torch.ones(3)), ValueError, "transform_points: scale must be a number or"),
    (lambda: transform_points(X, POSE, lengths=[1, 2, 3]), ValueError, "lengths: expected 2 lengths"),
    (lambda: rigid_fit(X, Y), ValueError, "rigid_fit: idx=None matches row i to row i and needs N == M"),
    (lambda: rigid_fit(X, Y[:1]), ValueError, "rigid_fit: batch sizes differ"),
    (lambda: rigid_fit(X, Y, idx=torch.zeros(2, 8)), TypeError, "rigid_fit: idx must be an int32 / int64 tensor"),
    (lambda: rigid_fit(X, Y, idx=torch.zeros(2, 9, dtype=torch.int32)), ValueError, "rigid_fit: idx must be a [2, 8] tensor"),
    (lambda: rigid_fit(X, X, weights=torch.ones(2, 7)), ValueError, "rigid_fit: weights must be a floating-point [2, 8]"),
    (lambda: rigid_fit(X, X, mode="line"), ValueError, "rigid_fit: mode must be 'point' or 'plane'"),
    (lambda: rigid_fit(X, X, mode="plane"), ValueError, "rigid_fit: mode='plane' needs dst_normals"),
    (lambda: rigid_fit(X, X, mode="plane", dst_normals=X, with_scale=True), ValueError,
     "rigid_fit: with_scale is for mode='point' only"),
    (lambda: rigid_fit(X, Y, idx=torch.zeros(2, 8, dtype=torch.int32), mode="plane", dst_normals=X), ValueError,
     "rigid_fit: dst_normals must be a floating-point tensor of dst's shape"),
    (lambda: rigid_fit(X, X, max_dist=0), ValueError, "rigid_fit: max_dist must be None or a number > 0"),
    (lambda: rigid_fit(X, X, init=torch.eye(3)), ValueError, "rigid_fit: init must be a floating-point [4, 4] or"),
    (lambda: icp(X, Y, iters=-1), ValueError, "icp: iters must be an integer >= 0"),
    (lambda: icp(X, Y, rtol=-1e-3), ValueError, "icp: rtol and atol must not be negative"),
    (lambda: icp(X.long(), Y), TypeError, "icp: src must be a floating-point tensor"),
    (lambda: aligned_chamfer(X, Y, iters=1.5), ValueError, "icp: iters must be an integer >= 0"),
])
def test_python_refusals_by_message(call, error, text):
    with pytest.raises(error) as info:
        call()
    assert text in str(info.value), str(info.value)


def test_every_prototype_of_the_header_is_exported():
    from sparenet_amd import _lib

    lib = _lib.lib()
    names = sorted(_lib.prototypes(_lib.op_headers()["rigid_fit"]))
    assert names == ["sn_rigid_apply", "sn_rigid_apply_host", "sn_rigid_step", "sn_rigid_step_host",
                     "sn_rigid_step_workspace_bytes"]
    for name in names:
        assert hasattr(lib, name), name
    assert lib.sn_abi_version() == 4


def test_metric_is_the_operator():
    from sparenet_amd.utils import metrics

    src, dst, _, _ = cases.icp_clouds("same", 10)
    a, b = torch.from_numpy(src.copy())[None, :512].contiguous(), torch.from_numpy(dst.copy())[None, :512].contiguous()
    assert torch.equal(metrics.aligned_chamfer(a, b, iters=5), aligned_chamfer(a, b, iters=5)[0])
