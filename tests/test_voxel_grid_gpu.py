"""Voxel-grid subsampling and pooling on the GPU: the kernels against the NumPy reference (tests/voxel_grid_ref.py) and
against the host entry points, in EXACT equality of every output on every case of tests/voxel_grid_cases.py -- the
rules of include/ops/voxel_grid.h fix every bit -- on the resident and on the workspace path (reached at small n through
SN_VOXEL_RESIDENT_MAX), for several launch sizes (SN_VOXEL_BLOCKS), row by row against one-cloud calls and call after
call."""
import numpy as np
import pytest
import torch

import voxel_grid_cases as cases

pytestmark = pytest.mark.gpu

CPU = torch.device("cpu")
RAGGED_1500 = (1500, 0, 1499, 257, 1, -3, 99999)


@pytest.mark.parametrize("name", cases.CASES)
def test_device_case_and_host_bits(dev, name):
    out = cases.check_case(name, dev)
    cases.same(out, cases.run_case(name, CPU), f"{name}: device against host")
    cases.same(cases.run_case(name, dev), out, f"{name}: two calls")


@pytest.mark.parametrize("blocks", [1, 3])
def test_device_any_number_of_workgroups(dev, blocks):
    """One workgroup for the whole batch, and three: no output of any case depends on the launch."""
    with cases.knobs(SN_VOXEL_BLOCKS=blocks):
        for name in cases.CASES:
            cases.check_case(name, dev)
        for c in (5, 64):
            cases.check_pool(c, "mean", dev)


@pytest.mark.parametrize("blocks", [None, 1, 3])
def test_every_case_on_the_workspace_path(dev, blocks):
    """SN_VOXEL_RESIDENT_MAX=256 sends every case above 256 points through chunks, merge passes and the reduce kernel
    (size16384: 64 chunks, six passes), at the default launch and at 1 and 3 workgroups: the reference's bits."""
    from sparenet_amd import _lib

    knobs = {"SN_VOXEL_RESIDENT_MAX": 256}
    if blocks is not None:
        knobs["SN_VOXEL_BLOCKS"] = blocks
    with cases.knobs(**knobs):
        assert _lib.op_call("voxel_grid", "sn_voxel_grid_workspace_bytes", 3, 1025) > 0
        for name in cases.CASES:
            cases.check_case(name, dev)


def _workspace_case(n, seed):
    """Seven clouds of n points, ragged (lengths outside [0, n] included), with points in no voxel."""
    xyz = cases._cube(seed, len(RAGGED_1500), n)
    xyz[:, ::97, 1] = np.nan
    xyz[2, 5:40] = xyz[2, 4]      # a run of equal points across positions
    return xyz, 0.2, (0.05, -0.1, 0.15), tuple(min(v, n + 9) for v in RAGGED_1500), None


@pytest.mark.parametrize("n", [257, 1500])
def test_workspace_path(dev, n):
    """SN_VOXEL_RESIDENT_MAX=256: n = 1500 is six chunks with an odd run in every merge pass (6 -> 3 -> 2 -> 1), n = 257
    a chunk of one point.  The same bits as the resident path, the reference and the host, for every launch size."""
    from sparenet_amd import _lib

    args = _workspace_case(n, 40 + n)
    want = cases.ref.voxel_grid(*args)
    resident = cases.run(*args, dev)
    cases.same(resident, want, f"n = {n}, resident")
    with cases.knobs(SN_VOXEL_RESIDENT_MAX=256):
        assert _lib.op_call("voxel_grid", "sn_voxel_grid_workspace_bytes", 7, n) > 0
        cases.same(cases.run(*args, dev), want, f"n = {n}, workspace path")
        for blocks in (1, 3):
            with cases.knobs(SN_VOXEL_BLOCKS=blocks):
                cases.same(cases.run(*args, dev), want, f"n = {n}, workspace path, {blocks} workgroups")
        capped = args[:4] + (37,)
        cases.same(cases.run(*capped, dev), cases.ref.voxel_grid(*capped), f"n = {n}, workspace path, cap 37")
    cases.same(cases.run(*args, CPU), want, f"n = {n}, host")


def test_workspace_path_at_its_own_size(dev):
    """n = 16385 and n = 40000 without a knob: two and three chunks of 16384."""
    for n in (16385, 40000):
        xyz = cases._cube(n, 1, n)
        got = cases.run(xyz, 0.05, None, None, None, dev)
        cases.same(got, cases.run(xyz, 0.05, None, None, None, CPU), f"n = {n}: device against host")
    cases.same(got, cases.ref.voxel_grid(xyz, 0.05), "n = 40000: device against the reference")


@pytest.mark.parametrize("name", cases.SIZE_CASES + ("ragged", "capbelow", "dropped"))
def test_device_rows_are_one_cloud_calls(dev, name):
    """Every size of the issue at b = 1 as well: the one-cloud call on each row of the b = 3 batch."""
    cases.check_rows_are_one_cloud_calls(name, dev)


def test_device_null_outputs_and_wrapper(dev):
    """Every output but count may be null; the wrapper on device tensors returns the host path's bits, and lengths on
    the device are not read on the host."""
    from sparenet_amd import _lib
    from sparenet_amd.cuda.voxel_grid import GridPool, grid_subsample, voxel_grid, voxel_pool

    xyz, size, origin, _, _ = cases.case("origin")
    pts = torch.tensor(xyz, device=dev)
    count = torch.empty(2, dtype=torch.int32, device=dev)
    _lib.op_call("voxel_grid", "sn_voxel_grid", pts, None, 2, 257, size, None, 7, count, *[None] * 6, None)
    assert np.array_equal(count.cpu().numpy(), cases.ref.voxel_grid(xyz, size, cap=7)["count"])
    grid = voxel_grid(pts, size, origin=origin)
    host = voxel_grid(torch.tensor(xyz), size, origin=origin)
    for got, want in zip(grid, host):
        assert got.is_cuda and torch.equal(got.cpu(), want)
    ragged = cases.case("ragged")
    lengths = torch.tensor(ragged[3], device=dev)
    sub, n_sub = grid_subsample(torch.tensor(ragged[0], device=dev), ragged[1], lengths=lengths, max_voxels=64)
    assert np.array_equal(n_sub.cpu().numpy(), cases.reference("ragged")["count"])
    assert np.array_equal(sub.cpu().numpy().view(np.uint32), cases.reference("ragged")["centroid"][:, :64].view(np.uint32))
    # gradients: the device's backward passes against the host's
    f = torch.tensor(cases.pool_case(5)[1])
    x = torch.tensor((cases._cube(21, 2, 257) * 0.3).astype(np.float32))
    grads = []
    for device in (dev, CPU):
        xd, fd = x.to(device).requires_grad_(True), f.to(device).requires_grad_(True)
        points, pooled, _, _ = GridPool(0.25, "max", max_voxels=40)(xd, fd)
        mean = voxel_pool(fd, voxel_grid(xd.detach(), 0.25), "mean")
        w = torch.linspace(-1, 1, points.numel(), device=device).reshape(points.shape)
        ((points * w).sum() + (pooled * pooled).sum() + (mean * mean).sum()).backward()
        grads.append((xd.grad.cpu(), fd.grad.cpu()))
    assert torch.equal(grads[0][0], grads[1][0]), "centroid backward"
    assert torch.equal(grads[0][1], grads[1][1]), "pool backward"


@pytest.mark.parametrize("c", cases.POOL_CHANNELS)
@pytest.mark.parametrize("mode", cases.POOL_MODES)
def test_device_pool(dev, c, mode):
    out, argmax = cases.check_pool(c, mode, dev)
    _, features, grid = cases.pool_case(c)
    host, host_arg = cases.run_pool(features, grid, mode, CPU)
    assert np.array_equal(out.view(np.uint32), host.view(np.uint32)) and np.array_equal(argmax, host_arg)
    again, again_arg = cases.run_pool(features, grid, mode, dev)
    assert np.array_equal(out.view(np.uint32), again.view(np.uint32)) and np.array_equal(argmax, again_arg)


def test_device_pool_foreign_arrays_and_null_argmax(dev):
    cases.check_pool_skips_foreign_entries(dev)
    _, features, grid = cases.pool_case(5)
    out, argmax = cases.run_pool(features, grid, "max", dev, with_argmax=False)
    assert argmax is None and np.array_equal(out, cases.pool_reference(5, "max")[0])


def test_device_refusals_carry_the_librarys_text(dev):
    from sparenet_amd import SparenetHipError, _lib

    x = torch.zeros(1, 20000, 3, device=dev)
    count = torch.full((1,), -7, dtype=torch.int32, device=dev)
    ws = _lib.op_workspace("voxel_grid", "sn_voxel_grid_workspace_bytes", x, 1, 20000)
    small = _lib.Workspace(ws.tensor, ws.nbytes - 1)
    tail = (count,) + (None,) * 6
    for args, text in (((x, None, 1, 20000, 0.0, None, 8) + tail + (ws,), "size must be finite"),
                       ((x, None, 1, 20000, 0.5, None, 20001) + tail + (ws,), "cap must not exceed n"),
                       ((x, None, 0, 20000, 0.5, None, 8) + tail + (ws,), ">= 1"),
                       ((None, None, 1, 20000, 0.5, None, 8) + tail + (ws,), "null pointer"),
                       ((x, None, 1, 20000, 0.5, None, 8) + tail + (small,), "workspace too small"),
                       ((x, None, 1, 20000, 0.5, None, 8) + tail + (None,), "workspace too small")):
        with pytest.raises(SparenetHipError, match=text):
            _lib.op_call("voxel_grid", "sn_voxel_grid", *args)
    assert int(count[0]) == -7, "a refused call writes nothing"
