"""Voxel-grid subsampling and pooling without a GPU: the header and its binding, every refusal of the library and of the
wrapper, the workspace size, the wrapper's call sequence under the converting stub (tests/lib_stub.py), the host entry
points (sn_voxel_grid_host, sn_voxel_pool_host) against the NumPy reference (tests/voxel_grid_ref.py) in EXACT equality
on the cases of tests/voxel_grid_cases.py with 1 and with 3 threads, and the three backward passes.
tests/test_voxel_grid_gpu.py runs the kernels on the same cases and compares them with this host path bit for bit.
test_reference_on_a_hand_made_cloud and test_host_case_details are mostly checks of the reference and of the case
builders themselves; each also makes the host entry point reproduce what it has checked."""
import ctypes
import os

import numpy as np
import pytest
import torch

import voxel_grid_cases as cases
import voxel_grid_ref as ref
from lib_stub import install

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ops", "voxel_grid.h")
NAMES = ["sn_voxel_grid", "sn_voxel_grid_host", "sn_voxel_grid_workspace_bytes", "sn_voxel_pool", "sn_voxel_pool_host"]
GRID = ["xyz", "lengths", "b", "n", "size", "origin", "cap", "count", "centroid", "members", "first", "inverse", "order",
        "start"]
POOL = ["features", "b", "c", "n", "order", "start", "count", "cap", "mode", "out", "argmax"]
CPU = torch.device("cpu")


# ------------------------------------------------------------------------------------------ header and binding
def test_header_and_exports():
    from sparenet_amd import _lib

    protos = _lib.prototypes(HEADER)
    assert sorted(protos) == NAMES
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name), f"{name} declared in include/ops/voxel_grid.h but not exported"
    assert _lib.op_headers()["voxel_grid"] == HEADER
    assert sorted(_lib._op_calls["voxel_grid"]) == sorted(protos)
    assert [p.name for p in protos["sn_voxel_grid"][1]] == GRID + ["workspace", "workspace_bytes", "stream"]
    assert [p.name for p in protos["sn_voxel_grid_host"][1]] == GRID + ["threads"]
    assert [p.name for p in protos["sn_voxel_pool"][1]] == POOL + ["stream"]
    assert [p.name for p in protos["sn_voxel_pool_host"][1]] == POOL + ["threads"]
    for name in ("sn_voxel_grid", "sn_voxel_pool"):
        assert protos[name][1][-1] == _lib.Param("stream", "void", True, False)
    assert _lib.Param("size", "float", False, False) in protos["sn_voxel_grid"][1]
    assert _lib.signature("sn_voxel_grid") == GRID + ["workspace"]
    assert L.sn_abi_version() == 4
    import sparenet_amd
    from sparenet_amd.cuda import voxel_grid as module

    for name in ("voxel_grid", "grid_subsample", "voxel_pool", "GridPool", "VoxelGrid"):
        assert getattr(sparenet_amd, name) is getattr(module, name)


def test_workspace_size(monkeypatch):
    from sparenet_amd import _lib

    size = lambda b, n: _lib.op_call("voxel_grid", "sn_voxel_grid_workspace_bytes", b, n)  # noqa: E731
    monkeypatch.delenv("SN_VOXEL_RESIDENT_MAX", raising=False)
    assert size(32, 16384) == 0 and size(1, 1) == 0, "a resident cloud needs no workspace"
    up = lambda x: (x + 255) // 256 * 256  # noqa: E731
    # two key arrays, two index arrays and the voxel starts, each rounded up to 256 bytes
    assert size(4, 65536) == 2 * up(4 * 65536 * 8) + 3 * up(4 * 65536 * 4)
    assert size(3, 16385) == 2 * up(3 * 16385 * 8) + 3 * up(3 * 16385 * 4)
    assert size(0, 8) == 0 and size(8, 0) == 0 and size(1, (1 << 24) + 1) == 0 and size(1 << 16, 1 << 15) == 0
    assert size(1, 1 << 24) == 2 * (8 << 24) + 3 * (4 << 24)
    monkeypatch.setenv("SN_VOXEL_RESIDENT_MAX", "256")      # only lowers the threshold
    assert size(2, 256) == 0 and size(2, 257) == 2 * up(2 * 257 * 8) + 3 * up(2 * 257 * 4)
    monkeypatch.setenv("SN_VOXEL_RESIDENT_MAX", "100000")
    assert size(2, 16384) == 0 and size(2, 16385) > 0


def test_library_refuses_bad_arguments(monkeypatch):
    import sparenet_amd

    monkeypatch.delenv("SN_VOXEL_RESIDENT_MAX", raising=False)
    L = sparenet_amd.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(8)      # `one` is never dereferenced: validation fails first
    nan, inf = float("nan"), float("inf")

    def grid_data(b=2, n=8, size=0.5, origin=null, cap=4, xyz=one, count=one):
        return (xyz, null, b, n, ctypes.c_float(size), origin, cap, count, one, one, one, one, one, one)

    def grid_device(**kw):
        return L.sn_voxel_grid(*grid_data(**kw), null, ctypes.c_size_t(0), null)

    def grid_host(**kw):
        return L.sn_voxel_grid_host(*grid_data(**kw), 1)

    def pool_data(b=2, c=3, n=8, cap=4, mode=1, **pointers):
        p = {"features": one, "order": one, "start": one, "count": one, "out": one}
        p.update(pointers)
        return (p["features"], b, c, n, p["order"], p["start"], p["count"], cap, mode, p["out"], one)

    for fn in (grid_device, grid_host):
        def refused(text, **kw):
            assert fn(**kw) == -22
            assert text in L.sn_last_error(), L.sn_last_error()

        for size in (0.0, -0.5, nan, inf, -inf):
            refused(b"size must be finite and > 0", size=size)
        for axis in range(3):
            for bad in (nan, inf, -inf):
                origin = (ctypes.c_float * 3)(0.25, 0.5, 0.75)
                origin[axis] = bad
                refused(b"origin must be finite", origin=origin)
        for name in ("b", "n", "cap"):
            refused(b">= 1", **{name: 0})
            refused(b">= 1", **{name: -3})
        refused(b"cap must not exceed n", cap=9)
        refused(b"too large", b=1 << 16, n=1 << 15)
        refused(b"at most 16777216 points", b=1, n=(1 << 24) + 1)
        refused(b"null pointer", xyz=null)
        refused(b"null pointer", count=null)
    # the device entry point alone has a workspace, for clouds above the resident size
    assert grid_device(b=1, n=20000) == -22 and b"workspace too small" in L.sn_last_error()
    need = L.sn_voxel_grid_workspace_bytes(1, 20000)
    assert L.sn_voxel_grid(*grid_data(b=1, n=20000), one, ctypes.c_size_t(need - 1), null) == -22
    assert b"workspace too small" in L.sn_last_error()

    for fn in (lambda **kw: L.sn_voxel_pool(*pool_data(**kw), null), lambda **kw: L.sn_voxel_pool_host(*pool_data(**kw), 1)):
        def refused(text, **kw):
            assert fn(**kw) == -22
            assert text in L.sn_last_error(), L.sn_last_error()

        for name in ("b", "c", "n", "cap"):
            refused(b">= 1", **{name: 0})
            refused(b">= 1", **{name: -1})
        refused(b"cap must not exceed n", cap=9)
        refused(b"too large", b=1 << 16, n=1 << 15)
        for mode in (-1, 3, 100):
            refused(b"unknown pooling mode", mode=mode)
        for name in ("features", "order", "start", "count", "out"):
            refused(b"null pointer", **{name: null})


def test_wrapper_refusals():
    from sparenet_amd import SparenetHipError, _lib
    from sparenet_amd.cuda.voxel_grid import GridPool, grid_subsample, voxel_grid, voxel_pool

    x = torch.rand(2, 8, 3)
    for bad in (torch.zeros(8, 3), torch.zeros(2, 8, 2), torch.zeros(0, 8, 3), torch.zeros(2, 0, 3)):
        with pytest.raises(ValueError, match=r"voxel_grid: xyz must be a non-empty \[B, N, 3\] tensor"):
            voxel_grid(bad, 0.5)
    with pytest.raises(TypeError, match="floating-point"):
        voxel_grid(torch.zeros(2, 8, 3, dtype=torch.int32), 0.5)
    for size in (0, -1.0, float("nan"), float("inf"), "1", None, True, torch.tensor(0.5)):
        with pytest.raises(ValueError, match="size must be a finite number > 0"):
            voxel_grid(x, size)
        with pytest.raises(ValueError, match="size must be a finite number > 0"):
            GridPool(size)
    for origin in ((0, 0), (0, 0, 0, 0), (0, float("nan"), 0), torch.zeros(2), (float("inf"), 0, 0)):
        with pytest.raises(ValueError, match="origin must be three finite numbers"):
            voxel_grid(x, 0.5, origin=origin)
    for cap in (0, -1, 9, 2.5, True):
        with pytest.raises(ValueError, match="max_voxels must be an integer >= 1 and <= 8"):
            voxel_grid(x, 0.5, max_voxels=cap)
    with pytest.raises(ValueError, match="lengths must be in"):
        voxel_grid(x, 0.5, lengths=[1, 9])
    with pytest.raises(ValueError, match="expected 2 lengths"):
        voxel_grid(x, 0.5, lengths=[1])
    with pytest.raises(ValueError, match="mode must be 'centroid' or 'first'"):
        grid_subsample(x, 0.5, mode="random")
    grid = voxel_grid(x, 0.5)
    f = torch.rand(2, 3, 8)
    with pytest.raises(ValueError, match="reduce must be one of max, mean, sum"):
        voxel_pool(f, grid, "min")
    with pytest.raises(ValueError, match="reduce must be one of max, mean, sum"):
        GridPool(0.5, "min")
    with pytest.raises(TypeError, match="grid must be the VoxelGrid"):
        voxel_pool(f, tuple(grid))
    for bad in (torch.rand(2, 8), torch.rand(2, 0, 8), torch.rand(3, 3, 8), torch.rand(2, 3, 9)):
        with pytest.raises(ValueError, match="features"):
            voxel_pool(bad, grid)
    with pytest.raises(TypeError, match="floating-point"):
        voxel_pool(torch.zeros(2, 3, 8, dtype=torch.int64), grid)
    # every SN_EINVAL reaches Python as the binding's error with the library's text
    count = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(SparenetHipError, match="cap must not exceed n"):
        _lib.op_call("voxel_grid", "sn_voxel_grid_host", x, None, 2, 8, 0.5, None, 9, count, *[None] * 6, 1, host=True)
    with pytest.raises(SparenetHipError, match="unknown pooling mode 7"):
        _lib.op_call("voxel_grid", "sn_voxel_pool_host", f, 2, 3, 8, grid.order, grid.start, grid.count, 8, 7,
                     torch.empty(2, 3, 8), None, 1, host=True)


def test_wrapper_call_sequence_under_the_stub(monkeypatch):
    """CPU tensors stand in for device tensors: which entry points the wrapper calls, with what scalars, and that it
    asks for the workspace it passes."""
    from sparenet_amd.cuda import voxel_grid as module

    calls = install(monkeypatch, ["_op_calls"], size_t=4096, record=lambda name, args: (name, args))

    class Device(torch.Tensor):      # a CPU tensor that says it is on the device: the wrapper's branch, the stub's pointers
        is_cuda = True

    monkeypatch.setattr(module._args, "fp32", lambda t: t.detach().contiguous().float().as_subclass(Device))
    x, f = torch.rand(2, 8, 3), torch.rand(2, 3, 8)
    grid = module.voxel_grid(x, 0.5, origin=(0.25, 0.5, 1.0), lengths=[8, 3], max_voxels=5)
    assert [c[0] for c in calls] == ["sn_voxel_grid_workspace_bytes", "sn_voxel_grid"]
    assert calls[0][1] == (2, 8)
    args = calls[1][1]
    assert len(args) == 17 and args[2:4] == (2, 8) and args[4] == 0.5 and args[6] == 5
    assert list(args[5]) == [0.25, 0.5, 1.0] and args[1] is not None and args[15] == 4096
    assert grid.centroids.shape == (2, 5, 3) and grid.start.shape == (2, 6) and grid.inverse.shape == (2, 8)
    del calls[:]
    module.voxel_grid(x, 2, max_voxels=None)
    assert calls[1][1][4:7] == (2.0, None, 8) and calls[1][1][1] is None
    del calls[:]
    for mode, reduce in enumerate(("sum", "mean", "max")):
        out = module.voxel_pool(f, grid, reduce)
        name, args = calls[-1]
        assert name == "sn_voxel_pool" and len(args) == 12 and args[1:4] == (2, 3, 8) and args[7:9] == (5, mode)
        assert (args[10] is not None) == (reduce == "max") and out.shape == (2, 3, 5)
    assert len(calls) == 3


# ------------------------------------------------------------------------------------------ the host entry points
def test_reference_on_a_hand_made_cloud():
    """The reference itself, on values worked out by hand: floor and not truncation, the order of the voxels (x
    slowest), members by index, the centroid's single rounding."""
    xyz = np.array([[[0.75, 0.25, 0.25], [-0.25, 0.25, 0.25], [0.25, 0.25, 1.25], [0.25, 0.25, 0.25], [0.5, 0.0, 0.0],
                     [-0.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [0.1, 0.2, 0.3]]], np.float32)
    out = ref.voxel_grid(xyz, 0.5)
    assert out["count"][0] == 4
    assert out["order"][0].tolist() == [1, 3, 5, 7, 2, 0, 4, -1] and out["inverse"][0].tolist() == [3, 0, 2, 1, 3, 1, -1, 1]
    assert out["start"][0].tolist() == [0, 1, 4, 5, 7, 7, 7, 7, 7] and out["members"][0].tolist() == [1, 3, 1, 2, 0, 0, 0, 0]
    assert out["first"][0].tolist() == [1, 3, 2, 0, -1, -1, -1, -1]
    third = np.float32((np.float64(np.float32(0.25)) + 0.0 + np.float64(np.float32(0.1))) / 3.0)
    assert out["centroid"][0, 1, 0] == third and out["centroid"][0, 3].tolist() == [0.625, 0.125, 0.125]
    cases.same(cases.run(xyz, 0.5, None, None, None, CPU, threads=1), out, "the host entry point on the hand-made cloud")
    # size 0.01, not a dyadic number: the cell is the floor of the ROUNDED double quotient, and never further than one
    # cell from the floor of the exact quotient
    from fractions import Fraction

    size = np.float32(0.01)
    xs = np.array([[k / 100.0, 0, 0] for k in range(-3000, 3000)], np.float32)
    for x, key in zip(xs[:, 0], ref.keys_of(xs, size, np.zeros(3, np.float32))):
        exact = (Fraction(float(x)) / Fraction(float(size))).__floor__()
        cell = (key >> 32) - 32768
        assert cell == int(np.floor(np.float64(x) / np.float64(size))) and cell in (exact, exact + 1)


@pytest.mark.parametrize("name", cases.CASES)
def test_host_case(name):
    out = cases.check_case(name, CPU, threads=1)
    cases.same(cases.run_case(name, CPU, threads=3), out, f"{name}: 3 threads against 1")


def test_host_case_details():
    """What the cases are there for: they reach the paths they name (read off the reference, which the host entry
    point reproduces: checked here on the three cases the assertions lean on most)."""
    r = cases.reference
    for name in ("dropped", "signs", "capbelow"):
        cases.same(cases.run_case(name, CPU, threads=2), r(name), f"{name} with 2 threads")
    assert r("onevoxel")["count"][0] == 1 and r("onevoxel")["members"][0, 0] == 4096
    assert r("distinct")["count"][0] == 1023 and (r("distinct")["members"][0] == 1).all()
    assert (r("duplicates")["members"][0][:r("duplicates")["count"][0]] % 8 == 0).all()
    assert r("ragged")["count"].tolist()[:2] == [0, 1] and min(r("ragged")["count"][[2, 3, 5]]) > 1
    assert r("ragged")["count"][4] == 0, "a negative length is an empty cloud"
    dropped = r("dropped")
    xyz = cases.case("dropped")[0]
    lost = (dropped["inverse"][0] == -1).sum()
    assert lost == 3 * 7 and dropped["count"][0] > 6, "NaN, +-inf, -32769, 32768 and +-3e38 per axis, nothing else"
    cell_min = np.argwhere((xyz[0] == -32768.0).all(axis=1))[0, 0]
    assert dropped["inverse"][0][cell_min] == 0, "cell (-32768, -32768, -32768) has key 0: the first voxel"
    signs = r("signs")
    pts = cases.case("signs")[0][0]
    zero = signs["inverse"][0][np.argwhere((pts == 0).all(axis=1))[0, 0]]      # (+-0.0, -0.0, 0.0)
    for i, p in enumerate(pts):
        if (np.abs(p) <= 1e-30).all():      # -0.0 and 1e-30 share cell 0 with 0.0; -1e-30 lies in cell -1
            assert (signs["inverse"][0][i] == zero) == (not (p == np.float32(-1e-30)).any()), p
    for name, want in (("cap1", 1), ("capbelow", None), ("capcount", None), ("capn", 257)):
        out, cap = r(name), cases.case(name)[4]
        assert want is None or cap == want
        full = r("capn")
        assert (out["count"] == full["count"]).all(), "count is not clipped"
        assert ((out["inverse"] == -1) == (full["inverse"] >= cap)).all(), "the points of dropped voxels"
    assert (r("capbelow")["count"] > cases.case("capbelow")[4]).all() and (r("origin_far")["count"] >= 2).all()
    faces = cases.case("faces")[0]
    assert (faces / np.float32(0.125) == np.round(faces / np.float32(0.125))).all()


@pytest.mark.parametrize("name", cases.SIZE_CASES + ("ragged", "capbelow", "dropped"))
def test_host_rows_are_one_cloud_calls(name):
    """Every size of the issue at b = 1 as well: the one-cloud call on each row of the b = 3 batch."""
    cases.check_rows_are_one_cloud_calls(name, CPU)


def test_host_null_outputs_and_wrapper():
    """Every output but count may be null; the wrapper returns the entry point's arrays."""
    from sparenet_amd import _lib
    from sparenet_amd.cuda.voxel_grid import grid_subsample, voxel_grid

    xyz, size, origin, _, _ = cases.case("origin")
    pts = torch.tensor(xyz)
    count = torch.empty(2, dtype=torch.int32)
    _lib.op_call("voxel_grid", "sn_voxel_grid_host", pts, None, 2, 257, size, (ctypes.c_float * 3)(*origin), 7, count,
                 *[None] * 6, 1, host=True)
    want = cases.reference("origin")
    assert np.array_equal(count.numpy(), want["count"])
    grid = voxel_grid(pts.double(), size, origin=torch.tensor(origin))      # read as fp32
    got = dict(zip(("centroid",) + cases.OUTPUTS[1:], (t.detach().numpy() for t in grid)))
    cases.same(got, want, "the wrapper on CPU tensors")
    assert all(not t.requires_grad for t in grid)
    ragged = cases.case("ragged")
    sub, n_sub = grid_subsample(torch.tensor(ragged[0]), ragged[1], lengths=[0, 1, 129, 130, 0, 130], max_voxels=64)
    assert sub.shape == (6, 64, 3) and np.array_equal(n_sub.numpy(), cases.reference("ragged")["count"])
    first, _ = grid_subsample(pts, size, "first", origin)
    idx = torch.tensor(want["first"]).long()
    assert torch.equal(first, torch.where((idx >= 0)[:, :, None], pts.gather(1, idx.clamp_min(0)[:, :, None].expand(-1, -1, 3)),
                                          torch.zeros(())))


# ------------------------------------------------------------------------------------------ pooling on the host
@pytest.mark.parametrize("c", cases.POOL_CHANNELS)
@pytest.mark.parametrize("mode", cases.POOL_MODES)
def test_host_pool(c, mode):
    out, argmax = cases.check_pool(c, mode, CPU, threads=1)
    again, again_arg = cases.check_pool(c, mode, CPU, threads=3)
    assert np.array_equal(out.view(np.uint32), again.view(np.uint32)) and np.array_equal(argmax, again_arg)


def test_host_pool_details():
    _, features, grid = cases.pool_case(5)
    cap, count = grid["start"].shape[1] - 1, grid["count"]
    assert (count < cap).all() and (grid["order"] == -1).any(), "an empty slot and -1 entries"
    out, argmax = cases.pool_reference(5, "max")
    shared = 0
    for i in range(2):
        for v in range(int(count[i])):
            members = grid["order"][i, grid["start"][i, v]:grid["start"][i, v + 1]]
            for ch in range(5):
                top = np.flatnonzero(features[i, ch, members] == out[i, ch, v])
                shared += len(top) > 1
                assert argmax[i, ch, v] == members[top].min(), "the lowest index among equal maxima"
        assert (out[i, :, int(count[i]):] == 0).all() and (argmax[i, :, int(count[i]):] == -1).all()
    assert shared >= 20, "equal maxima are ordinary in this case"
    cases.check_pool_skips_foreign_entries(CPU)
    out, argmax = cases.run_pool(features, grid, "max", CPU, with_argmax=False)      # argmax may be null
    assert argmax is None and np.array_equal(out, cases.pool_reference(5, "max")[0])


# ------------------------------------------------------------------------------------------ backward
def _upstream(shape, seed):
    """A realistic upstream gradient in float64: a mean's 1 / count times a factor of either sign and any size."""
    rng = np.random.default_rng(seed)
    return torch.tensor(rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 3, shape) / np.prod(shape[:-1]))


def test_centroid_backward_is_g_over_members():
    """d centroid[k] / d x[i] = 1 / members[k] for the members of k: the gradient of x[i] is the upstream row of its
    voxel over the member count, 0 for a point without a voxel -- against the analytic value in float64, to the two
    roundings the fp32 path makes (the upstream gradient's and the division's: 2 * 2^-24 relative)."""
    from sparenet_amd.cuda.voxel_grid import VoxelGridFunction, voxel_grid

    xyz, size, _, _, _ = cases.case("cap1")
    x = torch.tensor(xyz, requires_grad=True)
    x.data[0, 3, 1] = float("nan")
    grid = voxel_grid(x, size, max_voxels=20)
    g = _upstream((2, 20, 3), 1)
    (grid.centroids.double() * g).sum().backward()
    inverse, members = grid.inverse.long(), grid.members.double()
    want = torch.where((inverse >= 0)[:, :, None],
                       (g / members.clamp_min(1)[:, :, None]).gather(1, inverse.clamp_min(0)[:, :, None].expand(-1, -1, 3)),
                       torch.zeros((), dtype=torch.float64))
    assert (inverse < 0).sum() > 10 and x.grad[0, 3].abs().sum() == 0 and x.grad.dtype == torch.float32
    assert (x.grad.double() - want).abs().max() <= (2 * 2.0 ** -24) * want.abs().max()
    assert ((x.grad.double() - want).abs() <= 2 * 2.0 ** -24 * want.abs()).all()
    # the Function in float64, as gradcheck would drive it: the same expression without the roundings
    centroid = VoxelGridFunction.apply(x.detach().double().requires_grad_(True), size, None, None, 20)[0]
    assert centroid.dtype == torch.float32
    x64 = x.detach().double().requires_grad_(True)
    out = VoxelGridFunction.apply(x64, size, None, None, 20)[0]
    out.backward(g.float())
    assert x64.grad.dtype == torch.float64
    assert ((x64.grad - want).abs() <= 2 * 2.0 ** -24 * want.abs()).all()
    # a finite difference inside the cells: every point moves 1 % of the way to its cell's centre, which crosses no
    # face, so the assignment is unchanged and the centroid is linear along the step.  The displacement is taken from
    # the fp32 inputs themselves (exact); what remains is the single rounding of each of the two centroids, at most
    # 2^-24 of a coordinate below 1 each: |fd - lin| <= 2 * 2^-24 * sum |g|.
    base = torch.tensor(xyz)
    base[0, 3, 1] = float("nan")
    centre = (torch.floor(base.double() / size) + 0.5) * size
    moved_x = (base.double() + 0.01 * (centre - base.double())).float()
    moved = voxel_grid(moved_x, size, max_voxels=20)
    assert torch.equal(moved.inverse, grid.inverse) and torch.equal(moved.members, grid.members)
    assert base.abs().nan_to_num().max() < 1
    fd = ((moved.centroids.double() - grid.centroids.detach().double()) * g).sum()
    lin = (want * torch.nan_to_num(moved_x.double() - base.double())).sum()
    assert fd != 0 and abs(fd - lin) <= 2 * 2.0 ** -24 * g.abs().sum()


@pytest.mark.parametrize("reduce", cases.POOL_MODES)
def test_pool_backward(reduce):
    """voxel_pool is linear in the features (max: in the winners), so its gradient is exact: a gather through inverse
    (mean: over the member count), or the upstream value at each voxel's argmax."""
    from sparenet_amd.cuda.voxel_grid import voxel_grid, voxel_pool

    xyz, features, ref_grid = cases.pool_case(5)
    grid = voxel_grid(torch.tensor(xyz), 0.25)
    f = torch.tensor(features, dtype=torch.float64, requires_grad=True)
    out = voxel_pool(f, grid, reduce)
    g = _upstream(tuple(out.shape), 3)
    (out.double() * g).sum().backward()
    g32 = g.float().double()      # the upstream gradient as the fp32 output's backward sees it
    want = torch.zeros_like(f)
    inverse, members = ref_grid["inverse"], ref_grid["members"]
    argmax = cases.pool_reference(5, "max")[1]
    for i in range(2):
        if reduce == "max":
            for ch in range(5):
                for v in range(int(ref_grid["count"][i])):
                    want[i, ch, argmax[i, ch, v]] = g32[i, ch, v]
        else:
            for j in range(f.size(2)):
                k = inverse[i, j]
                if k >= 0:
                    scale = float(members[i, k]) if reduce == "mean" else 1.0
                    want[i, :, j] = (g32[i, :, k].float() / torch.tensor(scale).float()).double() if reduce == "mean" \
                        else g32[i, :, k]
    assert f.grad.dtype == torch.float64 and torch.equal(f.grad, want.detach())
    assert (f.grad[0, :, 5] == 0).all(), "a point without a voxel gets no gradient"
    f2 = torch.tensor(features, dtype=torch.float64, requires_grad=True)
    (voxel_pool(f2, grid, reduce).double() * g).sum().backward()
    assert torch.equal(f2.grad, f.grad), "two backward passes are equal"


def test_grid_pool_module_and_first_mode_gradient():
    from sparenet_amd.cuda.voxel_grid import GridPool, grid_subsample, voxel_grid, voxel_pool

    xyz, features, _ = cases.pool_case(5)
    x, f = torch.tensor(xyz), torch.tensor(features)
    x[0, 5], x[1, 200] = 0.1, 0.2      # finite: "first" gathers input rows
    pool = GridPool(0.25, "max", max_voxels=40)
    points, pooled, count, inverse = pool(x, f)
    grid = voxel_grid(x, 0.25, max_voxels=40)
    assert torch.equal(points, grid.centroids) and torch.equal(pooled, voxel_pool(f, grid, "max"))
    assert torch.equal(count, grid.count) and torch.equal(inverse, grid.inverse) and "size=0.25" in repr(pool)
    xr = x.clone().requires_grad_(True)
    picked, _ = grid_subsample(xr, 0.25, "first", max_voxels=40)
    g = _upstream((2, 40, 3), 4).float()
    picked.backward(g)
    want = torch.zeros_like(x)
    for i in range(2):
        for k in range(min(int(grid.count[i]), 40)):
            want[i, grid.first[i, k]] = g[i, k]
    assert torch.equal(xr.grad, want), "the gradient of a gathered row goes to that row"
