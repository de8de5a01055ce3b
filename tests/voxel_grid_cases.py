"""The cases of the voxel-grid tests, shared by tests/test_voxel_grid.py (the host entry points) and
tests/test_voxel_grid_gpu.py (the kernels): seeded inputs, the reference of each (tests/voxel_grid_ref.py, computed once
per process and left unchanged) and the comparison -- EXACT equality of every output; nothing here has a tolerance."""
import contextlib
import ctypes
import functools
import os

import numpy as np
import torch

import voxel_grid_ref as ref

OUTPUTS = ("centroid", "count", "members", "first", "inverse", "order", "start")
SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2049, 16384)
NAN, INF = float("nan"), float("inf")


def _cube(seed, b, n):
    return (np.random.default_rng(seed).random((b, n, 3)) * 2 - 1).astype(np.float32)


def _special_points():
    """Signs and zeros at size 0.125: negative coordinates (floor, not truncation), -0.0, +-1e-30, exact faces."""
    v = [-0.0, 0.0, 1e-30, -1e-30, -0.125, 0.125, -0.1249999, 0.1249999, -1.0, -0.9999999, 0.9999999, -3.5, 3.375]
    pts = [(a, b, c) for a in v for b in (-0.0, 1e-30, -1e-30) for c in (0.0, -0.125)]
    return np.array([pts], np.float32)


def _dropped_points():
    """Points in no voxel among ordinary ones, at size 1: NaN, +inf and -inf in each axis; cells -32768 and 32767 (kept),
    -32769 and 32768 (dropped) on each axis."""
    pts = [(0.5, 0.5, 0.5), (1.5, 0.5, 0.5), (0.25, 0.75, 0.5)]
    for axis in range(3):
        for bad in (NAN, INF, -INF, -32768.0, 32767.5, -32768.5, 32768.0, -32767.5, 3e38, -3e38):
            p = [0.5, 1.5, 2.5]
            p[axis] = bad
            pts.append(tuple(p))
    pts += [(-32768.0, -32768.0, -32768.0), (-32768.0, -32768.0, -32767.0), (32767.0, 32767.0, 32767.9), (0.5, 0.5, 0.75)]
    return np.array([pts, pts[::-1]], np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """(xyz [b, n, 3] fp32, size, origin or None, lengths or None, cap or None).  Lengths outside [0, n] are part of
    the `ragged` case: the library holds them to the range."""
    if name.startswith("size"):          # uniform cubes of three clouds; one-cloud calls are the batch's rows
        n = int(name[4:])
        return _cube(n, 3, n), 0.2, None, None, None
    if name == "many":                   # more clouds than workgroups
        return _cube(300, 300, 64), 0.5, None, None, None
    if name == "faces":                  # every coordinate an exact multiple of the size: points ON cell faces
        k = np.random.default_rng(5).integers(-8, 9, (2, 1025, 3))
        return (k * 0.125).astype(np.float32), 0.125, None, None, None
    if name == "nondyadic":
        return _cube(6, 1, 2049), 0.01, None, None, None
    if name == "signs":
        return _special_points(), 0.125, None, None, None
    if name == "origin_far":             # a large origin with small coordinates: cells near -15625
        return _cube(7, 2, 257), 64.0, (1e6, -1e6, 999936.0), None, None
    if name == "origin":
        return _cube(8, 2, 257), 0.1, (0.37, -0.21, 1.5), None, None
    if name == "dropped":
        return _dropped_points(), 1.0, None, None, None
    if name == "onevoxel":               # one lane adds all 4096 terms
        return ((_cube(9, 1, 4096) + 1) * 0.05).astype(np.float32), 1.0, None, None, None
    if name == "distinct":               # every point its own voxel
        p = np.random.default_rng(10).permutation(1023).astype(np.float32)
        return np.stack([p, p * 0 + 0.5, -p], axis=1)[None], 1.0, None, None, None
    if name == "duplicates":             # every point eight times
        base = _cube(11, 1, 128)[0]
        return np.repeat(base, 8, axis=0)[np.random.default_rng(12).permutation(1024)][None], 0.05, None, None, None
    if name == "ragged":
        n = 130
        xyz = _cube(13, 6, n)
        xyz[0, :], xyz[1, 1:], xyz[2, n - 1:] = NAN, NAN, NAN      # padding rows are never read
        return xyz, 0.25, None, (0, 1, n - 1, n, -5, n + 7), None
    if name.startswith("cap"):           # cap in {1, count - 1, count, n} on a cloud of 40 voxels at most
        xyz = (_cube(14, 2, 257) * 0.3).astype(np.float32)
        count = int(ref.voxel_grid(xyz, 0.25)["count"].min())
        cap = {"cap1": 1, "capbelow": count - 1, "capcount": count, "capn": 257}[name]
        return xyz, 0.25, None, None, cap
    raise KeyError(name)


SIZE_CASES = tuple(f"size{n}" for n in SIZES)
CASES = SIZE_CASES + ("many", "faces", "nondyadic", "signs", "origin_far", "origin", "dropped", "onevoxel", "distinct",
                      "duplicates", "ragged", "cap1", "capbelow", "capcount", "capn")


@functools.lru_cache(maxsize=None)
def reference(name):
    xyz, size, origin, lengths, cap = case(name)
    return ref.voxel_grid(xyz, size, origin, lengths, cap)


def run(xyz, size, origin, lengths, cap, device, threads=0):
    """The entry point itself (sn_voxel_grid, or sn_voxel_grid_host with `threads` for the CPU) -> dict of NumPy
    arrays.  Called below the wrapper so that lengths outside [0, n] reach the library."""
    from sparenet_amd import _lib

    pts = torch.tensor(xyz, device=device)
    b, n = pts.shape[:2]
    cap = n if cap is None else cap
    lens = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=device)
    org = None if origin is None else (ctypes.c_float * 3)(*origin)
    out = {"count": torch.full((b,), -7, dtype=torch.int32, device=device),
           "centroid": torch.full((b, cap, 3), NAN, device=device),
           "members": torch.full((b, cap), -7, dtype=torch.int32, device=device),
           "first": torch.full((b, cap), -7, dtype=torch.int32, device=device),
           "inverse": torch.full((b, n), -7, dtype=torch.int32, device=device),
           "order": torch.full((b, n), -7, dtype=torch.int32, device=device),
           "start": torch.full((b, cap + 1), -7, dtype=torch.int32, device=device)}      # every output is written whole
    args = (pts, lens, b, n, size, org, cap, out["count"], out["centroid"], out["members"], out["first"],
            out["inverse"], out["order"], out["start"])
    if pts.is_cuda:
        ws = _lib.op_workspace("voxel_grid", "sn_voxel_grid_workspace_bytes", pts, b, n)
        _lib.op_call("voxel_grid", "sn_voxel_grid", *args, ws)
    else:
        _lib.op_call("voxel_grid", "sn_voxel_grid_host", *args, threads, host=True)
    return {k: v.cpu().numpy() for k, v in out.items()}


def run_case(name, device, threads=0):
    return run(*case(name), device, threads)


def same(got, want, label):
    """Every output bit for bit (centroids as their bit patterns: -0.0 and NaN would be told apart)."""
    for key in OUTPUTS:
        g, w = np.asarray(got[key]), np.asarray(want[key])
        assert g.shape == w.shape, f"{label}: {key} has shape {g.shape}, expected {w.shape}"
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), w.view(np.uint32)
        bad = np.argwhere(g != w)
        assert not len(bad), f"{label}: {key} differs at {len(bad)} places, first {bad[0].tolist()}: {g[tuple(bad[0])]} != {w[tuple(bad[0])]}"


def check_case(name, device, threads=0):
    out = run_case(name, device, threads)
    same(out, reference(name), f"{name} on {device}")
    return out


def check_rows_are_one_cloud_calls(name, device):
    """Row i of the batch equals the one-cloud call on cloud i's first len rows (the tail of the wider row apart)."""
    xyz, size, origin, lengths, cap = case(name)
    batch = run(xyz, size, origin, lengths, cap, device)
    n = xyz.shape[1]
    for i in range(min(xyz.shape[0], 6)):
        length = n if lengths is None else min(max(lengths[i], 0), n)
        if length == 0:
            assert batch["count"][i] == 0 and (batch["inverse"][i] == -1).all() and (batch["order"][i] == -1).all()
            continue
        width = length if cap is None else min(cap, length)
        one = run(xyz[i:i + 1, :length], size, origin, None, width, device)
        kept = min(int(one["count"][0]), width)
        assert one["count"][0] == batch["count"][i]
        for key in ("centroid", "members", "first"):
            assert np.array_equal(one[key][0][:kept].view(np.uint32), batch[key][i][:kept].view(np.uint32)), (name, i, key)
        if cap is None or width == cap:
            assert np.array_equal(one["start"][0][:kept + 1], batch["start"][i][:kept + 1]), (name, i)
            assert np.array_equal(one["inverse"][0], batch["inverse"][i][:length]), (name, i)
        assert np.array_equal(one["order"][0], batch["order"][i][:length]), (name, i)


@contextlib.contextmanager
def knobs(**values):
    """SN_<NAME>=<value> for the calls inside (the suite reads the library's knobs per call)."""
    old = {k: os.environ.get(k) for k in values}
    os.environ.update({k: str(v) for k, v in values.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


# ---------------------------------------------------------------------------------------------------- pooling
POOL_CHANNELS = (1, 5, 64)
POOL_MODES = ("sum", "mean", "max")


@functools.lru_cache(maxsize=None)
def pool_case(c):
    """(features [2, c, 257], the grid's reference dict): a grid with an empty slot (cap above the count), dropped
    points (-1 entries at the end of order) and features on a coarse lattice, so that maxima are shared."""
    xyz = (_cube(21, 2, 257) * 0.3).astype(np.float32)
    xyz[0, 5], xyz[1, 200] = NAN, INF
    grid = ref.voxel_grid(xyz, 0.25)
    rng = np.random.default_rng(22 + c)
    features = (rng.integers(-3, 4, (2, c, 257)) * 0.25).astype(np.float32)
    features[:, 0, :7] = [1e30, -1e30, 1e-30, 3.0000002, 3.0, -0.0, 0.0]
    return xyz, features, grid


@functools.lru_cache(maxsize=None)
def pool_reference(c, mode):
    _, features, grid = pool_case(c)
    return ref.voxel_pool(features, grid, mode)


def run_pool(features, grid, mode, device, threads=0, with_argmax=True):
    from sparenet_amd import _lib

    f = torch.tensor(features, device=device)
    b, c, n = f.shape
    cap = grid["start"].shape[1] - 1
    order, start, count = (torch.tensor(np.ascontiguousarray(grid[k]), dtype=torch.int32, device=device)
                           for k in ("order", "start", "count"))
    out = torch.full((b, c, cap), NAN, device=device)
    argmax = torch.full((b, c, cap), -7, dtype=torch.int32, device=device) if with_argmax else None
    args = (f, b, c, n, order, start, count, cap, POOL_MODES.index(mode), out, argmax)
    if f.is_cuda:
        _lib.op_call("voxel_grid", "sn_voxel_pool", *args)
    else:
        _lib.op_call("voxel_grid", "sn_voxel_pool_host", *args, threads, host=True)
    return out.cpu().numpy(), None if argmax is None else argmax.cpu().numpy()


def check_pool(c, mode, device, threads=0):
    _, features, grid = pool_case(c)
    out, argmax = run_pool(features, grid, mode, device, threads)
    want, want_arg = pool_reference(c, mode)
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32)), f"pool {mode} c={c} on {device}"
    assert np.array_equal(argmax, want_arg if mode == "max" else np.full_like(argmax, -1)), f"argmax {mode} c={c}"
    return out, argmax


def check_pool_skips_foreign_entries(device):
    """Arrays that did not come from sn_voxel_grid: -1 and too large entries inside a segment are skipped, offsets are
    held to [0, n]; a segment without a member is the empty slot."""
    features = np.arange(2 * 3 * 8, dtype=np.float32).reshape(2, 3, 8)
    grid = {"order": np.array([[3, -1, 1, 99, 0, 2, -1, -1], [-1, -1, 7, 7, 8, -2, 0, 1]], np.int32),
            "start": np.array([[0, 4, 4, 6, 9], [0, 2, 5, 3, 8]], np.int32), "count": np.array([4, 3], np.int32)}
    for mode in POOL_MODES:
        out, argmax = run_pool(features, grid, mode, device)
        want, want_arg = ref.voxel_pool(features, grid, mode)
        assert np.array_equal(out.view(np.uint32), want.view(np.uint32)), (mode, out, want)
        assert np.array_equal(argmax, want_arg if mode == "max" else np.full_like(argmax, -1)), (mode, argmax, want_arg)
