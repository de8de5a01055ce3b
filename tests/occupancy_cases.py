"""What tests/test_occupancy.py (host entry point, CPU tensors) and tests/test_occupancy_gpu.py (device) share: the sets
of clouds, the reference's outputs (computed once per set and left unchanged) and the comparison.  The rule of
include/ops/occupancy.h is integer and fully specified, so every comparison is EXACT equality of cells, counts and
occupied: no row is excluded and no tolerance applies.

The one tolerance here is the bound on |jensen_shannon_divergence (torch float64) - occupancy_ref.jsd (NumPy float64)|.
u = 2^-53.  Both sides evaluate H(M) - (H(P) + H(Q)) / 2 with H(x) = -sum x log2 x over the K non-empty cells of the
mixture M (P and Q have no more).  Per term: x carries at most 2 roundings (quotient by the total; the sum P + Q for
M; the halving is exact), log2 is allowed 3 ulp = 6 u (the OpenCL / ocml limit for double; glibc, SLEEF and NumPy
promise 1), the product is 1 more: 9 u |x log2 x|, and 1 more for the three roundings that combine the entropies: c = 10.
A sum of K terms in any order adds at most (K - 1) u sum|terms|.  The rounding of x also moves log2 x by dx / (x ln 2):
sum x * 2 u / ln 2 = 2.9 u for M and half of 1.45 u each for P and Q, together below 5 u whatever the entropies are.
With A = sum|x log2 x| over M plus half of it over P and Q, each side is within (K + 10) u A + 5 u of the exact value
(the clamp to [0, 1] only moves a value towards it), so
    |torch - NumPy| <= 2 ((K + 10) u A + 5 u).
The worst observed fraction of this bound is printed by the tests and recorded in DESIGN.md ("Occupancy grid and JSD")."""
import functools
import os
import zlib

import numpy as np

import occupancy_ref as ref

U = 2.0 ** -53
C = 10.0
BOUNDARY_RES = (3, 5, 9, 17)      # the spacing is a power of two, and six cells lie exactly on the sphere


def jsd_bound(p_counts, q_counts):
    k, a = ref.jsd_terms(p_counts, q_counts)
    return 2.0 * ((k + C) * U * a + 5.0 * U)


# ---------------------------------------------------------------------------------------------------- clouds
def _frozen(a):
    a.setflags(write=False)
    return a


def ball(rng, s, n, radius=0.5):
    """Uniform in the ball of `radius`, fp32 [s,n,3]."""
    v = rng.standard_normal((s, n, 3))
    v /= np.linalg.norm(v, axis=2, keepdims=True)
    return (v * radius * rng.random((s, n, 1)) ** (1.0 / 3.0)).astype(np.float32)


def midpoint_points(res):
    """res - 1 a power of two.  For three pairs of neighbouring centres (at the rim, in the middle, at the other rim),
    every combination per axis of: the lower centre, the midpoint of the pair, and the fp32 neighbours of the midpoint on
    either side -- axis midpoints, face midpoints and the body midpoint of 8 cells among them: [192, 3] fp32."""
    spacing = np.float32(1.0 / (res - 1))
    out = []
    for b in (0, (res - 1) // 2, res - 2):
        centre = np.float32(b) * spacing - np.float32(0.5)
        mid = np.float32(b + 0.5) * spacing - np.float32(0.5)
        assert float(mid) == (b + 0.5) / (res - 1) - 0.5 and float(centre) == b / (res - 1) - 0.5      # exact in fp32
        values = np.array([centre, mid, np.nextafter(mid, np.float32(-1)), np.nextafter(mid, np.float32(1))], np.float32)
        out.append(np.stack(np.meshgrid(values, values, values, indexing="ij"), axis=-1).reshape(-1, 3))
    return np.concatenate(out).astype(np.float32)


def boundary_cells(res):
    """(centres [6,3] fp32, linear indices [6]) of the six cells with a0^2 + a1^2 + a2^2 == (res - 1)^2."""
    a = 2 * np.arange(res) - (res - 1)
    a2 = a * a
    on = np.argwhere(a2[:, None, None] + a2[None, :, None] + a2[None, None, :] == (res - 1) ** 2)
    assert len(on) == 6
    centres = (on / (res - 1) - 0.5).astype(np.float32)
    return centres, (on[:, 0] * res + on[:, 1]) * res + on[:, 2]


def zero_points():
    """res = 28, where 0 is a midpoint: +-0.0, +-1e-30 and +-1.4e-45 (the smallest subnormal) on each axis, the other two
    coordinates at a cell centre's 0.1: ([18,3] fp32, the expected index along the axis [18], the axis [18])."""
    values = np.array([0.0, -0.0, 1e-30, -1e-30, 1.4e-45, -1.4e-45], np.float32)
    assert values[4] > 0 and values[5] < 0
    want = [13, 13, 14, 13, 14, 13]
    pts, index, axes = [], [], []
    for axis in range(3):
        for v, w in zip(values, want):
            p = np.full(3, 0.1, np.float32)
            p[axis] = v
            pts.append(p), index.append(w), axes.append(axis)
    return np.array(pts, np.float32), np.array(index), np.array(axes)


FAR = np.array([[10, 0, 0], [-10, 0, 0], [0, 10, -10], [1e30, 0, 0], [0, -1e30, 1e30], [1e30, 1e30, 1e30],
                [3.4028234663852886e38, 0, 0], [-3.4028234663852886e38, 3.4028234663852886e38, 3.4028234663852886e38],
                [0.1, 0.2, -0.3], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan],
                [np.inf, -np.inf, np.nan], [0.25, -0.25, 0.0]], np.float32)
FAR_FINITE = 10


@functools.lru_cache(maxsize=None)
def case(name):
    """(xyz [S,n,3] fp32, res, in_sphere, lengths or None) of a named set."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if name in ("ball28", "ball32", "ball28cube"):
        return _frozen(ball(rng, 3, 257)), 32 if name == "ball32" else 28, name != "ball28cube", None
    if name in ("cube5", "cube28"):
        x = ((rng.random((2, 257, 3)) - 0.5) * 1.3).astype(np.float32)
        corners = np.array([[a, b, c] for a in (-0.5, 0.5) for b in (-0.5, 0.5) for c in (-0.5, 0.5)], np.float32)
        x = np.concatenate([x, np.broadcast_to(corners, (2, 8, 3))], axis=1)
        return _frozen(np.ascontiguousarray(x)), 5 if name == "cube5" else 28, True, None
    if name.startswith("mid"):      # mid3, mid5, mid9, mid17: with the sphere; the cube is run on the same points too
        res = int(name[3:])
        x = np.concatenate([midpoint_points(res), boundary_cells(res)[0]])[None]
        return _frozen(np.ascontiguousarray(x)), res, True, None
    if name == "far":
        return _frozen(FAR[None].copy()), 28, True, None
    if name == "onecell":      # 257 points of one cell (a centre of the res 28 grid and points within a quarter spacing)
        centre = np.array([14, 15, 12]) / 27.0 - 0.5
        x = (centre + (rng.random((257, 3)) - 0.5) / 54.0).astype(np.float32)
        return _frozen(np.ascontiguousarray(np.broadcast_to(x, (3, 257, 3)))), 28, True, None
    if name == "ragged":
        x = ball(rng, 3, 257)
        x[0, :] = np.nan
        x[1, 1:] = np.float32(3e38)      # padding rows: NaN in one cloud, huge finite values in another
        return _frozen(x), 28, True, (0, 1, 257)
    if name == "band":      # 0 .. 4 spacings outside the sphere: the nearest in-sphere centre is 0 .. 8 half spacings away,
        v = rng.standard_normal((2, 257, 3))      # on both sides of the 5 a bounded search around the cube cell may stop at
        v /= np.linalg.norm(v, axis=2, keepdims=True)
        return _frozen((v * (0.5 + rng.random((2, 257, 1)) * 4.0 / 27.0)).astype(np.float32)), 28, True, None
    if name == "limit5":      # res 5, u = (7, 4, 0): the cube cell (4, 4, 0) is clipped, the nearest in-sphere centre
        pts = []      # (4, 0, 0) is EXACTLY 5 half spacings away (D = 9 + 16): every axis pair and sign, and the fp32 neighbours
        for far in range(3):
            for mid in (a for a in range(3) if a != far):
                for sf in (1.0, -1.0):
                    for sm in (1.0, -1.0):
                        for nudge in (0, -1, 1):
                            p = np.zeros(3, np.float32)
                            p[far] = np.float32(0.875 * sf) if nudge == 0 else np.nextafter(np.float32(0.875 * sf), np.float32(2 * nudge))
                            p[mid] = np.float32(0.5 * sm)
                            pts.append(p)
        return _frozen(np.array(pts, np.float32)[None]), 5, True, None
    if name == "single":
        return _frozen(ball(rng, 1, 300)), 28, True, None
    if name == "many":      # more clouds than any launch has workgroups: every workgroup loops
        return _frozen(ball(rng, 700, 64)), 28, True, None
    if name == "wide":      # three chunks of a workgroup, the last with one point
        return _frozen(ball(rng, 2, 2049)), 28, True, None
    raise KeyError(name)


CLOUD_CASES = ["ball28", "ball32", "ball28cube", "cube5", "cube28", "mid3", "mid5", "mid9", "mid17", "far", "onecell",
               "ragged", "single", "many", "wide", "band", "limit5"]


@functools.lru_cache(maxsize=None)
def reference(name, in_sphere=None):
    xyz, res, sphere, lengths = case(name)
    out = ref.occupancy_grid(xyz, res, sphere if in_sphere is None else in_sphere, lengths)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------- running
def run(xyz, res, in_sphere, device, lengths=None):
    """occupancy_grid on `device`: dict(counts [res^3] int64, occupied [res^3] int32, cells [S,n] int32) as NumPy."""
    import torch

    from sparenet_amd.cuda.occupancy import occupancy_grid

    counts, occupied, cells = occupancy_grid(torch.tensor(np.asarray(xyz), device=device), res, in_sphere,
                                             None if lengths is None else list(lengths), return_cells=True)
    assert counts.dtype == torch.int64 and occupied.dtype == torch.int32 and cells.dtype == torch.int32
    assert tuple(counts.shape) == (res, res, res) and tuple(occupied.shape) == (res, res, res)
    assert not (counts.requires_grad or occupied.requires_grad or cells.requires_grad)
    return {"counts": counts.cpu().numpy().reshape(-1), "occupied": occupied.cpu().numpy().reshape(-1),
            "cells": cells.cpu().numpy()}


def run_raw(xyz, res, in_sphere, device, want, lengths=None):
    """The entry point itself with only the outputs named in `want` (the others are null pointers)."""
    import torch

    from sparenet_amd import _lib

    x = torch.tensor(np.asarray(xyz), device=device)
    s, n = x.shape[:2]
    out = {"counts": torch.full((res ** 3,), -7, dtype=torch.int64, device=device) if "counts" in want else None,
           "occupied": torch.full((res ** 3,), -7, dtype=torch.int32, device=device) if "occupied" in want else None,
           "cells": torch.full((s, n), -7, dtype=torch.int32, device=device) if "cells" in want else None}
    lens = None if lengths is None else torch.tensor(list(lengths), dtype=torch.int32, device=device)
    args = (x, lens, s, n, res, int(in_sphere), out["counts"], out["occupied"], out["cells"])
    if x.is_cuda:
        ws = _lib.op_workspace("occupancy", "sn_occupancy_grid_workspace_bytes", x, s, n, res, int(in_sphere))
        _lib.op_call("occupancy", "sn_occupancy_grid", *args, ws)
    else:
        _lib.op_call("occupancy", "sn_occupancy_grid_host", *args, 3, host=True)
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("counts", "occupied", "cells"))


# ---------------------------------------------------------------------------------------------------- checking
def check(out, xyz, res, in_sphere, want, lengths, label):
    """Exact equality with the reference, and the invariants of every case."""
    s, n = xyz.shape[:2]
    mismatch = int((out["cells"] != want["cells"]).sum())
    print(f"{label}: S {s} n {n} res {res} in_sphere {int(bool(in_sphere))}: {int(want['counts'].sum())} points counted, "
          f"Rule 2 decided {100 * want['rule2']:.2f} %; cells that differ from the reference: {mismatch}")
    assert mismatch == 0, f"{label}: {mismatch} cells differ from the reference"
    assert np.array_equal(out["counts"], want["counts"]), f"{label}: counts"
    assert np.array_equal(out["occupied"], want["occupied"]), f"{label}: occupied"
    assert np.array_equal(out["occupied"] > 0, out["counts"] > 0), f"{label}: occupied > 0 exactly where counts > 0"
    assert out["occupied"].max() <= s and out["occupied"].min() >= 0
    if in_sphere:
        outside = ~ref.sphere_mask(res).reshape(-1)
        assert (out["counts"][outside] == 0).all() and (out["occupied"][outside] == 0).all(), f"{label}: outside the sphere"
    cells = out["cells"]
    assert np.array_equal(out["counts"], np.bincount(cells[cells >= 0], minlength=res ** 3)), f"{label}: bincount"
    valid = np.arange(n)[None, :] < np.asarray([n] * s if lengths is None else lengths)[:, None]
    finite = np.isfinite(xyz).all(axis=2) & valid
    assert np.array_equal(cells >= 0, finite) and (cells[~finite] == -1).all(), f"{label}: -1 exactly at padding / non-finite"


def check_case(name, device, in_sphere=None):
    xyz, res, sphere, lengths = case(name)
    sphere = sphere if in_sphere is None else in_sphere
    out = run(xyz, res, sphere, device, lengths)
    check(out, xyz, res, sphere, reference(name, in_sphere), lengths, f"{name} on {device}")
    assert same(run(xyz, res, sphere, device, lengths), out), f"{name}: a second call differs"
    return out


def check_case_details(name, device, out):
    """What a named case promises beyond the reference."""
    xyz, res, _, lengths = case(name)
    if name.startswith("mid"):
        # the same points on the whole cube; there the six boundary cells and every midpoint rule can be read off
        cube = check_case(name, device, in_sphere=False)
        centres, index = boundary_cells(res)
        for o in (out, cube):
            assert np.array_equal(o["cells"][0, -6:], index), f"{name}: a boundary-equality cell did not take its own centre"
        assert (out["counts"][index] >= 1).all()
        pts = xyz[0, :-6].astype(np.float64) * (res - 1) + 0.5 * (res - 1)      # in units of the spacing: exact
        lower = np.ceil(pts - 0.5).astype(np.int64)      # a midpoint (x.5) goes down
        assert np.array_equal(cube["cells"][0, :-6], (lower[:, 0] * res + lower[:, 1]) * res + lower[:, 2])
        assert int((pts - np.floor(pts) == 0.5).sum()) >= 3 * 16 * 3, "the case must hold exact midpoints"
    if name == "limit5":
        exact = xyz[0, ::3]
        ijk = np.full((len(exact), 3), 2)
        far = np.abs(exact).argmax(axis=1)
        ijk[np.arange(len(exact)), far] = np.where(exact[np.arange(len(exact)), far] > 0, 4, 0)
        assert np.array_equal(out["cells"][0, ::3], (ijk[:, 0] * 5 + ijk[:, 1]) * 5 + ijk[:, 2]), "D = 25 exactly"
    if name == "far":
        assert (out["cells"][0, FAR_FINITE - 1:FAR_FINITE + 4] == -1).all() and out["cells"][0, -1] >= 0
        assert int(out["counts"].sum()) == FAR_FINITE == int(np.isfinite(FAR).all(axis=1).sum())
        lowest = int(np.flatnonzero(ref.sphere_mask(res).reshape(-1))[0])
        assert out["cells"][0, 5] == lowest, "(1e30, 1e30, 1e30): every D rounds alike, the lowest in-sphere cell wins"
    if name == "onecell":
        cell = (14 * 28 + 15) * 28 + 12
        assert out["counts"][cell] == 3 * 257 and out["occupied"][cell] == 3 and int(out["counts"].sum()) == 3 * 257
        one = run(xyz[:1], res, True, device)
        assert one["counts"][cell] == 257 and one["occupied"][cell] == 1 and int(one["occupied"].sum()) == 1
    if name == "ragged":
        assert (out["cells"][0] == -1).all() and (out["cells"][1, 1:] == -1).all()
        compact = run(xyz[2:], res, True, device)
        alone = run(xyz[1:2, :1], res, True, device)
        assert np.array_equal(out["counts"], compact["counts"] + alone["counts"])
        assert np.array_equal(out["occupied"], compact["occupied"] + alone["occupied"])
        assert np.array_equal(out["cells"][2], compact["cells"][0]) and out["cells"][1, 0] == alone["cells"][0, 0]


def check_zero_points(device):
    pts, index, axes = zero_points()
    for sphere in (True, False):
        out = run(pts[None], 28, sphere, device)
        check(out, pts[None], 28, sphere, ref.occupancy_grid(pts[None], 28, sphere), None, f"zeros on {device}")
        ijk = np.stack(np.unravel_index(out["cells"][0], (28, 28, 28)), axis=1)
        got = ijk[np.arange(len(pts)), axes]
        assert np.array_equal(got, index), f"x = 0 is a midpoint at res 28: expected {index.tolist()}, got {got.tolist()}"


def check_permutation(name, device):
    xyz, res, sphere, _ = case(name)
    out = run(xyz, res, sphere, device)
    order = np.random.default_rng(5).permutation(len(xyz))
    shuffled = run(np.ascontiguousarray(xyz[order]), res, sphere, device)
    assert np.array_equal(out["counts"], shuffled["counts"]) and np.array_equal(out["occupied"], shuffled["occupied"])
    assert np.array_equal(out["cells"][order], shuffled["cells"])


def check_null_outputs(device):
    xyz, res, sphere, _ = case("ball28")
    full = run(xyz, res, sphere, device)
    for want in (("cells",), ("counts",), ("occupied",), ("counts", "occupied")):
        got = run_raw(xyz, res, sphere, device, want)
        assert sorted(got) == sorted(want)
        for k in want:
            assert np.array_equal(got[k], full[k]), f"{k} alone"
    xyz, res, sphere, lengths = case("ragged")
    got = run_raw(xyz, res, sphere, device, ("counts", "occupied", "cells"), lengths)
    assert same(got, run(xyz, res, sphere, device, lengths))


def with_blocks(blocks, fn):
    """fn() with the device launch held to `blocks` workgroups (SN_OCCUPANCY_BLOCKS)."""
    old = os.environ.get("SN_OCCUPANCY_BLOCKS")
    os.environ["SN_OCCUPANCY_BLOCKS"] = str(blocks)
    try:
        return fn()
    finally:
        if old is None:
            del os.environ["SN_OCCUPANCY_BLOCKS"]
        else:
            os.environ["SN_OCCUPANCY_BLOCKS"] = old
