"""Input generators of the GRNet edge tests (TEST INFRASTRUCTURE): tests/test_grnet_edges.py runs the HIP kernels on
these inputs and tests/test_grnet_ref.py checks on the CPU that grnet_ref and oracle agree on exactly the same ones,
so a disagreement on the GPU is the kernel's.  NumPy only, deterministic; nothing here needs a GPU."""
import functools
import itertools

import numpy as np

import grnet_ref as R

LATTICE_HALF_SCALES = (2, 4)
CAP_BATCH, CAP_POINTS, CAP_SCALE = 3, 700001, 8          # 2,100,003 points: one more pass than cap * 256 threads
CAP_REVERSE_BATCH, CAP_REVERSE_SCALE = 3, 96             # 2,654,208 cells
CAP_EDGE = (2, 3, 3000, 20)                              # b, c, n, k: 360,000 elements (see the test's docstring)
CUBIC_SCALES, CUBIC_NS, CUBIC_CHANNELS = (5, 8), (1, 2, 3), (1, 3, 65, 130)
REVERSE_SCALES = (1, 2, 5, 32)
THRESHOLD = 1e-6
THRESHOLD_LEVELS = (0.5e-6, 0.9e-6, 1.1e-6, 2e-6)
THRESHOLD_CLEARANCE = 0.05                               # every 8-cell sum is at least 5 % away from 1e-6


def lattice_values(s):
    return [-s - 1.5, -s - 1, -s - 0.5, -s, -s + 0.25, -1, -0.5, -0.0, 0.0, 0.5, 1, s - 2, s - 1.5, s - 1, s - 0.5, s,
            s + 0.5]


@functools.lru_cache(None)
def lattice_batch(s):
    """[3, 4913, 3] fp32 in vertex units: sample 0 = the full product of the 17 values per axis, sample 1 = the same
    points reversed, sample 2 = 500 random interior points (all eight corners inside [-s, s - 1]) followed by zero
    rows (padding for the padded entry point; 4413 points on vertex 0 for the others)."""
    v = np.array(lattice_values(s), np.float32)
    pts = np.array(list(itertools.product(v, v, v)), np.float32)
    assert pts.shape == (4913, 3) and np.signbit(pts).any()
    rng = np.random.default_rng(100 + s)
    inner = np.zeros_like(pts)
    inner[:500] = (rng.random((500, 3)) * (2 * s - 1) - s).astype(np.float32)
    inner[:500] = np.clip(inner[:500], -s, np.nextafter(np.float32(s - 1), np.float32(0)))
    out = np.stack([pts, pts[::-1], inner])
    out.setflags(write=False)
    return out


def lattice_bounds(s, tighter):
    lo, hi = (-s + 1, s - 2) if tighter else (-s, s - 1)
    return (lo, hi, lo, hi, lo, hi)


def grad_like(shape, seed):
    return (np.random.default_rng(seed).random(shape) * 2 - 1).astype(np.float32)


PADDING_SCALE = 8
PADDING_ROWS = np.array([(0, 0, 0), (-0.0, 0, 0), (0.5, -0.5, 0), (0.25, 0.25, -0.5), (1e-30, -1e-30, 0),
                         (3e-4, -1e-4, -2e-4)], np.float32)


@functools.lru_cache(None)
def padding_batch():
    """([2, 206, 3] fp32 in module units [-1, 1), positions [2, 6] of the six special rows).  The 200 valid rows keep all
    eight corners inside the scale-8 grid, so every kept row carries one unit of weight."""
    rng = np.random.default_rng(7)
    out = np.zeros((2, 206, 3), np.float32)
    where = np.stack([np.sort(rng.choice(206, 6, replace=False)), np.array([0, 1, 100, 203, 204, 205])])
    for b in range(2):
        valid = np.setdiff1d(np.arange(206), where[b])
        out[b, valid] = (rng.random((200, 3)) * 1.6 - 0.9).astype(np.float32)
        out[b, where[b]] = PADDING_ROWS if b == 0 else PADDING_ROWS[::-1]
    out.setflags(write=False)
    return out, where


def dist_bounds(*clouds):
    """GriddingDistance's box: one vertex of margin around all (scaled) points of both clouds."""
    both = np.concatenate([c.reshape(-1, 3) for c in clouds])
    lo = np.floor(both.min(0)) - 1
    hi = np.ceil(both.max(0)) + 1
    return tuple(int(v) for v in (lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]))


@functools.lru_cache(None)
def cap_points():
    """[3, 700001, 3] fp32 in vertex units of a scale-8 grid, one in ten points up to half a cell outside it."""
    rng = np.random.default_rng(11)
    out = (rng.random((CAP_BATCH, CAP_POINTS, 3), np.float32) * np.float32(8.8) - np.float32(4.4)).astype(np.float32)
    out.setflags(write=False)
    return out


def cap_cubic_points():
    """The same points in the voxel units of a scale-8 volume."""
    return (cap_points() + np.float32(4)).astype(np.float32)


def _gridded(n, scale, b, seed):
    """What Gridding produces: a sparse fp32 grid [b, scale^3] of n random interior points per sample."""
    rng = np.random.default_rng(seed)
    s = scale // 2
    pt = (rng.random((b, n, 3)) * (2 * s - 1.5) - s + 0.25).astype(np.float32)
    return R.gridding(pt, s)["grid"].astype(np.float32)


@functools.lru_cache(None)
def cap_reverse_grid():
    g = _gridded(3000, CAP_REVERSE_SCALE, CAP_REVERSE_BATCH, 14)   # a seed that keeps the clearance
    g.setflags(write=False)
    return g


def cubic_points(scale, ns):
    """[2, 600, 3] fp32 in voxel units: 200 integer points (0 and scale - 1 included), 200 points up to ns + 1 cells outside
    a face (every face in turn, the other axes anywhere from outside to outside), 200 interior random points."""
    rng = np.random.default_rng(1000 * scale + ns)
    out = np.empty((2, 600, 3), np.float32)
    for b in range(2):
        ints = rng.integers(0, scale, (200, 3))
        ints[:8] = np.array(list(itertools.product((0, scale - 1), repeat=3)))
        far = rng.random((200, 3)) * (scale - 1 + 2 * (ns + 1)) - (ns + 1)
        beyond = rng.random(200) * (ns + 1)
        for i in range(200):
            axis, high = (i % 6) // 2, i % 2
            far[i, axis] = scale - 1 + beyond[i] if high else -beyond[i]
        out[b] = np.concatenate([ints, far, rng.random((200, 3)) * (scale - 1)]).astype(np.float32)
    return out


def cubic_feat(b, c, scale, seed):
    return np.random.default_rng(seed).random((b, c, scale, scale, scale), np.float32)


def cubic_one_cell_points():
    """[1, 600, 3]: every point strictly inside the cell [3, 4)^3 of a scale-8 volume."""
    return (3 + 0.01 + 0.98 * np.random.default_rng(5).random((1, 600, 3))).astype(np.float32)


def cubic_single_writer_points():
    """[1, 64, 3]: one point in every second cell of a scale-8 volume (ns = 1): no two points share a vertex."""
    c = np.array([0.5, 2.5, 4.5, 6.5], np.float32)
    return np.array(list(itertools.product(c, c, c)), np.float32)[None]


def _threshold_grid(scale, b):
    """Isolated vertices (even coordinates) carry one of the four levels; all others are zero, so every cell's 8-vertex sum
    is exactly one level (scale 2: 0.9e-6 in sample 0, 1.1e-6 in sample 1)."""
    g = np.zeros((b, scale, scale, scale), np.float32)
    ev = np.arange(0, scale, 2)
    x, y, z = np.meshgrid(ev, ev, ev, indexing="ij")
    for i in range(b):
        g[i, x, y, z] = np.array(THRESHOLD_LEVELS, np.float32)[(x // 2 + 3 * (y // 2) + 5 * (z // 2) + i + 1) % 4]
    return g.reshape(b, -1)


def _mixed_sign_grid(scale, b, seed):
    """Vertex (x, y, z) is the last vertex (raster order) of cell (x, y, z): choosing it fixes that cell's sum.  Every
    interior cell gets a sum of random sign with 0.15 <= |sum| <= 1; the vertices themselves grow well past that and
    cancel."""
    rng = np.random.default_rng(seed)
    g = rng.random((b, scale, scale, scale)) * 2 - 1
    for x in range(1, scale):
        for y in range(1, scale):
            for z in range(1, scale):
                target = (0.15 + 0.85 * rng.random(b)) * rng.choice((-1.0, 1.0), b)
                cell = g[:, x - 1:x + 1, y - 1:y + 1, z - 1:z + 1]
                g[:, x, y, z] = target - (cell.sum((1, 2, 3)) - g[:, x, y, z])
    return g.astype(np.float32).reshape(b, -1)


@functools.lru_cache(None)
def reverse_grids(scale):
    """{name: fp32 grid [2, scale^3]}.  sparse: 2,000 points gridded at scale 32, cropped around the centre for the smaller
    scales (Gridding itself takes even scales only)."""
    full = _gridded(2000, 32, 2, 18).reshape(2, 32, 32, 32)         # a seed that keeps the clearance
    o = 16 - scale // 2
    out = dict(sparse=np.ascontiguousarray(full[:, o:o + scale, o:o + scale, o:o + scale]).reshape(2, -1),
               threshold=_threshold_grid(scale, 2), mixed=_mixed_sign_grid(scale, 2, 19 + scale))
    for g in out.values():
        g.setflags(write=False)
    return out


def threshold_clearance(grid, scale, f=None):
    """The smallest relative distance of an interior cell's 8-vertex sum (float64 and the fp32 chain) from 1e-6.
    f: R.reverse_forward(grid, scale), if at hand."""
    f = f or R.reverse_forward(grid, scale)
    if not f["interior"].any():
        return np.inf
    m = np.broadcast_to(f["interior"][None], f["sum64"].shape)
    both = np.concatenate([f["sum64"][m], f["wsum"].astype(np.float64)[m]])
    return float(np.abs(both - THRESHOLD).min() / THRESHOLD)
