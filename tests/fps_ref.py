"""NumPy restatement of the farthest point sampling rule of include/ops/fps.h -- the reference of tests/test_fps.py and
tests/test_fps_gpu.py.  Every array is fp32 and every product and sum is rounded separately (NumPy never contracts),
np.argmax returns the first maximum = the lowest index, and overflow to +inf is an ordinary value."""
import numpy as np


def fps_ref(xyz, m, length=None, start=0):
    """(idx [m] int32, min_dist [m] fp32) of one cloud xyz [N,3]; only its first `length` rows are points."""
    xyz = np.asarray(xyz, dtype=np.float32)
    n = xyz.shape[0] if length is None else int(length)
    idx = np.full(m, -1, np.int32)
    min_dist = np.full(m, np.nan, np.float32)
    if n == 0:
        return idx, min_dist
    x, y, z = (np.ascontiguousarray(xyz[:n, a]) for a in range(3))
    mind = np.full(n, np.inf, np.float32)
    c = int(start)
    assert 0 <= c < n
    with np.errstate(all="ignore"):
        for k in range(m):
            idx[k] = c
            min_dist[k] = mind[c]
            dx, dy, dz = x - x[c], y - y[c], z - z[c]
            d = ((dx * dx) + (dy * dy)) + (dz * dz)
            mind = np.where(d < mind, d, mind)
            c = int(np.argmax(mind))
    return idx, min_dist


def fps_ref_batch(xyz, m, lengths=None, start=None):
    """(idx [B,m] int32, min_dist [B,m] fp32) of a batch xyz [B,N,3], cloud by cloud."""
    b = xyz.shape[0]
    rows = [fps_ref(xyz[i], m, None if lengths is None else lengths[i], 0 if start is None else start[i])
            for i in range(b)]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


def same_bits(a, b):
    """True when two fp32 arrays hold the same bit patterns (NaN payloads and the sign of zero included)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def lattice_cloud():
    """A shuffled 8 x 8 x 8 integer lattice: every distance is an exact small integer, so almost every pick is a tie."""
    g = np.stack(np.meshgrid(*[np.arange(8)] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    return g[np.random.default_rng(11).permutation(512)]


def overflow_cloud():
    """64 points scaled by 1e20 and at least 0.2e20 apart along an axis: every squared distance between two of them is
    beyond fp32 (3.4e38) and rounds to +inf, their coordinates and differences stay finite."""
    rng = np.random.default_rng(3)
    g = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)[rng.permutation(64)]
    return ((g * 0.25 + rng.random((64, 3)) * 0.05 - 0.5) * 1e20).astype(np.float32)
