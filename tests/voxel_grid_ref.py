"""include/ops/voxel_grid.h restated in NumPy float64, sentence by sentence, one cloud at a time: the cell rule in
element-wise array operations, the sort, the voxels and every sum in plain loops.  np.float64 (and a Python float)
arithmetic is IEEE double with every operation rounded separately and the division correctly rounded, which is what the
header asks for; nothing here shares code with the library."""
import numpy as np

CELL_MIN, CELL_MAX = -32768, 32767


def keys_of(xyz, size, origin):
    """The keys of the fp32 points xyz [m, 3] as Python ints, None where a point belongs to no voxel.  Element-wise
    NumPy float64 operations: each one rounded separately, the division correctly rounded."""
    with np.errstate(invalid="ignore", over="ignore"):
        q = (xyz.astype(np.float64) - origin.astype(np.float64)) / np.float64(size)
        c = np.floor(q)                                  # the ROUNDED quotient decides; -0.0 -> cell 0
    inside = np.isfinite(xyz).all(axis=1) & ((c >= CELL_MIN) & (c <= CELL_MAX)).all(axis=1)
    keys = []
    for ok, cell in zip(inside.tolist(), c.tolist()):
        cx, cy, cz = (int(v) for v in cell) if ok else (0, 0, 0)
        keys.append(((cx + 32768) << 32) | ((cy + 32768) << 16) | (cz + 32768) if ok else None)
    return keys


def voxel_grid_cloud(xyz, length, size, origin, cap):
    """One cloud xyz [n, 3] fp32 of `length` points -> dict of the header's outputs at width `cap`."""
    n = xyz.shape[0]
    length = min(max(int(length), 0), n)
    size, origin = np.float32(size), np.asarray(origin, np.float32)
    keyed = sorted((key, i) for i, key in enumerate(keys_of(xyz[:length], size, origin)) if key is not None)
    voxels = []                                 # [start, end] into keyed: ascending key, then ascending point index
    for r, (key, _) in enumerate(keyed):
        if r == 0 or key != keyed[r - 1][0]:
            voxels.append([r, r + 1])
        else:
            voxels[-1][1] = r + 1
    count, kept = len(voxels), min(len(voxels), cap)
    out = {"count": np.int32(count), "centroid": np.zeros((cap, 3), np.float32), "members": np.zeros(cap, np.int32),
           "first": np.full(cap, -1, np.int32), "inverse": np.full(n, -1, np.int32), "order": np.full(n, -1, np.int32),
           "start": np.zeros(cap + 1, np.int32)}
    out["order"][:len(keyed)] = [i for _, i in keyed]
    wide = xyz.astype(np.float64).tolist()      # Python floats are IEEE doubles: (double)x, exactly
    for k in range(kept):
        s, e = voxels[k]
        total = [0.0, 0.0, 0.0]
        for r in range(s, e):                   # ascending point index, one addition at a time
            i = keyed[r][1]
            out["inverse"][i] = k
            total = [total[axis] + wide[i][axis] for axis in range(3)]
        out["centroid"][k] = np.array([t / float(e - s) for t in total], np.float64).astype(np.float32)   # rounded once
        out["members"][k], out["first"][k], out["start"][k] = e - s, keyed[s][1], s
    out["start"][kept:] = voxels[kept - 1][1] if kept else 0
    return out


def voxel_grid(xyz, size, origin=None, lengths=None, cap=None):
    """The batch xyz [b, n, 3] -> dict of stacked outputs."""
    xyz = np.asarray(xyz, np.float32)
    b, n = xyz.shape[:2]
    origin = (0.0, 0.0, 0.0) if origin is None else origin
    cap = n if cap is None else cap
    rows = [voxel_grid_cloud(xyz[i], n if lengths is None else lengths[i], size, origin, cap) for i in range(b)]
    return {name: np.stack([row[name] for row in rows]) for name in rows[0]}


def voxel_pool(features, grid, mode):
    """features [b, c, n] fp32 pooled over `grid` (a dict of voxel_grid) -> (out [b, c, cap] fp32, argmax int32)."""
    features = np.asarray(features, np.float32)
    b, c, n = features.shape
    cap = grid["start"].shape[1] - 1
    out, argmax = np.zeros((b, c, cap), np.float32), np.full((b, c, cap), -1, np.int32)
    for i in range(b):
        kept = min(int(grid["count"][i]), cap)
        for v in range(kept):
            s = min(max(int(grid["start"][i, v]), 0), n)                  # offsets are held to [0, n] ...
            e = max(min(max(int(grid["start"][i, v + 1]), 0), n), s)      # ... and an end below its start is empty
            members = [int(j) for j in grid["order"][i, s:e] if 0 <= j < n]
            for ch in range(c):
                row = features[i, ch]
                if not members:
                    continue
                if mode == "max":
                    best, best_j = row[members[0]], members[0]
                    for j in members[1:]:
                        if row[j] > best:
                            best, best_j = row[j], j
                    out[i, ch, v], argmax[i, ch, v] = best, best_j
                else:
                    total = np.float64(0.0)
                    for j in members:
                        total = total + np.float64(row[j])
                    if mode == "mean":
                        total = total / np.float64(len(members))
                    out[i, ch, v] = np.float32(total)
    return out, argmax
