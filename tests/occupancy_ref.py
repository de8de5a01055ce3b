"""NumPy restatement of include/ops/occupancy.h -- the reference of tests/test_occupancy.py and
tests/test_occupancy_gpu.py -- and of the Jensen-Shannon divergence and occupancy entropy of
sparenet_amd/utils/set_metrics.py.  Written from the header's text; it does not call the library."""
import functools

import numpy as np


@functools.lru_cache(maxsize=None)
def sphere_mask(res):
    """[res,res,res] bool: a0^2 + a1^2 + a2^2 <= (res - 1)^2 with a = 2 i - (res - 1), in integers."""
    a = 2 * np.arange(res, dtype=np.int64) - (res - 1)
    a2 = a * a
    mask = a2[:, None, None] + a2[None, :, None] + a2[None, None, :] <= (res - 1) ** 2
    mask.setflags(write=False)
    return mask


@functools.lru_cache(maxsize=None)
def sphere_centres(res):
    """(linear indices [K] ascending, a [K,3] float64) of the cells in the sphere."""
    index = np.flatnonzero(sphere_mask(res).reshape(-1))
    ijk = np.stack(np.unravel_index(index, (res, res, res)), axis=1)
    a = (2 * ijk - (res - 1)).astype(np.float64)
    index.setflags(write=False), a.setflags(write=False)
    return index, a


def axis_index(u, res):
    """Rule 1: the number of midpoints 2 j + 2 - res, j = 0 .. res - 2, strictly below u (float64, compared exactly)."""
    mids = (2 * np.arange(res - 1, dtype=np.int64) + 2 - res).astype(np.float64)
    return (u[:, None] > mids[None, :]).sum(axis=1)


def cells_of(points, res, in_sphere, chunk=128):
    """points [m,3] fp32 -> (cells [m] int32, took_rule_2 [m] bool); -1 at non-finite points."""
    assert points.dtype == np.float32 and points.ndim == 2 and points.shape[1] == 3
    finite = np.isfinite(points).all(axis=1)
    u = np.where(finite[:, None], points, np.float32(0)).astype(np.float64) * np.float64(2 * (res - 1))
    ijk = [axis_index(u[:, axis], res) for axis in range(3)]
    cells = (ijk[0] * res + ijk[1]) * res + ijk[2]
    rule2 = np.zeros(len(points), bool)
    if in_sphere:
        rule2 = finite & ~sphere_mask(res)[ijk[0], ijk[1], ijk[2]]
        index, a = sphere_centres(res)
        rows = np.flatnonzero(rule2)
        for start in range(0, len(rows), chunk):
            r = rows[start:start + chunk]
            d0 = u[r, 0][:, None] - a[None, :, 0]
            d1 = u[r, 1][:, None] - a[None, :, 1]
            d2 = u[r, 2][:, None] - a[None, :, 2]
            D = (d0 * d0 + d1 * d1) + d2 * d2      # every product and sum a separately rounded float64 operation
            cells[r] = index[np.argmin(D, axis=1)]      # argmin: the first of equal minima, the lowest linear index
    return np.where(finite, cells, -1).astype(np.int32), rule2


def occupancy_grid(xyz, res, in_sphere, lengths=None):
    """xyz [S,n,3] fp32 -> dict(counts [res^3] int64, occupied [res^3] int32, cells [S,n] int32, rule2: the share of the
    counted points Rule 2 decided)."""
    s, n = xyz.shape[:2]
    lengths = [n] * s if lengths is None else list(lengths)
    counts = np.zeros(res ** 3, np.int64)
    occupied = np.zeros(res ** 3, np.int32)
    cells = np.full((s, n), -1, np.int32)
    slow = 0
    for c in range(s):
        got, rule2 = cells_of(np.ascontiguousarray(xyz[c, :lengths[c]]), res, in_sphere)
        cells[c, :lengths[c]] = got
        per_cloud = np.bincount(got[got >= 0], minlength=res ** 3)
        counts += per_cloud
        occupied += per_cloud > 0
        slow += int(rule2.sum())
    return {"counts": counts, "occupied": occupied, "cells": cells, "rule2": slow / max(int(counts.sum()), 1)}


def brute_force_cells(points, res):
    """The nearest in-sphere CENTRE in plain float64 (centres as published: i * spacing - 0.5), lowest index among equal
    distances: what Rule 1 + Rule 2 must agree with wherever the nearest centre is unique in float64."""
    index, _ = sphere_centres(res)
    ijk = np.stack(np.unravel_index(index, (res, res, res)), axis=1)
    centres = ijk * (1.0 / (res - 1)) - 0.5
    p = points.astype(np.float64)
    d = ((p[:, None, :] - centres[None, :, :]) ** 2).sum(axis=2)
    best = d.min(axis=1)
    unique = (d <= best[:, None] * (1 + 1e-9) + 1e-18).sum(axis=1) == 1
    return index[np.argmin(d, axis=1)].astype(np.int32), unique


# ---------------------------------------------------------------------------------------------------- metrics
def entropy_bits(x):
    x = x[x > 0]
    return -(x * np.log2(x)).sum()


def jsd(p_counts, q_counts):
    """Jensen-Shannon divergence in bits of two count grids, float64 NumPy."""
    p = p_counts.astype(np.float64).reshape(-1)
    q = q_counts.astype(np.float64).reshape(-1)
    p, q = p / p.sum(), q / q.sum()
    return entropy_bits((p + q) / 2) - (entropy_bits(p) + entropy_bits(q)) / 2


def jsd_terms(p_counts, q_counts):
    """(K, A): the number of non-empty cells of the mixture and sum |x log2 x| over the three entropies' terms."""
    p = p_counts.astype(np.float64).reshape(-1)
    q = q_counts.astype(np.float64).reshape(-1)
    p, q = p / p.sum(), q / q.sum()
    m = (p + q) / 2
    mag = lambda x: np.abs(x[x > 0] * np.log2(x[x > 0])).sum()      # noqa: E731
    return int((m > 0).sum()), mag(m) + (mag(p) + mag(q)) / 2


def occupancy_entropy(occupied, n_clouds, n_cells):
    """The published acc_entropy: sum over cells of the entropy (natural log) of Bernoulli(g / n_clouds), over n_cells."""
    total = 0.0
    for g in occupied.reshape(-1).tolist():
        if 0 < g < n_clouds:
            p = g / n_clouds
            total += -(p * np.log(p) + (1 - p) * np.log(1 - p))
    return total / n_cells
