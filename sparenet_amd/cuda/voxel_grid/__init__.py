"""Voxel-grid subsampling and pooling, backed by sn_voxel_grid / sn_voxel_pool (include/ops/voxel_grid.h states the
rules; sparenet_amd/csrc/voxel_grid.hip).

    voxel_grid(xyz [B,N,3], size, origin=None, lengths=None, max_voxels=None)
        -> VoxelGrid(centroids [B,V,3], count [B], members [B,V], first [B,V], inverse [B,N], order [B,N], start [B,V+1])
    grid_subsample(xyz, size, mode="centroid" | "first", origin=None, lengths=None, max_voxels=None)
        -> (points [B,V,3], count [B])
    voxel_pool(features [B,C,N], grid, reduce="mean" | "max" | "sum") -> [B,C,V]
    GridPool(size, reduce="mean", origin=None, max_voxels=None)(xyz, features)
        -> (points [B,V,3], pooled [B,C,V], count [B], inverse [B,N])

A point goes to the cell floor((x - origin) / size) per axis (in double, the rounded quotient decides); every occupied
cell is a voxel, the voxels of a cloud are ordered by cell (x slowest) and the points of a voxel by index.  V is
`max_voxels`, or N when it is None; `count` is the number of occupied voxels and is NOT clipped to V, so
`(count > V).any()` tells a caller that voxels were dropped.  Rows at and beyond min(count, V) are 0 (members 0, first
-1).  `inverse` is the row each point went to: -1 for padding rows, for points with a NaN or infinite coordinate or a
cell outside 16 bits per axis, and for points of a dropped voxel.  `lengths` makes the batch ragged as in
sparenet_amd.cuda.ragged.  All results are bit-identical from call to call, and CPU tensors (the library's host entry
points) give the device's bits.

`centroids` is differentiable in xyz (each member gets grad / members), `voxel_pool` in the features (mean, sum: a
gather through `inverse`; max: the gradient goes to the winning point, the lowest index among equals); both backward
passes are deterministic and make no library call.
"""
import collections
import ctypes
import math

import torch
from torch import nn
from torch.autograd import Function

from sparenet_amd import _lib
from sparenet_amd.cuda import _args

VoxelGrid = collections.namedtuple("VoxelGrid", "centroids count members first inverse order start")
REDUCTIONS = {"sum": 0, "mean": 1, "max": 2}      # the modes of sn_voxel_pool


def _host_origin(what, origin):
    """None, or the three finite floats of `origin` as the host array the entry points read."""
    if origin is None:
        return None
    if isinstance(origin, torch.Tensor):
        if origin.is_cuda:      # the entry points read it on the host: no device read here
            raise ValueError(f"{what}: origin is read on the host: pass three numbers or a CPU tensor")
        origin = origin.tolist()
    values = [float(v) for v in origin]
    if len(values) != 3 or not all(math.isfinite(v) for v in values):
        raise ValueError(f"{what}: origin must be three finite numbers, got {origin!r}")
    return (ctypes.c_float * 3)(*values)


def _check_size(what, size):
    if isinstance(size, (bool, torch.Tensor)) or not isinstance(size, (int, float)) or not math.isfinite(size) \
            or not size > 0:
        raise ValueError(f"{what}: size must be a finite number > 0, got {size!r}")
    return float(size)


def _gather_rows(rows, inverse):
    """rows [B, V, K] gathered at inverse [B, N] -> [B, N, K]; 0 where inverse < 0."""
    picked = rows.gather(1, inverse.clamp_min(0).long()[:, :, None].expand(-1, -1, rows.size(2)))
    return torch.where((inverse >= 0)[:, :, None], picked, torch.zeros((), dtype=rows.dtype, device=rows.device))


class VoxelGridFunction(Function):
    @staticmethod
    def forward(ctx, xyz, size, origin, lengths, max_voxels):
        what = "voxel_grid"
        _args.check_cloud(what, "xyz", xyz)
        size = _check_size(what, size)
        origin = _host_origin(what, origin)
        b, n, dev = xyz.size(0), xyz.size(1), xyz.device
        cap = n if max_voxels is None else _args.check_count(what, "max_voxels", max_voxels, top=n, refuse_bool=True)
        pts = _args.fp32(xyz)
        lens = _args.optional_lengths(lengths, b, n, dev, "lengths")
        count = torch.empty(b, dtype=torch.int32, device=dev)
        centroid = torch.empty(b, cap, 3, device=dev)
        members, first = (torch.empty(b, cap, dtype=torch.int32, device=dev) for _ in range(2))
        inverse, order = (torch.empty(b, n, dtype=torch.int32, device=dev) for _ in range(2))
        start = torch.empty(b, cap + 1, dtype=torch.int32, device=dev)
        args = (pts, lens, b, n, size, origin, cap, count, centroid, members, first, inverse, order, start)
        if pts.is_cuda:
            ws = _lib.op_workspace("voxel_grid", "sn_voxel_grid_workspace_bytes", pts, b, n)
            _lib.op_call("voxel_grid", "sn_voxel_grid", *args, ws)
        else:
            _lib.op_call("voxel_grid", "sn_voxel_grid_host", *args, 0, host=True)
        ctx.save_for_backward(inverse, members)
        ctx.mark_non_differentiable(count, members, first, inverse, order, start)
        return centroid, count, members, first, inverse, order, start

    @staticmethod
    def backward(ctx, grad, *_):
        inverse, members = ctx.saved_tensors
        share = grad / members.clamp_min(1).to(grad.dtype)[:, :, None]      # empty rows have no member to reach
        return _gather_rows(share, inverse), None, None, None, None


def voxel_grid(xyz, size, origin=None, lengths=None, max_voxels=None):
    """VoxelGrid(centroids, count, members, first, inverse, order, start) of xyz [B, N, 3] on the lattice of cell edge
    `size` through `origin` (see the module's text).  `order` and `start` are the voxels' member lists in CSR form:
    voxel k of cloud b is order[b, start[b, k] : start[b, k + 1]]."""
    return VoxelGrid(*VoxelGridFunction.apply(xyz, size, origin, lengths, max_voxels))


def grid_subsample(xyz, size, mode="centroid", origin=None, lengths=None, max_voxels=None):
    """(points [B, V, 3], count [B]): one point per occupied voxel -- its members' centroid, or with mode="first" its
    member of the lowest index, an input point -- in voxel order; rows at and beyond count are 0.  Differentiable in
    xyz.  With `count` as lengths the result goes straight into the ragged operators:

        from sparenet_amd.cuda.ragged import chamfer_ragged, masked_mean
        p, np_ = grid_subsample(pred, 0.05)
        g, ng = grid_subsample(gt, 0.05)
        d1, d2 = chamfer_ragged(p, g, np_, ng)          # count is not clipped: pass max_voxels=None, or clamp it
        loss = masked_mean(d1, np_).mean() + masked_mean(d2, ng).mean()
    """
    if mode not in ("centroid", "first"):
        raise ValueError(f"grid_subsample: mode must be 'centroid' or 'first', got {mode!r}")
    if mode == "centroid":
        grid = voxel_grid(xyz, size, origin, lengths, max_voxels)
        return grid.centroids, grid.count
    grid = voxel_grid(xyz.detach(), size, origin, lengths, max_voxels)
    rows = _gather_rows(xyz.float(), grid.first)      # first is -1 at the empty rows
    return rows, grid.count


class VoxelPoolFunction(Function):
    @staticmethod
    def forward(ctx, features, inverse, members, order, start, count, mode):
        b, c, n = features.shape
        cap = start.size(1) - 1
        feats = _args.fp32(features)
        out = torch.empty(b, c, cap, device=feats.device)
        argmax = torch.empty(b, c, cap, dtype=torch.int32, device=feats.device) if mode == REDUCTIONS["max"] else None
        args = (feats, b, c, n, order, start, count, cap, mode, out, argmax)
        if feats.is_cuda:
            _lib.op_call("voxel_grid", "sn_voxel_pool", *args)
        else:
            _lib.op_call("voxel_grid", "sn_voxel_pool_host", *args, 0, host=True)
        ctx.mode, ctx.n = mode, n
        ctx.save_for_backward(inverse, members, argmax)
        return out

    @staticmethod
    def backward(ctx, grad):
        inverse, members, argmax = ctx.saved_tensors
        if ctx.mode == REDUCTIONS["max"]:
            # every (cloud, channel, voxel) names a point of its own voxel: the indices of a row are unique, except -1,
            # which goes to a column that is cut off
            b, c, _ = grad.shape
            target = torch.where(argmax < 0, torch.full_like(argmax, ctx.n), argmax).long()
            wide = torch.zeros(b, c, ctx.n + 1, dtype=grad.dtype, device=grad.device)
            wide.scatter_(2, target, grad)
            return wide[:, :, :ctx.n].contiguous(), None, None, None, None, None, None
        if ctx.mode == REDUCTIONS["mean"]:
            grad = grad / members.clamp_min(1).to(grad.dtype)[:, None, :]
        out = _gather_rows(grad.transpose(1, 2), inverse).transpose(1, 2)
        return out.contiguous(), None, None, None, None, None, None


def voxel_pool(features, grid, reduce="mean"):
    """[B, C, V]: features [B, C, N] pooled over the voxels of `grid` (a VoxelGrid of the same clouds) -- the mean, the
    sum or the maximum of each voxel's members; 0 at the empty rows.  Differentiable in the features."""
    what = "voxel_pool"
    if reduce not in REDUCTIONS:
        raise ValueError(f"{what}: reduce must be one of {', '.join(sorted(REDUCTIONS))}, got {reduce!r}")
    if not isinstance(grid, VoxelGrid):
        raise TypeError(f"{what}: grid must be the VoxelGrid voxel_grid returns")
    if not isinstance(features, torch.Tensor) or features.dim() != 3 or features.size(1) == 0:
        raise ValueError(f"{what}: features must be a non-empty [B, C, N] tensor")
    if not features.is_floating_point():
        raise TypeError(f"{what}: features must be a floating-point tensor, got {features.dtype}")
    if (features.size(0), features.size(2)) != tuple(grid.inverse.shape):
        raise ValueError(f"{what}: features are [B, C, N] = {tuple(features.shape)}, the grid is of "
                         f"{tuple(grid.inverse.shape)} points")
    if features.device != grid.inverse.device:
        raise ValueError(f"{what}: features and grid are on different devices")
    return VoxelPoolFunction.apply(features, grid.inverse, grid.members, grid.order, grid.start, grid.count,
                                   REDUCTIONS[reduce])


class GridPool(nn.Module):
    """The grid pooling of a point network: (points [B,V,3], pooled [B,C,V], count [B], inverse [B,N]) of xyz [B,N,3]
    and features [B,C,N] -- the voxels' centroids and their members' pooled features.  `lengths` as in voxel_grid."""

    def __init__(self, size, reduce="mean", origin=None, max_voxels=None):
        super().__init__()
        if reduce not in REDUCTIONS:
            raise ValueError(f"GridPool: reduce must be one of {', '.join(sorted(REDUCTIONS))}, got {reduce!r}")
        self.size, self.reduce, self.origin, self.max_voxels = _check_size("GridPool", size), reduce, origin, max_voxels

    def forward(self, xyz, features, lengths=None):
        grid = voxel_grid(xyz, self.size, self.origin, lengths, self.max_voxels)
        return grid.centroids, voxel_pool(features, grid, self.reduce), grid.count, grid.inverse

    def extra_repr(self):
        return f"size={self.size}, reduce={self.reduce!r}, origin={self.origin}, max_voxels={self.max_voxels}"
