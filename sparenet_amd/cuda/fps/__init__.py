"""Exact farthest point sampling, backed by sn_fps (include/ops/fps.h states the rule; sparenet_amd/csrc/fps.hip).

    farthest_point_sample(xyz [B,N,3], npoint, lengths=None, start=0, return_min_dist=False)
        -> idx [B,npoint] int32 (, min_dist [B,npoint] fp32)
        pick 0 is `start`; every later pick is the lowest index among the points farthest (squared distance, fp32,
        separately rounded) from the picks so far.  min_dist[b,k] is pick k's distance to the earlier picks (+inf for
        pick 0).  npoint may exceed the cloud: the lowest index then repeats.  Not differentiable.
    furthest_point_sample = farthest_point_sample        the name PointNet++ code imports
    sample_points(xyz, npoint, lengths=None, start=0) -> [B,npoint,3], differentiable in xyz (gather_operation)

`lengths` makes the batch ragged as in sparenet_amd.cuda.ragged: the first lengths[b] rows of cloud b are its points,
the rest is never read into a result; an empty cloud's row is idx -1, min_dist NaN (sample_points: NaN).  `start` is an
int or B ints (list / tensor); host values are range-checked, a device tensor is used as it is (the kernel holds its
values to the cloud).  Two calls give identical bits, and a batch's row equals the one-cloud call on that cloud.
There is no host path: a CPU tensor raises SparenetHipError.
"""
import torch
from torch.autograd import Function

from sparenet_amd import _lib
from sparenet_amd.cuda import _args
from sparenet_amd.cuda.MDS.MDS_module import gather_operation
from sparenet_amd.cuda.ragged import device_lengths


def _device_start(start, b, host_lengths, n, dev):
    """int32 tensor [b] on dev, or None for the default 0.  Host values are checked against 0 <= start < max(len, 1)
    (len = n where the lengths are not known on the host); a device tensor is not read."""
    if isinstance(start, torch.Tensor):
        if start.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"start: expected an int, a list or an int32 / int64 tensor, got dtype {start.dtype}")
        if start.dim() != 1 or start.numel() != b:
            raise ValueError(f"start: expected {b} values, got shape {tuple(start.shape)}")
        if start.is_cuda:
            return start.to(device=dev, dtype=torch.int32).contiguous()
        host = [int(v) for v in start.tolist()]
    elif isinstance(start, (list, tuple)):
        host = [int(v) for v in start]
        if len(host) != b:
            raise ValueError(f"start: expected {b} values, got {len(host)}")
    else:
        if int(start) != start:
            raise TypeError(f"start: expected an integer, got {start!r}")
        host = [int(start)] * b
    for i, v in enumerate(host):
        width = max(host_lengths[i], 1) if host_lengths is not None else n
        if v < 0 or v >= width:
            raise ValueError(f"start: must be in [0, {width}) for cloud {i}, got {v}")
    if not any(host):
        return None
    return torch.tensor(host, dtype=torch.int32, device=dev)


class FarthestPointSampling(Function):
    @staticmethod
    def forward(ctx, xyz, npoint, lengths, start, return_min_dist):
        _args.check_cloud("farthest_point_sample", "xyz", xyz)
        npoint = _args.check_count("farthest_point_sample", "npoint", npoint)
        _lib.require_device(xyz, "xyz")      # CPU tensors are refused before anything is uploaded
        xyz = _args.fp32(xyz)
        b, n, dev = xyz.size(0), xyz.size(1), xyz.device
        lens, host_lengths = (None, None) if lengths is None else device_lengths(lengths, b, n, dev, "lengths")
        first = _device_start(start, b, host_lengths, n, dev)
        idx = torch.empty(b, npoint, device=dev, dtype=torch.int32)
        min_dist = torch.empty(b, npoint, device=dev) if return_min_dist else None
        ws = _lib.op_workspace("fps", "sn_fps_workspace_bytes", xyz, b, n)
        _lib.op_call("fps", "sn_fps", xyz, b, n, npoint, lens, first, idx, min_dist, ws)
        if return_min_dist:
            ctx.mark_non_differentiable(idx, min_dist)
            return idx, min_dist
        ctx.mark_non_differentiable(idx)
        return idx

    @staticmethod
    def backward(ctx, *grads):
        return None, None, None, None, None


def farthest_point_sample(xyz, npoint, lengths=None, start=0, return_min_dist=False):
    """idx [B, npoint] int32 -- and min_dist [B, npoint] fp32 with return_min_dist -- of the exact farthest point
    sampling of each cloud of xyz [B, N, 3] (see the module's text)."""
    return FarthestPointSampling.apply(xyz, npoint, lengths, start, bool(return_min_dist))


furthest_point_sample = farthest_point_sample


def sample_points(xyz, npoint, lengths=None, start=0):
    """xyz [B, N, 3] -> its npoint farthest-point samples [B, npoint, 3] in pick order; gradients flow to the picked
    rows of xyz (a row picked several times collects every copy's gradient)."""
    idx = farthest_point_sample(xyz.detach(), npoint, lengths, start)
    picked = gather_operation(xyz.transpose(1, 2).contiguous(), idx)      # [B, 3, npoint]
    return picked.transpose(1, 2).contiguous()
