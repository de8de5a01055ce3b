"""Minimum density sampling and point gathering -- host-side mirror of
cuda/MDS/MDS_module.py (MinimumDensitySampling :7-38, minimum_density_sample :41,
GatherOperation :44-75, gather_operation :78), backed by sn_mds / sn_gather_forward /
sn_gather_backward (include/sparenet_hip.h).

    minimum_density_sample(xyz [B,N,3], npoint, mean_mst_length [B]) -> idx [B,npoint] int32
        greedy sampling that repeatedly takes the point of lowest accumulated Gaussian
        density; mean_mst_length comes from the expansion penalty module.  Not differentiable.
    gather_operation(features [B,C,N], idx [B,npoint]) -> [B,C,npoint], differentiable in
        features.
"""
import torch
from torch.autograd import Function

from sparenet_amd import _lib


class MinimumDensitySampling(Function):
    @staticmethod
    def forward(ctx, xyz, npoint, mean_mst_length):
        if xyz.dim() != 3 or xyz.size(2) != 3:
            raise ValueError("minimum_density_sample: xyz must be [B, N, 3]")
        xyz = xyz.contiguous().float()
        mean_mst_length = mean_mst_length.contiguous().float()
        b, n, _ = xyz.shape
        idx = torch.empty(b, npoint, device=xyz.device, dtype=torch.int32)
        ws = _lib.workspace("sn_mds_workspace_bytes", xyz, b, n)
        _lib.call("sn_mds", xyz, b, n, npoint, mean_mst_length, idx, ws)
        ctx.mark_non_differentiable(idx)
        return idx

    @staticmethod
    def backward(ctx, grad_idx=None):
        return None, None, None


minimum_density_sample = MinimumDensitySampling.apply


class GatherOperation(Function):
    @staticmethod
    def forward(ctx, features, idx):
        features = features.contiguous().float()
        idx = idx.contiguous()
        b, c, n = features.size()
        m = idx.size(1)
        ctx.for_backwards = (idx, c, n)
        out = torch.empty(b, c, m, device=features.device)
        _lib.call("sn_gather_forward", features, idx, b, c, n, m, out)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        idx, c, n = ctx.for_backwards
        grad_out = grad_out.contiguous().float()
        b, _, m = grad_out.shape
        grad_features = torch.empty(b, c, n, device=grad_out.device)
        _lib.call("sn_gather_backward", grad_out, idx, b, c, n, m, grad_features)
        return grad_features, None


gather_operation = GatherOperation.apply
