"""EMD (auction) for clouds of any size n <= m, with gradients for both inputs.

emdModule / emdFunction mirror the reference and keep its limits (n == m, a multiple of 1024, at most 512 clouds,
no gradient for xyz2).  This module lifts them:

Input:  xyz1 [#batch, n, 3] (the bidders), xyz2 [#batch, m, 3] (the targets), 1 <= n <= m <= 2^20; pass the smaller
        cloud first.  eps and iters as in emdModule.
Output: dist [#batch, n] (squared distance of xyz1[j] to its matched target), assignment [#batch, n] int32 (index
        into xyz2; -1 only with iters == 0; several j may share a target when the auction was stopped before it
        converged).  Gradients flow to xyz1 and xyz2.

For n == m, n % 1024 == 0 the results equal emdModule's bit for bit (those sizes run the same persistent auction;
SN_EMD_GENERAL=1 forces the general kernels, which compute the same).  Backed by sn_emd_forward_general /
sn_emd_backward_general (include/sparenet_hip.h).
"""
import torch
from torch import nn
from torch.autograd import Function

from sparenet_amd import _lib


def emd_general_forward_raw(xyz1, xyz2, eps, iters, stats=None):
    """C-ABI call on contiguous fp32 CUDA tensors; returns (dist, assignment).
    stats: optional int64[2] CUDA tensor accumulating (effective pairs, active iterations of cloud 0)."""
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    dev = xyz1.device
    dist = torch.empty(b, n, device=dev)
    assignment = torch.empty(b, n, device=dev, dtype=torch.int32)
    ws = _lib.workspace("sn_emd_general_workspace_bytes", xyz1, b, n, m)
    _lib.call("sn_emd_forward_general", xyz1, xyz2, b, n, m, eps, iters, dist, assignment, ws, stats)
    return dist, assignment


def emd_general_backward_raw(xyz1, xyz2, graddist, assignment, need_xyz2=True):
    """(gradxyz1, gradxyz2 or None) for contiguous fp32 CUDA tensors."""
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    gradxyz1 = torch.empty_like(xyz1)
    gradxyz2 = torch.empty_like(xyz2) if need_xyz2 else None      # None: a null pointer, and no workspace is needed
    ws = _lib.workspace("sn_emd_general_backward_workspace_bytes", xyz1, b, n, m) if need_xyz2 else None
    _lib.call("sn_emd_backward_general", xyz1, xyz2, graddist, assignment, b, n, m, gradxyz1, gradxyz2, ws)
    return gradxyz1, gradxyz2


class EmdGeneralFunction(Function):
    @staticmethod
    def forward(ctx, xyz1, xyz2, eps, iters):
        if xyz1.dim() != 3 or xyz2.dim() != 3 or xyz1.size(2) != 3 or xyz2.size(2) != 3:
            raise ValueError(f"emd_general: expected [B, n, 3] and [B, m, 3], got {tuple(xyz1.shape)} and "
                             f"{tuple(xyz2.shape)}")
        if xyz1.size(0) != xyz2.size(0):
            raise ValueError(f"emd_general: batch sizes differ ({xyz1.size(0)} and {xyz2.size(0)})")
        if xyz1.size(1) > xyz2.size(1):
            raise ValueError(f"emd_general: n={xyz1.size(1)} > m={xyz2.size(1)}: pass the smaller cloud first")
        xyz1 = xyz1.contiguous().float()
        xyz2 = xyz2.contiguous().float()
        dist, assignment = emd_general_forward_raw(xyz1, xyz2, eps, iters)
        ctx.save_for_backward(xyz1, xyz2, assignment)
        ctx.mark_non_differentiable(assignment)
        return dist, assignment

    @staticmethod
    def backward(ctx, graddist, gradidx):
        xyz1, xyz2, assignment = ctx.saved_tensors
        gradxyz1, gradxyz2 = emd_general_backward_raw(xyz1, xyz2, graddist.contiguous().float(), assignment,
                                                      need_xyz2=ctx.needs_input_grad[1])
        return gradxyz1, gradxyz2, None, None


def emd_general(xyz1, xyz2, eps, iters):
    """(dist [B, n], assignment [B, n] int32) of the auction EMD of xyz1 [B, n, 3] against xyz2 [B, m, 3], n <= m;
    differentiable in both inputs."""
    return EmdGeneralFunction.apply(xyz1, xyz2, eps, iters)


class EmdGeneral(nn.Module):
    def forward(self, input1, input2, eps, iters):
        return EmdGeneralFunction.apply(input1, input2, eps, iters)
