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
import ctypes

import torch
from torch import nn
from torch.autograd import Function

from sparenet_amd import _lib


def _workspace(b, n, m, dev):
    nbytes = _lib.lib().sn_emd_general_workspace_bytes(b, n, m)
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev), nbytes


def emd_general_forward_raw(xyz1, xyz2, eps, iters, stats=None):
    """C-ABI call on contiguous fp32 CUDA tensors; returns (dist, assignment).
    stats: optional int64[2] CUDA tensor accumulating (effective pairs, active iterations of cloud 0)."""
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    dev = xyz1.device
    dist = torch.empty(b, n, device=dev)
    assignment = torch.empty(b, n, device=dev, dtype=torch.int32)
    with torch.cuda.device_of(xyz1):
        ws, nbytes = _workspace(b, n, m, dev)
        sp = ctypes.c_void_p(stats.data_ptr()) if stats is not None else ctypes.c_void_p(0)
        code = _lib.lib().sn_emd_forward_general(
            _lib.fptr(xyz1, "xyz1"), _lib.fptr(xyz2, "xyz2"), b, n, m, _lib.cfloat(eps), int(iters),
            _lib.fptr(dist, "dist"), _lib.iptr(assignment, "assignment"), ctypes.c_void_p(ws.data_ptr()),
            ctypes.c_size_t(nbytes), sp, _lib.stream_of(xyz1))
    _lib.check(code, "sn_emd_forward_general")
    return dist, assignment


def emd_general_backward_raw(xyz1, xyz2, graddist, assignment, need_xyz2=True):
    """(gradxyz1, gradxyz2 or None) for contiguous fp32 CUDA tensors."""
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    dev = xyz1.device
    gradxyz1 = torch.empty_like(xyz1)
    gradxyz2 = torch.empty_like(xyz2) if need_xyz2 else None
    with torch.cuda.device_of(xyz1):
        if need_xyz2:
            nbytes = _lib.lib().sn_emd_general_backward_workspace_bytes(b, n, m)
            ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
            wp = ctypes.c_void_p(ws.data_ptr())
        else:
            wp, nbytes = ctypes.c_void_p(0), 0
        g2 = _lib.fptr(gradxyz2, "gradxyz2") if need_xyz2 else ctypes.c_void_p(0)
        code = _lib.lib().sn_emd_backward_general(
            _lib.fptr(xyz1, "xyz1"), _lib.fptr(xyz2, "xyz2"), _lib.fptr(graddist, "graddist"),
            _lib.iptr(assignment, "assignment"), b, n, m, _lib.fptr(gradxyz1, "gradxyz1"), g2, wp,
            ctypes.c_size_t(nbytes), _lib.stream_of(xyz1))
    _lib.check(code, "sn_emd_backward_general")
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
