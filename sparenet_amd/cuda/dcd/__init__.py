"""Density-aware Chamfer distance (DCD, Wu et al., NeurIPS 2021) between two clouds (include/ops/dcd.h states the
definition; sparenet_amd/csrc/dcd.hip).  Chamfer is blind to density -- many predicted points may share one ground-truth
neighbour at no cost -- and the auction EMD, which is not, costs many times more on an untrained generator's output.
DCD divides every point's exponential Chamfer term by the number of points that chose the same neighbour: it sees
density, is bounded in [0, 1] (with `ratio="none"`) and costs a Chamfer call whatever the clouds look like.

    density_aware_chamfer(xyz1 [B,N,3], xyz2 [B,M,3], alpha=1000.0, n_lambda=1.0, ratio="none", lengths1=None,
                          lengths2=None, return_raw=False) -> [B]      differentiable in xyz1 and xyz2
    DensityAwareChamferDistance(alpha=1000.0, n_lambda=1.0, ratio="none")    the nn.Module of it
    dcd_from_search(xyz1, xyz2, dist1, idx1, dist2, idx2, ...) -> (sides, count1, count2, gradxyz1, gradxyz2)

Definition.  With the squared nearest-neighbour distances d and the neighbours' indices of the Chamfer search,
    loss = 1/2 (mean_i (1 - exp(-alpha d1_i) W1_i) + mean_j (1 - exp(-alpha d2_j) W2_j)),
    W1_i = r1 / count2[idx1_i] ** n_lambda,   count2[k] = how many points of xyz1 chose xyz2[k],
and the mirror image for W2.  `n_lambda` is exactly 0 (the plain exponential Chamfer), 0.5 or 1.  `ratio="size"` sets
r1 = N / M and r2 = M / N -- queries over targets, with which an ideal match between clouds of unequal size still reaches
0 -- and `"none"` leaves both at 1.  The exponential is sn_expf, the sums run in double in a fixed order and the result
is rounded once to fp32: two calls give identical bits, and CPU tensors give the bits of device tensors.

The search goes through the existing paths: dense device tensors through cd.forward_cuda (sorted or all pairs, as it
chooses), ragged ones through chamfer_ragged_forward_raw, CPU tensors through the host Chamfer.  The gradient (counts
held constant) is computed by the forward call when one is needed -- the inverse lists that give the counts are the
lists its gather walks -- and backward only scales it by the upstream gradient.
`lengths1` / `lengths2` make the batch ragged as in sparenet_amd.cuda.ragged: rows past a cloud's length are never read
into a result (they may hold NaN), their gradient is 0, and a pair with an empty side has value 0 and gradient 0.
`return_raw=True` returns (loss, raw) with raw = {"sides" [B,2] float64 (the two means), "dist1", "dist2", "idx1", "idx2"
(the search's own outputs, bit for bit), "count1" [B,N], "count2" [B,M] int32}.
"""
import math

import torch
from torch.autograd import Function

from sparenet_amd import _lib
from sparenet_amd.cuda import _args
from sparenet_amd.cuda.ragged import chamfer_search_raw

RATIOS = ("none", "size")
N_LAMBDAS = (0.0, 0.5, 1.0)


def _check_rule(what, alpha, n_lambda, ratio):
    """(alpha, n_lambda, ratio as the library's int)."""
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not math.isfinite(alpha) or alpha < 0:
        raise ValueError(f"{what}: alpha must be a finite number >= 0, got {alpha!r}")
    if isinstance(n_lambda, bool) or not isinstance(n_lambda, (int, float)) or n_lambda not in N_LAMBDAS:
        raise ValueError(f"{what}: n_lambda must be 0, 0.5 or 1, got {n_lambda!r}")
    if ratio not in RATIOS:
        raise ValueError(f"{what}: ratio must be one of {', '.join(RATIOS)}, got {ratio!r}")
    return float(alpha), float(n_lambda), RATIOS.index(ratio)


def dcd_from_search(xyz1, xyz2, dist1, idx1, dist2, idx2, alpha=1000.0, n_lambda=1.0, ratio="none", lengths1=None,
                    lengths2=None, with_grad=True):
    """(sides [B,2] float64, count1 [B,N], count2 [B,M] int32, gradxyz1 [B,N,3], gradxyz2 [B,M,3] fp32) for callers that
    already hold the Chamfer search of the pair: one library call, no second search.  The loss is
    0.5 * (sides[:, 0] + sides[:, 1]); the gradients are those of that loss (None without `with_grad`).  Device
    tensors, or CPU tensors throughout (the host entry point).  Not differentiable."""
    what = "dcd_from_search"
    alpha, n_lambda, ratio = _check_rule(what, alpha, n_lambda, ratio)
    _args.check_pair(what, "xyz1", xyz1, "xyz2", xyz2, same_device=True)
    b, n, m, dev = xyz1.size(0), xyz1.size(1), xyz2.size(1), xyz1.device
    for name, t, width in (("dist1", dist1, n), ("idx1", idx1, n), ("dist2", dist2, m), ("idx2", idx2, m)):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (b, width):
            raise ValueError(f"{what}: {name} must be a [{b}, {width}] tensor")
        if t.device != dev:
            raise ValueError(f"{what}: {name} is on {t.device}, the clouds on {dev}")
    xyz1, xyz2, dist1, dist2 = _args.fp32(xyz1), _args.fp32(xyz2), _args.fp32(dist1), _args.fp32(dist2)
    idx1, idx2 = idx1.contiguous().int(), idx2.contiguous().int()
    l1 = _args.optional_lengths(lengths1, b, n, dev, "lengths1")
    l2 = _args.optional_lengths(lengths2, b, m, dev, "lengths2")
    sides = torch.empty(b, 2, dtype=torch.float64, device=dev)
    count1 = torch.empty(b, n, dtype=torch.int32, device=dev)
    count2 = torch.empty(b, m, dtype=torch.int32, device=dev)
    grad1 = torch.empty(b, n, 3, device=dev) if with_grad else None
    grad2 = torch.empty(b, m, 3, device=dev) if with_grad else None
    args = (xyz1, xyz2, dist1, idx1, dist2, idx2, b, n, m, l1, l2, alpha, n_lambda, ratio, sides, count1, count2,
            grad1, grad2)
    if xyz1.is_cuda:
        ws = _lib.op_workspace("dcd", "sn_dcd_workspace_bytes", xyz1, b, n, m)
        _lib.op_call("dcd", "sn_dcd_from_search", *args, ws)
    else:
        _lib.op_call("dcd", "sn_dcd_from_search_host", *args, 0, host=True)
    return sides, count1, count2, grad1, grad2


class DensityAwareChamfer(Function):
    @staticmethod
    def forward(ctx, xyz1, xyz2, alpha, n_lambda, ratio, lengths1, lengths2):
        dist1, dist2, idx1, idx2, x1, x2, l1, l2 = chamfer_search_raw(xyz1.detach(), xyz2.detach(), lengths1, lengths2)
        with_grad = any(ctx.needs_input_grad[:2])
        sides, count1, count2, g1, g2 = dcd_from_search(x1, x2, dist1, idx1, dist2, idx2, alpha, n_lambda, ratio, l1, l2,
                                                        with_grad=with_grad)
        ctx.save_for_backward(*([g1, g2] if with_grad else []))
        raw = (sides, dist1, dist2, idx1, idx2, count1, count2)
        ctx.mark_non_differentiable(*raw)
        return ((sides[:, 0] + sides[:, 1]) * 0.5).float(), *raw

    @staticmethod
    def backward(ctx, grad, *_raw):
        g1, g2 = ctx.saved_tensors
        scale = grad.float()[:, None, None]
        return (scale * g1 if ctx.needs_input_grad[0] else None, scale * g2 if ctx.needs_input_grad[1] else None,
                None, None, None, None, None)


def density_aware_chamfer(xyz1, xyz2, alpha=1000.0, n_lambda=1.0, ratio="none", lengths1=None, lengths2=None,
                          return_raw=False):
    """[B] fp32: the density-aware Chamfer distance of the clouds xyz1 [B,N,3] and xyz2 [B,M,3] (in [0, 1] with `ratio="none"`);
    differentiable in both (see the module's text).  `return_raw=True`: (loss, dict of the search's and the op's raw
    outputs)."""
    what = "density_aware_chamfer"
    _check_rule(what, alpha, n_lambda, ratio)
    _args.check_pair(what, "xyz1", xyz1, "xyz2", xyz2, same_device=True)
    value, sides, dist1, dist2, idx1, idx2, count1, count2 = DensityAwareChamfer.apply(
        xyz1, xyz2, alpha, n_lambda, ratio, lengths1, lengths2)
    if not return_raw:
        return value
    return value, {"sides": sides, "dist1": dist1, "dist2": dist2, "idx1": idx1, "idx2": idx2, "count1": count1,
                   "count2": count2}


class DensityAwareChamferDistance(torch.nn.Module):
    """The density-aware Chamfer distance of two batches of clouds as a loss term: [B]."""

    def __init__(self, alpha=1000.0, n_lambda=1.0, ratio="none"):
        super().__init__()
        _check_rule("DensityAwareChamferDistance", alpha, n_lambda, ratio)
        self.alpha, self.n_lambda, self.ratio = float(alpha), float(n_lambda), ratio

    def forward(self, xyz1, xyz2, lengths1=None, lengths2=None):
        return density_aware_chamfer(xyz1, xyz2, self.alpha, self.n_lambda, self.ratio, lengths1, lengths2)
