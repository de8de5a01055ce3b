"""Sliced Wasserstein distance between two clouds (include/ops/swd.h states the definition;
sparenet_amd/csrc/swd.hip).  The third transport loss beside the auction EMD and Sinkhorn, and the one whose cost is
O((N + M) log^2) per slice whatever the clouds look like: both clouds are projected onto L directions, every 1-D
projection is sorted by one workgroup in LDS, the 1-D transport problem is solved exactly and the L costs are averaged.

    random_directions(L, device, generator=None) -> [L, 3]            unit vectors, normalised Gaussians
    sorted_projections(x [B,N,3], dirs [L,3] or [B,L,3], lengths=None) -> (values [B,L,N] fp32, perm [B,L,N] int32)
    sliced_wasserstein(x [B,N,3], y [B,M,3], n_slices=128, p=2, directions=None, generator=None, x_lengths=None,
                       y_lengths=None, reduction="mean") -> [B]        differentiable in x and y
    SlicedWassersteinDistance(n_slices=128, p=2, reduction="mean")     the nn.Module of it

Definition.  Uniform weights 1/len_x and 1/len_y.  A slice's cost is W_p^p of the two 1-D projections: the mean of
|sx_i - sy_i|^p over the sorted values when the lengths agree, the exact staircase plan otherwise (n' + m' - gcd terms),
computed in double from the fp32 projections.  `reduction="mean"` averages the slices (in double, rounded once to fp32),
`"max"` is the max-sliced variant: the largest slice cost, whose gradient is that of its one direction per cloud (a
second call).  Directions are used as given -- `directions` [L,3] shared or [B,L,3] per cloud; None draws `n_slices`
of them with `generator`.  Equal projections are ordered by point index (-0.0 equals +0.0), so the permutation and
with it the gradient are reproducible: two calls give identical bits, for every SN_SWD_CHUNK.
The gradient is computed by the forward call (the plan is known once the projections are sorted) and scaled by the
upstream gradient in backward: there is no second pass.
`x_lengths` / `y_lengths` make the batch ragged as in sparenet_amd.cuda.ragged: rows past a cloud's length are never
read into a result (they may hold NaN), their gradient is 0, and a pair with an empty side has value 0 and gradient 0.
Clouds of at most 16384 points.  There is no host path: a CPU tensor raises SparenetHipError.
"""
import torch
from torch.autograd import Function

from sparenet_amd import _lib
from sparenet_amd.cuda import _args

MAX_POINTS = 16384
REDUCTIONS = ("mean", "max")


def random_directions(n_slices, device, generator=None):
    """[n_slices, 3] fp32 unit vectors on `device`: Gaussians from `generator` (its device decides where they are
    drawn), normalised."""
    n_slices = _args.check_count("random_directions", "n_slices", n_slices, refuse_bool=True)
    where = generator.device if generator is not None else device
    g = torch.randn(n_slices, 3, generator=generator, device=where, dtype=torch.float32)
    g = g / g.norm(dim=1, keepdim=True).clamp_min(1e-30)
    return g.to(device)


def _directions(what, directions, b, dev):
    """(contiguous fp32 [1 or b, L, 3] on dev, L, dirs_per_cloud)."""
    d = directions
    if not isinstance(d, torch.Tensor) or not d.is_floating_point() or d.dim() not in (2, 3) or d.size(-1) != 3 \
            or d.size(-2) == 0:
        raise ValueError(f"{what}: directions must be a floating-point [L, 3] or [B, L, 3] tensor")
    if d.dim() == 3 and d.size(0) != b:
        raise ValueError(f"{what}: directions [B, L, 3] must have B = {b}, got {d.size(0)}")
    _args.on_device(d, "directions")
    return d.detach().to(dev).float().contiguous(), d.size(-2), int(d.dim() == 3)


def _check_p(what, p):
    if isinstance(p, bool) or p not in (1, 2):
        raise ValueError(f"{what}: p must be 1 or 2, got {p!r}")
    return int(p)


def sorted_projections(x, dirs, lengths=None):
    """(values [B, L, N] fp32, perm [B, L, N] int32): every cloud's projections onto every direction in ascending
    order and the point index at each rank -- the stable order, ties by index.  Ranks past a cloud's length hold +inf
    and -1.  Not differentiable."""
    _args.check_cloud("sorted_projections", "x", x, max_points=MAX_POINTS)
    _args.on_device(x, "x")
    b, n = x.size(0), x.size(1)
    d, slices, per_cloud = _directions("sorted_projections", dirs, b, x.device)
    x = _args.fp32(x)
    ln = _args.optional_lengths(lengths, b, n, x.device, "lengths")
    values = torch.empty(b, slices, n, device=x.device)
    perm = torch.empty(b, slices, n, dtype=torch.int32, device=x.device)
    _lib.op_call("swd", "sn_swd_project_sort", x, d, b, n, slices, per_cloud, ln, values, perm)
    return values, perm


def _forward(x, y, d, slices, per_cloud, lx, ly, p, with_grad):
    """(cost [B, L] float64, gradx or None, grady or None) of one library call."""
    b, n, m = x.size(0), x.size(1), y.size(1)
    cost = torch.empty(b, slices, dtype=torch.float64, device=x.device)
    gx = torch.empty(b, n, 3, device=x.device) if with_grad else None
    gy = torch.empty(b, m, 3, device=x.device) if with_grad else None
    ws = _lib.op_workspace("swd", "sn_swd_workspace_bytes", x, b, n, m, slices)
    _lib.op_call("swd", "sn_swd_forward", x, y, d, b, n, m, slices, per_cloud, lx, ly, p, cost, gx, gy, ws)
    return cost, gx, gy


class SlicedWasserstein(Function):
    @staticmethod
    def forward(ctx, x, y, directions, p, x_lengths, y_lengths, reduction):
        what = "sliced_wasserstein"
        b, n, m = x.size(0), x.size(1), y.size(1)
        d, slices, per_cloud = _directions(what, directions, b, x.device)
        lx = _args.optional_lengths(x_lengths, b, n, x.device, "x_lengths")
        ly = _args.optional_lengths(y_lengths, b, m, x.device, "y_lengths")
        xf, yf = _args.fp32(x), _args.fp32(y)
        with_grad = any(ctx.needs_input_grad[:2])
        if reduction == "mean":
            cost, gx, gy = _forward(xf, yf, d, slices, per_cloud, lx, ly, p, with_grad)
            value = cost.mean(dim=1)
        else:
            # the largest slice of a value-only call, then that one direction per cloud for value and gradient
            cost, _, _ = _forward(xf, yf, d, slices, per_cloud, lx, ly, p, False)
            best = cost.argmax(dim=1)
            rows = d.expand(b, slices, 3)[torch.arange(b, device=x.device), best]
            cost, gx, gy = _forward(xf, yf, rows[:, None, :].contiguous(), 1, 1, lx, ly, p, with_grad)
            value = cost[:, 0]
        ctx.save_for_backward(*([gx, gy] if with_grad else []))
        return value.float()

    @staticmethod
    def backward(ctx, grad):
        gx, gy = ctx.saved_tensors
        scale = grad.float()[:, None, None]
        return (scale * gx if ctx.needs_input_grad[0] else None, scale * gy if ctx.needs_input_grad[1] else None,
                None, None, None, None, None)


def sliced_wasserstein(x, y, n_slices=128, p=2, directions=None, generator=None, x_lengths=None, y_lengths=None,
                       reduction="mean"):
    """[B] fp32: the sliced Wasserstein distance W_p^p of the clouds x [B,N,3] and y [B,M,3] averaged over the slices
    (`reduction="max"`: its largest slice); differentiable in x and y (see the module's text)."""
    what = "sliced_wasserstein"
    p = _check_p(what, p)
    if reduction not in REDUCTIONS:
        raise ValueError(f"{what}: reduction must be one of {', '.join(REDUCTIONS)}, got {reduction!r}")
    _args.check_pair(what, "x", x, "y", y, device="any", same_device=True, max_points=MAX_POINTS)
    if directions is None:
        directions = random_directions(n_slices, x.device, generator)
    return SlicedWasserstein.apply(x, y, directions, p, x_lengths, y_lengths, reduction)


class SlicedWassersteinDistance(torch.nn.Module):
    """The sliced Wasserstein distance of two batches of clouds as a loss term: [B]."""

    def __init__(self, n_slices=128, p=2, reduction="mean"):
        super().__init__()
        n_slices = _args.check_count("SlicedWassersteinDistance", "n_slices", n_slices, refuse_bool=True)
        if reduction not in REDUCTIONS:
            raise ValueError(f"SlicedWassersteinDistance: reduction must be one of {', '.join(REDUCTIONS)}")
        self.n_slices, self.p, self.reduction = n_slices, _check_p("SlicedWassersteinDistance", p), reduction

    def forward(self, x, y, directions=None, generator=None, x_lengths=None, y_lengths=None):
        return sliced_wasserstein(x, y, self.n_slices, self.p, directions, generator, x_lengths, y_lengths,
                                  self.reduction)
