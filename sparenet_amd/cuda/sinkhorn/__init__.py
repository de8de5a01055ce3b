"""Entropic optimal transport (Sinkhorn) between two clouds (include/ops/sinkhorn.h states the definition;
sparenet_amd/csrc/sinkhorn.hip).  A transport loss beside the auction EMD whose run time depends only on
(B, N, M, iterations): every half-iteration is one dense O(N * M) streaming kernel -- bounded and data-independent, NOT
cheaper than the auction on friendly data -- in which no workgroup waits for another, launched plainly.

    sinkhorn_potentials(x [B,N,3], y [B,M,3], eps, iters=None, eps_start=None, decay=0.5, x_lengths=None,
                        y_lengths=None, g0=None) -> (f [B,N], g [B,M])                  not differentiable
    sinkhorn_ot(x, y, eps, ...) -> [B]            OT_eps, differentiable in x and y
    sinkhorn_divergence(x, y, eps, ...) -> [B]    S = OT(x,y) - OT(x,x)/2 - OT(y,y)/2, differentiable in x and y
    SinkhornDistance(eps, iters=None, eps_start=None, decay=0.5, debias=True)          the nn.Module of the two
    schedule(eps, iters=None, eps_start=None, decay=0.5) -> [eps_0, ..., eps_{iters-1}]

Definition.  Uniform weights a_i = 1/len_x, b_j = 1/len_y.  The cost is the SQUARED distance C_ij = |x_i - y_j|^2 in
separately rounded fp32, as Chamfer's -- no factor 1/2.  `eps` is the temperature in the units of C, and the schedule
acts on eps itself: eps_t = max(eps, eps_start * decay^t), computed in double from the fp32 values and rounded to fp32
(eps_start None or <= 0: constant eps).  From g = 0 (or `g0`), for t = 0 .. iters - 1 with e = eps_t:
    f_i = -e log sum_j exp(log b_j + (g_j - C_ij) / e),      g_j = -e log sum_i exp(log a_i + (f_i - C_ij) / e)
and OT_eps = sum_i a_i f_i + sum_j b_j g_j (the sums in float64, rounded once).  `iters=None` is the number of steps
the schedule needs to reach eps plus 5, or 20 without eps_start.
The gradient is the last-iterate (envelope) one -- nothing is back-propagated through the loop:
    dOT/dx_i = a_i * 2 * (x_i - sum_j w_ij y_j),  w_ij = softmax_j(log b_j + (g_j - C_ij) / eps)   at the final eps,
and the same for y with f; each side costs one more kernel pass and is computed only where a gradient is needed.
The debiased divergence is one ragged call of 3B problems, [x|x|y] against [y|x|y] padded to max(N, M); autograd sums
the two roles of x in the symmetric terms.
`x_lengths` / `y_lengths` make the batch ragged as in sparenet_amd.cuda.ragged: rows past a cloud's length are never
read into a result (they may hold NaN), f and g are 0 there, and a pair with an empty side has value 0 and gradient 0.
Two calls give identical bits.  There is no host path: a CPU tensor raises SparenetHipError.
"""
import ctypes
import math

import torch
from torch.autograd import Function

from sparenet_amd import _lib
from sparenet_amd.cuda import _args
from sparenet_amd.cuda.ragged import valid_mask

DEFAULT_ITERS = 20      # without an eps_start
EXTRA_ITERS = 5         # steps at the final eps behind an annealed schedule


def _f32(v):
    return ctypes.c_float(float(v)).value


def _params(what, eps, iters, eps_start, decay):
    """(eps, iters, eps_start, decay) as the library takes them: fp32 values, eps_start 0.0 for a constant eps, iters
    resolved."""
    eps, decay = float(eps), float(decay)
    if not (0.0 < eps < float("inf")) or _f32(eps) <= 0.0 or math.isinf(_f32(eps)):
        raise ValueError(f"{what}: eps must be finite and > 0, got {eps!r}")
    if not 0.0 < decay < 1.0 or not 0.0 < _f32(decay) < 1.0:
        raise ValueError(f"{what}: decay must be in (0, 1), got {decay!r}")
    eps_start = 0.0 if eps_start is None else float(eps_start)
    if math.isnan(eps_start) or math.isinf(eps_start) or math.isinf(_f32(eps_start)):
        raise ValueError(f"{what}: eps_start must be finite (None or <= 0: constant eps), got {eps_start!r}")
    eps, eps_start, decay = _f32(eps), max(_f32(eps_start), 0.0), _f32(decay)
    if iters is None:
        iters = DEFAULT_ITERS
        if eps_start > 0.0:
            reach = 0
            while eps_start * decay ** reach > eps:
                reach += 1
            iters = reach + EXTRA_ITERS
    return eps, _args.check_count(what, "iters", iters, refuse_bool=True), eps_start, decay


def schedule(eps, iters=None, eps_start=None, decay=0.5):
    """[eps_0, ..., eps_{iters-1}] as sn_sinkhorn_solve walks them: max(eps, eps_start * decay^t) in double from the
    fp32 arguments, rounded to fp32."""
    eps, iters, eps_start, decay = _params("schedule", eps, iters, eps_start, decay)
    return [_f32(max(eps, eps_start * decay ** t)) if eps_start > 0.0 else eps for t in range(iters)]


def _clouds(what, x, y):
    """The pair as contiguous fp32 device tensors, and (b, n, m)."""
    _args.check_pair(what, "x", x, "y", y, device="contiguous")
    return _args.fp32(x), _args.fp32(y), x.size(0), x.size(1), y.size(1)


def _lengths(x_lengths, y_lengths, b, n, m, dev):
    return (_args.optional_lengths(x_lengths, b, n, dev, "x_lengths"),
            _args.optional_lengths(y_lengths, b, m, dev, "y_lengths"))


def _solve(x, y, b, n, m, lx, ly, eps, iters, eps_start, decay, g0=None):
    f = torch.empty(b, n, device=x.device)
    if g0 is None:
        g = torch.empty(b, m, device=x.device)
    else:
        if not isinstance(g0, torch.Tensor) or g0.shape != (b, m) or not g0.is_floating_point():
            raise ValueError(f"sinkhorn: g0 must be a floating-point [B, M] = [{b}, {m}] tensor")
        _lib.require_device(g0, "g0")
        g = g0.detach().float().clone().contiguous()
    ws = _lib.op_workspace("sinkhorn", "sn_sinkhorn_workspace_bytes", x, b, n, m)
    _lib.op_call("sinkhorn", "sn_sinkhorn_solve", x, y, b, n, m, lx, ly, eps, eps_start, decay, iters,
                 int(g0 is not None), f, g, ws)
    return f, g


def _barycenter(q, t, pot, b, n, m, lq, lt, eps):
    bary = torch.empty(b, n, 3, device=q.device)
    ws = _lib.op_workspace("sinkhorn", "sn_sinkhorn_workspace_bytes", q, b, n, m)
    _lib.op_call("sinkhorn", "sn_sinkhorn_barycenter", q, t, pot, b, n, m, lq, lt, eps, bary, None, ws)
    return bary


def _counts(lengths, b, width, dev):
    """int64 [b]: each cloud's length held to the row, as the kernels hold it."""
    if lengths is None:
        return torch.full((b,), width, dtype=torch.int64, device=dev)
    return lengths.to(torch.int64).clamp(0, width)


def sinkhorn_potentials(x, y, eps, iters=None, eps_start=None, decay=0.5, x_lengths=None, y_lengths=None, g0=None):
    """(f [B, N], g [B, M]): the dual potentials after `iters` Sinkhorn iterations (see the module's text).  `g0`
    [B, M] starts the loop from a given g instead of 0.  Not differentiable."""
    eps, iters, eps_start, decay = _params("sinkhorn_potentials", eps, iters, eps_start, decay)
    x, y, b, n, m = _clouds("sinkhorn_potentials", x, y)
    lx, ly = _lengths(x_lengths, y_lengths, b, n, m, x.device)
    return _solve(x, y, b, n, m, lx, ly, eps, iters, eps_start, decay, g0)


class SinkhornOT(Function):
    @staticmethod
    def forward(ctx, x, y, eps, iters, eps_start, decay, x_lengths, y_lengths):
        eps, iters, eps_start, decay = _params("sinkhorn_ot", eps, iters, eps_start, decay)
        x, y, b, n, m = _clouds("sinkhorn_ot", x, y)
        lx, ly = _lengths(x_lengths, y_lengths, b, n, m, x.device)
        f, g = _solve(x, y, b, n, m, lx, ly, eps, iters, eps_start, decay)
        cx, cy = _counts(lx, b, n, x.device), _counts(ly, b, m, x.device)
        mask_x, mask_y = valid_mask(cx, n, x.device), valid_mask(cy, m, x.device)
        zero = torch.zeros((), dtype=torch.float64, device=x.device)
        total = (torch.where(mask_x, f.double(), zero).sum(dim=1) / cx.clamp_min(1)
                 + torch.where(mask_y, g.double(), zero).sum(dim=1) / cy.clamp_min(1))
        both = (cx > 0) & (cy > 0)
        ctx.save_for_backward(x, y, f, g, cx, cy)
        # the potentials belong to the last step's eps (the target eps once the schedule has reached it)
        ctx.lengths, ctx.eps = (lx, ly), (_f32(max(eps, eps_start * decay ** (iters - 1))) if eps_start > 0.0 else eps)
        return torch.where(both, total, zero).float()

    @staticmethod
    def backward(ctx, grad):
        x, y, f, g, cx, cy = ctx.saved_tensors
        lx, ly = ctx.lengths
        b, n, m = x.size(0), x.size(1), y.size(1)
        both = (cx > 0) & (cy > 0)
        grad = grad.float()

        def side(q, t, pot, nq, nt, lq, lt, cq):
            bary = _barycenter(q, t, pot, b, nq, nt, lq, lt, ctx.eps)
            live = valid_mask(cq, nq, q.device) & both[:, None]
            scale = (2.0 * grad / cq.clamp_min(1)).float()
            return torch.where(live[:, :, None], scale[:, None, None] * (q - bary), torch.zeros((), device=q.device))

        gx = side(x, y, g, n, m, lx, ly, cx) if ctx.needs_input_grad[0] else None
        gy = side(y, x, f, m, n, ly, lx, cy) if ctx.needs_input_grad[1] else None
        return gx, gy, None, None, None, None, None, None


def sinkhorn_ot(x, y, eps, iters=None, eps_start=None, decay=0.5, x_lengths=None, y_lengths=None):
    """[B]: OT_eps(x, y) = sum_i a_i f_i + sum_j b_j g_j (see the module's text); differentiable in x and y by the
    last-iterate gradient."""
    return SinkhornOT.apply(x, y, eps, iters, eps_start, decay, x_lengths, y_lengths)


def sinkhorn_divergence(x, y, eps, iters=None, eps_start=None, decay=0.5, x_lengths=None, y_lengths=None):
    """[B]: S(x, y) = OT(x, y) - OT(x, x) / 2 - OT(y, y) / 2, from one ragged call of 3B problems; differentiable in
    x and y."""
    _params("sinkhorn_divergence", eps, iters, eps_start, decay)
    _clouds("sinkhorn_divergence", x, y)
    b, n, m = x.size(0), x.size(1), y.size(1)
    width = max(n, m)
    lx, ly = _lengths(x_lengths, y_lengths, b, n, m, x.device)
    lx, ly = _counts(lx, b, n, x.device), _counts(ly, b, m, x.device)
    xp = torch.nn.functional.pad(x.float(), (0, 0, 0, width - n))
    yp = torch.nn.functional.pad(y.float(), (0, 0, 0, width - m))
    ot = sinkhorn_ot(torch.cat([xp, xp, yp]), torch.cat([yp, xp, yp]), eps, iters, eps_start, decay,
                     torch.cat([lx, lx, ly]), torch.cat([ly, lx, ly]))
    return ot[:b] - 0.5 * ot[b:2 * b] - 0.5 * ot[2 * b:]


class SinkhornDistance(torch.nn.Module):
    """The Sinkhorn divergence (debias=True) or OT_eps (debias=False) of two batches of clouds as a loss term: [B]."""

    def __init__(self, eps, iters=None, eps_start=None, decay=0.5, debias=True):
        super().__init__()
        _params("SinkhornDistance", eps, iters, eps_start, decay)
        self.eps, self.iters, self.eps_start, self.decay, self.debias = eps, iters, eps_start, decay, bool(debias)

    def forward(self, x, y, x_lengths=None, y_lengths=None):
        fn = sinkhorn_divergence if self.debias else sinkhorn_ot
        return fn(x, y, self.eps, self.iters, self.eps_start, self.decay, x_lengths, y_lengths)
