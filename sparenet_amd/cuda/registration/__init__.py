"""Rigid registration: the Kabsch / Umeyama fit of given correspondences and ICP on the exact nearest-neighbour search
(include/ops/rigid_fit.h states the rules; sparenet_amd/csrc/rigid_fit.hip and rigid_solve.hpp).

    transform_points(xyz [B,N,3], pose [4,4] | [B,4,4], scale=None, lengths=None) -> [B,N,3] fp32
    rigid_fit(src, dst, idx=None, weights=None, src_lengths=None, dst_lengths=None, with_scale=False, max_dist=None,
              mode="point", dst_normals=None, init=None) -> RigidFit(pose, scale, rmse, fitness, flags)
    icp(src, dst, iters=30, mode="point", dst_normals=None, max_dist=None, init=None, with_scale=False, rtol=1e-6,
        atol=1e-7, src_lengths=None, dst_lengths=None, normals_k=16)
        -> IcpResult(pose, scale, rmse, fitness, flags, iterations, converged)
    aligned_chamfer(pred, gt, **icp_options) -> (cd [B], IcpResult)

A pose is a float64 [4,4] matrix (R in the upper left block, t in the last column); with `scale` the map is
x -> scale * R x + t.  `flags` is an int32 [B] sum of EMPTY (no inlier: the pose was left alone), SINGULAR (plane mode:
the normal equations had no usable pivot, the pose was left alone) and FROZEN.  All sums run in double in a fixed order:
two calls give identical bits, a cloud's result does not depend on its batch, and CPU tensors (the library's host entry
points) give the device's bits.  Nothing is differentiable through the solver or the loop; `transform_points` is
differentiable in the points and in the pose.
"""
import collections

import torch
from torch.autograd import Function

from sparenet_amd import _lib
from sparenet_amd.cuda import _args
from sparenet_amd.cuda.ragged import chamfer_search_raw, masked_mean, valid_mask

RigidFit = collections.namedtuple("RigidFit", "pose scale rmse fitness flags")
IcpResult = collections.namedtuple("IcpResult", "pose scale rmse fitness flags iterations converged")
MODES = {"point": 0, "plane": 1}      # the modes of sn_rigid_step
EMPTY, SINGULAR, FROZEN = 1, 2, 4     # the flags of include/ops/rigid_fit.h


def _poses(what, name, pose, b, dev):
    """float64 [B,4,4], contiguous on `dev`, from a [4,4] or [B,4,4] tensor."""
    if not isinstance(pose, torch.Tensor) or not pose.is_floating_point() or tuple(pose.shape) not in ((4, 4), (b, 4, 4)):
        raise ValueError(f"{what}: {name} must be a floating-point [4, 4] or [{b}, 4, 4] tensor")
    if pose.device != dev:
        raise ValueError(f"{what}: {name} is on {pose.device}, the cloud on {dev}")
    pose = pose.detach().double()
    return (pose[None].expand(b, 4, 4) if pose.dim() == 2 else pose).contiguous()


def _scales(what, scale, b, dev):
    """None, or float64 [B] contiguous on `dev` from a number or a [B] tensor."""
    if scale is None:
        return None
    if isinstance(scale, (int, float)) and not isinstance(scale, bool):
        return torch.full((b,), float(scale), dtype=torch.float64, device=dev)
    if not isinstance(scale, torch.Tensor) or not scale.is_floating_point() or tuple(scale.shape) != (b,):
        raise ValueError(f"{what}: scale must be a number or a floating-point [{b}] tensor")
    if scale.device != dev:
        raise ValueError(f"{what}: scale is on {scale.device}, the cloud on {dev}")
    return scale.detach().double().contiguous()


def _apply(xyz, pose, scale, lengths):
    """sn_rigid_apply on prepared arguments: fp32 [B,N,3]."""
    out = torch.empty_like(xyz)
    args = (xyz, pose, scale, lengths, xyz.size(0), xyz.size(1), out)
    if xyz.is_cuda:
        _lib.op_call("rigid_fit", "sn_rigid_apply", *args)
    else:
        _lib.op_call("rigid_fit", "sn_rigid_apply_host", *args, 0, host=True)
    return out


class TransformPoints(Function):
    @staticmethod
    def forward(ctx, xyz, pose, scale, lengths):
        what = "transform_points"
        _args.check_cloud(what, "xyz", xyz)
        b, n, dev = xyz.size(0), xyz.size(1), xyz.device
        poses = _poses(what, "pose", pose, b, dev)
        scales = _scales(what, scale, b, dev)
        lens = _args.optional_lengths(lengths, b, n, dev, "lengths")
        pts = _args.fp32(xyz)
        ctx.save_for_backward(pts, poses, scales, lens)
        ctx.shared_pose, ctx.dtypes = pose.dim() == 2, (xyz.dtype, pose.dtype)
        return _apply(pts, poses, scales, lens)

    @staticmethod
    def backward(ctx, grad):
        pts, poses, scales, lens = ctx.saved_tensors
        g = grad.double()
        if lens is not None:
            g = torch.where(valid_mask(lens, g.size(1), g.device)[:, :, None], g, torch.zeros((), dtype=g.dtype, device=g.device))
        s = torch.ones(g.size(0), dtype=g.dtype, device=g.device) if scales is None else scales
        grad_xyz = grad_pose = None
        if ctx.needs_input_grad[0]:
            grad_xyz = (g @ (s[:, None, None] * poses[:, :3, :3])).to(ctx.dtypes[0])
        if ctx.needs_input_grad[1]:
            p = pts.double()
            if lens is not None:      # padding rows may hold NaN
                p = torch.where(valid_mask(lens, p.size(1), p.device)[:, :, None], p, torch.zeros((), dtype=p.dtype, device=p.device))
            grad_pose = torch.zeros_like(poses)
            grad_pose[:, :3, :3] = s[:, None, None] * (g.transpose(1, 2) @ p)
            grad_pose[:, :3, 3] = g.sum(dim=1)
            grad_pose = (grad_pose.sum(dim=0) if ctx.shared_pose else grad_pose).to(ctx.dtypes[1])
        return grad_xyz, grad_pose, None, None


def transform_points(xyz, pose, scale=None, lengths=None):
    """[B,N,3] fp32: scale * R xyz + t per cloud, with `pose` a [4,4] (one for the batch) or [B,4,4] matrix and `scale` a
    number or [B] (None: 1).  The point is widened to double, every product and sum is rounded separately and the result
    once to fp32; rows at and beyond `lengths` are 0.  Differentiable in xyz and in pose (float64 sums over the valid
    rows; the pose's last row gets 0), not in scale.  Device tensors, or CPU tensors throughout."""
    return TransformPoints.apply(xyz, pose, scale, lengths)


def _normals(what, dst_normals, dst):
    if not isinstance(dst_normals, torch.Tensor) or dst_normals.shape != dst.shape or not dst_normals.is_floating_point():
        raise ValueError(f"{what}: dst_normals must be a floating-point tensor of dst's shape {tuple(dst.shape)}")
    if dst_normals.device != dst.device:
        raise ValueError(f"{what}: dst_normals is on {dst_normals.device}, dst on {dst.device}")
    return _args.fp32(dst_normals)


def _mode(what, mode, with_scale):
    if mode not in MODES:
        raise ValueError(f"{what}: mode must be 'point' or 'plane', got {mode!r}")
    if mode == "plane" and with_scale:
        raise ValueError(f"{what}: with_scale is for mode='point' only")
    return MODES[mode]


def _limit(what, max_dist):
    """max_dist as the entry point takes it: 0 for None (no limit)."""
    if max_dist is None:
        return 0.0
    if isinstance(max_dist, (bool, torch.Tensor)) or not isinstance(max_dist, (int, float)) or not max_dist > 0:
        raise ValueError(f"{what}: max_dist must be None or a number > 0, got {max_dist!r}")
    return float(max_dist)


def _start(what, init, b, dev):
    """(pose [B,4,4], scale [B], state [B,4], stats [B,4]) float64 on `dev`: `init` or the identity, scale 1."""
    if init is None:
        pose = torch.eye(4, dtype=torch.float64, device=dev)[None].repeat(b, 1, 1)
    else:
        pose = _poses(what, "init", init, b, dev).clone()
    return (pose, torch.ones(b, dtype=torch.float64, device=dev), torch.zeros(b, 4, dtype=torch.float64, device=dev),
            torch.empty(b, 4, dtype=torch.float64, device=dev))


class _Step:
    """sn_rigid_step on one pair of clouds: the arguments that do not change between iterations, and the workspace."""

    def __init__(self, dst, normals, src_lengths, dst_lengths, n, mode, with_scale, max_dist, rtol, atol):
        self.dst, self.normals, self.lengths = dst, normals, (src_lengths, dst_lengths)
        self.shape = (dst.size(0), n, dst.size(1))
        self.rule = (mode, int(bool(with_scale)), max_dist, float(rtol), float(atol))
        self.ws = _lib.op_workspace("rigid_fit", "sn_rigid_step_workspace_bytes", dst, dst.size(0), n) if dst.is_cuda \
            else None

    def __call__(self, moved, idx, weight, freeze, pose, scale, state, stats):
        args = (moved, self.dst, idx, weight, self.normals, *self.lengths, *self.shape, *self.rule, int(freeze), pose,
                scale, state, stats)
        if moved.is_cuda:
            _lib.op_call("rigid_fit", "sn_rigid_step", *args, self.ws)
        else:
            _lib.op_call("rigid_fit", "sn_rigid_step_host", *args, 0, host=True)


def _result(pose, scale, stats):
    return pose, scale, stats[:, 0].contiguous(), stats[:, 1].contiguous(), stats[:, 3].to(torch.int32)


def _pair(what, src, dst):
    _args.check_pair(what, "src", src, "dst", dst, same_device=True)
    b, dev = src.size(0), src.device
    return b, src.size(1), dst.size(1), dev


@torch.no_grad()
def rigid_fit(src, dst, idx=None, weights=None, src_lengths=None, dst_lengths=None, with_scale=False, max_dist=None,
              mode="point", dst_normals=None, init=None):
    """RigidFit(pose [B,4,4] float64, scale [B], rmse [B], fitness [B], flags [B] int32): the rigid map that best takes
    src [B,N,3] onto its matches in dst [B,M,3], in one step from `init` (a [4,4] or [B,4,4] pose; None: the identity).
    idx [B,N] names the row of dst matched to each row of src (-1: none); None matches row i to row i and needs N == M.
    mode="point" minimises sum w |s R p + t - q|^2 in closed form (Horn's quaternion method; with_scale=True fits
    Umeyama's scale too); mode="plane" takes one Gauss-Newton step of sum w (n . (R p + t - q))^2 with the normals
    dst_normals [B,M,3].  `weights` [B,N] must not be negative (they are read on the host once to check that).
    `max_dist` drops the pairs farther apart than that under `init`.  rmse and fitness describe the pairs under `init`,
    as every ICP implementation reports them; see include/ops/rigid_fit.h for the rule, sentence by sentence.
    Device tensors, or CPU tensors throughout.  Not differentiable."""
    what = "rigid_fit"
    b, n, m, dev = _pair(what, src, dst)
    code = _mode(what, mode, with_scale)
    limit = _limit(what, max_dist)
    if idx is None:
        if n != m:
            raise ValueError(f"{what}: idx=None matches row i to row i and needs N == M (got {n} and {m})")
    else:
        if not isinstance(idx, torch.Tensor) or idx.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"{what}: idx must be an int32 / int64 tensor")
        if tuple(idx.shape) != (b, n):
            raise ValueError(f"{what}: idx must be a [{b}, {n}] tensor, got {tuple(idx.shape)}")
        if idx.device != dev:
            raise ValueError(f"{what}: idx is on {idx.device}, src on {dev}")
        idx = idx.to(torch.int32).contiguous()
    if weights is not None:
        if not isinstance(weights, torch.Tensor) or not weights.is_floating_point() or tuple(weights.shape) != (b, n):
            raise ValueError(f"{what}: weights must be a floating-point [{b}, {n}] tensor")
        if weights.device != dev:
            raise ValueError(f"{what}: weights is on {weights.device}, src on {dev}")
        weights = _args.fp32(weights)
    normals = None
    if code == MODES["plane"]:
        if dst_normals is None:
            raise ValueError(f"{what}: mode='plane' needs dst_normals, the normals of dst")
        normals = _normals(what, dst_normals, dst)
    sl = _args.optional_lengths(src_lengths, b, n, dev, "src_lengths")
    dl = _args.optional_lengths(dst_lengths, b, m, dev, "dst_lengths")
    if weights is not None:
        rows = weights if sl is None else torch.where(valid_mask(sl, n, dev), weights, torch.zeros((), device=dev))
        if bool(((rows < 0) | ~torch.isfinite(rows)).any()):
            raise ValueError(f"{what}: weights must be finite and not negative")
    pose, scale, state, stats = _start(what, init, b, dev)
    pts, target = _args.fp32(src), _args.fp32(dst)
    moved = pts if init is None else _apply(pts, pose, None, sl)
    _Step(target, normals, sl, dl, n, code, with_scale, limit, 0.0, 0.0)(moved, idx, weights, 0, pose, scale, state, stats)
    return RigidFit(*_result(pose, scale, stats))


@torch.no_grad()
def icp(src, dst, iters=30, mode="point", dst_normals=None, max_dist=None, init=None, with_scale=False, rtol=1e-6,
        atol=1e-7, src_lengths=None, dst_lengths=None, normals_k=16):
    """IcpResult(pose, scale, rmse, fitness, flags, iterations [B] int32, converged [B] bool): iterative closest point of
    src [B,N,3] onto dst [B,M,3] from `init` (None: the identity).  Exactly `iters` rounds of transform, exact
    nearest-neighbour search (the Chamfer search's src -> dst side) and one step (rigid_fit's, on the search's matches
    within `max_dist`): the number of rounds does not depend on the data and nothing in the loop reads a value back to
    the host.  A cloud FREEZES at the first round in which |rmse - previous rmse| <= rtol * previous rmse + atol and
    |fitness - previous fitness| <= rtol; from then on its pose keeps every bit, `iterations` is the number of steps it
    took before and `converged` is True.  Frozen clouds still cost their search in the remaining rounds but change
    nothing, so the result is the same for any larger `iters`.  `atol` defaults to 1e-7, the fp32 rounding of the
    moved points at unit scale -- a cloud matched to an exact copy of itself sits at an rmse of that order and never
    meets a purely relative test: scale it with your data's size.  After the loop one more transform and search measure
    rmse and fitness of the final pose, so a cloud that never froze reports the quality of the pose it ends on.
    mode="plane" minimises point-to-plane distances and takes far fewer rounds on surfaces; without dst_normals they
    are estimated with estimate_normals(dst, normals_k, dst_lengths) (device tensors only).  Device tensors, or CPU
    tensors throughout: both give the same bits.  Not differentiable."""
    what = "icp"
    b, n, m, dev = _pair(what, src, dst)
    code = _mode(what, mode, with_scale)
    limit = _limit(what, max_dist)
    if isinstance(iters, bool) or int(iters) != iters or iters < 0:
        raise ValueError(f"{what}: iters must be an integer >= 0, got {iters!r}")
    if not rtol >= 0 or not atol >= 0:
        raise ValueError(f"{what}: rtol and atol must not be negative (got {rtol!r} and {atol!r})")
    sl = _args.optional_lengths(src_lengths, b, n, dev, "src_lengths")
    dl = _args.optional_lengths(dst_lengths, b, m, dev, "dst_lengths")
    pts, target = _args.fp32(src), _args.fp32(dst)
    normals = None
    if code == MODES["plane"]:
        if dst_normals is None:
            from sparenet_amd.cuda.normals import estimate_normals

            dst_normals = estimate_normals(target, normals_k, dl)
        normals = _normals(what, dst_normals, dst)
    pose, scale, state, stats = _start(what, init, b, dev)
    step = _Step(target, normals, sl, dl, n, code, with_scale, limit, rtol, atol)
    for round_ in range(int(iters) + 1):      # the last round measures only
        moved = _apply(pts, pose, scale, sl)
        idx = chamfer_search_raw(moved, target, sl, dl)[2]
        if round_ < iters:
            step(moved, idx, None, 1, pose, scale, state, stats)
        else:
            step(moved, idx, None, 0, None, None, None, stats)
    frozen = state[:, 3] != 0
    flags = stats[:, 3].to(torch.int32) | (frozen.to(torch.int32) * FROZEN)
    return IcpResult(pose, scale, stats[:, 0].contiguous(), stats[:, 1].contiguous(), flags,
                     state[:, 2].to(torch.int32), frozen)


def aligned_chamfer(pred, gt, **icp_options):
    """(cd [B], IcpResult): the Chamfer distance -- mean squared nearest-neighbour distance pred -> gt plus gt -> pred --
    after pred [B,N,3] has been registered onto gt [B,M,3] by icp(pred, gt, **icp_options), a pose-free "aligned
    Chamfer".  The pose is a constant: cd is differentiable in pred through the final transform and the distance, and in
    gt through the distance.  src_lengths / dst_lengths among the options make the batch ragged."""
    from sparenet_amd.cuda.chamfer_distance.chamfer_distance import ChamferDistanceFunction
    from sparenet_amd.cuda.ragged import chamfer_ragged

    found = icp(pred.detach(), gt.detach(), **icp_options)
    l1, l2 = icp_options.get("src_lengths"), icp_options.get("dst_lengths")
    moved = transform_points(pred, found.pose, found.scale, l1)
    if l1 is None and l2 is None:
        dist1, dist2 = ChamferDistanceFunction.apply(moved, gt)
        return dist1.mean(dim=1) + dist2.mean(dim=1), found
    b = pred.size(0)
    l1 = [pred.size(1)] * b if l1 is None else l1
    l2 = [gt.size(1)] * b if l2 is None else l2
    dist1, dist2 = chamfer_ragged(moved, gt, l1, l2)
    return masked_mean(dist1, l1) + masked_mean(dist2, l2), found
