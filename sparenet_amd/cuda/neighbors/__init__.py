"""Neighbourhood queries between two clouds and the gathers over their result (include/ops/neighbors.h states the
rules; sparenet_amd/csrc/neighbors.hip).  Names and argument order follow pointnet2_ops, beside furthest_point_sample
(sparenet_amd.cuda.fps) and gather_operation (sparenet_amd.cuda.MDS):

    ball_query(radius, nsample, xyz [B,N,3], new_xyz [B,M,3], lengths=None, new_lengths=None, pad="first",
               return_count=False) -> idx [B,M,nsample] int32 (, cnt [B,M] int32)
        the first nsample points (ascending index) with squared distance < radius^2 of each query.  pad="first" fills
        the remaining slots with the first hit (PointNet++), pad="none" with -1 (PyTorch3D).  A query WITHOUT a hit
        gets -1 in every slot under both (PointNet++ would return index 0, an unrelated point).
    knn_query(k, xyz, new_xyz, lengths=None, new_lengths=None) -> (dist2 [B,M,k], idx [B,M,k] int32), 1 <= k <= 32
        the k nearest points of each query, nearest first, equal distances by lower index; -1 / +inf beyond the cloud.
    three_nn(unknown [B,M,3], known [B,N,3]) -> (dist [B,M,3], idx [B,M,3])      dist = sqrt(dist2), as PointNet++
    grouping_operation(features [B,C,N], idx [B,M,S]) -> [B,C,M,S]               differentiable in features
    three_interpolate(features [B,C,N], idx [B,M,S], weight [B,M,S]) -> [B,C,M]  differentiable in features only
    interpolate_features(unknown, known, known_feats [B,C,N], k=3, eps=1e-8) -> [B,C,M]

The searches are not differentiable, bit-reproducible, and independent of the batch.  `lengths` / `new_lengths` make
the batch ragged as in sparenet_amd.cuda.ragged: rows past a cloud's length are never read into a result, a padding
query's row is -1 / +inf / cnt 0.  An index of -1 gathers 0.0 and receives no gradient.  The backward sums in an order
that is not fixed: accurate to the bound of an fp32 sum, not bit-reproducible.  There is no host path: a CPU tensor
raises SparenetHipError.
"""
import torch
from torch.autograd import Function

from sparenet_amd import _lib
from sparenet_amd.cuda import _args

MAX_K = 32


def _clouds(what, xyz, new_xyz):
    """The pair as contiguous fp32 device tensors, and (b, n, m)."""
    _args.check_pair(what, "xyz", xyz, "new_xyz", new_xyz, device="contiguous")
    return _args.fp32(xyz), _args.fp32(new_xyz), xyz.size(0), xyz.size(1), new_xyz.size(1)


def _lengths(lengths, new_lengths, b, n, m, dev):
    return (_args.optional_lengths(lengths, b, n, dev, "lengths"),
            _args.optional_lengths(new_lengths, b, m, dev, "new_lengths"))


class BallQuery(Function):
    @staticmethod
    def forward(ctx, radius, nsample, xyz, new_xyz, lengths, new_lengths, pad, return_count):
        if pad not in ("first", "none"):
            raise ValueError(f"ball_query: pad must be 'first' or 'none', got {pad!r}")
        nsample = _args.check_count("ball_query", "nsample", nsample)
        radius = float(radius)
        if not 0.0 <= radius < float("inf"):
            raise ValueError(f"ball_query: radius must be finite and >= 0, got {radius!r}")
        xyz, new_xyz, b, n, m = _clouds("ball_query", xyz, new_xyz)
        lens, new_lens = _lengths(lengths, new_lengths, b, n, m, xyz.device)
        idx = torch.empty(b, m, nsample, device=xyz.device, dtype=torch.int32)
        cnt = torch.empty(b, m, device=xyz.device, dtype=torch.int32) if return_count else None
        ws = _lib.op_workspace("neighbors", "sn_neighbors_workspace_bytes", xyz, b, n, m, nsample)
        _lib.op_call("neighbors", "sn_ball_query", xyz, new_xyz, b, n, m, radius, nsample, int(pad == "first"), lens,
                     new_lens, idx, cnt, ws)
        if return_count:
            ctx.mark_non_differentiable(idx, cnt)
            return idx, cnt
        ctx.mark_non_differentiable(idx)
        return idx

    @staticmethod
    def backward(ctx, *grads):
        return (None,) * 8


class KnnQuery(Function):
    @staticmethod
    def forward(ctx, k, xyz, new_xyz, lengths, new_lengths):
        k = _args.check_count("knn_query", "k", k, MAX_K)
        xyz, new_xyz, b, n, m = _clouds("knn_query", xyz, new_xyz)
        lens, new_lens = _lengths(lengths, new_lengths, b, n, m, xyz.device)
        idx = torch.empty(b, m, k, device=xyz.device, dtype=torch.int32)
        dist2 = torch.empty(b, m, k, device=xyz.device)
        ws = _lib.op_workspace("neighbors", "sn_neighbors_workspace_bytes", xyz, b, n, m, k)
        _lib.op_call("neighbors", "sn_knn_query", xyz, new_xyz, b, n, m, k, lens, new_lens, idx, dist2, ws)
        ctx.mark_non_differentiable(dist2, idx)
        return dist2, idx

    @staticmethod
    def backward(ctx, *grads):
        return (None,) * 5


def ball_query(radius, nsample, xyz, new_xyz, lengths=None, new_lengths=None, pad="first", return_count=False):
    """idx [B, M, nsample] int32 -- and cnt [B, M] int32 with return_count -- of the points of xyz [B, N, 3] inside
    the ball of `radius` around each query of new_xyz [B, M, 3] (see the module's text)."""
    return BallQuery.apply(radius, nsample, xyz, new_xyz, lengths, new_lengths, pad, bool(return_count))


def knn_query(k, xyz, new_xyz, lengths=None, new_lengths=None):
    """(dist2 [B, M, k] fp32, idx [B, M, k] int32): the k nearest points of xyz [B, N, 3] to each query of
    new_xyz [B, M, 3], nearest first (see the module's text)."""
    return KnnQuery.apply(k, xyz, new_xyz, lengths, new_lengths)


def three_nn(unknown, known):
    """(dist [B, M, 3], idx [B, M, 3] int32): the three nearest points of known [B, N, 3] to each point of
    unknown [B, M, 3]; dist is the distance itself, sqrt(dist2), as PointNet++ returns it."""
    dist2, idx = knn_query(3, known, unknown)
    return torch.sqrt(dist2), idx


def _gather_args(what, features, idx, weight=None):
    """(features fp32 [B,C,N], idx int32 [B,M,S], weight fp32 [B,M,S] or None), contiguous, on features' device."""
    if not isinstance(features, torch.Tensor) or features.dim() != 3 or features.numel() == 0:
        raise ValueError(f"{what}: features must be a non-empty [B, C, N] tensor")
    if not features.is_floating_point():
        raise TypeError(f"{what}: features must be a floating-point tensor, got {features.dtype}")
    if not isinstance(idx, torch.Tensor) or idx.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"{what}: idx must be an int32 / int64 tensor")
    if idx.dim() != 3 or idx.size(0) != features.size(0) or idx.numel() == 0:
        raise ValueError(f"{what}: idx must be a non-empty [B, M, S] tensor with features' batch size, got "
                         f"{tuple(idx.shape)}")
    if weight is not None:
        if not isinstance(weight, torch.Tensor) or not weight.is_floating_point():
            raise TypeError(f"{what}: weight must be a floating-point tensor")
        if weight.shape != idx.shape:
            raise ValueError(f"{what}: weight must have idx's shape {tuple(idx.shape)}, got {tuple(weight.shape)}")
    _lib.require_device(features, "features")      # CPU tensors are refused before anything is uploaded
    _lib.require_device(idx, "idx")
    if weight is not None:
        _lib.require_device(weight, "weight")
        weight = _args.fp32(weight)
    return _args.fp32(features), idx.to(torch.int32).contiguous(), weight


def _backward(ctx, grad_out):
    """The shared backward of grouping (ctx.weight is None) and interpolation."""
    idx, weight = ctx.saved_tensors if ctx.weighted else (ctx.saved_tensors[0], None)
    b, c, n = ctx.shape
    m, s = idx.size(1), idx.size(2)
    grad_features = torch.empty(b, c, n, device=idx.device)
    ws = _lib.op_workspace("neighbors", "sn_group_backward_workspace_bytes", idx, b, n, m, s)
    _lib.op_call("neighbors", "sn_group_backward", grad_out.contiguous().float(), idx, weight, b, c, n, m, s,
                 grad_features, ws)
    return grad_features


class GroupingOperation(Function):
    @staticmethod
    def forward(ctx, features, idx):
        features, idx, _ = _gather_args("grouping_operation", features, idx)
        b, c, n = features.shape
        m, s = idx.size(1), idx.size(2)
        out = torch.empty(b, c, m, s, device=features.device)
        _lib.op_call("neighbors", "sn_group_forward", features, idx, b, c, n, m, s, out)
        ctx.save_for_backward(idx)
        ctx.weighted, ctx.shape = False, (b, c, n)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        return _backward(ctx, grad_out), None


class ThreeInterpolate(Function):
    @staticmethod
    def forward(ctx, features, idx, weight):
        features, idx, weight = _gather_args("three_interpolate", features, idx, weight)
        b, c, n = features.shape
        m, s = idx.size(1), idx.size(2)
        out = torch.empty(b, c, m, device=features.device)
        _lib.op_call("neighbors", "sn_interpolate_forward", features, idx, weight, b, c, n, m, s, out)
        ctx.save_for_backward(idx, weight)
        ctx.weighted, ctx.shape = True, (b, c, n)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        return _backward(ctx, grad_out), None, None


def grouping_operation(features, idx):
    """features [B, C, N], idx [B, M, S] (int32 / int64) -> [B, C, M, S] = features[b, c, idx[b, m, s]], 0.0 where idx
    is -1.  Differentiable in features: a point grouped several times collects every copy's gradient."""
    return GroupingOperation.apply(features, idx)


def three_interpolate(features, idx, weight):
    """features [B, C, N], idx [B, M, S], weight [B, M, S] -> [B, C, M] = sum over the S slots of weight * features at
    idx, slots left to right, a -1 slot skipped.  Any S, not only 3.  Differentiable in features only: weight is a
    constant, as in PointNet++ (no gradient flows to it, nor through it to the coordinates)."""
    return ThreeInterpolate.apply(features, idx, weight)


def interpolate_features(unknown, known, known_feats, k=3, eps=1e-8):
    """known_feats [B, C, N] at the points known [B, N, 3], carried to unknown [B, M, 3] by inverse-distance weights
    over the k nearest known points: the feature propagation step of PointNet++."""
    dist2, idx = knn_query(k, known, unknown)
    recip = 1.0 / (torch.sqrt(dist2) + eps)      # an empty slot (+inf) weighs 0
    return three_interpolate(known_feats, idx, recip / recip.sum(dim=2, keepdim=True))
