"""Normals and local geometry from neighbourhoods (include/ops/local_pca.h states the rule;
sparenet_amd/csrc/local_pca.hip), and the surface-aware metrics built on them:

    local_pca(xyz [B,N,3], idx [B,M,k], new_xyz=None, viewpoint=None, return_frames=False)
        -> (normals [B,M,3] fp32, eigenvalues [B,M,3] float64 ascending[, frames [B,M,3,3] fp32])
    surface_variation(eigenvalues) -> l0 / (l0 + l1 + l2)
    estimate_normals(xyz, k=16, lengths=None, viewpoint=None, return_curvature=False) -> normals [B,N,3] (, [B,N])
    normal_consistency(xyz1, xyz2, normals1=None, normals2=None, k=16, lengths1=None, lengths2=None) -> [B]
    point_to_plane_chamfer(xyz1, xyz2, normals2, lengths1=None, lengths2=None) -> [B]   differentiable in the clouds

`idx` is the table knn_query or ball_query wrote (sparenet_amd.cuda.neighbors): -1 is an empty slot and is skipped, and
a repeated index counts as often as it occurs -- so take ball_query's table with pad="none", not with the PointNet++
padding that repeats the first hit.  Per query the covariance of the named points is built and solved in double
(cyclic Jacobi) and rounded once: frames[..., r, :] is the unit eigenvector of eigenvalue r, row 0 the normal, row 2
the principal direction, row 1 = row 2 x row 0.  Signs: the component of largest magnitude of row 2 and of the normal
is positive; with `viewpoint` ([3] or [B,3]) and the query points `new_xyz` the normal looks at the viewpoint instead.
A query without a valid slot gets 0 everywhere.  Two calls give identical bits, a cloud's rows do not depend on the
batch, and nothing here is differentiable through the decomposition.
"""
import torch
from torch.autograd import Function

from sparenet_amd import _lib
from sparenet_amd.cuda import _args
from sparenet_amd.cuda.ragged import chamfer_search_raw, mean_over_mask, valid_mask

MAX_K = 64


def _viewpoint(what, viewpoint, b, like):
    """[B,3] fp32 contiguous on `like`'s device from a [3] or [B,3] tensor or sequence."""
    v = torch.as_tensor(viewpoint, dtype=torch.float32).to(like.device)
    if v.dim() == 1 and v.numel() == 3:
        v = v[None, :].expand(b, 3)
    if tuple(v.shape) != (b, 3):
        raise ValueError(f"{what}: viewpoint must be [3] or [{b}, 3], got {tuple(v.shape)}")
    return v.contiguous()


class LocalPca(Function):
    @staticmethod
    def forward(ctx, xyz, idx, new_xyz, viewpoint, return_frames):
        what = "local_pca"
        _args.check_cloud(what, "xyz", xyz)
        if not isinstance(idx, torch.Tensor) or idx.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"{what}: idx must be an int32 / int64 tensor")
        b, n = xyz.size(0), xyz.size(1)
        if idx.dim() != 3 or idx.size(0) != b or idx.size(1) == 0:
            raise ValueError(f"{what}: idx must be a [B, M, k] tensor with xyz's batch size, got {tuple(idx.shape)}")
        m, k = idx.size(1), idx.size(2)
        if not 1 <= k <= MAX_K:
            raise ValueError(f"{what}: k must be in 1..{MAX_K}, got {k}")
        if idx.device != xyz.device:
            raise ValueError(f"{what}: idx is on {idx.device}, xyz on {xyz.device}")
        if viewpoint is not None:
            if new_xyz is None:
                raise ValueError(f"{what}: a viewpoint needs new_xyz, the query points")
            viewpoint = _viewpoint(what, viewpoint, b, xyz)
        if new_xyz is not None:
            if not isinstance(new_xyz, torch.Tensor) or tuple(new_xyz.shape) != (b, m, 3):
                raise ValueError(f"{what}: new_xyz must be a [{b}, {m}, 3] tensor")
            if new_xyz.device != xyz.device:
                raise ValueError(f"{what}: new_xyz is on {new_xyz.device}, xyz on {xyz.device}")
            new_xyz = _args.fp32(new_xyz)
        xyz, idx, dev = _args.fp32(xyz), idx.to(torch.int32).contiguous(), xyz.device
        normals = torch.empty(b, m, 3, device=dev)
        eigenvalues = torch.empty(b, m, 3, dtype=torch.float64, device=dev)
        frames = torch.empty(b, m, 3, 3, device=dev) if return_frames else None
        args = (xyz, idx, b, n, m, k, new_xyz, viewpoint, eigenvalues, frames, normals)
        if xyz.is_cuda:
            _lib.op_call("local_pca", "sn_local_pca", *args, None)
        else:
            _lib.op_call("local_pca", "sn_local_pca_host", *args, 0, host=True)
        if return_frames:
            ctx.mark_non_differentiable(normals, eigenvalues, frames)
            return normals, eigenvalues, frames
        ctx.mark_non_differentiable(normals, eigenvalues)
        return normals, eigenvalues

    @staticmethod
    def backward(ctx, *grads):
        return (None,) * 5


def local_pca(xyz, idx, new_xyz=None, viewpoint=None, return_frames=False):
    """(normals [B,M,3] fp32, eigenvalues [B,M,3] float64, ascending[, frames [B,M,3,3] fp32]) of the neighbourhoods
    idx [B,M,k] (1 <= k <= 64, -1 = empty slot) names among the points xyz [B,N,3] (see the module's text).  With
    `viewpoint` ([3] or [B,3]) the normals look at it from the query points new_xyz [B,M,3], which are then required.
    Device tensors, or CPU tensors throughout (the host entry point).  Not differentiable."""
    return LocalPca.apply(xyz, idx, new_xyz, viewpoint, bool(return_frames))


def surface_variation(eigenvalues):
    """l0 / (l0 + l1 + l2) of eigenvalues [..., 3] (ascending, as local_pca returns them): Pauly's surface variation, 0
    on a plane and 1/3 at most; 0 where the trace is 0.  The dtype of the input."""
    trace = eigenvalues.sum(dim=-1)
    flat = trace == 0
    return torch.where(flat, torch.zeros_like(trace), eigenvalues[..., 0] / torch.where(flat, torch.ones_like(trace), trace))


def estimate_normals(xyz, k=16, lengths=None, viewpoint=None, return_curvature=False):
    """normals [B,N,3] fp32 of the cloud xyz [B,N,3] from each point's k nearest neighbours, the point itself among them
    (as Open3D and PyTorch3D count): knn_query(k, xyz, xyz, lengths, lengths), then local_pca; 1 <= k <= 32.  With
    `viewpoint` ([3] or [B,3]) the normals look at it.  `lengths` makes the batch ragged; padding rows get 0.
    return_curvature=True: (normals, surface variation [B,N] fp32).  Device tensors only: a CPU tensor raises as
    knn_query does."""
    from sparenet_amd.cuda.neighbors import knn_query

    _, idx = knn_query(k, xyz, xyz, lengths, lengths)
    normals, eigenvalues = local_pca(xyz, idx, xyz if viewpoint is not None else None, viewpoint)
    if return_curvature:
        return normals, surface_variation(eigenvalues).float()
    return normals


def _valid_rows(idx, lengths, width):
    """[B, width] bool: the rows that are points and found a neighbour."""
    found = idx >= 0
    return found if lengths is None else found & valid_mask(lengths, width, idx.device)


def _rows_of(t, idx):
    """t[b, idx[b, i], :] for t [B,M,C] and idx [B,N] (any value at idx < 0; the caller masks those rows)."""
    return torch.gather(t, 1, idx.clamp_min(0).long()[:, :, None].expand(-1, -1, t.size(2)))


def normal_consistency_from_search(idx1, idx2, normals1, normals2, lengths1=None, lengths2=None):
    """[B] fp32 from the Chamfer search's idx1 [B,N] / idx2 [B,M] and the normals of both clouds: for callers that hold
    the search already.  lengths as int32 tensors on the normals' device (or None)."""
    n1, n2 = normals1.detach().double(), normals2.detach().double()
    v1, v2 = _valid_rows(idx1, lengths1, n1.size(1)), _valid_rows(idx2, lengths2, n2.size(1))
    side1 = mean_over_mask((n1 * _rows_of(n2, idx1)).sum(dim=2).abs(), v1)
    side2 = mean_over_mask((n2 * _rows_of(n1, idx2)).sum(dim=2).abs(), v2)
    return (0.5 * (side1 + side2)).float()


def _normals_of(what, name, normals, xyz, k, lengths):
    if normals is None:
        return estimate_normals(xyz, k, lengths)
    if not isinstance(normals, torch.Tensor) or normals.shape != xyz.shape or not normals.is_floating_point():
        raise ValueError(f"{what}: {name} must be a floating-point tensor of its cloud's shape {tuple(xyz.shape)}")
    if normals.device != xyz.device:
        raise ValueError(f"{what}: {name} is on {normals.device}, its cloud on {xyz.device}")
    return normals


def normal_consistency(xyz1, xyz2, normals1=None, normals2=None, k=16, lengths1=None, lengths2=None):
    """[B] fp32 in [0, 1]: 0.5 * (mean_i |n1_i . n2[idx1_i]| + mean_j |n2_j . n1[idx2_j]|) over the nearest neighbours
    idx1 / idx2 of the ONE Chamfer search of the pair -- the normal-consistency metric reported beside the Chamfer
    distance and the F-score; the sign of a normal does not enter it.  Dot products in double, float64 means over the
    valid rows, rounded once.  Missing normals are estimated with estimate_normals(., k) (device tensors only; with
    both normals given CPU tensors work too).  `lengths1` / `lengths2` make the batch ragged; a pair with an empty
    side gives 0.  Not differentiable."""
    what = "normal_consistency"
    _args.check_pair(what, "xyz1", xyz1, "xyz2", xyz2, same_device=True)
    normals1 = _normals_of(what, "normals1", normals1, xyz1, k, lengths1)
    normals2 = _normals_of(what, "normals2", normals2, xyz2, k, lengths2)
    _, _, idx1, idx2, _, _, l1, l2 = chamfer_search_raw(xyz1.detach(), xyz2.detach(), lengths1, lengths2)
    return normal_consistency_from_search(idx1, idx2, normals1, normals2, l1, l2)


def _gather_points(points, idx):
    """points[b, idx[b, i], :] as [B,N,3], differentiable in points: on the device through grouping_operation, whose
    backward is the library's sum over inverse lists (no floating-point atomics); torch.gather on CPU tensors."""
    if not points.is_cuda:
        return _rows_of(points, idx)
    from sparenet_amd.cuda.neighbors import grouping_operation

    return grouping_operation(points.transpose(1, 2).contiguous(), idx[:, :, None])[:, :, :, 0].transpose(1, 2)


def point_to_plane_chamfer(xyz1, xyz2, normals2, lengths1=None, lengths2=None):
    """[B] fp32: mean_i (n2[idx1_i] . (x_i - y[idx1_i]))^2 + mean_j (n2_j . (y_j - x[idx2_j]))^2 with the nearest
    neighbours idx1 / idx2 of the Chamfer search of the pair and normals2 [B,M,3], the normals of xyz2 (the ground
    truth): squared distances to the tangent planes of xyz2, both ways.  Indices and normals are constants; the value
    is differentiable in xyz1 and xyz2 through torch autograd over the gathers.  On the device the gathers' backward is
    grouping_operation's: accurate to the bound of an fp32 sum of the list's terms, NOT bit-reproducible (as
    include/ops/neighbors.h says of its own).  `lengths1` / `lengths2` make the batch ragged: padding rows are never
    read into the value and get gradient 0; a pair with an empty side gives 0."""
    what = "point_to_plane_chamfer"
    _args.check_pair(what, "xyz1", xyz1, "xyz2", xyz2, same_device=True)
    if normals2 is None:
        raise ValueError(f"{what}: normals2, the normals of xyz2, are required")
    normals = _normals_of(what, "normals2", normals2, xyz2, None, None).detach().float()
    _, _, idx1, idx2, _, _, l1, l2 = chamfer_search_raw(xyz1.detach(), xyz2.detach(), lengths1, lengths2)
    v1, v2 = _valid_rows(idx1, l1, xyz1.size(1)), _valid_rows(idx2, l2, xyz2.size(1))
    zero = torch.zeros((), device=xyz1.device)
    x, y = xyz1.float(), xyz2.float()
    if l1 is not None:      # padding rows may hold NaN: they are replaced before anything is computed from them
        x = torch.where(valid_mask(l1, x.size(1), x.device)[:, :, None], x, zero)
        points = valid_mask(l2, y.size(1), y.device)[:, :, None]
        y, normals = torch.where(points, y, zero), torch.where(points, normals, zero)
    off1 = (_rows_of(normals, idx1) * (x - _gather_points(y, idx1))).sum(dim=2)
    off2 = (normals * (y - _gather_points(x, idx2))).sum(dim=2)
    side1 = torch.where(v1, off1 * off1, zero).sum(dim=1) / v1.sum(dim=1).clamp_min(1)
    side2 = torch.where(v2, off2 * off2, zero).sum(dim=1) / v2.sum(dim=1).clamp_min(1)
    return side1 + side2
