"""Chamfer and EMD for zero-padded batches of clouds with different numbers of points.

A ragged batch is a dense fp32 tensor [B, N, 3] plus lengths [B]: the first lengths[i] rows of cloud i are its points,
the rest is padding (the contract is stated in include/sparenet_hip.h).  Padding rows are never read -- they may hold
NaN -- and come back with distance 0, index / assignment -1 and gradient 0; a cloud's valid rows get exactly what the
dense op gives for that cloud alone, bit for bit, whatever else is in the batch.

    pad_compact(xyz)                               -> packed, lengths, src    zero rows (the reference's padding) -> ragged
    chamfer_ragged(xyz1, xyz2, lengths1, lengths2) -> dist1, dist2
    emd_ragged(xyz1, xyz2, lengths1, lengths2, eps, iters) -> dist, assignment    needs lengths1 <= lengths2 per cloud
    chamfer_search_raw(xyz1, xyz2, lengths1=None, lengths2=None) -> the one search, dense or ragged, without autograd
    masked_mean(dist, lengths)                     -> [B]

`lengths` is an int32 / int64 tensor on any device, or a list.  Host values are range-checked and uploaded; a device
tensor is used as it is, without a host read (the kernels hold its values to [0, N]).  CPU clouds are accepted by
chamfer_ragged only, as by the dense ops: it loops over the clouds through the library's host Chamfer.
"""
import torch
from torch.autograd import Function

from sparenet_amd import _lib
from sparenet_amd.cuda.chamfer_distance.chamfer_distance import cd


def device_lengths(lengths, b, width, dev, name):
    """(int32 tensor [b] on dev, host list or None): host values are range-checked and uploaded, device values are not
    read.  A caller of several ragged ops converts once and hands the tensor on: it then passes through as it is."""
    if isinstance(lengths, torch.Tensor):
        if lengths.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"{name}: expected an int32 / int64 tensor or a list, got dtype {lengths.dtype}")
        if lengths.dim() != 1 or lengths.numel() != b:
            raise ValueError(f"{name}: expected {b} lengths, got shape {tuple(lengths.shape)}")
        if lengths.is_cuda and dev.type == "cuda":
            return lengths.to(device=dev, dtype=torch.int32).contiguous(), None
        host = [int(v) for v in lengths.tolist()]
    else:
        host = [int(v) for v in lengths]
        if len(host) != b:
            raise ValueError(f"{name}: expected {b} lengths, got {len(host)}")
    bad = [(i, v) for i, v in enumerate(host) if v < 0 or v > width]
    if bad:
        raise ValueError(f"{name}: lengths must be in [0, {width}]; cloud {bad[0][0]} has {bad[0][1]}")
    return torch.tensor(host, dtype=torch.int32, device=dev), host


def _check_pair(what, xyz1, xyz2):
    if xyz1.dim() != 3 or xyz2.dim() != 3 or xyz1.size(2) != 3 or xyz2.size(2) != 3:
        raise ValueError(f"{what}: expected [B, N, 3] and [B, M, 3], got {tuple(xyz1.shape)} and {tuple(xyz2.shape)}")
    if xyz1.size(0) != xyz2.size(0) or xyz1.size(0) == 0 or xyz1.size(1) == 0 or xyz2.size(1) == 0:
        raise ValueError(f"{what}: batch sizes differ or a tensor is empty")
    if xyz1.device != xyz2.device:
        raise ValueError(f"{what}: xyz1 and xyz2 are on different devices")


# ---------------------------------------------------------------------------------------------------- pad_compact
class PadCompactFunction(Function):
    @staticmethod
    def forward(ctx, xyz):
        if xyz.dim() != 3 or xyz.size(2) != 3 or xyz.size(0) == 0 or xyz.size(1) == 0:
            raise ValueError(f"pad_compact: expected [B, N, 3], got {tuple(xyz.shape)}")
        xyz = xyz.contiguous().float()
        b, n, _ = xyz.shape
        packed = torch.empty_like(xyz)
        lengths = torch.empty(b, dtype=torch.int32, device=xyz.device)
        src = torch.empty(b, n, dtype=torch.int32, device=xyz.device)
        _lib.call("sn_pad_compact", xyz, b, n, packed, lengths, src)
        ctx.save_for_backward(src)
        ctx.mark_non_differentiable(lengths, src)
        return packed, lengths, src

    @staticmethod
    def backward(ctx, grad_packed, _gl, _gs):
        (src,) = ctx.saved_tensors
        return scatter_rows(grad_packed.contiguous().float(), src)


def scatter_rows(rows, src):
    """rows [B, N, C] of a packed batch back to their original places (src of pad_compact); 0 at padding rows."""
    b, n = src.shape
    c = rows.numel() // (b * n)
    out = torch.empty_like(rows)
    _lib.call("sn_pad_scatter_rows", rows, src, b, n, c, out)
    return out


def pad_compact(xyz):
    """xyz [B, N, 3] with the reference's padding (rows with (x + y) + z == 0) -> (packed [B, N, 3]: every cloud's
    points first, in their order; lengths [B] int32; src [B, N] int32: the original row of each packed row, -1 beyond
    the length).  Gradients of `packed` flow back to the rows they came from."""
    return PadCompactFunction.apply(xyz)


# -------------------------------------------------------------------------------------------------------- Chamfer
def _chamfer_host(xyz1, xyz2, h1, h2, dist1, dist2, idx1, idx2):
    """CPU tensors: cloud by cloud through the library's host Chamfer, on the valid slices."""
    dist1.zero_(), dist2.zero_(), idx1.fill_(-1), idx2.fill_(-1)
    for i, (n, m) in enumerate(zip(h1, h2)):
        if n == 0 or m == 0:
            continue
        d1, d2 = torch.empty(1, n), torch.empty(1, m)
        i1, i2 = torch.empty(1, n, dtype=torch.int), torch.empty(1, m, dtype=torch.int)
        cd.forward(xyz1[i:i + 1, :n].contiguous(), xyz2[i:i + 1, :m].contiguous(), d1, d2, i1, i2)
        dist1[i, :n], dist2[i, :m], idx1[i, :n], idx2[i, :m] = d1[0], d2[0], i1[0], i2[0]


def _chamfer_host_backward(xyz1, xyz2, h1, h2, gd1, gd2, idx1, idx2, g1, g2):
    g1.zero_(), g2.zero_()
    for i, (n, m) in enumerate(zip(h1, h2)):
        if n == 0 or m == 0:
            continue
        a, b = torch.empty(1, n, 3), torch.empty(1, m, 3)
        cd.backward(xyz1[i:i + 1, :n].contiguous(), xyz2[i:i + 1, :m].contiguous(), a, b,
                    gd1[i:i + 1, :n].contiguous(), gd2[i:i + 1, :m].contiguous(),
                    idx1[i:i + 1, :n].contiguous(), idx2[i:i + 1, :m].contiguous())
        g1[i, :n], g2[i, :m] = a[0], b[0]


def chamfer_ragged_forward_raw(xyz1, xyz2, lengths1, lengths2):
    """(dist1, dist2, idx1, idx2, xyz1, xyz2, lengths1, lengths2) without autograd: idx = lowest index of the nearest
    neighbour, -1 at padding; the inputs come back as the contiguous fp32 / int32 tensors the kernels read."""
    _check_pair("chamfer_ragged", xyz1, xyz2)
    xyz1 = xyz1.contiguous().float()
    xyz2 = xyz2.contiguous().float()
    b, n, _ = xyz1.shape
    m = xyz2.size(1)
    dev = xyz1.device
    l1, h1 = device_lengths(lengths1, b, n, dev, "lengths1")
    l2, h2 = device_lengths(lengths2, b, m, dev, "lengths2")
    dist1 = torch.empty(b, n, device=dev)
    dist2 = torch.empty(b, m, device=dev)
    idx1 = torch.empty(b, n, dtype=torch.int, device=dev)
    idx2 = torch.empty(b, m, dtype=torch.int, device=dev)
    if not xyz1.is_cuda:
        _chamfer_host(xyz1, xyz2, h1, h2, dist1, dist2, idx1, idx2)
    else:
        _lib.call("sn_chamfer_forward_ragged", xyz1, xyz2, b, n, m, l1, l2, dist1, idx1, dist2, idx2)
    return dist1, dist2, idx1, idx2, xyz1, xyz2, l1, l2


def chamfer_search_raw(xyz1, xyz2, lengths1=None, lengths2=None):
    """(dist1, dist2, idx1, idx2, xyz1, xyz2, l1, l2) of the one Chamfer search of a pair, without autograd: a dense
    batch through cd.forward_cuda (CPU tensors: the host Chamfer) with l1 = l2 = None, a ragged one -- either lengths
    given; None = every row -- through chamfer_ragged_forward_raw.  The clouds come back contiguous and fp32."""
    if lengths1 is not None or lengths2 is not None:
        b = xyz1.size(0)
        lengths1 = [xyz1.size(1)] * b if lengths1 is None else lengths1
        lengths2 = [xyz2.size(1)] * b if lengths2 is None else lengths2
        return chamfer_ragged_forward_raw(xyz1, xyz2, lengths1, lengths2)
    xyz1, xyz2 = xyz1.contiguous().float(), xyz2.contiguous().float()
    b, n, m, dev = xyz1.size(0), xyz1.size(1), xyz2.size(1), xyz1.device
    dist1, dist2 = torch.empty(b, n, device=dev), torch.empty(b, m, device=dev)
    idx1 = torch.empty(b, n, dtype=torch.int, device=dev)
    idx2 = torch.empty(b, m, dtype=torch.int, device=dev)
    (cd.forward_cuda if xyz1.is_cuda else cd.forward)(xyz1, xyz2, dist1, dist2, idx1, idx2)
    return dist1, dist2, idx1, idx2, xyz1, xyz2, None, None


class ChamferRaggedFunction(Function):
    @staticmethod
    def forward(ctx, xyz1, xyz2, lengths1, lengths2):
        dist1, dist2, idx1, idx2, xyz1, xyz2, l1, l2 = chamfer_ragged_forward_raw(xyz1, xyz2, lengths1, lengths2)
        ctx.save_for_backward(xyz1, xyz2, idx1, idx2, l1, l2)
        return dist1, dist2

    @staticmethod
    def backward(ctx, graddist1, graddist2):
        xyz1, xyz2, idx1, idx2, l1, l2 = ctx.saved_tensors
        graddist1 = graddist1.contiguous().float()
        graddist2 = graddist2.contiguous().float()
        gradxyz1 = torch.empty_like(xyz1)
        gradxyz2 = torch.empty_like(xyz2)
        b, n, _ = xyz1.shape
        m = xyz2.size(1)
        if not xyz1.is_cuda:
            _chamfer_host_backward(xyz1, xyz2, l1.tolist(), l2.tolist(), graddist1, graddist2, idx1, idx2,
                                   gradxyz1, gradxyz2)
            return gradxyz1, gradxyz2, None, None
        ws = _lib.workspace("sn_chamfer_backward_ragged_workspace_bytes", xyz1, b, n, m)
        _lib.call("sn_chamfer_backward_ragged", xyz1, xyz2, graddist1, graddist2, idx1, idx2, b, n, m, l1, l2,
                  gradxyz1, gradxyz2, ws)
        return gradxyz1, gradxyz2, None, None


def chamfer_ragged(xyz1, xyz2, lengths1, lengths2):
    """(dist1 [B, N], dist2 [B, M]): squared nearest-neighbour distances both ways between the first lengths1[i] rows
    of xyz1[i] and the first lengths2[i] rows of xyz2[i]; 0 at padding rows and for a cloud with an empty side.
    Differentiable in both clouds."""
    return ChamferRaggedFunction.apply(xyz1, xyz2, lengths1, lengths2)


# ------------------------------------------------------------------------------------------------------------ EMD
class EmdRaggedFunction(Function):
    @staticmethod
    def forward(ctx, xyz1, xyz2, lengths1, lengths2, eps, iters):
        _check_pair("emd_ragged", xyz1, xyz2)
        xyz1 = xyz1.contiguous().float()
        xyz2 = xyz2.contiguous().float()
        b, n, _ = xyz1.shape
        m = xyz2.size(1)
        dev = xyz1.device
        _lib.require_device(xyz1, "xyz1")      # CPU tensors are refused before anything is uploaded
        l1, h1 = device_lengths(lengths1, b, n, dev, "lengths1")
        l2, h2 = device_lengths(lengths2, b, m, dev, "lengths2")
        dist = torch.empty(b, n, device=dev)
        assignment = torch.empty(b, n, device=dev, dtype=torch.int32)
        ws = _lib.workspace("sn_emd_ragged_workspace_bytes", xyz1, b, n, m)
        _lib.call("sn_emd_forward_ragged", xyz1, xyz2, b, n, m, l1, l2, eps, iters, dist, assignment, ws, None)
        ctx.save_for_backward(xyz1, xyz2, assignment, l1, l2)
        ctx.mark_non_differentiable(assignment)
        return dist, assignment

    @staticmethod
    def backward(ctx, graddist, _ga):
        xyz1, xyz2, assignment, l1, l2 = ctx.saved_tensors
        graddist = graddist.contiguous().float()
        b, n, _ = xyz1.shape
        m = xyz2.size(1)
        need2 = ctx.needs_input_grad[1]
        gradxyz1 = torch.empty_like(xyz1)
        gradxyz2 = torch.empty_like(xyz2) if need2 else None
        # without gradxyz2 (None: a null pointer) the library needs no workspace either
        ws = _lib.workspace("sn_emd_ragged_backward_workspace_bytes", xyz1, b, n, m) if need2 else None
        _lib.call("sn_emd_backward_ragged", xyz1, xyz2, graddist, assignment, b, n, m, l1, l2, gradxyz1, gradxyz2, ws)
        return gradxyz1, gradxyz2, None, None, None, None


def emd_ragged(xyz1, xyz2, lengths1, lengths2, eps, iters):
    """(dist [B, N], assignment [B, N] int32) of the auction EMD of the first lengths1[i] rows of xyz1[i] (the bidders)
    against the first lengths2[i] rows of xyz2[i]; needs 1 <= lengths1[i] <= lengths2[i].  A cloud that does not
    satisfy it comes back with a NaN dist row, assignment -1 and zero gradients (lengths given as host values are
    not refused for it either: the batch's other clouds are served).  Differentiable in both clouds."""
    return EmdRaggedFunction.apply(xyz1, xyz2, lengths1, lengths2, eps, iters)


# ---------------------------------------------------------------------------------------------------- reductions
def valid_mask(lengths, width, device):
    """[B, width] bool: True at the rows that are points."""
    if not isinstance(lengths, torch.Tensor):
        lengths = torch.tensor([int(v) for v in lengths], dtype=torch.int64)
    return torch.arange(width, device=device)[None, :] < lengths.to(device)[:, None]


def mean_over_mask(values, mask):
    """[B] float64: the sum of the float64 `values` [B, W] at the bool `mask` over their number, 0 where there is
    none."""
    total = torch.where(mask, values, torch.zeros((), dtype=torch.float64, device=values.device)).sum(dim=1)
    count = mask.sum(dim=1)
    return torch.where(count > 0, total / count.clamp_min(1), torch.zeros_like(total))


def masked_mean(dist, lengths):
    """[B]: the sum of dist[i, :lengths[i]] divided by lengths[i], 0 for an empty cloud.  Accumulated in float64 and
    rounded once to dist's dtype, so the padded width does not enter the value; padding rows are not read into it."""
    return mean_over_mask(dist.double(), valid_mask(lengths, dist.size(1), dist.device)).to(dist.dtype)
