"""Validation metrics from one pass of the loss kernels.

The reference's `Metrics` (utils/misc.py:119-211) evaluates, per validation sample,
  F-Score@th   through open3d on the CPU: nearest-neighbour distances both ways, then
               precision = #{d(pred -> gt) < th} / |pred|, recall = #{d(gt -> pred) < th} / |gt|,
               F = 2 P R / (P + R)                                     (:178-190)
  ChamferDistance x 1000                                              (:198-201)
  EMD x 100 = mean sqrt(dist) of emdModule(eps 0.005, 50 iterations)  (:203-209)
The nearest-neighbour distances of the F-score are exactly the square roots of the Chamfer
distances the second metric computes anyway, so one Chamfer forward serves both and nothing
leaves the GPU.  d < th is evaluated as dist < th^2 on the fp32 squared distances (open3d works in
double on the same fp32 coordinates: the two can only disagree for |d - th| ~ 1e-9).
"""
import torch

from sparenet_amd.cuda import _args
from sparenet_amd.cuda.chamfer_distance.chamfer_distance import ChamferDistanceFunction
from sparenet_amd.cuda.emd.emd_general import emd_general
from sparenet_amd.cuda.emd.emd_module import emdModule
from sparenet_amd.cuda.ragged import chamfer_search_raw
from sparenet_amd.utils.set_metrics import set_metrics  # noqa: F401  (MMD-CD, COV-CD, 1-NNA-CD of two SETS of clouds)


def f_score_from_chamfer(dist1, dist2, th=0.01):
    """dist1 [B,N] = squared NN distance pred -> gt, dist2 [B,M] = gt -> pred; returns [B]."""
    th2 = float(th) * float(th)
    precision = (dist1 < th2).double().mean(dim=1)
    recall = (dist2 < th2).double().mean(dim=1)
    denom = precision + recall
    return torch.where(denom > 0, 2 * precision * recall / denom.clamp_min(1e-300),
                       torch.zeros_like(denom))


def fused_validation_metrics(pred, gt, th=0.01, emd_eps=0.005, emd_iters=50, with_emd=True, emd_any_size=False,
                             pred_lengths=None, gt_lengths=None, with_dcd=False, dcd_alpha=1000.0, dcd_n_lambda=1.0,
                             with_normals=False, normals_k=16):
    """pred [B,N,3], gt [B,M,3] on the GPU -> dict of per-sample tensors [B]:
    'F-Score', 'ChamferDistance' (x1000, mean dist1 + mean dist2, utils/misc.py:198-201 with
    ChamferDistanceMean) and 'EMD' (x100; needs N == M, a multiple of 1024).
    emd_any_size=True computes 'EMD' with emd_general for any N and M: the smaller cloud bids for the larger one
    (pred when N == M, the same value as the default path for N == M a multiple of 1024) and the mean runs over it.
    pred_lengths / gt_lengths (a list or an int tensor [B]; one may be left None = every row) make the batch ragged
    (sparenet_amd.cuda.ragged): cloud i is its first lengths[i] rows, the rest is padding that is never read.
    Precision and recall then count the valid rows, the means run over them: the distances are bit for bit those of a
    call on that cloud alone, and so is 'F-Score'.  The means ('ChamferDistance', 'EMD') are float64 sums over the valid
    rows rounded once to fp32, where the dense path takes torch's fp32 mean: the two agree to fp32 rounding, not bit
    for bit.
    'EMD' then needs emd_any_size=True and pred_lengths[i] <= gt_lengths[i] for every cloud (pred bids; checked when
    the lengths are host values).
    with_dcd=True adds 'DCD', the density-aware Chamfer distance (sparenet_amd.cuda.dcd) with dcd_alpha and
    dcd_n_lambda, from the SAME search: there is no second one, the other keys keep their bits, and -- the call being
    the distance op's own -- only 'DCD' carries a gradient then.
    with_normals=True adds 'NormalConsistency' (sparenet_amd.cuda.normals.normal_consistency, normals estimated from
    normals_k neighbours) from the SAME search as well: the other keys keep their bits; the search is then called
    without autograd, so 'ChamferDistance' carries no gradient."""
    if pred_lengths is not None or gt_lengths is not None:
        return _ragged_metrics(pred, gt, th, emd_eps, emd_iters, with_emd, emd_any_size, pred_lengths, gt_lengths,
                               with_dcd, dcd_alpha, dcd_n_lambda, with_normals, normals_k)
    if with_dcd:
        value, raw = _dcd_with_search(pred, gt, dcd_alpha, dcd_n_lambda)
        dist1, dist2 = raw["dist1"], raw["dist2"]
        found = (raw["idx1"], raw["idx2"])
    elif with_normals:
        dist1, dist2, *found = _plain_search(pred, gt)[:4]
    else:
        dist1, dist2 = ChamferDistanceFunction.apply(pred, gt)
    out = {"F-Score": f_score_from_chamfer(dist1, dist2, th),
           "ChamferDistance": (dist1.mean(dim=1) + dist2.mean(dim=1)) * 1000}
    if with_emd and emd_any_size:
        small, large = (pred, gt) if pred.size(1) <= gt.size(1) else (gt, pred)
        dist, _ = emd_general(small, large, emd_eps, emd_iters)
        out["EMD"] = torch.sqrt(dist).mean(dim=1) * 100
    elif with_emd:
        dist, _ = emdModule()(pred, gt, emd_eps, emd_iters)
        out["EMD"] = torch.sqrt(dist).mean(dim=1) * 100
    if with_dcd:
        out["DCD"] = value
    if with_normals:
        out["NormalConsistency"] = _consistency_from_search(pred, gt, found, normals_k)
    return out


def _plain_search(pred, gt, pred_lengths=None, gt_lengths=None):
    """(dist1, dist2, idx1, idx2, ...) of the one Chamfer search, without autograd: the distances' bits are those of
    the differentiable call."""
    _args.check_pair("fused_validation_metrics", "xyz1", pred, "xyz2", gt, same_device=True)
    return chamfer_search_raw(pred.detach(), gt.detach(), pred_lengths, gt_lengths)


def _consistency_from_search(pred, gt, found, k, pred_lengths=None, gt_lengths=None):
    from sparenet_amd.cuda.normals import estimate_normals, normal_consistency_from_search

    return normal_consistency_from_search(found[0], found[1], estimate_normals(pred.detach(), k, pred_lengths),
                                          estimate_normals(gt.detach(), k, gt_lengths), pred_lengths, gt_lengths)


def _dcd_with_search(pred, gt, alpha, n_lambda, pred_lengths=None, gt_lengths=None):
    """(DCD [B], the raw outputs of its one Chamfer search)."""
    from sparenet_amd.cuda.dcd import density_aware_chamfer

    return density_aware_chamfer(pred, gt, alpha, n_lambda, "none", pred_lengths, gt_lengths, return_raw=True)


def _ragged_metrics(pred, gt, th, emd_eps, emd_iters, with_emd, emd_any_size, pred_lengths, gt_lengths,
                    with_dcd=False, dcd_alpha=1000.0, dcd_n_lambda=1.0, with_normals=False, normals_k=16):
    from sparenet_amd.cuda.ragged import chamfer_ragged, device_lengths, emd_ragged, masked_mean, valid_mask

    b = pred.size(0)
    if pred_lengths is None:
        pred_lengths = [pred.size(1)] * b
    if gt_lengths is None:
        gt_lengths = [gt.size(1)] * b
    # converted (host values: range-checked and uploaded) once; every op below takes the device tensors as they are
    l1, hp = device_lengths(pred_lengths, b, pred.size(1), pred.device, "pred_lengths")
    l2, hg = device_lengths(gt_lengths, b, gt.size(1), gt.device, "gt_lengths")
    if with_emd:
        if not emd_any_size:
            raise ValueError("fused_validation_metrics: 'EMD' of a ragged batch needs emd_any_size=True")
        if hp is not None and hg is not None:
            bad = [i for i, (p, g) in enumerate(zip(hp, hg)) if p > g]
            if bad:
                raise ValueError(f"fused_validation_metrics: 'EMD' needs pred_lengths[i] <= gt_lengths[i] (pred bids for "
                                 f"gt); cloud {bad[0]} has {hp[bad[0]]} > {hg[bad[0]]}")
    if with_dcd:
        value, raw = _dcd_with_search(pred, gt, dcd_alpha, dcd_n_lambda, l1, l2)
        dist1, dist2 = raw["dist1"], raw["dist2"]
        found = (raw["idx1"], raw["idx2"])
    elif with_normals:
        dist1, dist2, *found = _plain_search(pred, gt, l1, l2)[:4]
    else:
        dist1, dist2 = chamfer_ragged(pred, gt, l1, l2)
    th2 = float(th) * float(th)
    m1, m2 = valid_mask(l1, pred.size(1), pred.device), valid_mask(l2, gt.size(1), gt.device)
    precision = ((dist1 < th2) & m1).sum(dim=1).double() / l1.clamp(1, pred.size(1))
    recall = ((dist2 < th2) & m2).sum(dim=1).double() / l2.clamp(1, gt.size(1))
    denom = precision + recall
    out = {"F-Score": torch.where(denom > 0, 2 * precision * recall / denom.clamp_min(1e-300), torch.zeros_like(denom)),
           "ChamferDistance": (masked_mean(dist1, l1) + masked_mean(dist2, l2)) * 1000}
    if with_emd:
        dist, _ = emd_ragged(pred, gt, l1, l2, emd_eps, emd_iters)
        out["EMD"] = masked_mean(torch.sqrt(dist), l1) * 100
    if with_dcd:
        out["DCD"] = value
    if with_normals:
        out["NormalConsistency"] = _consistency_from_search(pred, gt, found, normals_k, l1, l2)
    return out


def swd(pred, gt, n_slices=128, p=2, directions=None, generator=None, pred_lengths=None, gt_lengths=None):
    """Sliced Wasserstein distance of pred [B,N,3] and gt [B,M,3] per sample [B] (sparenet_amd.cuda.swd): for p = 2 the
    root of the mean squared 1-D transport cost over the slices -- a distance in the clouds' units -- for p = 1 the mean
    cost itself."""
    from sparenet_amd.cuda.swd import sliced_wasserstein

    value = sliced_wasserstein(pred, gt, n_slices, p, directions, generator, pred_lengths, gt_lengths)
    return torch.sqrt(value) if p == 2 else value


def dcd(pred, gt, alpha=1000.0, n_lambda=1.0, ratio="none", pred_lengths=None, gt_lengths=None):
    """Density-aware Chamfer distance of pred [B,N,3] and gt [B,M,3] per sample [B] (in [0, 1] with ratio="none")
    (sparenet_amd.cuda.dcd): the exponential Chamfer terms, each divided by the number of points that share its
    neighbour to the power n_lambda (0, 0.5 or 1)."""
    from sparenet_amd.cuda.dcd import density_aware_chamfer

    return density_aware_chamfer(pred, gt, alpha, n_lambda, ratio, pred_lengths, gt_lengths)


def normal_consistency(pred, gt, k=16, pred_lengths=None, gt_lengths=None, pred_normals=None, gt_normals=None):
    """Normal consistency of pred [B,N,3] and gt [B,M,3] per sample [B], in [0, 1] (sparenet_amd.cuda.normals): the mean
    |cosine| between each point's normal and the normal of its nearest neighbour in the other cloud, both ways.  Normals
    that are not given are estimated from k neighbours."""
    from sparenet_amd.cuda.normals import normal_consistency as consistency

    return consistency(pred, gt, pred_normals, gt_normals, k, pred_lengths, gt_lengths)


def aligned_chamfer(pred, gt, **icp_options):
    """Chamfer distance of pred [B,N,3] and gt [B,M,3] per sample [B] after pred has been registered onto gt by ICP
    (sparenet_amd.cuda.registration.aligned_chamfer, whose options these are: iters, mode, max_dist, init, ...): the
    pose-free distance for scans that do not share the prediction's frame.  mean dist1 + mean dist2, not scaled."""
    from sparenet_amd.cuda.registration import aligned_chamfer as aligned

    return aligned(pred, gt, **icp_options)[0]


def jsd(pred, gt, resolution=28, in_sphere=True, pred_lengths=None, gt_lengths=None, gt_counts=None):
    """Jensen-Shannon divergence (bits, float64 scalar in [0, 1]) between the occupancy distributions of the SETS pred
    [N,n,3] and gt [M,m,3] on the resolution^3 grid clipped to the unit sphere
    (sparenet_amd.utils.set_metrics.jsd_between_sets); `gt_counts` takes gt's grid where it has been computed before."""
    from sparenet_amd.utils.set_metrics import jsd_between_sets

    return jsd_between_sets(pred, gt, resolution, in_sphere, pred_lengths, gt_lengths, gt_counts)


def fpd(pred, gt, model, batch_size=100):
    """Frechet Point-cloud Distance of the SETS pred [N,n,3] and gt [M,m,3] (one scalar, float64) with `model`, a loaded
    sparenet_amd.Frechet.pointnet.PointNetCls(k=16): calculate_fpd on the clouds' own device (the fused PointNet
    kernel for CUDA tensors).  As in the reference the clouds after the last full batch of `batch_size` are dropped."""
    from sparenet_amd.Frechet.FPD import calculate_fpd

    device = pred.device if pred.is_cuda else None
    return calculate_fpd(pred, gt, batch_size=batch_size, device=device, model=model)
