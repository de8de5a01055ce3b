"""GRNet-style Chamfer loss -- host-side mirror of cuda/chamfer_dist/__init__.py
(ChamferFunction :6-18, ChamferDistance :21-35, ChamferDistanceSeperate :38-52).

The reference builds a second copy of the Chamfer kernels for this module (`chamfer`
extension, cuda/chamfer_dist/chamfer.cu); here it is the same HIP path as
sparenet_amd.cuda.chamfer_distance (sn_chamfer_forward[_sorted] / sn_chamfer_backward).

ChamferDistance(ignore_zeros=True) honours the zero-row padding rule at batch size 1 only, as the reference does.
ChamferDistancePadded / ChamferDistanceSeperatePadded apply it at any batch size (sparenet_amd.cuda.ragged).
"""
import torch

from sparenet_amd.cuda.chamfer_distance.chamfer_distance import ChamferDistanceFunction

ChamferFunction = ChamferDistanceFunction


def _drop_padding(xyz1, xyz2, ignore_zeros):
    """With batch size 1, rows whose coordinates sum to zero are padding (reference :27-31)."""
    if xyz1.size(0) == 1 and ignore_zeros:
        xyz1 = xyz1[torch.sum(xyz1, dim=2).ne(0)].unsqueeze(dim=0)
        xyz2 = xyz2[torch.sum(xyz2, dim=2).ne(0)].unsqueeze(dim=0)
    return xyz1, xyz2


class ChamferDistance(torch.nn.Module):
    """mean_j dist1 + mean_k dist2 (squared distances, both directions)."""

    def __init__(self, ignore_zeros=False):
        super().__init__()
        self.ignore_zeros = ignore_zeros

    def forward(self, xyz1, xyz2):
        dist1, dist2 = ChamferFunction.apply(*_drop_padding(xyz1, xyz2, self.ignore_zeros))
        return torch.mean(dist1) + torch.mean(dist2)


class ChamferDistanceSeperate(torch.nn.Module):
    """The two directed terms separately (the reference's spelling is kept)."""

    def __init__(self, ignore_zeros=False):
        super().__init__()
        self.ignore_zeros = ignore_zeros

    def forward(self, xyz1, xyz2):
        dist1, dist2 = ChamferFunction.apply(*_drop_padding(xyz1, xyz2, self.ignore_zeros))
        return torch.mean(dist1), torch.mean(dist2)


def _padded_means(xyz1, xyz2):
    """Per-cloud means over the rows that are not padding, [B] each way."""
    from sparenet_amd.cuda.ragged import chamfer_ragged, masked_mean, pad_compact

    p1, l1, _ = pad_compact(xyz1)
    p2, l2, _ = pad_compact(xyz2)
    dist1, dist2 = chamfer_ragged(p1, p2, l1, l2)
    return masked_mean(dist1, l1), masked_mean(dist2, l2)


def _cloud_mean(per_cloud):
    """Mean over the clouds in float64, rounded once (for one cloud: that cloud's value itself)."""
    return per_cloud.double().mean().to(per_cloud.dtype)


class ChamferDistancePadded(torch.nn.Module):
    """ChamferDistance(ignore_zeros=True) for any batch size: in every cloud the rows whose coordinates sum to zero
    are padding.  Returns the mean over the clouds of (mean_j dist1 + mean_k dist2), each mean over the cloud's own
    points.  For one cloud that is what ChamferDistance(ignore_zeros=True) computes, from bit-equal distances; the
    values agree to fp32 rounding and are not identical: every mean here is a float64 sum rounded once to fp32 (so
    neither the padded width nor the batch enters it), ChamferDistance's is torch's fp32 mean."""

    def forward(self, xyz1, xyz2):
        m1, m2 = _padded_means(xyz1, xyz2)
        return _cloud_mean(m1) + _cloud_mean(m2)


class ChamferDistanceSeperatePadded(torch.nn.Module):
    """The two directed terms of ChamferDistancePadded separately."""

    def forward(self, xyz1, xyz2):
        m1, m2 = _padded_means(xyz1, xyz2)
        return _cloud_mean(m1), _cloud_mean(m2)
