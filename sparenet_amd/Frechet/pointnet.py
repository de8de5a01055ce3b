"""PointNet classifier used as the feature extractor of the Frechet Point-cloud Distance.

Same public names, state-dict keys and shapes as the reference's Frechet/pointnet.py (`PointNetCls(k=16)` loads
`cls_model_39.pth` unchanged) and the same outputs in eval mode.  What differs is how the two per-point MLPs
(conv 3 -> 64 -> 128 -> 1024 with batch norm, then a max over the points) are evaluated:

  * eval-mode batch norm is folded into the convolution's weight and bias (in float64, rounded once to the
    module's dtype; a negative batch-norm scale simply ends up in the weight);
  * CUDA tensors ALWAYS go through the fused HIP kernel `sn_pointnet_pool_forward` (fp32 matrix cores; the
    [B, 1024, N] activation never exists) -- there is no torch path for them, a missing library is an error;
  * CPU tensors run the folded layers with stock torch ops, as the reference does with `device=None`.

FPD is an evaluation metric: there is NO autograd through the fused op, `forward` runs under `torch.no_grad()`,
and training mode raises (batch statistics would need the per-point activations).  PointNetDenseCls is not provided.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib


def fold_batch_norm(layer, bn, dtype):
    """(W [out, in], b [out]) of `bn(layer(x))` in eval mode; layer = Conv1d(kernel 1) or Linear."""
    w = layer.weight.detach().double().reshape(layer.weight.shape[0], -1)
    b = layer.bias.detach().double()
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    return ((w * scale[:, None]).to(dtype).contiguous(),
            ((b - bn.running_mean.detach().double()) * scale + bn.bias.detach().double()).to(dtype).contiguous())


def pool_mlp_torch(x, trans, folded, relu_last):
    """The fused op in stock torch ops (the CPU path; tools/fpd_bench.py times it on the GPU): x [B, 3, N],
    trans [B, 3, 3] or None, folded = ((W1, b1), (W2, b2), (W3, b3)) -> [B, 1024].  Writes [B, 1024, N]."""
    (w1, b1), (w2, b2), (w3, b3) = folded
    if trans is not None:
        x = torch.bmm(x.transpose(2, 1), trans).transpose(2, 1)
    h = F.relu(torch.matmul(w1, x) + b1[:, None])
    h = F.relu(torch.matmul(w2, h) + b2[:, None])
    h = torch.matmul(w3, h) + b3[:, None]
    if relu_last:
        h = F.relu(h)
    return torch.max(h, 2)[0]


def pool_mlp_fused(x, trans, folded, relu_last):
    """x [B, 3, N] fp32 CUDA -> [B, 1024] through sn_pointnet_pool_forward on the current stream."""
    if x.dtype != torch.float32:
        raise TypeError(f"the fused PointNet kernel is fp32 only, got {x.dtype}")
    (w1, b1), (w2, b2), (w3, b3) = folded
    xyz = x.transpose(2, 1).contiguous()
    _lib.require_device(xyz, "x")   # raises for a CPU tensor: this op has no other path
    b, n = xyz.shape[0], xyz.shape[1]
    out = torch.empty(b, 1024, dtype=torch.float32, device=x.device)
    ws = _lib.workspace("sn_pointnet_pool_workspace_bytes", xyz, b, n)
    trans = None if trans is None else trans.contiguous()   # None: a null pointer, the identity
    _lib.call("sn_pointnet_pool_forward", xyz, trans, w1, b1, w2, b2, w3, b3, bool(relu_last), b, n, out, ws)
    return out


class _PoolMLP(nn.Module):
    """conv1/bn1, conv2/bn2, conv3/bn3 and the max over the points."""

    force_torch = False   # tools/fpd_bench.py only: time the stock layers on the GPU

    def _make_convs(self):
        self.conv1 = nn.Conv1d(3, 64, 1)
        self.conv2 = nn.Conv1d(64, 128, 1)
        self.conv3 = nn.Conv1d(128, 1024, 1)

    def _pool(self, x, trans, relu_last):
        if self.training:
            raise RuntimeError("sparenet_amd.Frechet.pointnet supports eval mode only: call model.eval() "
                               "(training-mode batch norm needs the per-point activations the fused kernel never writes)")
        dtype = self.conv1.weight.dtype
        folded = tuple(fold_batch_norm(c, n, dtype) for c, n in
                       ((self.conv1, self.bn1), (self.conv2, self.bn2), (self.conv3, self.bn3)))
        if x.is_cuda and not self.force_torch:
            return pool_mlp_fused(x, trans, folded, relu_last)
        return pool_mlp_torch(x, trans, folded, relu_last)


class STN3d(_PoolMLP):
    """Input transform: [B, 3, N] -> [B, 3, 3] (identity added)."""

    def __init__(self):
        super().__init__()
        self._make_convs()
        self.fc1 = nn.Linear(1024, 512)
        self.fc2 = nn.Linear(512, 256)
        self.fc3 = nn.Linear(256, 9)
        self.relu = nn.ReLU()
        self.bn1 = nn.BatchNorm1d(64)
        self.bn2 = nn.BatchNorm1d(128)
        self.bn3 = nn.BatchNorm1d(1024)
        self.bn4 = nn.BatchNorm1d(512)
        self.bn5 = nn.BatchNorm1d(256)

    def forward(self, x):
        g = self._pool(x, None, True)
        g = F.relu(self.bn4(self.fc1(g)))
        g = F.relu(self.bn5(self.fc2(g)))
        g = self.fc3(g) + torch.eye(3, dtype=g.dtype, device=g.device).reshape(1, 9)
        return g.view(-1, 3, 3)


class PointNetfeat(_PoolMLP):
    """Global feature: [B, 3, N] -> ([B, 1024], trans [B, 3, 3]).  Only global_feat=True (what FPD uses)."""

    def __init__(self, global_feat=True):
        super().__init__()
        if not global_feat:
            raise NotImplementedError("per-point features (PointNetDenseCls) are not part of the FPD path")
        self.stn = STN3d()
        self._make_convs()
        self.bn1 = nn.BatchNorm1d(64)
        self.bn2 = nn.BatchNorm1d(128)
        self.bn3 = nn.BatchNorm1d(1024)
        self.global_feat = global_feat

    def forward(self, x):
        trans = self.stn(x)
        return self._pool(x, trans, False), trans


class PointNetCls(nn.Module):
    """forward(x [B, 3, N]) -> (log_softmax(x4, dim=0), trans [B, 3, 3], actv [B, 1024 + 512 + 256 + k]), as the
    reference returns them.  Eval mode only, no gradients (see the module docstring)."""

    def __init__(self, k=2):
        super().__init__()
        self.feat = PointNetfeat(global_feat=True)
        self.fc1 = nn.Linear(1024, 512)
        self.fc2 = nn.Linear(512, 256)
        self.fc3 = nn.Linear(256, k)
        self.bn1 = nn.BatchNorm1d(512)
        self.bn2 = nn.BatchNorm1d(256)
        self.relu = nn.ReLU()

    @torch.no_grad()
    def forward(self, x):
        if x.dim() != 3 or x.size(1) != 3:
            raise ValueError(f"expected points as [B, 3, N], got {tuple(x.shape)}")
        x1, trans = self.feat(x)
        x2 = F.relu(self.bn1(self.fc1(x1)))
        x3 = F.relu(self.bn2(self.fc2(x2)))
        x4 = self.fc3(x3)
        return F.log_softmax(x4, dim=0), trans, torch.cat((x1, x2, x3, x4), dim=1)
