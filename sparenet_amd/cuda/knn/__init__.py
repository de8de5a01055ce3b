"""EdgeConv's k-NN graph in feature space -- host-side mirror of knn() and get_graph_feature()
(models/sparenet_generator.py:852-877, :880-906), backed by sn_knn_topk and
sn_graph_feature_forward / backward (include/sparenet_hip.h).

The reference's GPU branch calls the un-vendored KNN_CUDA wheel; its CPU branch ranks
-|x_i|^2 + 2 x_i.x_j - |x_j|^2 with topk.  For k <= 8 and up to 128 channels the whole search is ONE kernel on the fp32 matrix
cores (sn_knn, knn_mfma.hip: score tiles in the MFMA accumulators, the k best of every query in registers,
no [B,N,N] matrix in HBM); wider features or larger k take the inner products from one batched GEMM (torch.bmm = rocBLAS)
and ranks them with sn_knn_topk.  Neighbours come out ascending by distance, the point itself first,
equal scores by lower index.
"""
import torch

from sparenet_amd import _lib

FUSED_MAX_K = 8    # sn_knn accepts k <= 20; above 8 the GEMM + ranking pair is faster (measured)
FUSED_MAX_C = 128  # measured at B=32, N=3000: C=3 0.30 vs 0.86 ms, C=256 1.75-2.2 vs 1.77-2.0 ms, C=512 3.1 vs 2.8 ms


def knn(x, k: int):
    """x [B, C, N] float32 on the GPU -> idx [B, N, k] int64 (indices of the k nearest points)."""
    if x.dim() != 3:
        raise ValueError("knn expects x [batch, feature_dim, num_points]")
    return knn_fused(x, k) if k <= FUSED_MAX_K and x.shape[1] <= FUSED_MAX_C else knn_unfused(x, k)


def knn_fused(x, k: int):
    """The one-kernel search on the fp32 matrix cores (sn_knn); k <= 20."""
    x = x.contiguous().float()
    b, c, n = x.shape
    idx = torch.empty(b, n, k, dtype=torch.int64, device=x.device)
    _lib.call("sn_knn", x, b, c, n, k, idx, _lib.workspace("sn_knn_workspace_bytes", x, b, n))
    return idx


def knn_unfused(x, k: int):
    """The two-step path (library GEMM + sn_knn_topk); any k <= 32."""
    x = x.contiguous().float()
    b, _, n = x.shape
    inner = torch.bmm(x.transpose(2, 1), x).contiguous()        # [B, N, N]
    xx = (x * x).sum(dim=1).contiguous()                        # [B, N]
    idx = torch.empty(b, n, k, dtype=torch.int64, device=x.device)
    _lib.call("sn_knn_topk", inner, xx, b, n, k, idx)
    return idx


class GraphFeatureFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, idx):
        x = x.contiguous().float()
        idx = idx.contiguous()
        b, c, n = x.shape
        k = idx.size(2)
        out = torch.empty(b, 2 * c, n, k, device=x.device)
        _lib.call("sn_graph_feature_forward", x, idx, b, c, n, k, out)
        ctx.save_for_backward(idx)
        ctx.shape = (b, c, n, k)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        b, c, n, k = ctx.shape
        grad_out = grad_out.contiguous().float()
        grad_x = torch.empty(b, c, n, device=grad_out.device)
        ws = _lib.workspace("sn_graph_feature_backward_workspace_bytes", grad_out, b, n, k)
        _lib.call("sn_graph_feature_backward", grad_out, idx, b, c, n, k, grad_x, ws)
        return grad_x, None


def get_graph_feature(x, k: int = 20, idx=None):
    """x [B, C, N] -> edge features [B, 2C, N, k]: (neighbour - point, point) per neighbour."""
    batch_size, num_points = x.size(0), x.size(2)
    x = x.view(batch_size, -1, num_points)
    if idx is None:
        idx = knn(x, k=k)
    if idx.dtype != torch.int64:
        idx = idx.long()
    return GraphFeatureFunction.apply(x, idx)
