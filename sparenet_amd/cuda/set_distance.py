"""Chamfer distance between every cloud of one set and every cloud of another, from one kernel call per direction
(sn_set_chamfer_sums, include/sparenet_hip_ext.h; kernel: sparenet_amd/csrc/set_chamfer.hip).

    chamfer_direction_sums(x, y) -> float64 [Nx, Ny]    S[i, j] = sum over the points of x_i of their squared distance
                                                        to the nearest point of y_j
    chamfer_matrix(x, y)         -> float64 [Nx, Ny]    CD[i, j] = S_xy[i, j] / n + S_yx[j, i] / m

x [Nx, n, 3] and y [Ny, m, 3] are contiguous fp32 CUDA tensors on one device.  Every nearest-neighbour distance is bit
for bit the one ChamferDistanceFunction returns for that pair of clouds; the sums are float64, added in an order that
depends on n alone, so a matrix entry equals the 1 x 1 call on its pair and two calls agree bit for bit.  Not
differentiable: these are evaluation metrics (sparenet_amd/utils/set_metrics.py builds MMD-CD, COV-CD and 1-NNA-CD on
them).
"""
import torch

from sparenet_amd import _lib


def _check_set(t, name):
    _lib.require_device(t, name)      # a CPU tensor is refused with the message of a device entry point
    if t.dim() != 3 or t.size(2) != 3 or t.size(0) == 0 or t.size(1) == 0:
        raise ValueError(f"{name}: expected a non-empty set of clouds [N, n, 3], got {tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected dtype torch.float32, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: tensor must be contiguous")


def chamfer_direction_sums(x, y):
    """S [Nx, Ny] float64: S[i, j] = sum_q min_t d(x_i[q], y_j[t]), d the squared distance as the Chamfer kernels
    evaluate it.  One direction; the other is chamfer_direction_sums(y, x)."""
    _check_set(x, "x")
    _check_set(y, "y")
    if x.device != y.device:
        raise ValueError(f"y is on {y.device}, x on {x.device}")
    nx, n, _ = x.shape
    ny, m, _ = y.shape
    with torch.no_grad():
        sums = torch.empty(nx, ny, dtype=torch.float64, device=x.device)
        ws = _lib.ext_workspace("sn_set_chamfer_workspace_bytes", x, nx, ny, n)
        _lib.ext_call("sn_set_chamfer_sums", x, y, nx, n, ny, m, sums, ws)
    return sums


def chamfer_matrix(x, y):
    """CD [Nx, Ny] float64: the Chamfer distance (mean of the squared nearest-neighbour distances, both ways) between
    x_i and y_j.  For a set against itself (`y is x`, or the same storage and shape) one kernel call serves both
    directions: the result is then exactly symmetric with an exactly zero diagonal."""
    n, m = x.size(1), y.size(1)
    s_xy = chamfer_direction_sums(x, y)
    same = y is x or (x.data_ptr() == y.data_ptr() and x.shape == y.shape)
    s_yx = s_xy if same else chamfer_direction_sums(y, x)
    # divisors as device tensors: a host number would be applied as a multiplication by its rounded reciprocal
    per_n, per_m = (torch.full((), float(k), dtype=torch.float64, device=x.device) for k in (n, m))
    return s_xy / per_n + s_yx.t() / per_m
