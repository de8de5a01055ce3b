"""Chamfer distance and auction EMD between every cloud of one set and every cloud of another.

Chamfer: one kernel call per direction (sn_set_chamfer_sums, include/sparenet_hip_ext.h; kernel:
sparenet_amd/csrc/set_chamfer.hip).

    chamfer_direction_sums(x, y) -> float64 [Nx, Ny]    S[i, j] = sum over the points of x_i of their squared distance
                                                        to the nearest point of y_j
    chamfer_matrix(x, y)         -> float64 [Nx, Ny]    CD[i, j] = S_xy[i, j] / n + S_yx[j, i] / m

x [Nx, n, 3] and y [Ny, m, 3] are contiguous fp32 CUDA tensors on one device.  Every nearest-neighbour distance is bit
for bit the one ChamferDistanceFunction returns for that pair of clouds; the sums are float64, added in an order that
depends on n alone, so a matrix entry equals the 1 x 1 call on its pair and two calls agree bit for bit.  Not
differentiable: these are evaluation metrics (sparenet_amd/utils/set_metrics.py builds MMD-CD, COV-CD and 1-NNA-CD on
them).

EMD: one kernel call for the whole matrix (sn_set_emd_sums, include/sparenet_hip_ext_set_emd.h; kernel:
sparenet_amd/csrc/set_emd.hip), one workgroup per pair of clouds with the auction state in LDS.

    emd_direction_sums(x, y, eps, iters) -> float64 [Nx, Ny]    S[i, j] = sum over the bidders of x_i of sqrt(dist) after
                                                                the auction of x_i for y_j, n <= m
    emd_matrix(x, y, eps, iters)         -> float64 [Nx, Ny]    EMD[i, j] = S[i, j] / n, the smaller clouds bidding

dist and the assignment of a pair are bit for bit those of emd_general on it; the sums are float64, added in an order
that depends on n alone.  Clouds of more than 2048 points do not fit the kernel's LDS and take a loop of emd_general
calls (`_emd_sums_loop`): the same per-bidder distances, another summation order.  Not differentiable either
(MMD-EMD, COV-EMD and 1-NNA-EMD are built on emd_matrix).
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


EMD_KERNEL_MAX_POINTS = 2048        # what sn_set_emd_lds_bytes takes: the auction state of a pair in one CU's LDS
# the loop's bound on expanded memory: a chunk of pairs holds copies of its clouds (12 (n + m) bytes per pair) and
# emd_general's outputs and workspace (about 40 (n + m) bytes per pair); the copies are kept below this many bytes and
# a chunk below 256 pairs
_EMD_LOOP_EXPANDED_BYTES = 64 << 20


def _uses_emd_kernel(n, m):
    """Which route a size takes: the kernel wherever the auction fits its LDS.  Measured ("Set-level EMD
    matrix"): the kernel is 2 x faster than the emd_general loop at 1024 and 2047 points; at 2048 x 2048, where the loop
    is the persistent auction, neither wins on both measured geometries, and the kernel needs no co-resident
    workgroups and no workspace."""
    return m <= EMD_KERNEL_MAX_POINTS


def _emd_sums_loop(x, y, eps, iters, return_assignment):
    """The route without the kernel: emd_general on chunks of pairs (x_i, y_j), the clouds of a chunk gathered into a
    batch.  At most _EMD_LOOP_EXPANDED_BYTES of gathered clouds and 256 pairs per call."""
    from sparenet_amd.cuda.emd.emd_general import emd_general_forward_raw

    nx, n, _ = x.shape
    ny, m, _ = y.shape
    pairs = nx * ny
    chunk = max(1, min(256, _EMD_LOOP_EXPANDED_BYTES // (12 * (n + m))))
    sums = torch.empty(pairs, dtype=torch.float64, device=x.device)
    assignment = torch.empty(pairs, n, dtype=torch.int32, device=x.device) if return_assignment else None
    for p0 in range(0, pairs, chunk):
        idx = torch.arange(p0, min(p0 + chunk, pairs), device=x.device)
        dist, assign = emd_general_forward_raw(x[idx // ny], y[idx % ny], eps, iters)
        sums[p0:p0 + chunk] = dist.sqrt().double().sum(dim=1)
        if return_assignment:
            assignment[p0:p0 + chunk] = assign
    return sums.view(nx, ny), (assignment.view(nx, ny, n) if return_assignment else None)


def emd_direction_sums(x, y, eps=0.005, iters=50, return_assignment=False):
    """S [Nx, Ny] float64: S[i, j] = sum over the points q of x_i of sqrt(dist[q]), dist the squared distance of q to
    the target the auction of x_i (bidders) for y_j (targets) assigned it -- emd_general(x_i, y_j, eps, iters), 0 for
    a bidder left unassigned (iters == 0).  n <= m is required: pass the smaller clouds first.
    return_assignment: also the int32 [Nx, Ny, n] assignments."""
    _check_set(x, "x")
    _check_set(y, "y")
    if x.device != y.device:
        raise ValueError(f"y is on {y.device}, x on {x.device}")
    nx, n, _ = x.shape
    ny, m, _ = y.shape
    if n > m:
        raise ValueError(f"x: n={n} > m={m}: pass the smaller clouds first (x bids for y)")
    if int(iters) != iters or iters < 0:
        raise ValueError(f"iters must be a non-negative integer, got {iters!r}")
    with torch.no_grad():
        if not _uses_emd_kernel(n, m):
            sums, assignment = _emd_sums_loop(x, y, float(eps), int(iters), return_assignment)
        else:
            sums = torch.empty(nx, ny, dtype=torch.float64, device=x.device)
            assignment = torch.empty(nx, ny, n, dtype=torch.int32, device=x.device) if return_assignment else None
            _lib.topic_call("set_emd", "sn_set_emd_sums", x, y, nx, n, ny, m, eps, iters, sums, assignment)
    return (sums, assignment) if return_assignment else sums


def emd_matrix(x, y, eps=0.005, iters=50):
    """EMD [Nx, Ny] float64: the mean over the bidders of sqrt(dist) after the auction between x_i and y_j, the
    SMALLER clouds bidding (for n > m: the call with the sets swapped, transposed).
    An auction is directed -- x_i bids for x_j is another auction than x_j bids for x_i -- so a set against itself
    is NOT symmetric: [i, j] and [j, i] are two results, both valid.  Its diagonal is exactly 0 for finite clouds
    without duplicate points (every bidder takes its own point at distance 0)."""
    _check_set(x, "x")      # here, under the caller's names: the swapped call would report them crosswise
    _check_set(y, "y")
    if x.device != y.device:
        raise ValueError(f"y is on {y.device}, x on {x.device}")
    n, m = x.size(1), y.size(1)
    sums = emd_direction_sums(y, x, eps, iters).t() if n > m else emd_direction_sums(x, y, eps, iters)
    # the divisor as a device tensor: a host number would be applied as a multiplication by its rounded reciprocal
    return sums / torch.full((), float(min(n, m)), dtype=torch.float64, device=sums.device)
