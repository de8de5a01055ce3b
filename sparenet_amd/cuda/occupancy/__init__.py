"""The occupancy grid of a set of clouds (include/ops/occupancy.h states the rule; sparenet_amd/csrc/occupancy.hip):

    occupancy_grid(clouds [S,n,3], resolution=28, in_sphere=True, lengths=None, return_cells=False)
        -> (counts [res,res,res] int64, occupied [res,res,res] int32[, cells [S,n] int32])

Every point goes to the nearest centre of the resolution^3 lattice over [-0.5, 0.5]^3 -- with `in_sphere` to the nearest
centre inside the unit sphere, the grid of the Jensen-Shannon divergence between point-cloud sets
(sparenet_amd.utils.set_metrics.jsd_between_sets).  counts[i,j,k] is the number of the set's points in cell (i, j, k),
occupied[i,j,k] the number of clouds with a point there, cells the linear index (i * res + j) * res + k of each point:
-1 at padding rows and at points with a NaN or infinite coordinate, which are counted nowhere.  A point exactly half-way
between two centres goes to the lower index, points outside the cube to its rim.  All three are integers and exact:
two calls, a permutation of the clouds, and the CPU path (CPU tensors run the library's host entry point) give the
same bits.  `lengths` makes the batch ragged (padding rows are never read; a length of 0 is allowed).  Nothing here is
differentiable; inputs are detached.
"""
import torch

from sparenet_amd import _lib
from sparenet_amd.cuda import _args

MIN_RESOLUTION, MAX_RESOLUTION = 2, 32


def occupancy_grid(clouds, resolution=28, in_sphere=True, lengths=None, return_cells=False):
    """(counts [res,res,res] int64, occupied [res,res,res] int32[, cells [S,n] int32]) of the set clouds [S,n,3] (see
    the module's text).  Device tensors go through the kernel, CPU tensors through the host entry point."""
    what = "occupancy_grid"
    _args.check_cloud(what, "clouds", clouds, "[S, n, 3]")
    res = int(resolution)
    if res != resolution or not MIN_RESOLUTION <= res <= MAX_RESOLUTION:
        raise ValueError(f"{what}: resolution must be an integer in {MIN_RESOLUTION}..{MAX_RESOLUTION}, got {resolution!r}")
    xyz, dev = _args.fp32(clouds), clouds.device
    s, n = xyz.size(0), xyz.size(1)
    sphere = 1 if in_sphere else 0
    lens = _args.optional_lengths(lengths, s, n, dev, "lengths")
    counts = torch.empty(res, res, res, dtype=torch.int64, device=dev)
    occupied = torch.empty(res, res, res, dtype=torch.int32, device=dev)
    cells = torch.empty(s, n, dtype=torch.int32, device=dev) if return_cells else None
    args = (xyz, lens, s, n, res, sphere, counts, occupied, cells)
    if xyz.is_cuda:
        ws = _lib.op_workspace("occupancy", "sn_occupancy_grid_workspace_bytes", xyz, s, n, res, sphere)
        _lib.op_call("occupancy", "sn_occupancy_grid", *args, ws)
    else:
        _lib.op_call("occupancy", "sn_occupancy_grid_host", *args, 0, host=True)
    return (counts, occupied, cells) if return_cells else (counts, occupied)
