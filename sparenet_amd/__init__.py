"""sparenet_amd -- MI355X (gfx950) native SpareNet loss/render hot path.

Host-side mirror of the reference's operator API lives in sparenet_amd.cuda.*
and sparenet_amd.utils.p2i_utils (same module names, class names and argument
meaning as /root/reference/cuda/* and utils/p2i_utils.py); every op calls the
hand-written HIP kernels in libsparenet_hip.so through the C ABI declared in
include/sparenet_hip.h.  There is no CPU or eager-PyTorch fallback.
"""
from ._lib import LIB_PATH, SparenetHipError, call, device_check, lib  # noqa: F401

__version__ = "0.1.0"

_REFERENCE_OP_PACKAGES = ("chamfer_distance", "chamfer_dist", "emd", "expansion_penalty", "MDS", "p2i_op",
                          "gridding", "gridding_loss", "cubic_feature_sampling")


_SINKHORN_NAMES = ("sinkhorn_potentials", "sinkhorn_ot", "sinkhorn_divergence", "SinkhornDistance")
_SWD_NAMES = ("sliced_wasserstein", "sorted_projections", "random_directions", "SlicedWassersteinDistance")
_DCD_NAMES = ("density_aware_chamfer", "dcd_from_search", "DensityAwareChamferDistance")
_NORMALS_NAMES = ("local_pca", "surface_variation", "estimate_normals", "normal_consistency", "point_to_plane_chamfer")
_OCCUPANCY_NAMES = ("occupancy_grid",)
_VOXEL_GRID_NAMES = ("voxel_grid", "grid_subsample", "voxel_pool", "GridPool", "VoxelGrid")
_REGISTRATION_NAMES = ("transform_points", "rigid_fit", "icp", "aligned_chamfer", "RigidFit", "IcpResult")


def __getattr__(name):
    """`sparenet_amd.sinkhorn_divergence` ...: the Sinkhorn transport loss (sparenet_amd.cuda.sinkhorn), imported at
    its first use."""
    if name in _SINKHORN_NAMES:
        import importlib

        return getattr(importlib.import_module("sparenet_amd.cuda.sinkhorn"), name)
    if name in _SWD_NAMES:      # the sliced Wasserstein distance (sparenet_amd.cuda.swd), the same way
        import importlib

        return getattr(importlib.import_module("sparenet_amd.cuda.swd"), name)
    if name in _DCD_NAMES:      # the density-aware Chamfer distance (sparenet_amd.cuda.dcd)
        import importlib

        return getattr(importlib.import_module("sparenet_amd.cuda.dcd"), name)
    if name in _NORMALS_NAMES:      # normals, local frames and the metrics on them (sparenet_amd.cuda.normals)
        import importlib

        return getattr(importlib.import_module("sparenet_amd.cuda.normals"), name)
    if name in _OCCUPANCY_NAMES:      # the occupancy grid of a set of clouds (sparenet_amd.cuda.occupancy)
        import importlib

        return getattr(importlib.import_module("sparenet_amd.cuda.occupancy"), name)
    if name in _VOXEL_GRID_NAMES:      # voxel-grid subsampling and pooling (sparenet_amd.cuda.voxel_grid)
        import importlib

        return getattr(importlib.import_module("sparenet_amd.cuda.voxel_grid"), name)
    if name in _REGISTRATION_NAMES:      # rigid registration: Kabsch fit and ICP (sparenet_amd.cuda.registration)
        import importlib

        return getattr(importlib.import_module("sparenet_amd.cuda.registration"), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


WAIT_POLICIES = ("fail", "recover", "nowait")   # SN_WAIT_FAIL / SN_WAIT_RECOVER / SN_WAIT_NOWAIT (sparenet_hip.h)


def set_wait_policy(name):
    """What the ops whose workgroups wait for each other (the EMD auction's teams, the density sampler's teams) do on a
    GPU shared with another process: "fail" (default: a team that gives up leaves NaN / -1 rows and the next op, or
    `loss_item`, raises), "recover" (the same call recomputes those clouds with kernels that wait for nobody -- exact
    -- and later calls on that device skip the teams) or "nowait" (never launch a team).  Process-wide; the
    environment variable SN_WAIT_POLICY gives the initial value.  Setting a policy clears the per-device latch of
    "recover"."""
    if name not in WAIT_POLICIES:
        raise ValueError(f"unknown wait policy {name!r}: expected one of {', '.join(WAIT_POLICIES)}")
    call("sn_set_wait_policy", WAIT_POLICIES.index(name))


def wait_policy():
    """The current wait policy's name (see set_wait_policy)."""
    return WAIT_POLICIES[call("sn_wait_policy")]


def wait_report():
    """Recoveries on the CURRENT device since the process started: {"emd_recovered": clouds, "mds_recovered": clouds,
    "latched": whether later calls there skip the teams}.  Reads pinned host words without a synchronisation: it
    covers work that has finished (call it after a `.item()` / synchronize)."""
    import ctypes

    out = (ctypes.c_longlong * 3)()
    call("sn_wait_report", out, 3)
    return {"emd_recovered": int(out[0]), "mds_recovered": int(out[1]), "latched": bool(out[2])}


def loss_item(loss):
    """`loss.item()` that cannot hand back the number of a failed step: the host waits for the GPU (as `.item()` always
    does), then the device's sticky error word is read (sn_device_status) -- if a team barrier of the persistent EMD
    auction or of the density sampler timed out in any launch up to here (a shared device, a debugger holding a compute
    unit), its outputs were NaN / -1 and this raises SparenetHipError instead of returning NaN to the training loop.
    That is the default wait policy ("fail"); under `set_wait_policy("recover")` the call that met the time-out has
    already recomputed those clouds exactly, nothing is raised and the loss is the one an undisturbed step computes
    (`wait_report()` counts the recoveries); under "nowait" no op waits for another workgroup in the first place.
    Where the reference's runners log `_loss.item()` every step (runners/sparenet_runner.py:113-116), log
    `sparenet_amd.loss_item(_loss)` -- before `optimizer.step()` if a failed step must not touch the weights."""
    value = loss.item()
    device_check("loss_item")
    return value


def alias_reference_modules():
    """Make the reference's import lines resolve to this package without touching its checkout:
    `from cuda.emd.emd_module import emdModule` (runners/sparenet_runner.py:9), `import cuda.MDS.MDS_module`
    (models/sparenet_generator.py:8), `from cuda.p2i_op import p2i`, `from utils.p2i_utils import
    ComputeDepthMaps` (utils/model_init.py:9) ... -- INTEGRATION.md section 2.  Call it once at start-up,
    before the runners are imported."""
    import importlib
    import sys

    amd_cuda = importlib.import_module("sparenet_amd.cuda")
    sys.modules["cuda"] = amd_cuda
    for name in _REFERENCE_OP_PACKAGES:
        mod = importlib.import_module(f"sparenet_amd.cuda.{name}")
        sys.modules[f"cuda.{name}"] = mod
        for sub in ("emd_module", "expansion_penalty_module", "MDS_module", "chamfer_distance"):
            try:
                sys.modules[f"cuda.{name}.{sub}"] = importlib.import_module(f"sparenet_amd.cuda.{name}.{sub}")
            except ModuleNotFoundError:
                pass
    amd_p2i = importlib.import_module("sparenet_amd.utils.p2i_utils")
    sys.modules["utils.p2i_utils"] = amd_p2i
    utils_pkg = sys.modules.get("utils")
    if utils_pkg is not None:                 # the reference's own `utils` package, already imported
        setattr(utils_pkg, "p2i_utils", amd_p2i)
    return amd_cuda


def alias_frechet_modules():
    """Make the reference's `from Frechet.FPD import calculate_fpd` / `from Frechet.pointnet import PointNetCls`
    resolve to sparenet_amd.Frechet.  A separate opt-in from alias_reference_modules(): an evaluation script may
    want one without the other.  Returns the package."""
    import importlib
    import sys

    pkg = importlib.import_module("sparenet_amd.Frechet")
    sys.modules["Frechet"] = pkg
    for sub in ("FPD", "pointnet"):
        sys.modules[f"Frechet.{sub}"] = importlib.import_module(f"sparenet_amd.Frechet.{sub}")
    return pkg
