"""Frechet Point-cloud Distance (FPD): the reference's `Frechet` package under the same module and public names
(`Frechet.pointnet.PointNetCls`, `Frechet.FPD.calculate_fpd`, ...).  On the GPU the per-point MLPs and their max over
the points run as one fused HIP kernel (sn_pointnet_pool_forward, csrc/pointnet_pool.hip); the Frechet term needs no
scipy.  `sparenet_amd.alias_frechet_modules()` makes `from Frechet.FPD import calculate_fpd` resolve here."""
from . import FPD, pointnet  # noqa: F401
from .FPD import calculate_fpd  # noqa: F401
from .pointnet import PointNetCls  # noqa: F401
