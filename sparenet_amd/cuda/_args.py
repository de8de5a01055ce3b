"""The argument checks the operator wrappers share (sinkhorn, swd, dcd, neighbors, fps, normals, occupancy): a cloud, a
pair of clouds, optional lengths, a count, and the conversion to what the kernels read.  Plain functions; a wrapper
states only its operator's own parameter rules beside them.  `what` is the entry point's name, as its messages begin.
The older wrappers (Chamfer, EMD, set_distance, knn, gridding, p2i, MDS) refuse in other words and keep their own.
"""
import torch

from sparenet_amd import _lib
from sparenet_amd.cuda.ragged import device_lengths


def check_cloud(what, name, t, shape_text="[B, N, 3]", max_points=None):
    """`t` is a non-empty floating-point [B, N, 3] tensor (of at most `max_points` points per cloud)."""
    if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.size(2) != 3 or t.size(0) == 0 or t.size(1) == 0:
        raise ValueError(f"{what}: {name} must be a non-empty {shape_text} tensor")
    if not t.is_floating_point():
        raise TypeError(f"{what}: {name} must be a floating-point tensor, got {t.dtype}")
    if max_points is not None and t.size(1) > max_points:
        raise ValueError(f"{what}: {name} has {t.size(1)} points per cloud, at most {max_points} are supported")


def on_device(t, name):
    """A CPU tensor is refused, with the message of a device entry point, before anything is uploaded or allocated; a
    device tensor of any layout passes (`_lib.require_device` itself refuses one that is not contiguous)."""
    if not t.is_cuda:
        _lib.require_device(t, name)


def check_pair(what, name1, t1, name2, t2, device=None, same_device=False, max_points=None):
    """Each cloud's own checks, then the batch sizes, then the operator's device policy: `device` None (CPU tensors
    have a host path), "contiguous" (`_lib.require_device` on each) or "any" (`on_device` on each), and with
    `same_device` both on one device."""
    check_cloud(what, name1, t1, max_points=max_points)
    check_cloud(what, name2, t2, max_points=max_points)
    if t1.size(0) != t2.size(0):
        raise ValueError(f"{what}: batch sizes differ ({t1.size(0)} and {t2.size(0)})")
    if device is not None:
        refuse = _lib.require_device if device == "contiguous" else on_device
        refuse(t1, name1)
        refuse(t2, name2)
    if same_device and t1.device != t2.device:
        raise ValueError(f"{what}: {name1} and {name2} are on different devices")


def optional_lengths(lengths, b, width, dev, name):
    """None, or the int32 tensor [b] on `dev` of ragged.device_lengths."""
    return None if lengths is None else device_lengths(lengths, b, width, dev, name)[0]


def check_count(what, name, v, top=None, refuse_bool=False):
    """`v` as an int: an integer >= 1 (and <= top).  A bool counts as the integer it is unless `refuse_bool`."""
    if (refuse_bool and isinstance(v, bool)) or int(v) != v or v < 1 or (top is not None and v > top):
        limit = "" if top is None else f" and <= {top}"
        raise ValueError(f"{what}: {name} must be an integer >= 1{limit}, got {v!r}")
    return int(v)


def fp32(t):
    """`t` as the kernels read it: detached, contiguous, fp32.  (A tensor that needs no gradient is detached as it is:
    the searches, which never detached, get no tensor operation they did not have.)"""
    return (t.detach() if t.requires_grad else t).contiguous().float()
