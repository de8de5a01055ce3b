"""NumPy restatement of include/ops/local_pca.h -- the reference of tests/test_normals.py and tests/test_normals_gpu.py.
The covariance is built in float64 in the header's order (valid slots left to right, every product, sum and quotient
rounded separately: NumPy never contracts); the eigen-decomposition is np.linalg.eigh, NOT the library's Jacobi, so the
two solvers check each other; the signs follow the header's rule."""
import numpy as np


def covariance(xyz, idx):
    """(c [m] int, C [m,3,3] float64, mu [m,3]) of the neighbourhoods idx [m,k] names among xyz [n,3] fp32.  A slot
    outside [0, n) adds 0.0, which leaves a sum as it is.  c == 0 gives C = 0."""
    xyz, idx = np.asarray(xyz, np.float32), np.asarray(idx)
    n, (m, k) = len(xyz), idx.shape
    valid = (idx >= 0) & (idx < n)
    p = xyz[np.where(valid, idx, 0)].astype(np.float64)      # [m,k,3]
    c = valid.sum(axis=1)
    count = np.maximum(c, 1).astype(np.float64)
    s = np.zeros((m, 3))
    for t in range(k):
        s = s + np.where(valid[:, t, None], p[:, t], 0.0)
    mu = s / count[:, None]
    acc = np.zeros((m, 3, 3))
    for t in range(k):
        d = p[:, t] - mu
        acc = acc + np.where(valid[:, t, None, None], d[:, :, None] * d[:, None, :], 0.0)
    return c, acc / count[:, None, None], mu


def canonical(v):
    """v [m,3] with the component of largest magnitude positive; equal magnitudes go to the lowest axis (argmax takes
    the first)."""
    big = np.take_along_axis(v, np.argmax(np.abs(v), axis=1)[:, None], axis=1)
    return np.where(big < 0, -v, v)


def local_pca(xyz, idx, new_xyz=None, viewpoint=None):
    """dict of c [m], C [m,3,3], eigenvalues [m,3] ascending, frames [m,3,3] float64 (row r: unit eigenvector of
    eigenvalue r, signed and right-handed as the header says) and normals [m,3] = frames[:, 0] for one cloud."""
    c, C, _ = covariance(xyz, idx)
    w, v = np.linalg.eigh(C)
    e2 = canonical(v[:, :, 2])
    e0 = canonical(v[:, :, 0])
    if viewpoint is not None:
        toward = np.asarray(viewpoint, np.float32).astype(np.float64)[None, :] - np.asarray(new_xyz, np.float32).astype(np.float64)
        dot = ((e0[:, 0] * toward[:, 0]) + (e0[:, 1] * toward[:, 1])) + (e0[:, 2] * toward[:, 2])
        e0 = np.where((dot < 0)[:, None], -e0, e0)
    frames = np.stack([e0, np.cross(e2, e0), e2], axis=1)
    empty = c == 0
    w[empty], frames[empty] = 0.0, 0.0
    return {"c": c, "C": C, "eigenvalues": w, "frames": frames, "normals": frames[:, 0]}


def surface_variation(eigenvalues):
    trace = eigenvalues.sum(axis=-1)
    return np.where(trace == 0, 0.0, eigenvalues[..., 0] / np.where(trace == 0, 1.0, trace))


def chamfer_indices(x, y):
    """(idx1 [n], idx2 [m]): the lowest index of the nearest neighbour each way, fp32 distances as the Chamfer search
    forms them (neighbors_ref.dist_matrix has the same expression)."""
    from neighbors_ref import dist_matrix

    d = dist_matrix(x, y)
    return np.argmin(d, axis=1).astype(np.int32), np.argmin(d, axis=0).astype(np.int32)


def normal_consistency(n1, n2, idx1, idx2):
    """0.5 * (mean_i |n1_i . n2[idx1_i]| + mean_j |n2_j . n1[idx2_j]|) in float64."""
    n1, n2 = n1.astype(np.float64), n2.astype(np.float64)
    return 0.5 * (np.abs((n1 * n2[idx1]).sum(axis=1)).mean() + np.abs((n2 * n1[idx2]).sum(axis=1)).mean())


def point_to_plane(x, y, n2, idx1, idx2):
    """The point-to-plane Chamfer expression in float64."""
    x, y, n2 = x.astype(np.float64), y.astype(np.float64), n2.astype(np.float64)
    off1 = (n2[idx1] * (x - y[idx1])).sum(axis=1)
    off2 = (n2 * (y - x[idx2])).sum(axis=1)
    return (off1 * off1).mean() + (off2 * off2).mean()
