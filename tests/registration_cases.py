"""What tests/test_registration.py (host entry points, CPU tensors) and tests/test_registration_gpu.py (device) share: the
clouds, the cases, the reference's answers and the comparison at derived tolerances.

Tolerances.  u = 2^-53.  All quantities below come from the REFERENCE's float64 arrays of the case.

Fit, point mode.  The library adds w (p-a)(q-c)^T over a tree of at most 4 + 8 + 3 + n / 1024 additions per entry, so S
carries a backward error of a small multiple of u T, T = sum w |p - a| |q - c| (a, c the pivots: the first rows).  N(S)
is linear in S, the Jacobi solver makes at most 96 rotations, each an orthogonal similarity with an error of a few
u ||N||, and ||N|| <= 3 T.  By Davis-Kahan the quaternion, and with it R, moves by at most (perturbation) / gap, gap =
lambda_1 - lambda_2 of N(S).  LAPACK's SVD in the reference has an error of the same form.  So
    |R - R_ref|  <= K E_R,   E_R = u T / gap                                    (dimensionless)
    |t - t_ref|  <= K E_t,   E_t = E_R s |mu_p| + u (|mu_q| + s |mu_p|)          (t = mu_q - s R mu_p)
    |s - s_ref|  <= K E_R s
T is taken about the pivots, so a cloud translated to (1000, -2000, 500) has the T, the gap and therefore the SAME
tolerance on R as at the origin: that is what the pivots are for.
Fit, plane mode.  x solves (J^T J) x = -J^T r; both sides solve it backward-stably, so x moves by a multiple of
u cond(J^T J) |x|, and t = a + tau - R a adds u |a|:
    |pose - pose_ref| <= K E_P,   E_P = u (cond(J^T J) |x| + 1 + |a|)
Measures.  rmse is the root of a sum of n positive terms over W: |rmse - rmse_ref| <= K u rmse_ref.  fitness and the
flags are exact.
The derivation leaves K.  It is MEASURED: the host entry point's worst deviation from the reference over every case
below, in the units above, was 8.9 (on the CPU, LAPACK of NumPy 2.x); K is 8 times that, which covers the different but
equally valid rounding of another LAPACK against Jacobi.
Where R is not unique (mirrored, coplanar, collinear targets, a single pair, n <= 2) the checks are: R is proper --
|det R - 1| <= 16 u, |R^T R - I| <= 16 u -- and attains the reference's objective: |f - f_ref| <= (n + 16) u sum w (|p -
mu_p| + |q - mu_q|)^2 + n (8 u (|p| + |q| + |t|))^2, the rounding of evaluating f itself -- of the sum, and of each
residual where f is 0 -- (R enters f in the second order only).

ICP.  Library and reference walk the same trajectory while their searches agree, and each step's deviation is that of
a fit; a step's deviation is carried on by the following steps with a factor below 1 (the iteration contracts).  So
    |pose - pose_ref| <= K_ICP u (iterations + 1)
K_ICP is measured the same way: the worst figure over the ICP cases was 30.6 (plane mode from 30 degrees; the
point-to-plane systems of the box are the worse conditioned); K_ICP is 8 times that.  "Recovers the true pose": the freeze rule stops when
the rmse moves by less than atol = 1e-7; with a contraction rate of at most 0.9 the remaining rmse is below 1e-6, which at
the shape's lever arm of about 1 is 1e-6 rad = 6e-5 degrees: angle error <= 1e-4 degrees, translation error <= 2e-6.
The reported rmse is taken from points rounded to fp32, and a pose that differs in the last bits may round a
coordinate the other way: |rmse - rmse_ref| <= K_ICP u rmse_ref + 2^-23 (one fp32 step at unit scale per point).
Every figure is printed before anything is asserted."""
import functools

import numpy as np
import torch

import registration_ref as ref

U = 2.0 ** -53
K = 8 * 8.9             # 8 x the measured worst deviation of the host entry point (8.9), in the units of the module text
K_ICP = 8 * 30.6        # 8 x the measured worst figure of the ICP cases (30.6)
C = 1024                # the chunk of include/ops/rigid_fit.h
NS = [1, 2, 3, 63, 64, 65, C - 1, C, C + 1, 2 * C + 5]
TRUE_ANGLE_DEG, TRUE_SHIFT = 1e-4, 2e-6


def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def _tensor(a):
    """A tensor of a copy of the array (the cases' arrays are read-only)."""
    return torch.from_numpy(np.array(a))


def rotation(deg, axis=(1.0, 2.0, 3.0)):
    axis = np.asarray(axis, np.float64)
    return ref.rodrigues(np.deg2rad(deg) * axis / np.linalg.norm(axis))


def pose_of(deg, shift=(0.0, 0.0, 0.0)):
    pose = np.eye(4)
    pose[:3, :3], pose[:3, 3] = rotation(deg), shift
    return pose


SHIFT = (0.05, -0.03, 0.02)


# ------------------------------------------------------------------------------------------------------ clouds
@functools.lru_cache(maxsize=None)
def two_box(n, seed):
    """(points [n,3] fp32, normals [n,3] fp32) on the asymmetric two-box surface: a 1.0 x 0.6 x 0.3 box with a 0.3 x 0.2 x
    0.4 box set on it, sampled uniformly by area (the small box has no bottom face)."""
    rng = np.random.default_rng(seed)
    faces = []      # (origin, edge 1, edge 2, normal)
    for lo, size, bottom in (((0.0, 0.0, 0.0), (1.0, 0.6, 0.3), True), ((0.1, 0.05, 0.3), (0.3, 0.2, 0.4), False)):
        lo, size = np.array(lo), np.array(size)
        for axis in range(3):
            e1, e2 = np.zeros(3), np.zeros(3)
            e1[(axis + 1) % 3], e2[(axis + 2) % 3] = size[(axis + 1) % 3], size[(axis + 2) % 3]
            for side in (0, 1):
                if axis == 2 and side == 0 and not bottom:
                    continue
                origin, normal = lo.copy(), np.zeros(3)
                origin[axis] += side * size[axis]
                normal[axis] = 2.0 * side - 1.0
                faces.append((origin, e1, e2, normal))
    area = np.array([np.linalg.norm(np.cross(f[1], f[2])) for f in faces])
    pick = rng.choice(len(faces), size=n, p=area / area.sum())
    uv = rng.random((n, 2))
    pts = np.stack([faces[k][0] + uv[i, 0] * faces[k][1] + uv[i, 1] * faces[k][2] for i, k in enumerate(pick)])
    nrm = np.stack([faces[k][3] for k in pick])
    return _frozen(pts.astype(np.float32), nrm.astype(np.float32))


def moved_copy(p, pose, scale=1.0, noise=0.0, rng=None):
    q = scale * p.astype(np.float64) @ pose[:3, :3].T + pose[:3, 3]
    if noise:
        q = q + noise * rng.standard_normal(q.shape)
    return q.astype(np.float32)


# ------------------------------------------------------------------------------------------------------ fit cases
def _case(name, src, dst, check="pose", **options):
    return dict(name=name, src=src, dst=dst, check=check, **options)


@functools.lru_cache(maxsize=None)
def fit_cases():
    rng = np.random.default_rng(7)
    pose = pose_of(70.0, (0.3, -0.2, 0.1))
    cases = []
    for n in NS:
        p = rng.random((n, 3)).astype(np.float32)
        cases.append(_case(f"rows{n}", p, moved_copy(p, pose, noise=0.01, rng=rng), check="pose" if n >= 3 else "objective"))
    p = rng.random((300, 3)).astype(np.float32)
    cases.append(_case("exact", p, moved_copy(p, pose)))
    cases.append(_case("noise", p, moved_copy(p, pose, noise=0.01, rng=rng)))
    cases.append(_case("mirrored", p, moved_copy(p * np.float32([-1, 1, 1]), pose), check="objective"))
    flat = p * np.float32([1, 1, 0])
    cases.append(_case("coplanar", flat, moved_copy(flat, pose), check="objective"))
    line = (p[:, :1] * np.float32([1.0, 0.5, -0.25])).astype(np.float32)
    cases.append(_case("collinear", line, moved_copy(line, pose), check="objective"))
    w = rng.random(300).astype(np.float32)
    w[::3] = 0
    cases.append(_case("weights", p, moved_copy(p, pose, noise=0.01, rng=rng), weight=w))
    idx = rng.permutation(300).astype(np.int32)
    q = np.empty_like(p)
    q[idx] = moved_copy(p, pose, noise=0.01, rng=rng)
    holes = idx.copy()
    holes[[3, 50]], holes[[7, 90]], holes[11] = -1, (300, 305), -7
    cases.append(_case("idx_holes", p, q, idx=holes))
    cases.append(_case("idx_perm_longer", p, np.concatenate([q, rng.random((37, 3)).astype(np.float32)]), idx=idx))
    far = moved_copy(p, pose, noise=0.01, rng=rng)
    far[::7] += np.float32(0.5)
    cases.append(_case("max_dist_some", p, far, max_dist=0.2, init=pose))
    cases.append(_case("max_dist_all", p, far + np.float32(5.0), max_dist=0.2, init=pose, check="empty"))
    bad_p, bad_q = p.copy(), moved_copy(p, pose, noise=0.01, rng=rng)
    bad_p[5, 1], bad_q[9, 0] = np.nan, np.inf
    cases.append(_case("nonfinite", bad_p, bad_q))
    bad_first = bad_p.copy()
    bad_first[0, 2] = np.inf
    cases.append(_case("nonfinite_pivot", bad_first, bad_q))
    for s in (0.5, 3.0):
        cases.append(_case(f"scale{s}", p, moved_copy(p, pose, scale=s, noise=0.01, rng=rng), with_scale=True))
    off = np.float32([1000.0, -2000.0, 500.0])
    unit_q = moved_copy(p, pose, noise=0.01, rng=rng)
    cases.append(_case("origin_twin", p, unit_q))
    cases.append(_case("translated", p + off, unit_q + off))
    box, normals = two_box(600, 11)
    small = pose_of(3.0, (0.01, -0.02, 0.015))
    cases.append(_case("plane_box", moved_copy(box, small), box, mode="plane", normals=normals))
    cases.append(_case("plane_box_far", moved_copy(box, small) + off, box + off, mode="plane", normals=normals))
    one = (rng.random((200, 3)) * [1, 1, 0] + [0, 0, 0.2]).astype(np.float32)
    up = np.tile(np.float32([0, 0, 1]), (200, 1))
    cases.append(_case("plane_single", moved_copy(one, small), one, mode="plane", normals=up, check="singular"))
    for c in cases:
        _frozen(*[v for v in c.values()])
    return cases


def fit_case(name):
    return next(c for c in fit_cases() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def fit_reference(name):
    """(the reference's Fit -- its pose is the UPDATE --, the source under init) of a listed case."""
    return reference_of(fit_case(name))


def reference_of(c):
    init = c.get("init")
    moved = c["src"] if init is None else ref.transform(c["src"], init)
    f = ref.step(moved, c["dst"], c.get("idx"), c.get("weight"), None, None, c.get("max_dist"), c.get("mode", "point"),
                 c.get("normals"), c.get("with_scale", False))
    return f, moved


def _filler(c, seed):
    rng = np.random.default_rng(seed)
    n, m = c["src"].shape[0], c["dst"].shape[0]
    src = rng.random((n, 3)).astype(np.float32)
    dst = rng.random((m, 3)).astype(np.float32)
    return src, dst, rng.integers(0, m, n).astype(np.int32), rng.random(n).astype(np.float32), \
        rng.standard_normal((m, 3)).astype(np.float32)


def run_fit(c, device, batch):
    """RigidFit fields of the case's cloud as NumPy arrays, from a call on a batch of 1 or 3 clouds (the case in the
    middle, fillers of the same shape around it)."""
    from sparenet_amd.cuda.registration import rigid_fit

    at = 0 if batch == 1 else 1
    parts = [(c["src"], c["dst"], c.get("idx"), c.get("weight"), c.get("normals"))]
    if batch == 3:
        f0, f1 = _filler(c, 1), _filler(c, 2)
        parts = [f0, parts[0], f1]

    def stack(k, like, dtype=None):
        if c.get(like) is None:
            return None
        return _tensor(np.stack([np.asarray(p[k]) for p in parts])).to(device)

    src = _tensor(np.stack([p[0] for p in parts])).to(device)
    dst = _tensor(np.stack([p[1] for p in parts])).to(device)
    init = None if c.get("init") is None else _tensor(np.asarray(c["init"])).to(device)
    out = rigid_fit(src, dst, stack(2, "idx"), stack(3, "weight"), None, None, c.get("with_scale", False),
                    c.get("max_dist"), c.get("mode", "point"), stack(4, "normals"), init)
    return tuple(t[at].cpu().numpy() for t in out)


def _proper(R, what):
    det, orth = abs(np.linalg.det(R) - 1.0), np.abs(R.T @ R - np.eye(3)).max()
    print(f"{what}: |det R - 1| = {det:.3g}, |R^T R - I| = {orth:.3g} (bound {16 * U:.3g})")
    return det <= 16 * U and orth <= 16 * U


def fit_deviation(c, got, reference=None):
    """The worst deviation of a "pose" case from the reference in the module text's units (what K bounds)."""
    pose, scale, rmse, fitness, flags = got
    f, moved = reference or fit_reference(c["name"])
    init = np.eye(4) if c.get("init") is None else np.asarray(c["init"])
    want, want_scale = ref.compose(f.pose, f.scale, init, 1.0)
    rows, j, w, _ = ref.inliers(moved, c["dst"], c.get("idx"), c.get("weight"), moved.shape[0], c["dst"].shape[0],
                                c.get("max_dist"), c.get("normals") if c.get("mode") == "plane" else None)
    p, q = moved.astype(np.float64)[rows], c["dst"].astype(np.float64)[j]
    a = moved[0].astype(np.float64) if np.isfinite(moved[0]).all() else np.zeros(3)
    cc = c["dst"][0].astype(np.float64) if np.isfinite(c["dst"][0]).all() else np.zeros(3)
    if c.get("mode", "point") == "point":
        T = (w * np.linalg.norm(p - a, axis=1) * np.linalg.norm(q - cc, axis=1)).sum()
        mp, mq = (w[:, None] * p).sum(0) / w.sum(), (w[:, None] * q).sum(0) / w.sum()
        S = ((w[:, None] * (p - mp)).T @ (q - mq))
        lam = np.linalg.eigvalsh(_horn(S))
        e_r = U * T / (lam[-1] - lam[-2])
        s = f.scale
        e_t = e_r * s * np.linalg.norm(mp) + U * (np.linalg.norm(mq) + s * np.linalg.norm(mp))
        # the update is what the tolerances describe: compare it, not its product with init
        upd_r = pose[:3, :3] @ init[:3, :3].T
        upd_t = pose[:3, 3] - scale * upd_r @ init[:3, 3]
        dev = max(np.abs(upd_r - f.pose[:3, :3]).max() / e_r, np.abs(upd_t - f.pose[:3, 3]).max() / e_t,
                  abs(scale - want_scale) / (e_r * s))
    else:
        u = p - a
        nrm = c["normals"].astype(np.float64)[j]
        J = np.concatenate([np.cross(u, nrm), nrm], axis=1)
        A = (w[:, None] * J).T @ J
        x = np.linalg.solve(A, -(w[:, None] * J).T @ (nrm * (p - q)).sum(1))
        e_p = U * (np.linalg.cond(A) * np.linalg.norm(x) + 1 + np.linalg.norm(a))
        dev = np.abs(pose - want).max() / e_p
    dev = max(dev, abs(rmse - f.rmse) / (U * f.rmse) if f.rmse > 0 else abs(rmse))
    return float(dev)


def _horn(S):
    return np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                     [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                     [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], -S[0, 0] + S[1, 1] - S[2, 2], S[1, 2] + S[2, 1]],
                     [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], -S[0, 0] - S[1, 1] + S[2, 2]]])


def check_fit(c, got):
    """The case's check on the RigidFit fields of its cloud."""
    pose, scale, rmse, fitness, flags = got
    name, kind = c["name"], c["check"]
    f, moved = fit_reference(name)
    init = np.eye(4) if c.get("init") is None else np.asarray(c["init"])
    print(f"{name}: flags {int(flags)} (reference {f.flags}), fitness {fitness!r} (reference {f.fitness!r}), "
          f"rmse {rmse!r} (reference {f.rmse!r})")
    assert int(flags) == f.flags
    assert fitness == f.fitness
    assert np.array_equal(pose[3], [0, 0, 0, 1])
    if kind in ("empty", "singular"):
        assert int(flags) == (ref.EMPTY if kind == "empty" else ref.SINGULAR)
        assert pose.tobytes() == init.tobytes() and scale == 1.0, "the pose must keep every bit"
        if kind == "empty":
            assert rmse == 0.0 and fitness == 0.0
        return
    if kind == "pose":
        dev = fit_deviation(c, got)
        print(f"{name}: deviation {dev:.3g} (bound K = {K:.3g})")
        assert dev <= K
        return
    # the minimiser is not unique: a proper rotation that attains the reference's objective
    assert _proper(pose[:3, :3], name)
    rows, j, w, _ = ref.inliers(moved, c["dst"], c.get("idx"), c.get("weight"), moved.shape[0], c["dst"].shape[0],
                                c.get("max_dist"))
    want, want_scale = ref.compose(f.pose, f.scale, init, 1.0)
    mine = ref.objective(pose, float(scale), c["src"], c["dst"], rows, j, w)
    theirs = ref.objective(want, want_scale, c["src"], c["dst"], rows, j, w)
    p, q = c["src"].astype(np.float64)[rows], c["dst"].astype(np.float64)[j]
    spread = (w * (np.linalg.norm(p - p.mean(0), axis=1) + np.linalg.norm(q - q.mean(0), axis=1)) ** 2).sum()
    reach = np.abs(p).max() + np.abs(q).max() + np.abs(pose[:3, 3]).max()
    bound = (len(rows) + 16) * U * spread + len(rows) * (8 * U * reach) ** 2
    print(f"{name}: objective {mine!r}, reference {theirs!r}, bound on the difference {bound:.3g}")
    assert abs(mine - theirs) <= bound
    assert abs(rmse - f.rmse) <= K * U * f.rmse


# ------------------------------------------------------------------------------------------------------ ICP cases
ICP_N = 2048
ICP_ITERS = 60


@functools.lru_cache(maxsize=None)
def icp_clouds(kind, deg):
    """(src, dst, dst normals, the true pose src -> dst) of the two-box shape started `deg` degrees about (1,2,3) plus
    SHIFT off: kind "same" moves the very points, "resampled" draws the target anew from the surface."""
    pts, _ = two_box(ICP_N, 21)
    truth = pose_of(deg, SHIFT)
    if kind == "same":
        dst, normals = moved_copy(pts, truth), None
    else:
        base, nrm = two_box(ICP_N, 22)
        dst = moved_copy(base, truth)
        normals = (nrm.astype(np.float64) @ truth[:3, :3].T).astype(np.float32)
    return _frozen(pts, dst, normals, truth)


@functools.lru_cache(maxsize=None)
def icp_reference(kind, deg, mode, max_dist=None, init_deg=None, length=None):
    src, dst, normals, _ = icp_clouds(kind, deg)
    init = None if init_deg is None else pose_of(init_deg, SHIFT)
    n = ICP_N if length is None else length
    return ref.icp(src, dst, ICP_ITERS, mode, normals if mode == "plane" else None, max_dist, init, src_len=n, dst_len=n)


def run_icp(device, kind, deg, mode, iters=ICP_ITERS, max_dist=None, init_deg=None):
    from sparenet_amd.cuda.registration import icp

    src, dst, normals, _ = icp_clouds(kind, deg)
    to = lambda a: None if a is None else _tensor(np.asarray(a))[None].to(device)      # noqa: E731
    init = None if init_deg is None else _tensor(pose_of(init_deg, SHIFT)).to(device)
    return icp(to(src), to(dst), iters, mode, to(normals) if mode == "plane" else None, max_dist, init)


def icp_deviation(got_pose, want):
    return float(np.abs(got_pose - want.pose).max() / (U * (want.iterations + 1)))


def check_icp(what, out, want, at=0):
    pose = out.pose[at].cpu().numpy()
    dev = icp_deviation(pose, want)
    print(f"{what}: iterations {int(out.iterations[at])} (reference {want.iterations}), converged "
          f"{bool(out.converged[at])}, rmse {float(out.rmse[at])!r} (reference {want.rmse!r}), fitness "
          f"{float(out.fitness[at])!r} (reference {want.fitness!r}), deviation {dev:.3g} (bound K_ICP = {K_ICP:.3g})")
    assert bool(out.converged[at]) and want.converged
    assert int(out.flags[at]) & ref.FROZEN
    assert dev <= K_ICP
    assert float(out.fitness[at]) == want.fitness
    assert abs(float(out.rmse[at]) - want.rmse) <= K_ICP * U * want.rmse + 2.0 ** -23
    return dev


def pose_error(pose, truth):
    """(angle in degrees, translation error) between two poses."""
    d = pose[:3, :3] @ truth[:3, :3].T
    angle = np.degrees(np.arccos(np.clip((np.trace(d) - 1) / 2, -1, 1)))
    # arccos loses half the digits near 0: the skew part is exact to first order
    skew = 0.5 * np.array([d[2, 1] - d[1, 2], d[0, 2] - d[2, 0], d[1, 0] - d[0, 1]])
    angle = min(angle, np.degrees(np.linalg.norm(skew))) if angle < 1 else angle
    return float(angle), float(np.abs(pose[:3, 3] - truth[:3, 3]).max())


def same_bits(a, b):
    """Every field of two results agrees in every bit."""
    return all(torch.equal(x.cpu(), y.cpu()) and x.dtype == y.dtype for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------------ scenarios
# What both test files run, on their device; each returns the tensors it got, which the GPU file compares with the
# host's bit for bit.
def ragged_fit_scenario(device):
    """A batch of three clouds with lengths (n, 0, n / 2): each cloud is the reference's fit of its valid rows."""
    from sparenet_amd.cuda.registration import rigid_fit

    rng = np.random.default_rng(31)
    n, pose = 1500, pose_of(70.0, (0.3, -0.2, 0.1))
    src = rng.random((3, n, 3)).astype(np.float32)
    dst = np.stack([moved_copy(s, pose, noise=0.01, rng=rng) for s in src])
    src_len, dst_len = [n, 0, n // 2], [n, n, n // 2 - 10]
    src[2, n // 2:], dst[2, n // 2 - 10:] = np.nan, np.nan      # padding is never read
    out = rigid_fit(_tensor(src).to(device), _tensor(dst).to(device), src_lengths=src_len,
                    dst_lengths=torch.tensor(dst_len))
    for i in range(3):
        c = _case(f"ragged{i}", src[i], dst[i])
        f = ref.step(src[i], dst[i], None, None, src_len[i], dst_len[i])
        got = tuple(t[i].cpu().numpy() for t in out)
        print(f"ragged cloud {i}: flags {int(got[4])} (reference {f.flags}), fitness {got[3]!r} (reference {f.fitness!r})")
        assert int(got[4]) == f.flags and got[3] == f.fitness
        if f.flags & ref.EMPTY:
            assert got[0].tobytes() == np.eye(4).tobytes() and got[2] == 0.0
            continue
        rows = f.inliers      # the deviation in the module's units, from the valid pairs alone
        sub = _case(c["name"], src[i][rows], dst[i][rows])
        dev = fit_deviation(sub, got, reference_of(sub))
        print(f"ragged cloud {i}: deviation {dev:.3g} (bound K = {K:.3g})")
        assert dev <= K
    return list(out)


def transform_scenario(device):
    from sparenet_amd.cuda.registration import transform_points

    rng = np.random.default_rng(41)
    outs = []
    for n in (1, 255, 256, 257, 1000):
        xyz = (rng.standard_normal((3, n, 3)) * 10).astype(np.float32)
        poses = np.stack([pose_of(d, (1.5, -2.5, 0.25)) for d in (70.0, 0.0, 200.0)])
        scale = np.array([1.0, 0.37, 3.0])
        lengths = [n, n // 2, 0]
        xyz[1, n // 2:] = np.nan
        for use_scale, use_lengths in ((False, False), (True, True)):
            got = transform_points(_tensor(xyz).to(device), _tensor(poses).to(device),
                                   _tensor(scale).to(device) if use_scale else None,
                                   lengths if use_lengths else None)
            for i in range(3):
                want = ref.transform(xyz[i], poses[i], scale[i] if use_scale else 1.0, lengths[i] if use_lengths else None)
                assert got[i].cpu().numpy().tobytes() == want.tobytes(), (n, use_scale, i)
            outs.append(got)
        shared = transform_points(_tensor(xyz[:1]).to(device), _tensor(poses[0]).to(device), 2.0)
        assert shared[0].cpu().numpy().tobytes() == ref.transform(xyz[0], poses[0], 2.0).tobytes()
    return outs


def gradient_scenario(device):
    """Both gradients against float64 torch autograd of s R x + t over the valid rows: the forward is rounded to fp32,
    the backward is float64 arithmetic on the same inputs, so the comparison is at a few units of float64 rounding
    (pose) and of fp32 rounding (xyz, whose gradient is returned in the cloud's dtype)."""
    from sparenet_amd.cuda.registration import transform_points

    rng = np.random.default_rng(43)
    b, n = 3, 77
    xyz = _tensor(rng.standard_normal((b, n, 3)).astype(np.float32)).to(device)
    g = _tensor(rng.standard_normal((b, n, 3)).astype(np.float32)).to(device)
    scale = torch.tensor([1.0, 0.5, 3.0], dtype=torch.float64, device=device)
    lengths = [n, 40, 0]
    mask = (torch.arange(n)[None, :] < torch.tensor(lengths)[:, None]).to(device)
    outs = []
    for shared in (False, True):
        pose = _tensor(pose_of(70.0, SHIFT) if shared else np.stack([pose_of(d, SHIFT) for d in (70.0, 10.0, 200.0)]))
        pose = pose.to(device)
        x1, p1 = xyz.clone().requires_grad_(True), pose.clone().requires_grad_(True)
        (transform_points(x1, p1, scale, lengths) * g).sum().backward()
        x2, p2 = xyz.double().requires_grad_(True), pose.clone().requires_grad_(True)
        full = p2 if p2.dim() == 3 else p2[None].expand(b, 4, 4)
        y = scale[:, None, None] * (x2 @ full[:, :3, :3].transpose(1, 2)) + full[:, None, :3, 3]
        (torch.where(mask[:, :, None], y, torch.zeros((), dtype=y.dtype, device=device)) * g.double()).sum().backward()
        ex = float((x1.grad.double() - x2.grad).abs().max())
        ep = float((p1.grad - p2.grad).abs().max())
        bound_x = 2.0 ** -23 * float(x2.grad.abs().max())
        bound_p = 64 * n * U * float((g.double().abs().sum(dim=1).max()) * (xyz.double().abs().max() + 1) * 3.0)
        print(f"shared pose {shared}: |grad xyz - ref| = {ex:.3g} (bound {bound_x:.3g}), |grad pose - ref| = {ep:.3g} "
              f"(bound {bound_p:.3g})")
        assert x1.grad.dtype == torch.float32 and p1.grad.shape == pose.shape and p1.grad.dtype == torch.float64
        assert ex <= bound_x and ep <= bound_p
        assert float(p1.grad[..., 3, :].abs().max()) == 0.0 and float(x1.grad[~mask].abs().max()) == 0.0
        outs += [x1.grad, p1.grad]
    return outs


def icp_same_scenario(device, deg):
    out = run_icp(device, "same", deg, "point")
    want = icp_reference("same", deg, "point")
    check_icp(f"same points, {deg} degrees", out, want)
    angle, shift = pose_error(out.pose[0].cpu().numpy(), icp_clouds("same", deg)[3])
    print(f"same points, {deg} degrees: angle error {angle:.3g} degrees (bound {TRUE_ANGLE_DEG}), translation error "
          f"{shift:.3g} (bound {TRUE_SHIFT})")
    assert angle <= TRUE_ANGLE_DEG and shift <= TRUE_SHIFT
    return list(out)


def icp_resampled_scenario(device, deg):
    outs, taken = [], {}
    for mode in ("point", "plane"):
        out = run_icp(device, "resampled", deg, mode)
        check_icp(f"resampled surface, {deg} degrees, {mode}", out, icp_reference("resampled", deg, mode))
        taken[mode] = int(out.iterations[0])
        outs += list(out)
    assert taken["plane"] < taken["point"], taken
    return outs


def icp_options_scenario(device):
    """A ragged batch of three lengths, max_dist = 0.1 and a given init."""
    from sparenet_amd.cuda.registration import icp

    src, dst, _, _ = icp_clouds("resampled", 10)
    lengths = [ICP_N, 1500, 700]
    s = _tensor(np.stack([src] * 3)).to(device)
    d = _tensor(np.stack([dst] * 3)).to(device)
    s[1, 1500:], d[2, 700:] = float("nan"), float("nan")
    out = icp(s, d, ICP_ITERS, src_lengths=lengths, dst_lengths=torch.tensor(lengths, dtype=torch.int32))
    for i, length in enumerate(lengths):
        check_icp(f"ragged batch, length {length}", out, icp_reference("resampled", 10, "point", length=length), at=i)
    near = run_icp(device, "resampled", 10, "point", max_dist=0.1)
    check_icp("max_dist 0.1", near, icp_reference("resampled", 10, "point", max_dist=0.1))
    assert float(near.fitness[0]) <= 1.0
    start = run_icp(device, "resampled", 30, "point", init_deg=25)
    check_icp("init 25 degrees", start, icp_reference("resampled", 30, "point", init_deg=25))
    assert int(start.iterations[0]) < int(run_icp(device, "resampled", 30, "point").iterations[0])
    return list(out) + list(near) + list(start)


def aligned_chamfer_scenario(device):
    """The distance after registration is far below the distance before it, equals the Chamfer mean of the moved cloud,
    and its gradient in pred is the plain Chamfer gradient carried back through s R (the pose is a constant)."""
    from sparenet_amd.cuda.chamfer_distance import ChamferDistanceFunction
    from sparenet_amd.cuda.registration import aligned_chamfer, transform_points

    src, dst, _, _ = icp_clouds("resampled", 10)
    pred = _tensor(src[:1024])[None].to(device).requires_grad_(True)
    gt = _tensor(dst[:1024])[None].to(device)
    value, found = aligned_chamfer(pred, gt, iters=40)
    d1, d2 = ChamferDistanceFunction.apply(pred.detach(), gt)
    before = float(d1.mean() + d2.mean())
    print(f"aligned Chamfer {float(value[0].detach()):.3g}, before registration {before:.3g}, converged {bool(found.converged[0])}")
    assert float(value[0].detach()) < 0.5 * before
    value.sum().backward()
    moved = transform_points(pred.detach(), found.pose, found.scale).requires_grad_(True)
    m1, m2 = ChamferDistanceFunction.apply(moved, gt)
    assert torch.equal(value.detach(), (m1.mean(dim=1) + m2.mean(dim=1)).detach())
    (m1.mean(dim=1) + m2.mean(dim=1)).sum().backward()
    want = (moved.grad.double() @ (found.scale[:, None, None] * found.pose[:, :3, :3])).float()
    assert torch.equal(pred.grad, want)
    lengths = [700]
    ragged, _ = aligned_chamfer(pred.detach(), gt, iters=5, src_lengths=lengths, dst_lengths=lengths)
    alone, _ = aligned_chamfer(pred.detach()[:, :700].contiguous(), gt[:, :700].contiguous(), iters=5)
    print(f"ragged {float(ragged[0])!r}, the valid rows alone {float(alone[0])!r}")
    assert abs(float(ragged[0]) - float(alone[0])) <= 2.0 ** -22 * float(alone[0])
    return [value.detach(), pred.grad, found.pose, ragged]
