"""NumPy restatement of the definition in include/ops/sinkhorn.h -- the reference of tests/test_sinkhorn.py and
tests/test_sinkhorn_gpu.py.  Every function takes a dtype: np.float64 gives the reference, np.float32 the same code as
an fp32 restatement whose distance from the reference is the yardstick of the GPU tests (tolerance()).  The cost matrix
is the fp32 rule in both (it is part of the definition, not of the arithmetic under test), and both walk the same
schedule: max(eps, eps_start * decay^t) in double from the fp32 arguments, rounded to fp32."""
import numpy as np


def _length(length, n):
    return n if length is None else min(max(int(length), 0), n)


def cost_matrix(x, y, dtype=np.float64):
    """C[i, j] = ((dx * dx) + (dy * dy)) + (dz * dz) with dx = y[j].x - x[i].x, every step rounded to fp32."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    with np.errstate(all="ignore"):
        dx = y[None, :, 0] - x[:, None, 0]
        dy = y[None, :, 1] - x[:, None, 1]
        dz = y[None, :, 2] - x[:, None, 2]
        return (((dx * dx) + (dy * dy)) + (dz * dz)).astype(dtype)


def default_iters(eps, eps_start=None, decay=0.5):
    """The steps the schedule needs to reach eps plus 5; 20 without an eps_start."""
    eps, decay = float(np.float32(eps)), float(np.float32(decay))
    start = 0.0 if eps_start is None else float(np.float32(eps_start))
    if start <= 0.0:
        return 20
    reach = 0
    while start * decay ** reach > eps:
        reach += 1
    return reach + 5


def schedule(eps, iters=None, eps_start=None, decay=0.5):
    """[eps_0 .. eps_{iters-1}] as np.float32."""
    iters = default_iters(eps, eps_start, decay) if iters is None else int(iters)
    eps, decay = float(np.float32(eps)), float(np.float32(decay))
    start = 0.0 if eps_start is None else float(np.float32(eps_start))
    return [np.float32(max(eps, start * decay ** t)) if start > 0.0 else np.float32(eps) for t in range(iters)]


def _terms(C, pot, e, dtype):
    """(e, top [n,1], p [n,m]): the terms exp(z - top) of log(1/m) + (pot_j - C_ij) / e against each row's maximum."""
    e = dtype(e)
    z = np.log(dtype(1) / dtype(C.shape[1])) + (pot.astype(dtype)[None, :] - C) / e
    top = z.max(axis=1, keepdims=True)
    z -= top
    return e, top, np.exp(z, out=z)


def softmin(C, pot, e, dtype):
    """out_i = -e log sum_j exp(log(1/m) + (pot_j - C_ij) / e) for the rows of C [n,m], in `dtype`."""
    e, top, p = _terms(C, pot, e, dtype)
    return (-e * (top[:, 0] + np.log(p.sum(axis=1)))).astype(dtype)


def softmin_weights(C, pot, e, dtype):
    """(softmin [n], w [n,m]): the same and its normalised terms, w = softmax over j."""
    e, top, p = _terms(C, pot, e, dtype)
    total = p.sum(axis=1, keepdims=True)
    return (-e * (top[:, 0] + np.log(total[:, 0]))).astype(dtype), p / total


def solve(x, y, eps, iters=None, eps_start=None, decay=0.5, dtype=np.float64, x_length=None, y_length=None, g0=None):
    """(f [n], g [m]) of one cloud pair in `dtype`; padding rows 0, an empty side gives zeros."""
    n, m = x.shape[0], y.shape[0]
    lx, ly = _length(x_length, n), _length(y_length, m)
    f, g = np.zeros(n, dtype), np.zeros(m, dtype)
    if lx == 0 or ly == 0:
        return f, g
    C = cost_matrix(x[:lx], y[:ly], dtype)
    Ct = np.ascontiguousarray(C.T)
    gl = np.zeros(ly, dtype) if g0 is None else np.asarray(g0)[:ly].astype(dtype)
    for e in schedule(eps, iters, eps_start, decay):
        fl = softmin(C, gl, e, dtype)
        gl = softmin(Ct, fl, e, dtype)
    f[:lx], g[:ly] = fl, gl
    return f, g


def solve_batch(x, y, eps, iters=None, eps_start=None, decay=0.5, dtype=np.float64, x_lengths=None, y_lengths=None,
                g0=None):
    """(f [b,n], g [b,m])."""
    out = [solve(x[i], y[i], eps, iters, eps_start, decay, dtype, None if x_lengths is None else x_lengths[i],
                 None if y_lengths is None else y_lengths[i], None if g0 is None else g0[i]) for i in range(len(x))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def barycenter(q, t, pot, eps, dtype=np.float64, q_length=None, t_length=None):
    """(bary [n,3], softmin [n]): sum_j w_ij t_j with w = softmax_j(log(1/len_t) + (pot_j - C_ij) / eps); 0 at padding
    rows and for an empty side."""
    n, m = q.shape[0], t.shape[0]
    lq, lt = _length(q_length, n), _length(t_length, m)
    bary, out = np.zeros((n, 3), dtype), np.zeros(n, dtype)
    if lq == 0 or lt == 0:
        return bary, out
    o, w = softmin_weights(cost_matrix(q[:lq], t[:lt], dtype), np.asarray(pot)[:lt], np.float32(eps), dtype)
    bary[:lq], out[:lq] = w @ np.asarray(t[:lt], np.float32).astype(dtype), o
    return bary, out


def value(f, g, x_length=None, y_length=None):
    """OT = sum_i a_i f_i + sum_j b_j g_j in float64, rounded once to the potentials' dtype."""
    lx, ly = _length(x_length, f.shape[0]), _length(y_length, g.shape[0])
    if lx == 0 or ly == 0:
        return f.dtype.type(0)
    return f.dtype.type(f[:lx].astype(np.float64).sum() / lx + g[:ly].astype(np.float64).sum() / ly)


def gradients(x, y, f, g, eps, dtype=np.float64, x_length=None, y_length=None):
    """(dOT/dx [n,3], dOT/dy [m,3]) by the last-iterate formula from the given potentials."""
    lx, ly = _length(x_length, x.shape[0]), _length(y_length, y.shape[0])
    gx, gy = np.zeros((x.shape[0], 3), dtype), np.zeros((y.shape[0], 3), dtype)
    if lx == 0 or ly == 0:
        return gx, gy
    bx, _ = barycenter(x, y, g, eps, dtype, lx, ly)
    by, _ = barycenter(y, x, f, eps, dtype, ly, lx)
    gx[:lx] = dtype(2) / dtype(lx) * (np.asarray(x[:lx], np.float32).astype(dtype) - bx[:lx])
    gy[:ly] = dtype(2) / dtype(ly) * (np.asarray(y[:ly], np.float32).astype(dtype) - by[:ly])
    return gx, gy


def plan(x, y, f, g, eps):
    """The float64 transport plan P_ij = a_i b_j exp((f_i + g_j - C_ij) / eps) of dense clouds, and C."""
    C = cost_matrix(x, y, np.float64)
    e = np.float64(np.float32(eps))
    P = np.exp((f.astype(np.float64)[:, None] + g.astype(np.float64)[None, :] - C) / e) / (C.shape[0] * C.shape[1])
    return P, C


def divergence(x, y, eps, iters=None, eps_start=None, decay=0.5, dtype=np.float64):
    """(S, dS/dx, dS/dy) of one dense pair: OT(x,y) - OT(x,x)/2 - OT(y,y)/2, each term solved on its own, the two roles
    of a cloud in its symmetric term added."""
    def term(a, b):
        f, g = solve(a, b, eps, iters, eps_start, decay, dtype)
        ga, gb = gradients(a, b, f, g, schedule(eps, iters, eps_start, decay)[-1], dtype)
        return dtype(value(f, g)), ga, gb

    vxy, gx, gy = term(x, y)
    vxx, a1, a2 = term(x, x)
    vyy, b1, b2 = term(y, y)
    return vxy - vxx / 2 - vyy / 2, gx - (a1 + a2) / 2, gy - (b1 + b2) / 2


def tolerance(q32, q64):
    """(bound, E32, floor) of the rule for a compared quantity: the kernel must satisfy
    max|q_gpu - q64| <= 4 * max(E32, floor), E32 = max|q32 - q64|, floor = 2^-22 * max(1, max|q64|)."""
    q32, q64 = np.asarray(q32, np.float64), np.asarray(q64, np.float64)
    e32 = float(np.max(np.abs(q32 - q64))) if q64.size else 0.0
    floor = 2.0 ** -22 * max(1.0, float(np.max(np.abs(q64))) if q64.size else 0.0)
    return 4.0 * max(e32, floor), e32, floor
