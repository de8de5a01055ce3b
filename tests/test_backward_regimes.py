"""Backward passes under the upstream gradients a training step sends, against float64 references.

The other suites draw upstream gradients from torch.rand: positive, dense, finite, within a decade.  Here one
generator (_upstream) draws four regimes instead -- `signed` (standard normal), `wide` (random sign, magnitude
10**U(-6, 3)), `sparse` (99 % exact zeros, one image all zero) and `nonfinite` (`signed` plus NaN / +inf / -inf at
entries that have a winner / owner and at entries that have none) -- and every op is driven through its public
autograd path and compared with a reference built from the forward's own indices, assignments or winners:

- entry for entry, isfinite(gpu) == isfinite(ref); where the reference is +-inf the GPU gives that infinity or NaN;
- finite entries lie within the op's stated bound of the float64 reference (bit-equal for the ops that are
  bit-equal to the oracle).
"""
import functools
import math

import numpy as np
import pytest
import torch

import oracle

REGIMES = ["signed", "wide", "sparse", "nonfinite"]
EPS = 2.0 ** -24
_SEEDS = {r: i for i, r in enumerate(REGIMES)}


def _upstream(shape, regime, seed, owned=None, image_axis=None):
    """float32 upstream gradient of `shape` in `regime`.  owned: boolean mask of the entries that reach some input
    (a winner, an owner); `nonfinite` puts NaN, +inf and -inf both into owned and into not-owned entries.
    image_axis: `sparse` zeroes the first slice along this axis (one all-zero image)."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(shape).astype(np.float32)
    if regime == "wide":
        g = (np.where(rng.random(shape) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-6, 3, shape)).astype(np.float32)
    elif regime == "sparse":
        g[rng.random(shape) < 0.99] = 0.0
        if image_axis is not None:
            np.moveaxis(g, image_axis, 0)[0] = 0.0
    elif regime == "nonfinite":
        flat = g.reshape(-1)
        own = np.ones(flat.size, bool) if owned is None else np.asarray(owned).reshape(-1)
        for pool in (np.flatnonzero(own), np.flatnonzero(~own)):
            if pool.size:
                pick = rng.choice(pool, size=min(pool.size, 6), replace=False)
                flat[pick[0::3]] = np.nan
                flat[pick[1::3]] = np.inf
                flat[pick[2::3]] = -np.inf
    elif regime != "signed":
        raise ValueError(regime)
    return g


def _assert_regime(gpu, ref, bound, what):
    """gpu: the kernel's fp32 result; ref: float64 reference; bound: per-entry float64 bound (or a scalar)."""
    gpu = np.asarray(gpu, np.float64)
    ref = np.asarray(ref, np.float64)
    with np.errstate(over="ignore"):
        ref32 = ref.astype(np.float32).astype(np.float64)   # what an fp32 result can be: beyond FLT_MAX is inf
    fin = np.isfinite(ref32)
    bad = np.flatnonzero(np.isfinite(gpu).reshape(-1) != fin.reshape(-1))
    assert bad.size == 0, (what, "finite mask", bad[:8], gpu.reshape(-1)[bad[:8]], ref.reshape(-1)[bad[:8]])
    inf = np.isinf(ref32)
    ok = (gpu[inf] == ref32[inf]) | np.isnan(gpu[inf])
    assert ok.all(), (what, "infinity of the wrong sign", gpu[inf][~ok][:8], ref32[inf][~ok][:8])
    bound = np.broadcast_to(np.asarray(bound, np.float64), ref.shape)
    with np.errstate(invalid="ignore"):   # inf - inf where both are infinite: checked above
        err = np.abs(gpu - ref)
    over = np.flatnonzero((fin & ~(err <= bound)).reshape(-1))
    assert over.size == 0, (what, over.size, "entries over the bound", over[:8], gpu.reshape(-1)[over[:8]],
                            ref.reshape(-1)[over[:8]], bound.reshape(-1)[over[:8]])


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ----------------------------------------------------------------------------------------------- p2i max
def _p2i_terms(og, ids, points, feat, radius):
    """The three terms every winning pixel sends to its winner (oracle/p2i.c, oracle_p2i_max_backward_exact), in
    float64: returns per feature entry and per point coordinate (sum of the terms, sum of |terms|, number of
    terms, the envelope of the kernel's fp32 series: 1.5e-6 * sum |g| (weight, kWeightErr in p2i.hip) and
    1e-6 * sum |g f| pi^2 / (2 R^2) |d| (slope))."""
    B, C, H, W = og.shape
    n = points.shape[0]
    b, c, y, x = np.nonzero(ids >= 0)
    pid = ids[b, c, y, x].astype(np.int64)
    g = og[b, c, y, x].astype(np.float64)
    f = feat[pid, c].astype(np.float64)
    dy = y - points[pid, 0].astype(np.float64)
    dx = x - points[pid, 1].astype(np.float64)
    r = np.sqrt(dx * dx + dy * dy)
    with np.errstate(invalid="ignore", over="ignore"):
        tf = g * (np.cos(r * math.pi / radius) + 1) / 2
        k = g * f * np.sin(r * math.pi / radius) * 0.5 * math.pi / radius / np.maximum(r, 1e-10)
        env = np.abs(g) * np.abs(f) * (math.pi ** 2 / (2 * radius * radius))
    out = {}
    for key, idx, size, terms, envs in (("feat", pid * C + c, n * C, [tf], [1.5e-6 * np.abs(g)]),
                                        ("pts", np.concatenate([pid * 2, pid * 2 + 1]), n * 2,
                                         [np.concatenate([k * dy, k * dx])],
                                         [1e-6 * np.concatenate([env * np.abs(dy), env * np.abs(dx)])])):
        t = terms[0]
        s, a, cnt, e = (np.zeros(size) for _ in range(4))
        with np.errstate(invalid="ignore"):
            np.add.at(s, idx, t)
            np.add.at(a, idx, np.abs(t))
            np.add.at(e, idx, envs[0])
        np.add.at(cnt, idx, 1.0)
        out[key] = (s, a, cnt, e)
    return out


def _p2i_max_check(og_r, ids_r, points, feat, radii, gp, gf, what, fixed_point=True):
    """og_r / ids_r: [R, B, C, H, W]; gp / gf: the GPU's points / feature gradients (summed over the radii)."""
    n, C = feat.shape
    ref_p = np.zeros(n * 2)
    ref_f = np.zeros(n * C)
    acc = {"pts": [0, 0, 0, 0], "feat": [0, 0, 0, 0]}
    for r, R in enumerate(radii):
        ep, ef = oracle.p2i_max_backward_exact(og_r[r], ids_r[r], points, feat, R)
        ref_p += ep.reshape(-1).astype(np.float64)
        ref_f += ef.reshape(-1).astype(np.float64)
        for key, v in _p2i_terms(og_r[r], ids_r[r], points, feat, R).items():
            acc[key] = [a + b for a, b in zip(acc[key], v)]
    with np.errstate(invalid="ignore"):
        gmax = float(np.abs(og_r[np.isfinite(og_r)]).max(initial=0.0))
        fmax = float(np.abs(feat[np.isfinite(feat)]).max(initial=0.0))
    m = gmax * max(1.0, fmax * math.pi / (2 * min(radii)) * 1.01)
    for key, gpu, ref in (("pts", gp, ref_p), ("feat", gf, ref_f)):
        _, sabs, cnt, series = acc[key]
        if fixed_point:
            # Per entry p (a feature entry or a point coordinate), with n_p terms t_p of magnitude sum S_p:
            #   |gpu - ref| <= 4 2^-24 S_p + series_p + (n_p + 1) 2^-43 m
            # 4 2^-24 S_p: the last bits of each fp32 term and the one rounding of the result; series_p: the kernel's
            # weight / slope series are within 1.5e-6 / 1e-6 of cos / sin; (n_p + 1) 2^-43 m: the fixed-point step is
            # 2^(ilogb(m) - 43) <= 2^-43 m with m = max|og| * max(1, max|feat| * pi / (2 r_min) * 1.01) over the
            # finite values, the kernel's bound on a term, and every term rounds to the step once.
            bound = 4 * EPS * sabs + series + (cnt + 1) * 2.0 ** -43 * m
        else:
            # fp32 sums in some order: (n_p + 4) 2^-24 S_p + series_p
            bound = (cnt + 4) * EPS * sabs + series
        _assert_regime(gpu.reshape(-1), ref, bound, (what, key))


def _cloud2d(rng, B, n, S, C, regime):
    pts = ((rng.random((B * n, 2)) * 1.2 - 0.1) * (S - 1)).astype(np.float32)
    feat = (rng.random((B * n, C)) * 0.9 + 0.1).astype(np.float32)
    if regime == "nonfinite":   # non-finite features, too (a diverged step): NaN, +inf, -inf on a few points
        rows = rng.choice(B * n, size=6, replace=False)
        feat[rows[0::3], 0] = np.nan
        feat[rows[1::3], -1] = np.inf
        feat[rows[2::3], 0] = -np.inf
    bi = np.repeat(np.arange(B, dtype=np.int32), n)
    return pts, feat, bi


_P2I_CONFIGS = {   # (C, radii, image_major, entry point)
    "single-C1": (1, [5.0], False, "single"),
    "R2-C3-im": (3, [3.0, 6.0], True, "multi"),
    "R3-C1-im": (1, [5.0, 7.0, 10.0], True, "multi"),
    "R4-C3": (3, [2.0, 4.0, 6.0, 8.0], False, "multi"),
}


def _run_p2i_max(pts, feat, bi, B, S, C, radii, image_major, entry, regime, seed, dev, bg_grad=True):
    from sparenet_amd.cuda.p2i_op import P2IMaxFunction, P2IMaxMultiFunction

    p = _t(pts, dev).requires_grad_(True)
    f = _t(feat, dev).requires_grad_(True)
    bg = torch.zeros(B, C, S, S, device=dev).requires_grad_(bg_grad)
    if entry == "single":
        out = P2IMaxFunction.apply(p, f, _t(bi, dev), bg, 0, radii[0])
        ids = out.grad_fn.saved_tensors[2].cpu().numpy()[None]          # [1, B, C, S, S]
    else:
        out = P2IMaxMultiFunction.apply(p, f, _t(bi, dev), bg, 0, radii, image_major)
        ids = out.grad_fn.saved_tensors[2].cpu().numpy()
        if image_major:
            ids = ids.transpose(1, 0, 2, 3, 4)
    ids = np.ascontiguousarray(ids)
    og = _upstream((len(radii), B, C, S, S), regime, seed, owned=ids >= 0, image_axis=1)
    og_dev = og[0] if entry == "single" else (og.transpose(1, 0, 2, 3, 4) if image_major else og)
    torch.autograd.backward(out, _t(og_dev, dev))
    return p.grad.cpu().numpy(), f.grad.cpu().numpy(), bg.grad.cpu().numpy() if bg_grad else None, og, ids


@pytest.mark.gpu
@pytest.mark.parametrize("config", list(_P2I_CONFIGS))
@pytest.mark.parametrize("regime", REGIMES)
def test_p2i_max_backward_regimes(regime, config, dev):
    """P2IMaxFunction / P2IMaxMultiFunction autograd (sn_p2i_max_backward_multi: fixed-point accumulation) against
    the oracle's exact sum of the fp32 terms, the background gradient against its float64 sum, a second backward
    bit-equal to the first, and the single-radius sn_p2i_max_backward (fp32 gather) under the same upstream."""
    from sparenet_amd.cuda.p2i_op import ext

    C, radii, image_major, entry = _P2I_CONFIGS[config]
    B, n, S = 2, 1500, 64
    seed = 1000 * _SEEDS[regime] + list(_P2I_CONFIGS).index(config)
    pts, feat, bi = _cloud2d(np.random.default_rng(seed), B, n, S, C, regime)
    gp, gf, gb, og, ids = _run_p2i_max(pts, feat, bi, B, S, C, radii, image_major, entry, regime, seed, dev)
    _p2i_max_check(og, ids, pts, feat, radii, gp, gf, (regime, config))
    with np.errstate(invalid="ignore"):
        ref_bg = np.where(ids < 0, og.astype(np.float64), 0.0).sum(0)
        bg_bound = len(radii) * EPS * np.where(ids < 0, np.abs(og.astype(np.float64)), 0.0).sum(0)
    _assert_regime(gb, ref_bg, bg_bound, (regime, config, "background"))
    again = _run_p2i_max(pts, feat, bi, B, S, C, radii, image_major, entry, regime, seed, dev)
    for a, b in zip((gp, gf, gb), again[:3]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "two backward calls differ"
    # the single-radius gather path (sn_p2i_max_backward) under the same upstream gradient, radius by radius
    r = len(radii) - 1
    sp, sf, sb = ext.p2i_max_backward_gpu(_t(og[r], dev), _t(ids[r], dev), _t(pts, dev), _t(feat, dev), 0, radii[r])
    _p2i_max_check(og[r:r + 1], ids[r:r + 1], pts, feat, radii[r:r + 1], sp.cpu().numpy(), sf.cpu().numpy(),
                   (regime, config, "single-radius gather"), fixed_point=False)
    assert np.array_equal(sb.cpu().numpy(), np.where(ids[r] < 0, og[r], np.float32(0)), equal_nan=True)


@pytest.mark.gpu
def test_p2i_max_backward_wide_at_bench_size(dev):
    """The renderer's shape: S = 256, B = 8, radii 5 / 7 / 10, `wide` upstream gradients, image-major."""
    B, n, S, C, radii = 8, 16384, 256, 1, [5.0, 7.0, 10.0]
    pts, feat, bi = _cloud2d(np.random.default_rng(77), B, n, S, C, "wide")
    gp, gf, _, og, ids = _run_p2i_max(pts, feat, bi, B, S, C, radii, True, "multi", "wide", 78, dev, bg_grad=False)
    _p2i_max_check(og, ids, pts, feat, radii, gp, gf, "bench size")


@pytest.mark.gpu
def test_p2i_max_backward_zero_upstream_and_large_finite(dev):
    """An upstream gradient that is zero everywhere (no scale can be derived from it) gives exact zeros; finite
    values so large that max|og| * max(1, max|feat| * pi / (2 r_min) * 1.01) reaches 3e38 or leaves fp32 -- a point
    off the image with a feature of 1e37; gradients of 1e30 at a few winning pixels and 3.2e38 at one -- stay
    within the bound of the fixed-point accumulation."""
    from sparenet_amd.cuda.p2i_op import P2IMaxMultiFunction

    B, n, S, C, radii = 2, 1500, 64, 1, [5.0, 7.0]
    pts, feat, bi = _cloud2d(np.random.default_rng(5), B, n, S, C, "signed")
    p = _t(pts, dev).requires_grad_(True)
    f = _t(feat, dev).requires_grad_(True)
    out = P2IMaxMultiFunction.apply(p, f, _t(bi, dev), torch.zeros(B, C, S, S, device=dev), 0, radii)
    out.backward(torch.zeros_like(out))
    assert not p.grad.any() and not f.grad.any()
    for seed, kind in ((7, "feature"), (8, "gradient")):
        pk, fk = pts.copy(), feat.copy()
        if kind == "feature":            # m overflows fp32 through max|feat|: a point off the image, feature 1e37
            pk[0] = [-500.0, -500.0]
            fk[0, 0] = 1e37
        p = _t(pk, dev).requires_grad_(True)
        f = _t(fk, dev).requires_grad_(True)
        out = P2IMaxMultiFunction.apply(p, f, _t(bi, dev), torch.zeros(B, C, S, S, device=dev), 0, radii)
        ids = out.grad_fn.saved_tensors[2].cpu().numpy()
        og = _upstream(tuple(out.shape), "signed", seed)
        if kind == "gradient":           # max|og| = 3.2e38 and terms of 1e30 at some winners
            won = np.flatnonzero(ids.reshape(-1) >= 0)
            og.reshape(-1)[won[::997]] = 1e30
            og.reshape(-1)[won[1]] = 3.2e38
        out.backward(_t(og, dev))
        _p2i_max_check(og, ids, pk, fk, radii, p.grad.cpu().numpy(), f.grad.cpu().numpy(), ("large", kind))


@functools.lru_cache(None)
def _crowded_oracle(S, C, R):
    import p2i_cases as pc

    case = pc.crowded(S, C)
    out, ids = oracle.p2i_max_forward(case.pts, case.feat, case.bi, case.bg, R)
    out.setflags(write=False)
    ids.setflags(write=False)
    return out, ids


@pytest.mark.gpu
@pytest.mark.parametrize("regime", ["wide", "signed"])
@pytest.mark.parametrize("image_major", [False, True], ids=["radius-major", "image-major"])
@pytest.mark.parametrize("radii", [[0.7, 1.0], [1.0, 2.0]], ids=["R0.7-1", "R1-2"])
@pytest.mark.parametrize("S,C", [(64, 1), (64, 3), (40, 1), (40, 3), (43, 3)])
def test_p2i_max_backward_crowded_regions(S, C, radii, image_major, regime, dev):
    """One point per pixel (tests/p2i_cases.crowded): a full 32 x 32 region holds about 1020 distinct winners, twice the
    512 slots of the hash table of p2i_max_bwd_accum_kernel, so most terms leave through its direct-to-global branch
    (test_p2i_edges.test_crowded_regions_overflow_the_hash_table asserts that on the oracle's ids).  S = 40: partial
    regions; S = 43: partial 8 x 8 tiles as well.  The bounds are those of test_p2i_max_backward_regimes; the forward that produced
    the ids is held to the oracle as well."""
    import p2i_cases as pc
    from sparenet_amd.cuda.p2i_op import ext
    from test_p2i import _close_maps

    case = pc.crowded(S, C)
    B = pc.CROWDED_BATCH
    pts, feat, bi = (np.array(a) for a in case[:3])
    seed = 9000 + 100 * S + 10 * C + _SEEDS[regime]
    gp, gf, gb, og, ids = _run_p2i_max(pts, feat, bi, B, S, C, radii, image_major, "multi", regime, seed, dev)
    _p2i_max_check(og, ids, pts, feat, radii, gp, gf, (regime, S, C, radii, image_major))
    ref_bg = np.where(ids < 0, og.astype(np.float64), 0.0).sum(0)
    bg_bound = len(radii) * EPS * np.where(ids < 0, np.abs(og.astype(np.float64)), 0.0).sum(0)
    _assert_regime(gb, ref_bg, bg_bound, (regime, S, C, radii, "background"))
    again = _run_p2i_max(pts, feat, bi, B, S, C, radii, image_major, "multi", regime, seed, dev)
    for a, b in zip((gp, gf, gb), again[:3]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "two backward calls differ"
    out, fids = ext.p2i_max_forward_multi_gpu(_t(pts, dev), _t(feat, dev), _t(bi, dev), _t(np.array(case.bg), dev), 0, radii,
                                              image_major=image_major)
    if image_major:
        out, fids = out.transpose(0, 1), fids.transpose(0, 1)
    assert np.array_equal(fids.cpu().numpy(), ids)
    for r, R in enumerate(radii):
        o, i = _crowded_oracle(S, C, R)
        _close_maps(out[r].cpu().numpy(), ids[r], o, i, f"crowded S={S} C={C} R={R}", pts, feat, case.bg, R)


# ----------------------------------------------------------------------------------------------- p2i sum
@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("regime", REGIMES)
def test_p2i_sum_backward_regimes(regime, C, dev):
    """P2ISumFunction against the float64 sum of the reference functor's terms (p2i_sum.h; every pixel of a point's
    footprint), within (n_p + 4) 2^-24 sum|t_p| + 5e-7 of the terms' magnitude."""
    from sparenet_amd.cuda.p2i_op import P2ISumFunction

    B, n, S, R = 2, 800, 48, 3.0
    seed = 2000 + 10 * _SEEDS[regime] + C
    rng = np.random.default_rng(seed)
    pts, feat, bi = _cloud2d(rng, B, n, S, C, regime)
    bi[::97] = -1                                           # skipped points: zero gradient
    p = _t(pts, dev).requires_grad_(True)
    f = _t(feat, dev).requires_grad_(True)
    out = P2ISumFunction.apply(p, f, _t(bi, dev), torch.zeros(B, C, S, S, device=dev), 0, R)
    # the footprints: every in-image pixel within R of a live point
    ry, rx = np.meshgrid(np.arange(-4, 5), np.arange(-4, 5), indexing="ij")
    cy = np.floor(pts[:, 0:1]).astype(np.int64) + ry.reshape(1, -1)
    cx = np.floor(pts[:, 1:2]).astype(np.int64) + rx.reshape(1, -1)
    dy = (cy - pts[:, 0:1].astype(np.float64))
    dx = (cx - pts[:, 1:2].astype(np.float64))
    rr = np.sqrt((cy - pts[:, 0:1]).astype(np.float32) ** 2 + (cx - pts[:, 1:2]).astype(np.float32) ** 2)
    live = (bi[:, None] >= 0) & (cy >= 0) & (cy < S) & (cx >= 0) & (cx < S) & (rr <= R)
    covered = np.zeros((B, C, S, S), bool)
    pi_, ki = np.nonzero(live)
    for c in range(C):
        covered[bi[pi_], c, cy[pi_, ki], cx[pi_, ki]] = True
    og = _upstream((B, C, S, S), regime, seed, owned=covered, image_axis=0)
    out.backward(_t(og, dev))
    r = np.sqrt(dx * dx + dy * dy)[pi_, ki]
    ref_p, ref_f = np.zeros(n * B * 2), np.zeros(n * B * C)
    abs_p, abs_f, cnt_p, cnt_f, env_p, env_f = (np.zeros_like(a) for a in (ref_p, ref_f, ref_p, ref_f, ref_p, ref_f))
    for c in range(C):
        gv = og[bi[pi_], c, cy[pi_, ki], cx[pi_, ki]].astype(np.float64)
        fv = feat[pi_, c].astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            tf = gv * (np.cos(r * math.pi / R) + 1) / 2
            k = gv * fv * np.sin(r * math.pi / R) * 0.5 * math.pi / R / np.maximum(r, 1e-10)
            ty, tx = k * dy[pi_, ki], k * dx[pi_, ki]
            np.add.at(ref_f, pi_ * C + c, tf)
            np.add.at(abs_f, pi_ * C + c, np.abs(tf))
            np.add.at(env_f, pi_ * C + c, 5e-7 * np.abs(gv))
            for a, t, d in ((0, ty, dy), (1, tx, dx)):
                np.add.at(ref_p, pi_ * 2 + a, t)
                np.add.at(abs_p, pi_ * 2 + a, np.abs(t))
                np.add.at(env_p, pi_ * 2 + a, 5e-7 * np.abs(gv * fv) * math.pi ** 2 / (2 * R * R) * np.abs(d[pi_, ki]))
        np.add.at(cnt_f, pi_ * C + c, 1.0)
        np.add.at(cnt_p, pi_ * 2, 1.0)
        np.add.at(cnt_p, pi_ * 2 + 1, 1.0)
    # fp32 sums of (n_p) terms in some order, each term within a few ulps and the 5e-7 series of its fp64 value:
    _assert_regime(f.grad.cpu().numpy().reshape(-1), ref_f, (cnt_f + 4) * EPS * abs_f + env_f, (regime, C, "feat"))
    _assert_regime(p.grad.cpu().numpy().reshape(-1), ref_p, (cnt_p + 4) * EPS * abs_p + env_p, (regime, C, "pts"))


# ----------------------------------------------------------------------------------------------- point clouds
@pytest.mark.gpu
@pytest.mark.parametrize("n,m", [(1000, 700), (2048, 4096)])    # n m below / above SORTED_MIN_PAIRS (2^22)
@pytest.mark.parametrize("regime", REGIMES)
def test_chamfer_backward_regimes(regime, n, m, dev):
    """ChamferDistanceFunction backward, both gradients bit-equal to oracle.chamfer_backward (NaN where NaN)."""
    from sparenet_amd.cuda.chamfer_distance import ChamferDistanceFunction
    from sparenet_amd.cuda.chamfer_distance.chamfer_distance import _CdBinding

    assert (n * m >= _CdBinding.SORTED_MIN_PAIRS) == (n == 2048)
    b = 2
    rng = np.random.default_rng(3000 + n + _SEEDS[regime])
    x = rng.random((b, n, 3), dtype=np.float32)
    y = rng.random((b, m, 3), dtype=np.float32)
    _, _, i1, i2 = oracle.chamfer_forward(x, y, mt=True)
    gd1 = _upstream((b, n), regime, 1 + n, image_axis=0)
    gd2 = _upstream((b, m), regime, 2 + n, image_axis=0)
    xt, yt = _t(x, dev).requires_grad_(True), _t(y, dev).requires_grad_(True)
    d1, d2 = ChamferDistanceFunction.apply(xt, yt)
    torch.autograd.backward([d1, d2], [_t(gd1, dev), _t(gd2, dev)])
    r1, r2 = oracle.chamfer_backward(x, y, gd1, gd2, i1, i2)
    assert np.array_equal(xt.grad.cpu().numpy(), r1, equal_nan=True)
    assert np.array_equal(yt.grad.cpu().numpy(), r2, equal_nan=True)


@pytest.mark.gpu
@pytest.mark.parametrize("regime", REGIMES)
def test_emd_and_expansion_backward_regimes(regime, dev):
    """emdModule and expansionPenaltyModule backward, bit-equal to oracle.emd_backward / expansion_backward built
    from the forward's own assignment (NaN where NaN)."""
    from sparenet_amd.cuda.emd.emd_module import emdModule
    from sparenet_amd.cuda.expansion_penalty.expansion_penalty_module import expansionPenaltyModule

    b, n = 2, 1024
    rng = np.random.default_rng(4000 + _SEEDS[regime])
    x = rng.random((b, n, 3), dtype=np.float32)
    y = rng.random((b, n, 3), dtype=np.float32)
    xt = _t(x, dev).requires_grad_(True)
    dist, assign = emdModule()(xt, _t(y, dev), 0.005, 10)
    a = assign.cpu().numpy()
    gd = _upstream((b, n), regime, 11, owned=a >= 0, image_axis=0)
    dist.backward(_t(gd, dev))
    assert np.array_equal(xt.grad.cpu().numpy(), oracle.emd_backward(x, y, gd, a), equal_nan=True)
    xt = _t(x, dev).requires_grad_(True)
    pen, asg, _ = expansionPenaltyModule()(xt, 64, 1.5)
    a = asg.cpu().numpy()
    gd = _upstream((b, n), regime, 12, owned=a >= 0, image_axis=0)
    pen.backward(_t(gd, dev))
    assert np.array_equal(xt.grad.cpu().numpy(), oracle.expansion_backward(x, gd, a), equal_nan=True)


@pytest.mark.gpu
@pytest.mark.parametrize("regime", REGIMES)
def test_gather_backward_regimes(regime, dev):
    """gather_operation backward (duplicated indices: several terms per entry) against the float64 sum,
    within (n_e + 1) 2^-24 sum|t_e|."""
    from sparenet_amd.cuda.MDS.MDS_module import gather_operation

    b, c, n, m = 3, 4, 1000, 2500
    rng = np.random.default_rng(5000 + _SEEDS[regime])
    f = rng.random((b, c, n), dtype=np.float32)
    idx = rng.integers(0, n - 100, (b, m)).astype(np.int32)    # the last 100 entries are never gathered
    ft = _t(f, dev).requires_grad_(True)
    out = gather_operation(ft, _t(idx, dev))
    go = _upstream((b, c, m), regime, 13, image_axis=0)
    out.backward(_t(go, dev))
    ref, sabs, cnt = np.zeros((b, c, n)), np.zeros((b, c, n)), np.zeros((b, c, n))
    bb, cc, jj = np.meshgrid(np.arange(b), np.arange(c), np.arange(m), indexing="ij")
    tgt = (bb, cc, idx[bb, jj])
    with np.errstate(invalid="ignore"):
        np.add.at(ref, tgt, go.astype(np.float64))
        np.add.at(sabs, tgt, np.abs(go.astype(np.float64)))
    np.add.at(cnt, tgt, 1.0)
    _assert_regime(ft.grad.cpu().numpy(), ref, (cnt + 1) * EPS * sabs, regime)


# ----------------------------------------------------------------------------------------------- gridding
@pytest.mark.gpu
@pytest.mark.parametrize("regime", REGIMES)
def test_gridding_backward_regimes(regime, dev):
    """GriddingFunction backward against the float64 sum of its eight corner terms (oracle_gridding_backward's
    weights and indexes), within 16 2^-24 sum|t|."""
    from sparenet_amd.cuda.gridding import GriddingFunction

    scale, b, n = 16, 2, 3000
    rng = np.random.default_rng(6000 + _SEEDS[regime])
    pc = ((rng.random((b, n, 3)) * 1.8 - 0.9) * (scale // 2)).astype(np.float32)
    _, w, ix = oracle.gridding_forward(pc, scale)
    pt = _t(pc, dev).requires_grad_(True)
    grid = GriddingFunction.apply(scale // 2, pt)
    owned = np.zeros((b, scale ** 3), bool)
    for i in range(b):
        owned[i, ix[i][(ix[i] >= 0) & (ix[i] < scale ** 3)]] = True
    gg = _upstream((b, scale ** 3), regime, 14, owned=owned, image_axis=0)
    grid.backward(_t(gg, dev))
    valid = (ix >= 0) & (ix < scale ** 3)
    g = np.where(valid, np.take_along_axis(gg, np.where(valid, ix, 0).reshape(b, -1), 1).reshape(ix.shape), 0.0)
    g = g.astype(np.float64)
    w = w.astype(np.float64)
    c = np.arange(8)
    sgn = np.stack([np.where(c & 4, 1.0, -1.0), np.where(c & 2, 1.0, -1.0), np.where(c & 1, 1.0, -1.0)], 1)
    with np.errstate(invalid="ignore"):
        terms = np.stack([sgn[:, 0] * g * w[..., 1] * w[..., 2], sgn[:, 1] * g * w[..., 0] * w[..., 2],
                          sgn[:, 2] * g * w[..., 0] * w[..., 1]], -1)    # [b, n, 8, 3]
        ref, sabs = terms.sum(2), np.abs(terms).sum(2)
    _assert_regime(pt.grad.cpu().numpy(), ref, 16 * EPS * sabs, regime)


@pytest.mark.gpu
@pytest.mark.parametrize("regime", REGIMES)
def test_gridding_reverse_backward_regimes(regime, dev):
    """GriddingReverseFunction backward against a float64 restatement of oracle_gridding_reverse_backward (each
    vertex with x, y, z >= 1 and a weight sum >= 1e-6 sends gp . (corner - p) / wsum to its eight cells), within
    (n_e + 8) 2^-24 sum|t_e|; rows of vertices that produce no point carry the not-owned non-finite values."""
    from sparenet_amd.cuda.gridding import GriddingReverseFunction

    scale, b = 12, 2
    rng = np.random.default_rng(7000 + _SEEDS[regime])
    grid = (rng.random((b, scale, scale, scale)) + 0.05).astype(np.float32)
    grid[1, 5:8, 5:8, 5:8] = 0.0                                     # vertices whose weight sum is below 1e-6
    gr = _t(grid, dev).requires_grad_(True)
    pc = GriddingReverseFunction.apply(scale, gr)
    pcn = pc.detach().cpu().numpy()
    j = np.arange(scale ** 3)
    x, y, z = j // scale ** 2, j % scale ** 2 // scale, j % scale
    inner = (x > 0) & (y > 0) & (z > 0)
    corners = np.stack([((x - 1 + (cc >> 2 & 1)) * scale + (y - 1 + (cc >> 1 & 1))) * scale + (z - 1 + (cc & 1))
                        for cc in range(8)], 1)                       # the order of rev_setup
    corners = np.where(inner[:, None], corners, 0)
    gflat = grid.reshape(b, -1)
    wsum = np.zeros((b, scale ** 3), np.float32)
    for cc in range(8):                                               # fp32, in order: the kernel's decision
        wsum = (wsum + gflat[:, corners[:, cc]]).astype(np.float32)
    live = inner[None] & ~(wsum < 1e-6)
    owned = np.broadcast_to(live[..., None], (b, scale ** 3, 3))
    gp = _upstream((b, scale ** 3, 3), regime, 15, owned=owned, image_axis=0)
    pc.backward(_t(gp, dev))
    ref, sabs, cnt = np.zeros((b, scale ** 3)), np.zeros((b, scale ** 3)), np.zeros((b, scale ** 3))
    off = np.stack([x, y, z], 1) - scale // 2
    for i in range(b):
        jl = np.flatnonzero(live[i])
        for cc in range(8):
            hi = np.array([cc >> 2 & 1, cc >> 1 & 1, cc & 1])
            corner = (off[jl] - 1 + hi).astype(np.float64) - pcn[i, jl].astype(np.float64)
            with np.errstate(invalid="ignore"):
                comp = gp[i, jl].astype(np.float64) * corner / wsum[i, jl, None].astype(np.float64)
                np.add.at(ref[i], corners[jl, cc], comp.sum(1))
                np.add.at(sabs[i], corners[jl, cc], np.abs(comp).sum(1))
            np.add.at(cnt[i], corners[jl, cc], 1.0)
    _assert_regime(gr.grad.cpu().numpy().reshape(b, -1), ref, (cnt + 8) * EPS * sabs, regime)


@pytest.mark.gpu
@pytest.mark.parametrize("ns", [1, 2, 3])
@pytest.mark.parametrize("regime", REGIMES)
def test_cubic_feature_sampling_backward_regimes(regime, ns, dev):
    """CubicFeatureSamplingFunction backward against the float64 scatter of grad_out over the forward's own
    neighbour indices (oracle_cubic_backward), within (n_e + 1) 2^-24 sum|t_e|."""
    from sparenet_amd.cuda.cubic_feature_sampling import CubicFeatureSamplingFunction

    b, n, c, s = 2, 600, 3, 8
    rng = np.random.default_rng(8000 + 10 * _SEEDS[regime] + ns)
    pc = (rng.random((b, n, 3)) * (s + 2) - 1).astype(np.float32)   # some neighbourhoods leave the grid (-1)
    feat = rng.random((b, c, s, s, s), dtype=np.float32)
    ft = _t(feat, dev).requires_grad_(True)
    out = CubicFeatureSamplingFunction.apply(_t(pc, dev), ft, ns)
    _, idx = oracle.cubic_forward(pc, feat, ns)
    go = _upstream(tuple(out.shape), regime, 16, owned=np.broadcast_to((idx >= 0)[..., None], out.shape),
                   image_axis=0)
    out.backward(_t(go, dev))
    ref, sabs, cnt = (np.zeros((b, c, s ** 3)) for _ in range(3))
    for i in range(b):
        pp, vv = np.nonzero(idx[i] >= 0)
        for k in range(c):
            t = go[i, pp, vv, k].astype(np.float64)
            with np.errstate(invalid="ignore"):
                np.add.at(ref[i, k], idx[i, pp, vv], t)
                np.add.at(sabs[i, k], idx[i, pp, vv], np.abs(t))
            np.add.at(cnt[i, k], idx[i, pp, vv], 1.0)
    _assert_regime(ft.grad.cpu().numpy().reshape(b, c, -1), ref, (cnt + 1) * EPS * sabs, regime)


# ----------------------------------------------------------------------------------------------- depth projection
@pytest.mark.gpu
@pytest.mark.parametrize("views", [[3], [0, 2, 5, 7]])
@pytest.mark.parametrize("regime", REGIMES)
def test_depth_project_backward_regimes(regime, views, dev):
    """DepthProjectFunction (one view) and DepthProjectViewsFunction (forward_views' projection) against torch
    float64 autograd of the expressions of depth_project.hip:1-11 (ComputeDepthMaps.project and the NDC -> pixel
    rescale; torch's full-reduction min / max share the gradient evenly between the points that attain them).
    Bound per entry: 16 2^-24 D + (n + 16) 2^-24 E, D the magnitude of the point's own chain (the four gradients
    times |d pixel / d data| and |d feat / d data|), E that of the zmin / zmax paths at the points that attain
    them (sum |g_feat| |d feat / d z| |d z / d data| over all n points of the view)."""
    from sparenet_amd.utils.p2i_utils import ComputeDepthMaps, DepthProjectFunction, DepthProjectViewsFunction

    B, N, S = 2, 700, 64
    cdm = ComputeDepthMaps("orthorgonal", 1.0, S).to(dev)
    g = torch.Generator().manual_seed(90 + _SEEDS[regime])
    base = torch.rand(B, N, 3, generator=g) - 0.5
    base[1, 7] = base[0, 3]                        # a duplicated point: ties at whatever extreme it reaches
    n = B * N
    gpix = _upstream((len(views), n, 2), regime, 91 + len(views))
    gfeat = _upstream((len(views), n, 1), regime, 92 + len(views))
    d = base.clone().to(dev).requires_grad_(True)
    if len(views) == 1:
        pix, feat = DepthProjectFunction.apply(d, cdm._host_mats[views[0]], S)
    else:
        pix, feat = DepthProjectViewsFunction.apply(d, [cdm._host_mats[v] for v in views], S)
    torch.autograd.backward([pix, feat], [_t(gpix.reshape(-1, 2), dev), _t(gfeat.reshape(-1, 1), dev)])
    d64 = base.clone().double().requires_grad_(True)
    ref_out, ref_in = [], []
    D = np.zeros((n, 3))
    E = np.zeros((n, 3))
    for k, v in enumerate(views):
        pos, f64 = cdm.project(d64, v)
        ref_out += [(pos + 1) / 2 * (S - 1), f64]
        ref_in += [torch.from_numpy(gpix[k].astype(np.float64)), torch.from_numpy(gfeat[k].astype(np.float64))]
        M = np.array(cdm._host_mats[v], np.float64).reshape(4, 4)
        assert np.array_equal(M[3], [0, 0, 0, 1])   # orthographic: w = 1, the chain is linear in the matrix
        zz = (base.double().reshape(-1, 3).numpy() @ M[2, :3]) + M[2, 3]
        span = zz.max() - zz.min()
        with np.errstate(invalid="ignore", over="ignore"):
            D += ((S - 1) / 2 * (np.abs(gpix[k, :, 0:1]) * np.abs(M[1, :3]) + np.abs(gpix[k, :, 1:2]) * np.abs(M[0, :3]))
                  + np.abs(gfeat[k]) * np.abs(M[2, :3]) / span)
            ext = (zz <= zz.min() + 1e-6 * span) | (zz >= zz.max() - 1e-6 * span)
            E += np.where(ext[:, None], np.nansum(np.abs(gfeat[k])) / span * np.abs(M[2, :3]) * 2, 0.0)
    torch.autograd.backward(ref_out, ref_in)
    ref = d64.grad.numpy().reshape(n, 3)
    _assert_regime(d.grad.cpu().numpy().reshape(n, 3), ref, 16 * EPS * D + (n + 16) * EPS * E, (regime, views))
