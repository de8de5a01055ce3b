"""Input generators of the p2i edge tests (TEST INFRASTRUCTURE): tests/test_p2i_edges.py and the crowded cases of
tests/test_backward_regimes.py run the HIP kernels on these inputs, and the CPU tests of test_p2i_edges.py run the
oracle on exactly the same ones and assert the condition that makes each GPU comparison discriminating (pixels won on
the rim of the kernel, exact value ties between distinct points, winners two cells away, more winners per region than
the backward's hash table has slots).  NumPy only, deterministic; nothing here needs a GPU.

A case is a `Case(pts [n, 2] fp32 (row, col) in pixels, feat [n, C] fp32, bi [n] int32, bg [B, C, S, S] fp32)`.  Point
ids are shuffled inside every image, so the order of the cell-sorted arrays is never the order of the ids, while image b
still owns one contiguous block of ids: with equal counts per image (isolated, crowded; every one-image case) the
forward takes the one-launch grouped binning that ComputeDepthMaps uses, with unequal counts (the two lattices: 64 and
100 points) the generic binning kernels."""
import collections
import functools

import numpy as np

Case = collections.namedtuple("Case", "pts feat bi bg")

BACKGROUND = -0.5          # below every rim value (f * 0 = +-0): a rim pixel must be owned by its point
R_TILE = (5.0, 10.0, 13.0)  # the tile gather (<= 16 px)
R_SPLAT = 20.0              # the global splat
RIM_SQUARES = (2, 5, 8)     # radii sqrt(k): pixels at squared distance exactly k


def sqrt_radii(k):
    """(float32(sqrt(k)), the fp32 below it, the fp32 above it).  For k = 2, 5, 8 sqrtf(k) == float32(sqrt(k)), so the
    pixels at squared distance exactly k are in range for the first and the third and out of range for the second."""
    r = np.float32(np.sqrt(np.float64(k)))
    return float(r), float(np.nextafter(r, np.float32(0))), float(np.nextafter(r, np.float32(np.inf)))


def sqrt_radii_f64(k):
    """The same three radii for the float64 entry point (distances and radius in double)."""
    r = np.sqrt(np.float64(k))
    return float(r), float(np.nextafter(r, 0.0)), float(np.nextafter(r, np.inf))


def _background(B, C, S, kind, seed):
    if kind == "flat":
        return np.full((B, C, S, S), BACKGROUND, np.float32)
    assert kind == "random"
    return np.random.default_rng(seed).uniform(-1.0, -0.1, (B, C, S, S)).astype(np.float32)


def _shuffled(pts, feat, bi, bg, seed):
    rng = np.random.default_rng(seed)
    perm = np.concatenate([rng.permutation(np.flatnonzero(bi == b)) for b in np.unique(bi)])   # inside each image
    out = Case(np.ascontiguousarray(pts[perm], np.float32), np.ascontiguousarray(feat[perm], np.float32),
               np.ascontiguousarray(bi[perm], np.int32), bg)
    for a in out:
        a.setflags(write=False)
    return out


def _signed_levels(n, C, seed):
    """features from {0.25, 0.5, 0.75}, the sign flipped on every third point.  (Not 1.0: -1.0 times the weight 1 / 2 at
    half the radius lies within an ulp of the background -0.5 on every pixel at r = R / 2.)"""
    rng = np.random.default_rng(seed)
    f = rng.choice(np.array([0.25, 0.5, 0.75], np.float32), size=(n, C))
    f[2::3] *= -1
    return f.astype(np.float32)


# ------------------------------------------------------------------------------------------------ A: rim and ties
ISOLATED_S = 96
# (row, col): pairwise farther apart than 2 * 20 + 2; six within 5 px of the border; (-5, 47) lies outside the image at
# exactly 5 px from pixel (0, 47), (46, 108) at exactly 13 px from pixel (46, 95)
_ISOLATED = np.array([(2, 3), (-5, 47), (4, 92), (46, 20), (46, 64), (90, 3), (90, 47), (93, 91), (46, 108)],
                     np.float32)


@functools.lru_cache(None)
def isolated(B=2, C=1, bg="flat"):
    """S = 96, integer points whose footprints never overlap up to R = 20; image 1 holds image 0 transposed."""
    pts = np.concatenate([_ISOLATED if b % 2 == 0 else _ISOLATED[:, ::-1] for b in range(B)])
    bi = np.repeat(np.arange(B, dtype=np.int32), len(_ISOLATED))
    rng = np.random.default_rng(11 + C)
    feat = (rng.uniform(0.25, 1.0, (len(pts), C)) * np.where(rng.random((len(pts), C)) < 0.3, -1, 1)).astype(np.float32)
    return _shuffled(pts, feat, bi, _background(B, C, ISOLATED_S, bg, 12), 13)


LATTICE_S = 48
LATTICE_STEPS = (6, 5)


@functools.lru_cache(None)
def lattice(B=2, C=1, bg="flat"):
    """S = 48; image 0: the integer lattice of step 6, image 1: of step 5 (B = 1: step 6 only)."""
    pts, bi = [], []
    for b in range(B):
        v = np.arange(0, LATTICE_S, LATTICE_STEPS[b], dtype=np.float32)
        yy, xx = np.meshgrid(v, v, indexing="ij")
        pts.append(np.stack([yy.ravel(), xx.ravel()], 1))
        bi.append(np.full(yy.size, b, np.int32))
    pts, bi = np.concatenate(pts), np.concatenate(bi)
    return _shuffled(pts, _signed_levels(len(pts), C, 21 + C), bi, _background(B, C, LATTICE_S, bg, 22), 23)


ZERO_PAIR_S = 48
ZERO_PAIR_RADII = (5.0, 10.0, R_SPLAT)      # the tile gather twice, the global splat


@functools.lru_cache(None)
def zero_pairs(R, bg="flat"):
    """Zeros of both signs on one pixel.  S = 48, four images, each with one pair of integer points exactly 2 R apart
    around the image centre (along a row in images 0 and 2, along a column in 1 and 3): the centre pixel lies on the
    rim of both and in the interior of neither, so its two candidates are f * 0 = -0 (negative feature) and +0.  Images
    0 and 1 give the LOWER id the negative feature -- the reference's `out < v` sees a tie and keeps the lower id,
    an order of bit patterns prefers the +0 of the higher id -- images 2 and 3 the higher one.  Not shuffled: the ids
    are the point.  bg "flat": -0.5; "negative_zero": -0.0 everywhere, which no +0 may replace (0 < 0 is false): every
    rim pixel stays unowned and keeps its sign bit."""
    S, c = ZERO_PAIR_S, ZERO_PAIR_S // 2
    pts, feat = [], []
    for b in range(4):
        a, z = ((c, c - R), (c, c + R)) if b % 2 == 0 else ((c - R, c), (c + R, c))
        pts += [a, z]
        feat += [-0.75, 0.5] if b < 2 else [0.5, -0.75]
    bi = np.repeat(np.arange(4, dtype=np.int32), 2)
    bgv = {"flat": BACKGROUND, "negative_zero": -0.0}[bg]
    out = Case(np.array(pts, np.float32), np.array(feat, np.float32).reshape(-1, 1), bi,
               np.full((4, 1, S, S), bgv, np.float32))
    for a in out:
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ D: borders
BORDER_SIZES = (17, 40, 43)   # 17, 43: partial 8 x 8 tiles; 40: whole tiles, a partial 32 x 32 region
BORDER_RADII = (1.0, 5.0)
BORDER_SEED = 33            # the first seed whose five cases hold no pixel decided inside WEIGHT_NOISE (31: 3, 32: 2)


@functools.lru_cache(None)
def borders(S, C=1):
    """Coordinates on cell borders (8k and the fp32 below), on the image border (-0.0, S - 1 and the fp32 above),
    exactly R outside a border and one ulp farther (R = 1, 5), as the full product rows x columns, and two points at
    +-9.9e8 (finite, binned, reaching nothing).  One image, background -0.5, features in +-[0.25, 1]."""
    f32 = np.float32
    below = lambda v: np.nextafter(f32(v), f32(-np.inf))
    above = lambda v: np.nextafter(f32(v), f32(np.inf))
    vals = [f32(-0.0), f32(S - 1), above(S - 1)]
    for k in range(8, S, 8):
        vals += [f32(k), np.nextafter(f32(k), f32(0))]
    for R in BORDER_RADII:
        vals += [f32(-R), below(-R), f32(S - 1 + R), above(S - 1 + R)]
    vals = np.array(list(dict.fromkeys(vals)), f32)           # S = 17: S - 1 is a cell border, too
    assert np.signbit(vals[0]) and len(np.unique(vals)) == len(vals)
    yy, xx = np.meshgrid(vals, vals, indexing="ij")
    pts = np.concatenate([np.stack([yy.ravel(), xx.ravel()], 1),
                          np.array([(9.9e8, 3.0), (3.0, -9.9e8)], f32)]).astype(f32)
    assert np.abs(pts).max() < 1e9
    bi = np.zeros(len(pts), np.int32)
    # continuous features: two points one ulp apart with EQUAL features would be a near-tie on every pixel they reach
    rng = np.random.default_rng(BORDER_SEED + S + C)
    feat = rng.uniform(0.25, 1.0, (len(pts), C)).astype(np.float32)
    feat[2::3] *= -1
    return _shuffled(pts, feat, bi, _background(1, C, S, "flat", 0), 33 + S)


# ------------------------------------------------------------------------------------------------ B: dim near, bright far
DIM_S = 64
DIM_RADII = (16.0, 12.0, 7.0)
DIM_SEED = 3


@functools.lru_cache(None)
def dim_near_bright_far(variant="base"):
    """1500 dim points (features in [0.001, 0.02]) and 12 bright ones ([0.8, 1.0]) over [-0.1, 1.1] * (S - 1): most
    pixels are won by a bright point several cells away.  `two_channel`: the bright values sit in channel 1 only
    (the call's largest |feature| then widens the band and the bounds of channel 0); `mirrored`: all features
    negated over a background of -1; `pairs`: the bright points placed where the size of the ring bound decides."""
    rng = np.random.default_rng(DIM_SEED)
    n_dim, n_bright, S = 1500, 12, DIM_S
    pts = (rng.uniform(-0.1, 1.1, (n_dim + n_bright, 2)) * (S - 1)).astype(np.float32)
    dim = rng.uniform(0.001, 0.02, (n_dim + n_bright, 1)).astype(np.float32)
    bright = rng.uniform(0.8, 1.0, (n_bright, 1)).astype(np.float32)
    feat = dim.copy()
    feat[n_dim:] = bright
    bgv = 0.0
    if variant == "pairs":
        # The bright points as six (near, far) pairs around a tile: `near` (0.8) one pixel beside the tile lifts every
        # pixel of it above HALF of what a point two cells away can reach, at both large radii; `far` (1.0), 9 px from
        # the tile's last column in the second cell beyond, still wins pixels there.  A ring bound that is too small by
        # a factor of two drops `far` for the whole tile (ring_bound_losses).
        near, far = [], []
        for ty, tx, side in ((1, 2, 1), (3, 5, -1), (5, 2, 1), (6, 5, -1), (2, 0, 1), (4, 7, -1)):
            row = ty * 8 + 3.5
            near.append((row, tx * 8 - 1.0 if side > 0 else tx * 8 + 8.0))
            far.append((row, tx * 8 + 16.0 if side > 0 else tx * 8 - 9.0))
        pts[n_dim:] = np.array(near + far, np.float32)
        feat[n_dim:, 0] = [0.8] * 6 + [1.0] * 6
    elif variant == "two_channel":
        feat = np.concatenate([dim, feat], 1)
    elif variant == "mirrored":
        feat, bgv = -feat, -1.0
    else:
        assert variant == "base"
    bi = np.zeros(len(pts), np.int32)
    return _shuffled(pts, feat, bi, np.full((1, feat.shape[1], S, S), bgv, np.float32), 4)


# ------------------------------------------------------------------------------------------------ C: crowded regions
CROWDED_SIZES = (64, 40, 43)  # four full regions; partial regions; partial regions and partial 8 x 8 tiles
CROWDED_RADII = ((0.7, 1.0), (1.0, 2.0))
CROWDED_BATCH = 2
ACC_SLOTS = 512            # kAccSlots of p2i.hip: the backward's hash table per 32 x 32 region
ACC_REGION = 32
# Constants of the gather's per-ring skip that ring_bound_losses restates (p2i_gather_max_kernel, the `if (ring >= 2)`
# block at the head of its ring loop, and kCell / kWeightErr): if that rule changes, the model below must follow.
CELL = 8                   # kCell: pixels per side of a binning cell / a wave's tile
RING_TESTED = 2            # the first ring the skip test is applied to: its points lie >= (RING_TESTED - 1) * CELL px away
RING_BAND = 2 * 1.5e-6     # band = 2 * kWeightErr, times the call's largest |feature|


@functools.lru_cache(None)
def crowded(S, C):
    """One point per pixel (centre + U[-0.3, 0.3] jitter), features in [0.1, 1], B = 2.  No background here: the
    backward cases run over the zero background of test_backward_regimes._run_p2i_max."""
    B = CROWDED_BATCH
    rng = np.random.default_rng(500 + S + C)
    yy, xx = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing="ij")
    centres = np.tile(np.stack([yy.ravel(), xx.ravel()], 1), (B, 1))
    pts = (centres + rng.uniform(-0.3, 0.3, centres.shape)).astype(np.float32)
    feat = rng.uniform(0.1, 1.0, (len(pts), C)).astype(np.float32)
    bi = np.repeat(np.arange(B, dtype=np.int32), S * S)
    return _shuffled(pts, feat, bi, np.zeros((B, C, S, S), np.float32), 501 + S)


# ------------------------------------------------------------------------------------------------ census (CPU, oracle)
def candidate_values(case, R):
    """Every in-range (point, pixel) pair of the case with the oracle's arithmetic (oracle/p2i_check._value):
    arrays (b, y, x, pid, s2 [fp32], value [n_pairs, C] fp32)."""
    from p2i_check import _value

    pts, feat, bi, bg = case
    B, C, H, W = bg.shape
    R32 = np.float32(R)
    out = []
    for pid in range(len(pts)):
        if not (0 <= bi[pid] < B):
            continue
        py, px = pts[pid]
        y0, y1 = np.clip([np.floor(py - R32), np.ceil(py + R32)], 0, H - 1).astype(np.int64)
        x0, x1 = np.clip([np.floor(px - R32), np.ceil(px + R32)], 0, W - 1).astype(np.int64)
        y, x = [a.ravel() for a in np.meshgrid(np.arange(y0, y1 + 1), np.arange(x0, x1 + 1), indexing="ij")]
        dx, dy = x.astype(np.float32) - px, y.astype(np.float32) - py
        s2 = dx * dx + dy * dy
        keep = np.sqrt(s2, dtype=np.float32) <= R32
        y, x, s2 = y[keep], x[keep], s2[keep]
        pidv = np.full(len(y), pid, np.int64)
        vals = np.stack([_value(pidv, np.full(len(y), c), y, x, pts, feat, R)[0] for c in range(C)], 1)
        out.append((np.full(len(y), bi[pid], np.int64), y, x, pidv, s2, vals.astype(np.float32)))
    return [np.concatenate(a) for a in zip(*out)]


def rim_won(case, R, ids, s2_rim):
    """Number of pixels (over all channels) whose oracle winner `ids` lies at squared distance exactly s2_rim (fp32)."""
    pts = case.pts
    b, c, y, x = np.nonzero(ids >= 0)
    pid = ids[b, c, y, x]
    dx, dy = x.astype(np.float32) - pts[pid, 1], y.astype(np.float32) - pts[pid, 0]
    return int(np.count_nonzero(dx * dx + dy * dy == np.float32(s2_rim)))


# The reference's weight is 0.5 * cos(x) + 0.5 with the cosine rounded to a double: next to -1 that is a grid of
# 2^-54 = 5.6e-17, and the HIP path's exact weight is a series within 2.3e-16 of it (cos_weight_inv, p2i.hip).  Next
# to the rim, where weights are 1e-13 and less, two candidates closer than that times |feature| are ordered by the
# last bit of a double cosine -- by neither side's arithmetic -- although they are thousands of fp32 ulps apart.
WEIGHT_NOISE = 2.3e-16 + 2.0 ** -54


def tie_census(case, R):
    """(exact, near, noise): pixels whose best value is attained, bit-equal and above the background, by two or more
    distinct points; pixels whose two largest distinct candidate values -- the background among them -- lie within one
    fp32 ulp; pixels where they lie farther apart than that, yet within WEIGHT_NOISE * |feature|."""
    b, y, x, pid, _, vals = candidate_values(case, R)
    B, C, H, W = case.bg.shape
    exact = near = noise = 0
    for c in range(C):
        pix = (b * H + y) * W + x
        v = vals[:, c]
        fa = np.abs(case.feat[pid, c]).astype(np.float64)
        bgp = case.bg[:, c].reshape(-1)
        pix = np.concatenate([pix, np.arange(B * H * W)])          # the background: a candidate of every pixel
        v = np.concatenate([v, bgp])
        fa = np.concatenate([fa, np.zeros(B * H * W)])
        is_pt = np.concatenate([np.ones(len(vals), bool), np.zeros(B * H * W, bool)])
        order = np.lexsort((v, pix))                                 # by pixel, then by value ascending
        pix, v, fa, is_pt = pix[order], v[order], fa[order], is_pt[order]
        last = np.flatnonzero(np.r_[pix[1:] != pix[:-1], True])     # the best candidate of every pixel
        first = np.r_[0, last[:-1] + 1]
        for lo, hi in zip(first, last):
            top = v[hi]
            k = hi
            while k > lo and v[k - 1] == top:
                k -= 1
            if hi - k >= 1 and is_pt[k:hi + 1].all():
                exact += 1
            if k > lo:
                gap = abs(np.float64(top) - np.float64(v[k - 1]))
                if gap <= np.spacing(max(abs(top), abs(v[k - 1]))):
                    near += 1
                elif gap <= WEIGHT_NOISE * max(fa[k:hi + 1].max(), fa[k - 1]):
                    noise += 1
    return exact, near, noise


def far_winner_share(case, R, ids):
    """Share of the pixels of channel C - 1 won by a point whose cell (floor(coord) // 8, clamped into the image) is two
    or more cells away (Chebyshev) from the pixel's own cell: candidates the gather meets in ring >= 2."""
    _, C, H, W = case.bg.shape
    b, y, x = np.nonzero(ids[:, C - 1] >= 0)
    pid = ids[b, C - 1, y, x]
    cells_y, cells_x = (H + CELL - 1) // CELL, (W + CELL - 1) // CELL
    cy = np.clip(np.floor(case.pts[pid, 0]).astype(np.int64) // CELL, 0, cells_y - 1)
    cx = np.clip(np.floor(case.pts[pid, 1]).astype(np.int64) // CELL, 0, cells_x - 1)
    ring = np.maximum(np.abs(cy - y // CELL), np.abs(cx - x // CELL))
    return float(np.count_nonzero(ring >= 2)) / (ids.shape[0] * H * W)


def ring_bound_losses(case, radii, ids_by_radius, factor):
    """Pixels that lose their oracle winner if the gather's per-ring bound (largest |feature| of the call times the
    weight at the ring's distance, p2i.hip) were `factor` times what it is: a tile stops after ring 1 when, for every
    radius that reaches ring 2, the weakest pixel's best value from the background and rings 0 - 1 lies above the bound;
    counted are the pixels of such tiles whose winner sits in ring >= 2.  factor = 1 must give 0: the bound is sound."""
    pts, feat, _, bg = case
    _, C, H, W = bg.shape
    cells_y, cells_x = (H + CELL - 1) // CELL, (W + CELL - 1) // CELL
    cy = np.clip(np.floor(pts[:, 0]).astype(np.int64) // CELL, 0, cells_y - 1)
    cx = np.clip(np.floor(pts[:, 1]).astype(np.int64) // CELL, 0, cells_x - 1)
    fmax = float(np.abs(feat).max())
    g2 = float(((RING_TESTED - 1) * CELL) ** 2)                 # squared distance every point of the tested ring keeps
    weight = lambda u: 0.5 * np.cos(np.pi * np.sqrt(np.minimum(u, 1.0))) + 0.5
    lost = 0
    for c in range(C):
        for ty in range(cells_y):
            for tx in range(cells_x):
                close = (np.abs(cy - ty) < RING_TESTED) & (np.abs(cx - tx) < RING_TESTED)
                yy, xx = np.meshgrid(np.arange(ty * CELL, min(ty * CELL + CELL, H)), np.arange(tx * CELL, min(tx * CELL + CELL, W)),
                                     indexing="ij")
                d2 = (yy[..., None] - pts[close, 0].astype(np.float64)) ** 2 + (xx[..., None] - pts[close, 1]) ** 2
                live = False
                for R in radii:
                    if g2 > R * R:
                        continue
                    val = np.where(d2 <= R * R, feat[close, c] * weight(d2 / (R * R)), -np.inf)
                    weakest = np.maximum(val.max(-1, initial=-np.inf), bg[0, c, yy, xx]).min()
                    live = live or weakest <= factor * fmax * weight(g2 / (R * R)) + RING_BAND * fmax
                if live:
                    continue
                for R in radii:
                    p = ids_by_radius[R][0, c, yy, xx]
                    ring = np.maximum(np.abs(cy[np.maximum(p, 0)] - ty), np.abs(cx[np.maximum(p, 0)] - tx))
                    lost += int(np.count_nonzero((p >= 0) & (ring >= RING_TESTED)))
    return lost


def winners_per_region(ids_r):
    """ids_r [R, B, C, H, W]: (image, channel, distinct winners) of every 32 x 32 region, the winners counted once over
    all radii of the call -- the backward's table is keyed by the point id alone, so that is the number of slots the
    region asks for."""
    nr, B, C, H, W = ids_r.shape
    out = []
    for b in range(B):
        for c in range(C):
            for y0 in range(0, H, ACC_REGION):
                for x0 in range(0, W, ACC_REGION):
                    blk = ids_r[:, b, c, y0:y0 + ACC_REGION, x0:x0 + ACC_REGION]
                    out.append((b, c, len(np.unique(blk[blk >= 0]))))
    return out
