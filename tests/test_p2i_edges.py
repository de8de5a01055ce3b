"""p2i max forward where a depth map never takes it: the rim of the kernel (r == R), value ties between distinct points
in bulk, coordinates on cell and image borders, and dim points near with bright points far.

The other p2i suites draw uniform random points, features in [0, 1) and a background >= 0.  On those inputs
s2 == R * R never happens -- and would not show: the rim weight is (cos(pi) + 1) / 2 = 0, the value f * 0 is not above
a background >= 0, so the id stays -1 whether or not the kernel put the pixel in range.  Here the background is
negative (0 > background: the point must own every rim pixel), the points sit on integers (tests/p2i_cases.py), and
every entry point -- sn_p2i_max_forward, sn_p2i_max_forward_multi in both layouts, the global splat behind radii
> 16 px, sn_p2i_max_forward_f64 -- is held to the oracle with the project's own bounds (test_p2i._close_maps: values
2e-6 / 1e-7, ids exact up to verified one-ulp ties, at most max(2, pixels / 10000) of those).

CPU half (-m "not gpu"): the oracle alone on the same inputs, asserting what makes each GPU comparison discriminating.
Measured (oracle, B = 2, C = 1, background -0.5):
  rim-won pixels   isolated 130 / 104 / 112 / 110 at R = 5 / 10 / 13 / 20; lattice step 6: 115, step 5: 33 at R = 5 and none
                   at R >= 10; at sqrt(2) / sqrt(5) / sqrt(8): isolated 56 / 112 / 56, lattice 586 / 1172 / 586 -- and 0 at
                   the fp32 radius below each
  exact id ties    lattice 249 / 308 / 324 pixels at R = 5 / 10 / 13 (C = 2: 404 / 498 / 514; one image, C = 2: 217 / 270 / 288)
  near-ties        0 on every case and radius (cap 2 ... 3)
  ring >= 2        9.2 % of the pixels at R = 16 (2.1 % at 12, none at 7); sign-mirrored 71 %; `pairs`: 24 pixels that half
                   the ring bound would lose (0 on the random variants)
  crowded regions  1013 ... 1029 distinct winners in a full 32 x 32 region (512 slots)"""
import functools

import numpy as np
import pytest
import torch

import oracle
import p2i_cases as pc
from test_p2i import _close_maps, _np_p2i_f64

# name -> (builder, arguments, radius groups of the tile gather (one multi-radius call each), radii of the global splat)
_SQRT_GROUPS = tuple(pc.sqrt_radii(k) for k in pc.RIM_SQUARES)
_CASES = {
    "isolated-B2-C1": ("isolated", (2, 1, "flat"), (pc.R_TILE,) + _SQRT_GROUPS, (pc.R_SPLAT,)),
    "isolated-B1-C2": ("isolated", (1, 2, "flat"), (pc.R_TILE,) + _SQRT_GROUPS, (pc.R_SPLAT,)),
    "isolated-B2-C2-random-bg": ("isolated", (2, 2, "random"), (pc.R_TILE,), (pc.R_SPLAT,)),
    "lattice-B2-C1": ("lattice", (2, 1, "flat"), (pc.R_TILE,) + _SQRT_GROUPS, ()),
    "lattice-B1-C2": ("lattice", (1, 2, "flat"), (pc.R_TILE,) + _SQRT_GROUPS, ()),
    "lattice-B2-C2-random-bg": ("lattice", (2, 2, "random"), (pc.R_TILE,), ()),
    "borders-S17-C1": ("borders", (17, 1), (pc.BORDER_RADII,), ()),
    "borders-S17-C2": ("borders", (17, 2), (pc.BORDER_RADII,), ()),
    "borders-S40-C1": ("borders", (40, 1), (pc.BORDER_RADII,), ()),
    "borders-S40-C2": ("borders", (40, 2), (pc.BORDER_RADII,), ()),
    "borders-S43-C2": ("borders", (43, 2), (pc.BORDER_RADII,), ()),
}
_LATTICES = [k for k in _CASES if k.startswith("lattice")]
_DIM_VARIANTS = ("base", "two_channel", "mirrored", "pairs")


def _case(name):
    builder, args, _, _ = _CASES[name]
    return getattr(pc, builder)(*args)


@functools.lru_cache(None)
def _oracle(builder, args, R):
    """the oracle's (out, ids) of a case at one radius: computed once, shared, read-only"""
    case = getattr(pc, builder)(*args)
    out, ids = oracle.p2i_max_forward(case.pts, case.feat, case.bi, case.bg, R)
    out.setflags(write=False)
    ids.setflags(write=False)
    return out, ids


def _ref(name, R):
    return _oracle(_CASES[name][0], _CASES[name][1], R)


def _radii(name):
    _, _, groups, splat = _CASES[name]
    return sorted({R for g in groups for R in g} | set(splat))


def _cap(case):
    return max(2, case.bg.size // 10000)


# ---------------------------------------------------------------------------------------------------------- CPU side
def test_isolated_points_are_isolated_and_touch_the_border():
    """No two points of an image within 2 * 20 + 2 px (a pixel has one candidate at most, up to the splat's radius);
    integer coordinates; some within 5 px of the border, two outside the image at exactly 5 and 13 px from a border
    pixel; every image owns one block of ids (the grouped binning's layout) and inside it the ids do not follow the cells."""
    S = pc.ISOLATED_S
    case = pc.isolated(2, 1)
    assert np.array_equal(case.pts, np.round(case.pts))
    d = np.linalg.norm(case.pts[:, None].astype(np.float64) - case.pts[None], axis=2)
    d[(case.bi[:, None] != case.bi[None]) | np.eye(len(d), dtype=bool)] = np.inf
    assert d.min() > 2 * pc.R_SPLAT + 2
    inside = ((case.pts >= 0) & (case.pts <= S - 1)).all(1)
    near = inside & ((case.pts < 5) | (case.pts > S - 1 - 5)).any(1)
    assert near.sum() >= 6 and (~inside).sum() == 4            # two outside points per image
    gap = np.maximum(np.maximum(-case.pts, case.pts - (S - 1)), 0).max(1)[~inside]
    assert sorted(gap.tolist()) == [5.0, 5.0, 13.0, 13.0]
    assert np.all(np.diff(case.bi) >= 0) and np.all(np.bincount(case.bi) == len(case.bi) // 2)
    cell = (np.clip(np.floor(case.pts[:, 0]), 0, S - 1) // pc.CELL) * 100 + np.clip(np.floor(case.pts[:, 1]), 0, S - 1) // pc.CELL
    assert all(np.any(np.diff(cell[case.bi == b]) < 0) for b in range(2))


@pytest.mark.parametrize("R", pc.R_TILE + (pc.R_SPLAT,))
def test_rim_won_pixels_integer_radii(R):
    """Per radius at least 30 pixels whose oracle winner lies at s2 == R * R in fp32: the isolated points give them at
    every radius, the lattices of step 6 and of step 5 at R = 5 each."""
    name = "isolated-B2-C1"
    n = pc.rim_won(_case(name), R, _ref(name, R)[1], R * R)
    print(f"isolated R={R}: {n} rim-won pixels")
    assert n >= 30
    if R == 5.0:
        lat, ids = _case("lattice-B2-C1"), _ref("lattice-B2-C1", R)[1]
        for b, step in enumerate(pc.LATTICE_STEPS):
            one = np.where(np.arange(2).reshape(2, 1, 1, 1) == b, ids, -1)
            n = pc.rim_won(lat, R, one, R * R)
            print(f"lattice step {step} R={R}: {n} rim-won pixels")
            assert n >= 30


@pytest.mark.parametrize("name", ["isolated-B2-C1", "lattice-B2-C1"])
@pytest.mark.parametrize("k", pc.RIM_SQUARES)
def test_rim_won_pixels_at_sqrt_radii(k, name):
    """R = float32(sqrt(k)) and the fp32 above it own at least 30 pixels at squared distance exactly k; the fp32 below
    owns none of them (they fall to the background): an s_max one ulp off in either direction changes ids."""
    case = _case(name)
    r0, dn, up = pc.sqrt_radii(k)
    assert dn < r0 < up and np.sqrt(np.float32(k), dtype=np.float32) == np.float32(r0)
    i0, idn, iup = (_ref(name, R)[1] for R in (r0, dn, up))
    n0, ndn, nup = pc.rim_won(case, r0, i0, k), pc.rim_won(case, dn, idn, k), pc.rim_won(case, up, iup, k)
    print(f"{name} k={k}: {n0} / {ndn} / {nup} pixels won at s2 == k (R, below, above)")
    assert n0 >= 30 and nup >= 30 and ndn == 0
    pts = case.pts
    b, c, y, x = np.nonzero(i0 >= 0)
    pid = i0[b, c, y, x]
    rim = (x.astype(np.float32) - pts[pid, 1]) ** 2 + (y.astype(np.float32) - pts[pid, 0]) ** 2 == np.float32(k)
    assert np.all(idn[b, c, y, x][rim] != pid[rim])


@pytest.mark.parametrize("name", _LATTICES)
@pytest.mark.parametrize("R", pc.R_TILE)
def test_lattice_has_exact_id_ties_in_bulk(R, name):
    """At least 200 pixels whose best value is attained bit-equal by two or more distinct points (the lowest id must
    win; the ids are shuffled against the cell order)."""
    exact, _, _ = pc.tie_census(_case(name), R)
    print(f"{name} R={R}: {exact} pixels with an exact tie between points")
    assert exact >= 200


@pytest.mark.parametrize("R", pc.ZERO_PAIR_RADII)
def test_zero_pairs_put_both_zeros_on_one_pixel(R):
    """The centre pixel of every image has exactly two candidates, both on their rim: -0 from the negative feature and
    +0 from the positive one; in images 0 and 1 the -0 belongs to the lower id.  The oracle gives that pixel to the
    lower id over a background of -0.5 and to nobody over a background of -0.0, which keeps its sign there and on the
    whole rim of every positive point (at least 4 in-image rim pixels per image)."""
    c = pc.ZERO_PAIR_S // 2
    flat, nz = pc.zero_pairs(R), pc.zero_pairs(R, "negative_zero")
    b, y, x, pid, s2, vals = pc.candidate_values(flat, R)
    for img in range(4):
        m = (b == img) & (y == c) & (x == c)
        assert sorted(pid[m]) == [2 * img, 2 * img + 1] and np.all(s2[m] == np.float32(R * R)) and np.all(vals[m] == 0)
        assert np.signbit(vals[m][np.argsort(pid[m]), 0]).tolist() == ([True, False] if img < 2 else [False, True])
    out, ids = _oracle("zero_pairs", (R, "flat"), R)
    assert ids[:, 0, c, c].tolist() == [0, 2, 4, 6] and np.all(out[:, 0, c, c] == 0)
    out, ids = _oracle("zero_pairs", (R, "negative_zero"), R)
    assert np.all(ids[:, 0, c, c] == -1) and np.all(np.signbit(out[ids < 0])) and (ids >= 0).any()
    rim = (s2 == np.float32(R * R)) & (nz.feat[pid, 0] > 0)
    assert np.all(ids[b[rim], 0, y[rim], x[rim]] == -1) and all(np.count_nonzero(rim & (b == img)) >= 4 for img in range(4))


@pytest.mark.parametrize("name", list(_CASES))
def test_near_tie_census_stays_under_the_cap(name):
    """Pixels whose two largest distinct candidate values (the background among them) lie within one fp32 ulp are the
    only ones where the HIP path may legitimately pick another winner than the oracle: on every case and radius there
    are no more of them than _close_maps allows, so the oracle alone stays inside the cap.  And no pixel is decided
    inside the rounding noise of the double cosine next to the rim (p2i_cases.WEIGHT_NOISE): there the oracle's
    own winner is an accident of the last bit of glibc's cos, and no implementation could be held to it."""
    case = _case(name)
    for R in _radii(name):
        _, near, noise = pc.tie_census(case, R)
        print(f"{name} R={R}: {near} near-ties, cap {_cap(case)}; {noise} inside the noise of the double cosine")
        assert near <= _cap(case) and noise == 0


@pytest.mark.parametrize("S", pc.BORDER_SIZES)
def test_border_coordinates_are_what_they_claim(S):
    """-0.0, cell borders and the fp32 below them (another cell), S - 1 and the fp32 above, points exactly R outside
    and one ulp farther, +-9.9e8; some rim pixel is won at both radii."""
    case = pc.borders(S, 1)
    v = case.pts[:, 0]
    assert np.any(np.signbit(v) & (v == 0)) and np.abs(case.pts).max() == np.float32(9.9e8)
    for k in range(8, S, 8):
        lo = np.nextafter(np.float32(k), np.float32(0))
        assert np.any(v == k) and np.any(v == lo) and int(np.floor(lo)) // 8 == k // 8 - 1
    assert np.any(v == S - 1) and np.any(v == np.nextafter(np.float32(S - 1), np.float32(np.inf)))
    for R in pc.BORDER_RADII:
        for edge, out in ((-R, -np.inf), (S - 1 + R, np.inf)):
            assert np.any(v == np.float32(edge)) and np.any(v == np.nextafter(np.float32(edge), np.float32(out)))
        n = pc.rim_won(case, R, _oracle("borders", (S, 1), R)[1], R * R)
        print(f"borders S={S} R={R}: {n} rim-won pixels")
        assert n >= 3


def test_dim_near_bright_far_wins_from_two_cells_away():
    """At the largest radius at least 5 % of the pixels are won by a point whose cell is two or more cells from the
    pixel's own: candidates of ring >= 2, which the per-ring skip must not drop."""
    R = max(pc.DIM_RADII)
    for variant in ("base", "two_channel", "mirrored"):
        case = pc.dim_near_bright_far(variant)
        share = pc.far_winner_share(case, R, _oracle("dim_near_bright_far", (variant,), R)[1])
        print(f"{variant} R={R}: {100 * share:.1f} % of the pixels won from ring >= 2")
        assert share >= 0.05
    assert np.abs(pc.dim_near_bright_far("two_channel").feat[:, 0]).max() <= 0.02   # bright in channel 1 only


def test_bright_pairs_sit_where_the_ring_bound_decides():
    """The random bright points of the other variants never meet a tile whose weakest pixel lies between half the ring
    bound and the bound (0 pixels would change under a halved bound).  `pairs` puts them there: the sound bound loses
    nothing, half of it loses at least 20 pixels."""
    for variant in _DIM_VARIANTS:
        case = pc.dim_near_bright_far(variant)
        ids = {R: _oracle("dim_near_bright_far", (variant,), R)[1] for R in pc.DIM_RADII}
        sound, halved = (pc.ring_bound_losses(case, pc.DIM_RADII, ids, f) for f in (1.0, 0.5))
        print(f"{variant}: {sound} pixels lost under the ring bound, {halved} under half of it")
        assert sound == 0
        if variant == "pairs":
            assert halved >= 20
    feat = pc.dim_near_bright_far("pairs").feat
    assert np.count_nonzero(feat >= 0.8) == 12 and feat.max() == 1.0 and np.count_nonzero(feat <= 0.02) == 1500


@pytest.mark.parametrize("S", pc.CROWDED_SIZES)
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("radii", pc.CROWDED_RADII)
def test_crowded_regions_overflow_the_hash_table(radii, C, S):
    """Per channel some 32 x 32 region holds at least 600 distinct winners over the call's radii: the backward's
    table has 512 slots, so at least 88 winners of that region leave through the direct-to-global branch."""
    ids = np.stack([_oracle("crowded", (S, C), R)[1] for R in radii])
    per = pc.winners_per_region(ids)
    for c in range(C):
        most = max(n for _, cc, n in per if cc == c)
        print(f"crowded S={S} C={C} radii={radii} channel {c}: {most} distinct winners in one region")
        assert most >= 600 and most - pc.ACC_SLOTS >= 88


# ---------------------------------------------------------------------------------------------------------- GPU side
def _dev(case, dev):
    return tuple(torch.from_numpy(np.array(a)).to(dev) for a in case)      # the cases are read-only: copies


def _check_group(ext, case, t, radii, oracle_of, what):
    """one multi-radius call in both layouts == one single-radius call per radius (bit for bit) == the oracle"""
    pts, feat, bi, bg = t
    out, ids = ext.p2i_max_forward_multi_gpu(pts, feat, bi, bg, 0, list(radii))
    assert out.shape == (len(radii),) + tuple(bg.shape)
    if max(radii) <= 16.0:
        out_im, ids_im = ext.p2i_max_forward_multi_gpu(pts, feat, bi, bg, 0, list(radii), image_major=True)
        assert torch.equal(out_im.transpose(0, 1), out) and torch.equal(ids_im.transpose(0, 1), ids), what
    for r, R in enumerate(radii):
        o1, i1 = ext.p2i_max_forward_gpu(pts, feat, bi, bg, 0, R)
        assert torch.equal(out[r], o1) and torch.equal(ids[r], i1), (what, R)
        o, i = oracle_of(R)
        _close_maps(out[r].cpu().numpy(), ids[r].cpu().numpy(), o, i, f"{what} R={R!r}", case.pts, case.feat, case.bg, R)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(_CASES))
def test_hip_rim_ties_and_borders_match_oracle(name, dev):
    """Groups A and D on sn_p2i_max_forward and sn_p2i_max_forward_multi (radius-major and image-major): rim pixels
    (value 0 over a negative background) must be owned, exact ties go to the lowest id, radii one fp32 ulp below
    sqrt(k) leave the pixels at s2 == k to the background; radii > 16 px take the global splat."""
    from sparenet_amd.cuda.p2i_op import ext

    case, t = _case(name), _dev(_case(name), dev)
    _, _, groups, splat = _CASES[name]
    for radii in groups:
        _check_group(ext, case, t, radii, lambda R: _ref(name, R), name)
    if splat:
        _check_group(ext, case, t, splat, lambda R: _ref(name, R), name + " (global splat)")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["isolated-B2-C1", "isolated-B1-C2", "lattice-B2-C1", "lattice-B2-C2-random-bg",
                                  "borders-S17-C1", "borders-S43-C2"])
def test_hip_float64_rim_ties_and_borders_match_numpy(name, dev):
    """The same inputs on sn_p2i_max_forward_f64 against the numpy float64 restatement (test_p2i._np_p2i_f64): all of
    group A's radii -- 5, 10, 13 (the rim at r == R in double; 20 on the isolated points) and sqrt(2), sqrt(5), sqrt(8)
    each with its two float64 neighbours -- and the border radii on the border cases."""
    from sparenet_amd.cuda.p2i_op import ext

    case = _case(name)
    pts, feat, bg = (a.astype(np.float64) for a in (case.pts, case.feat, case.bg))
    builder = _CASES[name][0]
    sqrt_all = tuple(R for k in pc.RIM_SQUARES for R in pc.sqrt_radii_f64(k))
    radii = {"isolated": pc.R_TILE + (pc.R_SPLAT,) + sqrt_all, "lattice": pc.R_TILE + sqrt_all,
             "borders": pc.BORDER_RADII}[builder]
    T = lambda a: torch.from_numpy(np.array(a)).to(dev)
    owned = []
    for R in radii:
        out, ids = ext.p2i_max_forward_gpu(T(pts), T(feat), T(case.bi), T(bg), 0, R)
        ro, ri = _np_p2i_f64(pts, feat, case.bi, bg, R, "max")
        np.testing.assert_allclose(out.cpu().numpy(), ro, rtol=1e-13, atol=1e-15, err_msg=f"{name} R={R!r}")
        assert np.array_equal(ids.cpu().numpy(), ri), (name, R)
        owned.append(int((ri >= 0).sum()))
    if builder != "borders":          # the reference itself: sqrt(k) and above own the rim, the double below does not
        for k in range(len(pc.RIM_SQUARES)):
            at, below, above = owned[len(owned) - 3 * (k + 1):][:3]
            assert at == above > below


@pytest.mark.gpu
@pytest.mark.parametrize("variant", _DIM_VARIANTS)
def test_hip_dim_near_bright_far_matches_oracle(variant, dev):
    """Group B: a pixel's winner sits two or more cells away, behind many dim candidates: neither the per-ring skip nor
    the cull of 64 candidates (both scaled by the call's largest |feature|) may drop it.  Which variant checks what:
    `pairs` alone carries the per-ring bound (half of it loses 24 pixels there and none on the others,
    test_bright_pairs_sit_where_the_ring_bound_decides); `base` and `two_channel` exercise the cull and the band with
    winners in ring >= 2 (`two_channel`: a band and bounds of channel 0 fifty times its own features); `mirrored`
    only the cull's max(feature, 0) bound -- its running bests are negative, so the ring test can never fire."""
    from sparenet_amd.cuda.p2i_op import ext

    case = pc.dim_near_bright_far(variant)
    _check_group(ext, case, _dev(case, dev), pc.DIM_RADII, lambda R: _oracle("dim_near_bright_far", (variant,), R),
                 f"dim near, bright far ({variant})")


@pytest.mark.gpu
@pytest.mark.parametrize("bg", ["flat", "negative_zero"])
@pytest.mark.parametrize("R", pc.ZERO_PAIR_RADII)
def test_hip_zeros_of_both_signs_tie(R, bg, dev):
    """-0 and +0 are one value: the centre pixel of p2i_cases.zero_pairs goes to the lower id whichever sign it brings,
    and a background of -0.0 is replaced by no +0 and comes out with its sign.  Ids EXACTLY equal to the oracle's (two
    zeros would pass as a 0-ulp tie in _close_maps), on the single-radius entry and on the multi-radius one -- the tile
    gather at R = 5 and 10, the global splat with its order-preserving keys at R = 20 -- and on the float64 entry."""
    from sparenet_amd.cuda.p2i_op import ext

    case = pc.zero_pairs(R, bg)
    o, i = _oracle("zero_pairs", (R, bg), R)
    pts, feat, bi, bgt = _dev(case, dev)
    runs = {"single": ext.p2i_max_forward_gpu(pts, feat, bi, bgt, 0, R),
            "multi": tuple(a[0] for a in ext.p2i_max_forward_multi_gpu(pts, feat, bi, bgt, 0, [R])),
            "float64": ext.p2i_max_forward_gpu(pts.double(), feat.double(), bi, bgt.double(), 0, R)}
    o64, i64 = _np_p2i_f64(case.pts.astype(np.float64), case.feat.astype(np.float64), case.bi,
                           case.bg.astype(np.float64), R, "max")
    assert np.array_equal(i64, i)                     # the two references agree on who owns what
    for what, (out, ids) in runs.items():
        out, ids = out.cpu().numpy(), ids.cpu().numpy()
        assert np.array_equal(ids, i), (what, R, bg, np.argwhere(ids != i)[:8])
        if what == "float64":
            np.testing.assert_allclose(out, o64, rtol=1e-13, atol=1e-15, err_msg=f"{what} R={R}")
        else:
            np.testing.assert_allclose(out, o, rtol=2e-6, atol=1e-7, err_msg=f"{what} R={R}")
        assert np.array_equal(np.signbit(out[i < 0]), np.signbit(o[i < 0])), (what, R, bg, "sign of an unowned pixel")
