"""Ragged batches on the GPU (sn_*_ragged, sn_pad_compact, sparenet_amd.cuda.ragged): the contract of
include/sparenet_hip.h.  A cloud's valid rows equal what the dense entry point gives for that cloud alone BIT FOR BIT
(distances, indices, assignments, gradients), whatever its neighbours, its batch position and the padded width;
padding rows -- NaN is planted in every one of them -- come back as 0 / -1 / 0."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _embed(clouds, width, dev):
    """clouds: list of [n_i, 3] arrays -> ([B, width, 3] tensor with NaN in every padding row, lengths)."""
    out = np.full((len(clouds), width, 3), np.nan, np.float32)
    for i, c in enumerate(clouds):
        out[i, :len(c)] = c
    return torch.from_numpy(out).to(dev), [len(c) for c in clouds]


def _rows(values, lengths, width, fill):
    """per-cloud row arrays -> [B, width, ...] with `fill` beyond the lengths"""
    shape = (len(values), width) + tuple(np.asarray(values[0]).shape[1:])
    out = np.full(shape, fill, np.asarray(values[0]).dtype)
    for i, v in enumerate(values):
        out[i, :lengths[i]] = v
    return out


def _filler(r, n):
    return r.random((n, 3), dtype=np.float32)


# ------------------------------------------------------------------------------------------------ goldens, embedded
@pytest.mark.parametrize("name", ["chamfer_rand_2x1300x777", "chamfer_ties_2x600x500", "chamfer_tiny_3x1x5"])
def test_chamfer_golden_embedded_between_other_clouds(name, golden_dir, dev):
    from sparenet_amd.cuda.ragged import chamfer_ragged, chamfer_ragged_forward_raw

    z = np.load(os.path.join(golden_dir, name + ".npz"))
    r = np.random.default_rng(7)
    nb, n, m = z["xyz1"].shape[0], z["xyz1"].shape[1], z["xyz2"].shape[1]
    c1, c2, pos = [], [], []
    for i in range(nb):   # fillers of other lengths before, between and after the golden clouds
        c1 += [_filler(r, 1 + 37 * i), z["xyz1"][i]]
        c2 += [_filler(r, 2051 - 500 * i), z["xyz2"][i]]
        pos.append(2 * i + 1)
    c1 += [_filler(r, 0), _filler(r, 1500)]
    c2 += [_filler(r, 9), _filler(r, 0)]
    w1, w2 = 1531, 2077                       # padded widths: no multiple of 1024
    x, l1 = _embed(c1, w1, dev)
    y, l2 = _embed(c2, w2, dev)
    d1, d2, i1, i2, *_ = chamfer_ragged_forward_raw(x, y, l1, l2)
    for k, p in enumerate(pos):
        assert np.array_equal(d1[p, :n].cpu().numpy(), z["dist1"][k]) and np.array_equal(i1[p, :n].cpu().numpy(), z["idx1"][k])
        assert np.array_equal(d2[p, :m].cpu().numpy(), z["dist2"][k]) and np.array_equal(i2[p, :m].cpu().numpy(), z["idx2"][k])
    for t, lens, fill in ((d1, l1, 0), (d2, l2, 0), (i1, l1, -1), (i2, l2, -1)):
        t = t.cpu().numpy()
        for i, ln in enumerate(lens):
            assert (t[i, ln:] == fill).all()
    # gradients: the golden's upstream gradients at its rows, NaN at every padding row
    xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    e1, e2 = chamfer_ragged(xg, yg, torch.tensor(l1, device=dev), torch.tensor(l2, dtype=torch.int32, device=dev))
    gd1 = _rows([r.standard_normal((len(c),)).astype(np.float32) for c in c1], l1, w1, np.float32(np.nan))
    gd2 = _rows([r.standard_normal((len(c),)).astype(np.float32) for c in c2], l2, w2, np.float32(np.nan))
    for k, p in enumerate(pos):
        gd1[p, :n], gd2[p, :m] = z["graddist1"][k], z["graddist2"][k]
    torch.autograd.backward([e1, e2], [torch.from_numpy(gd1).to(dev), torch.from_numpy(gd2).to(dev)])
    g1, g2 = xg.grad.cpu().numpy(), yg.grad.cpu().numpy()
    for k, p in enumerate(pos):
        assert np.array_equal(g1[p, :n], z["gradxyz1"][k]) and np.array_equal(g2[p, :m], z["gradxyz2"][k])
    for g, lens, other in ((g1, l1, l2), (g2, l2, l1)):
        for i, ln in enumerate(lens):
            assert not g[i, (ln if other[i] else 0):].any()     # padding rows, and a cloud with an empty side: 0


def test_emd_goldens_embedded_between_other_clouds(golden_dir, dev):
    from sparenet_amd.cuda.ragged import emd_ragged

    files = sorted(glob.glob(os.path.join(golden_dir, "emd_*.npz")))
    assert len(files) >= 10 and sum("negeps" in f for f in files) >= 3
    r = np.random.default_rng(8)
    for f in files:
        z = np.load(f)
        nb, n = z["xyz1"].shape[:2]
        c1, c2, pos = [_filler(r, 100)], [_filler(r, 1333)], []
        for i in range(nb):
            c1 += [z["xyz1"][i], _filler(r, 700 + i)]
            c2 += [z["xyz2"][i], _filler(r, 701 + i)]
            pos.append(1 + 2 * i)
        x, l1 = _embed(c1, n + 300, dev)      # n is a multiple of 1024: n + 300 is none
        y, l2 = _embed(c2, n + 555, dev)
        d, a = emd_ragged(x, y, l1, l2, float(z["eps"]), int(z["iters"]))
        for k, p in enumerate(pos):
            assert np.array_equal(a[p, :n].cpu().numpy(), z["assignment"][k]), f
            assert np.array_equal(d[p, :n].cpu().numpy(), z["dist"][k]), f
        a, d = a.cpu().numpy(), d.cpu().numpy()
        for i, ln in enumerate(l1):
            assert (a[i, ln:] == -1).all() and not d[i, ln:].any(), f


# -------------------------------------------------------------------------------------- against the dense kernels
LENGTHS = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3000]


def _random_batch(seed, b, n, m, shift, scale, dev, emd=False, collapsed=()):
    r = np.random.default_rng(seed)
    l1 = [min(int(v), n) for v in r.choice(LENGTHS, b)]
    l2 = [min(int(v), m) for v in r.choice(LENGTHS, b)]
    l1[0], l2[0] = n, m                                   # one full-width cloud
    if emd:
        l1 = [min(a, c) if k % 5 else a for k, (a, c) in enumerate(zip(l1, l2))]   # every fifth may be invalid
        l1[0], l2[0] = min(n, m), m
    c1 = [(_filler(r, a) * scale + shift).astype(np.float32) for a in l1]
    c2 = [(_filler(r, a) * scale + shift).astype(np.float32) for a in l2]
    for i in collapsed:                                   # every point within 1e-3 of one point
        if len(c1[i]):
            c1[i] = (c1[i][:1] + (r.random(c1[i].shape, dtype=np.float32) - 0.5) * np.float32(1e-3) * scale).astype(np.float32)
    x, l1 = _embed(c1, n, dev)
    y, l2 = _embed(c2, m, dev)
    return x, y, l1, l2, r


@pytest.mark.parametrize("b,shift,scale,device_lengths", [(32, 0.0, 1.0, False), (7, -40.0, 25.0, True)])
def test_chamfer_ragged_equals_dense_on_every_slice(b, shift, scale, device_lengths, dev):
    from sparenet_amd.cuda.chamfer_distance import ChamferDistanceFunction
    from sparenet_amd.cuda.ragged import chamfer_ragged, chamfer_ragged_forward_raw

    n, m = 3000, 2500
    x, y, l1, l2, r = _random_batch(21 + b, b, n, m, shift, scale, dev, collapsed=(0, 3))
    xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    given = (torch.tensor(l1, device=dev), torch.tensor(l2, device=dev)) if device_lengths else (l1, l2)
    d1, d2 = chamfer_ragged(xg, yg, *given)
    gd1 = torch.from_numpy(r.standard_normal((b, n)).astype(np.float32)).to(dev)
    gd2 = torch.from_numpy(r.standard_normal((b, m)).astype(np.float32)).to(dev)
    for i in range(b):
        gd1[i, l1[i]:] = NAN
        gd2[i, l2[i]:] = NAN
    torch.autograd.backward([d1, d2], [gd1, gd2])
    # cloud 0 is full-width and collapsed: its inverse lists (the queries that share a nearest target, the targets that
    # share a nearest query) are longer than the 64 entries the gather kernel serves -- the long-list kernel's work
    _, _, idx1, idx2, *_ = chamfer_ragged_forward_raw(x, y, *given)
    assert l1[0] == n and l2[0] == m
    assert torch.bincount(idx1[0, :n].long()).max().item() > 64 and torch.bincount(idx2[0, :m].long()).max().item() > 64
    for i in range(b):
        a, c = l1[i], l2[i]
        if a == 0 or c == 0:
            assert not d1[i].any() and not d2[i].any() and not xg.grad[i].any() and not yg.grad[i].any()
            continue
        xs, ys = x[i:i + 1, :a].clone().requires_grad_(True), y[i:i + 1, :c].clone().requires_grad_(True)
        e1, e2 = ChamferDistanceFunction.apply(xs, ys)
        torch.autograd.backward([e1, e2], [gd1[i:i + 1, :a].contiguous(), gd2[i:i + 1, :c].contiguous()])
        assert torch.equal(d1[i, :a], e1[0]) and torch.equal(d2[i, :c], e2[0]), i
        assert torch.equal(xg.grad[i, :a], xs.grad[0]) and torch.equal(yg.grad[i, :c], ys.grad[0]), i
        assert not d1[i, a:].any() and not d2[i, c:].any() and not xg.grad[i, a:].any() and not yg.grad[i, c:].any()


@pytest.mark.parametrize("b,shift,scale", [(12, 0.0, 1.0), (6, 3.0, 0.25)])
def test_emd_ragged_equals_general_and_persistent_on_every_slice(b, shift, scale, dev, monkeypatch):
    from sparenet_amd.cuda.emd.emd_general import emd_general
    from sparenet_amd.cuda.ragged import emd_ragged

    n, m = 2048, 3000
    x, y, l1, l2, r = _random_batch(50 + b, b, n, m, shift, scale, dev, emd=True, collapsed=(2,))
    # a slice the persistent auction serves: n_i == m_i == 1024
    l1[1], l2[1] = 1024, 1024
    x[1, 1024:], y[1, 1024:] = NAN, NAN
    x[1, :1024] = torch.from_numpy((_filler(r, 1024) * scale + shift).astype(np.float32)).to(dev)
    y[1, :1024] = torch.from_numpy((_filler(r, 1024) * scale + shift).astype(np.float32)).to(dev)
    eps, iters = 0.005 * scale, 20
    xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    d, a = emd_ragged(xg, yg, torch.tensor(l1, device=dev), torch.tensor(l2, device=dev), eps, iters)
    gd = torch.from_numpy(r.standard_normal((b, n)).astype(np.float32)).to(dev)
    for i in range(b):
        gd[i, l1[i]:] = NAN
    d.backward(gd)
    valid = 0
    for i in range(b):
        p, q = l1[i], l2[i]
        if p == 0 or p > q:
            assert torch.isnan(d[i]).all() and (a[i] == -1).all() and not xg.grad[i].any() and not yg.grad[i].any()
            continue
        valid += 1
        for force_general in ("1", "0"):
            if force_general == "0" and not (p == q and p % 1024 == 0):
                continue
            monkeypatch.setenv("SN_EMD_GENERAL", force_general)
            xs, ys = x[i:i + 1, :p].clone().requires_grad_(True), y[i:i + 1, :q].clone().requires_grad_(True)
            e, c = emd_general(xs, ys, eps, iters)
            e.backward(gd[i:i + 1, :p].contiguous())
            assert torch.equal(a[i, :p], c[0]) and torch.equal(d[i, :p], e[0]), (i, force_general)
            assert torch.equal(xg.grad[i, :p], xs.grad[0]) and torch.equal(yg.grad[i, :q], ys.grad[0]), (i, force_general)
        assert (a[i, p:] == -1).all() and not d[i, p:].any() and not xg.grad[i, p:].any() and not yg.grad[i, q:].any()
    assert valid >= b // 2


def test_invalid_emd_clouds_give_nan_rows_and_leave_neighbours_alone(dev):
    from sparenet_amd.cuda.emd.emd_general import emd_general
    from sparenet_amd.cuda.ragged import emd_ragged

    r = np.random.default_rng(3)
    x, _ = _embed([_filler(r, 900), _filler(r, 1200), _filler(r, 0), _filler(r, 500)], 1200, dev)
    y, _ = _embed([_filler(r, 1000), _filler(r, 700), _filler(r, 800), _filler(r, 500)], 1000, dev)
    l1 = torch.tensor([900, 1200, 0, 500], dtype=torch.int32, device=dev)     # cloud 1: 1200 > 700; cloud 2: no bidder
    l2 = torch.tensor([1000, 700, 800, 500], dtype=torch.int32, device=dev)
    d, a = emd_ragged(x, y, l1, l2, 0.005, 15)
    for i in (1, 2):
        assert torch.isnan(d[i]).all() and (a[i] == -1).all()
    for i, p, q in ((0, 900, 1000), (3, 500, 500)):
        e, c = emd_general(x[i:i + 1, :p].contiguous(), y[i:i + 1, :q].contiguous(), 0.005, 15)
        assert torch.equal(d[i, :p], e[0]) and torch.equal(a[i, :p], c[0])
    torch.cuda.synchronize()
    assert torch.equal(torch.arange(4, device=dev).sum().cpu(), torch.tensor(6))   # the device still answers


# ------------------------------------------------------------------------------------------------------ independence
def test_results_do_not_depend_on_width_position_or_run(dev):
    from sparenet_amd.cuda.ragged import chamfer_ragged, emd_ragged

    r = np.random.default_rng(4)
    p, q = _filler(r, 1500), _filler(r, 1777)
    outs = []
    for width, pos, b in ((1800, 0, 3), (2600, 4, 6), (2600, 4, 6)):
        c1 = [_filler(r, 1 + 97 * k) for k in range(b)]
        c2 = [_filler(r, 5 + 131 * k) for k in range(b)]
        c1[pos], c2[pos] = p, q
        x, l1 = _embed(c1, width, dev)
        y, l2 = _embed(c2, width + 77, dev)
        xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        d1, d2 = chamfer_ragged(xg, yg, l1, l2)
        e, a = emd_ragged(xg, yg, l1, l2, 0.005, 10)
        (d1[pos, :1500].sum() + d2[pos, :1777].sum() + e[pos, :1500].sum()).backward()
        outs.append([t.detach().clone() for t in (d1[pos, :1500], d2[pos, :1777], e[pos, :1500], a[pos, :1500],
                                                  xg.grad[pos, :1500], yg.grad[pos, :1777])])
    for other in outs[1:]:
        for u, v in zip(outs[0], other):
            assert torch.equal(u, v)


# ------------------------------------------------------------------------------------------------------- pad_compact
def test_pad_compact_follows_the_gridding_rule_and_keeps_order(dev):
    from sparenet_amd.cuda.gridding import Gridding  # noqa: F401  (the module whose padding rule is mirrored)
    from sparenet_amd.cuda.ragged import pad_compact
    import sparenet_amd
    from sparenet_amd import _lib

    r = np.random.default_rng(6)
    b, n = 4, 2500                      # longer than one workgroup's span of 1024 rows: the carry is exercised
    x = (r.random((b, n, 3), dtype=np.float32) - 0.5) * 6
    x[0, :40] = 0                       # zero rows at the front ...
    x[0, 1000:1100] = 0                 # ... in the middle (across a 1024 boundary) ...
    x[0, -7:] = 0                       # ... and at the end
    x[1, 5] = (1.5, -1.5, 0)            # (a, -a, 0): padding by the rule although it is not the origin
    x[1, 6] = (0.25, 0.5, -0.75)
    # (x + y) + z == 0 but x + (y + z) != 0 and (x + z) + y != 0: only the rule's order calls it padding
    x[1, 7] = (np.float32(2 ** 24), np.float32(1), np.float32(-2 ** 24))
    x[1, 9] = (np.float32(1), np.float32(2 ** 24), np.float32(-2 ** 24))
    # and the converse: (x + y) + z != 0 while x + (y + z) == 0: a point
    x[1, 8] = (np.float32(-2 ** 24), np.float32(2 ** 24), np.float32(1))
    x[2] = 0                            # an empty cloud
    for row in (7, 9):
        a, c, e = x[1, row]
        assert (a + c) + e == 0 and a + (c + e) != 0
    a, c, e = x[1, 8]
    assert (a + c) + e != 0 and a + (c + e) == 0
    xt = torch.from_numpy(x).to(dev).requires_grad_(True)
    packed, lengths, src = pad_compact(xt)
    # the rows sn_gridding_forward_padded marks as padding (index -1)
    scale = 8
    grid = torch.empty(b, scale ** 3, device=dev)
    weights = torch.empty(b, n, 8, 3, device=dev)
    indexes = torch.empty(b, n, 8, dtype=torch.int32, device=dev)
    xd = xt.detach().contiguous()
    _lib.check(sparenet_amd.lib().sn_gridding_forward_padded(_lib.fptr(xd, "x"), b, n, scale, _lib.fptr(grid, "g"),
                                                             _lib.fptr(weights, "w"), _lib.iptr(indexes, "i"),
                                                             _lib.stream_of(xd)), "sn_gridding_forward_padded")
    keep = (indexes[:, :, 0] != -1).cpu().numpy()
    assert not keep[1, 5] and not keep[1, 6] and not keep[1, 7] and keep[1, 8] and not keep[1, 9] and not keep[2].any()
    want_keep = ~((x[..., 0] + x[..., 1]) + x[..., 2] == 0)
    assert np.array_equal(keep, want_keep)
    packed_h, src_h = packed.detach().cpu().numpy(), src.cpu().numpy()
    assert lengths.dtype == torch.int32 and np.array_equal(lengths.cpu().numpy(), keep.sum(axis=1))
    for i in range(b):
        rows = np.nonzero(keep[i])[0]
        assert np.array_equal(src_h[i, :len(rows)], rows) and (src_h[i, len(rows):] == -1).all()   # order preserved
        assert np.array_equal(packed_h[i, :len(rows)], x[i, rows]) and not packed_h[i, len(rows):].any()
    # gradient scatter against indexing in torch
    g = torch.from_numpy(r.standard_normal((b, n, 3)).astype(np.float32)).to(dev)
    packed.backward(g)
    want = torch.zeros_like(g)
    for i in range(b):
        k = int(lengths[i])
        want[i, src[i, :k].long()] = g[i, :k]
    assert torch.equal(xt.grad, want)


def test_chamfer_distance_padded_classes(dev):
    from sparenet_amd.cuda.chamfer_dist import (ChamferDistance, ChamferDistancePadded, ChamferDistanceSeperate,
                                                ChamferDistanceSeperatePadded)

    r = np.random.default_rng(9)
    b, n, m = 4, 1500, 1100
    x, y = r.random((b, n, 3), dtype=np.float32), r.random((b, m, 3), dtype=np.float32)
    for i in range(b):
        x[i, r.choice(n, 200 * i + 3, replace=False)] = 0
        y[i, r.choice(m, 150 * i + 1, replace=False)] = 0
    xt, yt = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    # The classes take their means from distances that are bit-equal to the dense kernel's on the cloud without its zero
    # rows (test_chamfer_ragged_equals_dense_on_every_slice), so both sides are restated from those fp32 distances:
    #  - exactly: the padded classes' per-cloud mean is the float64 sum over the cloud's own points divided by their
    #    number, rounded once to fp32, and their mean over clouds is the float64 mean of those fp32 values rounded once
    #    (a sum of four fp32 values is exact in float64).  One row too many or too few, or a wrong divisor, moves the
    #    value by about 1 / 1500 of itself, 10^4 ulps: nothing but the right mean is equal.
    #  - ChamferDistance(ignore_zeros=True) itself takes torch's fp32 mean of the same distances, which agrees with
    #    the correctly rounded mean to rounding only.  Bound: the terms are non-negative, so the relative error of an
    #    fp32 summation is at most (longest chain of additions) * 2^-24; a reduction that is at least 32 lanes wide
    #    gives no lane more than ceil(1500 / 32) = 47 terms and adds 5 tree levels, 52 additions, then one division
    #    and the sum of the two means: 64 * 2^-24 = 3.8e-6 relative, 1 / 175 of what one row contributes.
    from sparenet_amd.cuda.chamfer_dist import ChamferFunction

    ulp = 2.0 ** -24
    singles, sep1, sep2 = [], [], []
    for i in range(b):
        xs, ys = xt[i:i + 1], yt[i:i + 1]
        d1, d2 = ChamferFunction.apply(xs[xs.sum(dim=2).ne(0)].unsqueeze(0), ys[ys.sum(dim=2).ne(0)].unsqueeze(0))
        assert d1.size(1) == n - (200 * i + 3) and d2.size(1) == m - (150 * i + 1)
        e1, e2 = d1.double().mean().float(), d2.double().mean().float()
        g1, g2 = ChamferDistanceSeperatePadded()(xs, ys)
        got = ChamferDistancePadded()(xs, ys)
        print(f"cloud {i}: padded {got.item():.9g}  restated {(e1 + e2).item():.9g}")
        assert g1.item() == e1.item() and g2.item() == e2.item(), i
        assert got.item() == (e1 + e2).item(), i
        want = ChamferDistance(ignore_zeros=True)(xs, ys)
        w1, w2 = ChamferDistanceSeperate(ignore_zeros=True)(xs, ys)
        print(f"cloud {i}: ChamferDistance(ignore_zeros=True) {want.item():.9g}  "
              f"relative difference in ulps {abs(got.item() - want.item()) / want.item() / ulp:.2f}")
        assert abs(got.item() - want.item()) <= 64 * ulp * want.item(), i
        assert abs(g1.item() - w1.item()) <= 64 * ulp * w1.item() and abs(g2.item() - w2.item()) <= 64 * ulp * w2.item(), i
        singles.append(got.item())
        sep1.append(g1.item())
        sep2.append(g2.item())
    # B = 4: the mean of the four B = 1 calls, exactly for each directed term ...
    g1, g2 = ChamferDistanceSeperatePadded()(xt, yt)
    assert g1.item() == float(np.float32(np.mean(np.float64(sep1)))) and g2.item() == float(np.float32(np.mean(np.float64(sep2))))
    # ... and for their sum to the roundings that differ: each single is fl(m1_i + m2_i), the batch value is
    # fl(fl(mean m1) + fl(mean m2)) -- at most one rounding per single and three on the batch side, 4 * 2^-24
    got = ChamferDistancePadded()(xt, yt).item()
    assert got == (g1 + g2).item()
    print(f"B = 4: padded {got:.9g}  mean of singles {np.mean(singles):.9g}")
    assert abs(got - np.mean(singles)) <= 4 * ulp * np.mean(singles)
    # the padding really is left out: the reference's B > 1 behaviour (flag ignored) gives another value
    assert abs(float(ChamferDistance(ignore_zeros=True)(xt, yt)) - got) > 1e-2 * got
    # differentiable down to the unpacked input, zero at padding rows
    xg = xt.clone().requires_grad_(True)
    ChamferDistancePadded()(xg, yt).backward()
    zero_rows = torch.from_numpy((x.sum(axis=2) == 0)).to(dev)
    assert not xg.grad[zero_rows].any() and xg.grad[~zero_rows].abs().sum() > 0


# ----------------------------------------------------------------------------------------------------------- metrics
def test_ragged_metrics_equal_per_sample_dense_calls(dev):
    from sparenet_amd.cuda.chamfer_distance import ChamferDistanceFunction
    from sparenet_amd.cuda.emd.emd_general import emd_general
    from sparenet_amd.cuda.ragged import emd_ragged
    from sparenet_amd.utils.metrics import fused_validation_metrics

    r = np.random.default_rng(10)
    gts = [_filler(r, k) for k in (2048, 1500, 2048, 900, 1)]
    preds = [(g[r.choice(len(g), k)] + r.standard_normal((k, 3)).astype(np.float32) * np.float32(0.004)).astype(np.float32)
             for g, k in zip(gts, (2048, 700, 1025, 900, 1))]
    x, l1 = _embed(preds, 2048, dev)
    y, l2 = _embed(gts, 2048, dev)
    out = fused_validation_metrics(x, y, th=0.01, emd_iters=20, with_emd=True, emd_any_size=True,
                                   pred_lengths=l1, gt_lengths=torch.tensor(l2, device=dev))
    d_all, _ = emd_ragged(x, y, l1, l2, 0.005, 20)
    th2 = 0.01 * 0.01
    for i, (p, q) in enumerate(zip(l1, l2)):
        xs, ys = x[i:i + 1, :p].contiguous(), y[i:i + 1, :q].contiguous()
        d1, d2 = ChamferDistanceFunction.apply(xs, ys)
        # float64 from identical fp32 distances: exact counts, and means that round once
        pr, rc = (d1 < th2).double().mean().item(), (d2 < th2).double().mean().item()
        f = 2 * pr * rc / (pr + rc) if pr + rc > 0 else 0.0
        assert out["F-Score"][i].item() == f, i
        cd = (d1.double().mean().float() + d2.double().mean().float()) * 1000
        assert out["ChamferDistance"][i].item() == cd.item(), i
        e, _ = emd_general(xs, ys, 0.005, 20)
        assert torch.equal(d_all[i, :p], e[0]), i                      # bit-equal per cloud before the mean
        assert out["EMD"][i].item() == (torch.sqrt(e).double().mean().float() * 100).item(), i
    assert 0 < out["F-Score"][0].item() < 1
    with pytest.raises(ValueError):
        fused_validation_metrics(x, y, with_emd=True, emd_any_size=True, pred_lengths=[2048] * 5, gt_lengths=l2)


# --------------------------------------------------------------------------------------------------- launched kernels
def _launches(lib, name, fn):
    lib.sn_prof_reset()
    lib.sn_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        lib.sn_prof_enable(0)
    ms = ctypes.c_double(0)
    count = lib.sn_prof_read(name.encode(), ctypes.byref(ms))
    lib.sn_prof_reset()
    return count


def test_ragged_calls_launch_the_ragged_kernels_and_never_the_persistent_auction(dev):
    import sparenet_amd
    from sparenet_amd.cuda.ragged import chamfer_ragged, emd_ragged

    lib = sparenet_amd.lib()
    x = torch.rand(2, 1024, 3, device=dev)
    y = torch.rand(2, 1024, 3, device=dev)
    full = [1024, 1024]                  # the shape the dense dispatch hands to the persistent auction
    emd = lambda: emd_ragged(x, y, full, full, 0.005, 7)
    assert _launches(lib, "emd_auction", emd) == 0
    assert _launches(lib, "emd_general_bid", emd) == 0
    assert _launches(lib, "emd_ragged_bid", emd) == 7
    cham = lambda: chamfer_ragged(x, y, full, full)
    assert _launches(lib, "chamfer_fwd", cham) == 0
    assert _launches(lib, "chamfer_fwd_ragged", cham) == 1
