"""What tests/test_dcd.py (host entry point) and tests/test_dcd_gpu.py (device) share: the clouds, their reference
(computed once per shape) and the comparison at the derived tolerances.

Tolerances.  sn_expf is within 2 ulp: a relative error <= 2^-22 of e; everything after it is double.  So
    |loss - ref|  <= 2^-22 * max W + 1e-12
    |g - g_ref|   <= 2^-21 * S     per component, S the sum of the absolute values of its contributions in the reference
                                   (2^-22 S for the exponential, 2^-24 S for the final rounding, slack for the double sums)
and counts, idx and dist are exact.  No case is excluded.  Both bounds speak of NORMAL fp32 numbers -- a subnormal e or
gradient has fewer bits than the ulp argument assumes -- so the clouds are scaled to keep alpha * dist <= 40
(e >= 4e-18); the underflow end (e == 0 below -104) has exact-value tests of its own."""
import functools

import numpy as np

import dcd_ref as ref

SHAPES = [(1, 1), (5, 3), (200, 130), (513, 64), (1025, 1025)]
RULES = [(n_lambda, ratio) for n_lambda in (0.0, 0.5, 1.0) for ratio in ("none", "size")]
ALPHA = {(1, 1): 40.0, (5, 3): 1000.0, (200, 130): 200.0, (513, 64): 1000.0, (1025, 1025): 1000.0}
BATCH = 3
MAX_ARGUMENT = 40.0
LOSS_REL, LOSS_ABS, GRAD_REL = 2.0 ** -22, 1e-12, 2.0 ** -21


def clouds(n, m, alpha, seed, batch=BATCH):
    """x [batch,n,3], y [batch,m,3] fp32 inside a cube whose squared diagonal times alpha is MAX_ARGUMENT.  Cloud 0:
    both uniform.  Cloud 1: y scattered around points of x (a trained generator's output).  Cloud 2: x crowded around
    the first few points of y, so that few targets are chosen by many points (long lists)."""
    rng = np.random.default_rng(seed)
    side = np.sqrt(MAX_ARGUMENT / (3.0 * alpha))
    x, y = rng.random((batch, n, 3)), rng.random((batch, m, 3))
    if batch > 1:
        y[1] = np.clip(x[1][rng.integers(0, n, m)] + 0.02 * rng.standard_normal((m, 3)), 0.0, 1.0)
    if batch > 2:
        x[2] = np.clip(y[2][rng.integers(0, min(m, 3), n)] + 0.01 * rng.standard_normal((n, 3)), 0.0, 1.0)
    return (x * side).astype(np.float32), (y * side).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(n, m):
    """(x, y, alpha, [the search of each cloud]) of a shape of SHAPES: computed once, never modified."""
    alpha = ALPHA[(n, m)]
    x, y = clouds(n, m, alpha, seed=n * 7919 + m)
    found = [ref.search(x[i], y[i]) for i in range(len(x))]
    for a in (x, y) + tuple(t for f in found for t in f):
        a.setflags(write=False)
    assert max(float(f[k].max()) for f in found for k in (0, 2)) * alpha <= MAX_ARGUMENT
    return x, y, alpha, found


def check_cloud(out, want, label):
    """`out` = (sides [2] float64, count1, count2, grad1 [n,3], grad2 [m,3]) of one cloud as NumPy arrays, `want` the
    dict of dcd_ref.dcd.  Every figure is printed before anything is asserted."""
    sides, count1, count2, grad1, grad2 = out
    loss = 0.5 * (float(sides[0]) + float(sides[1]))
    loss_err, loss_tol = abs(loss - want["loss"]), LOSS_REL * want["max_w"] + LOSS_ABS
    side_err = np.abs(np.asarray(sides, np.float64) - want["sides"]).max()
    rows = []
    for name, g, gref, total in (("grad1", grad1, want["grad1"], want["abs1"]), ("grad2", grad2, want["grad2"], want["abs2"])):
        err, tol = np.abs(g.astype(np.float64) - gref), GRAD_REL * total
        worst = float((err / np.where(tol > 0, tol, 1.0)).max())      # in units of the bound; a zero bound wants 0
        rows.append((name, float(err.max()), worst, bool((err <= tol).all())))
    print(f"{label}: loss {loss:.12g} ref {want['loss']:.12g} err {loss_err:.3g} tol {loss_tol:.3g}; sides err {side_err:.3g}; "
          + "; ".join(f"{n} max err {e:.3g} worst err/tol {w:.3g}" for n, e, w, _ in rows))
    assert np.array_equal(count1, want["count1"]) and np.array_equal(count2, want["count2"]), f"{label}: counts"
    assert loss_err <= loss_tol, f"{label}: loss {loss} against {want['loss']}"
    assert side_err <= loss_tol,f"{label}: sides {sides} against {want['sides']}"
    for name, _, _, ok in rows:
        assert ok, f"{label}: {name} outside 2^-21 S"
    assert 0.0 <= loss <= 1.0 + LOSS_ABS or want["max_w"] > 1.0, f"{label}: loss {loss} outside [0, 1]"


def ragged_batch():
    """B = 5, widths 300 / 260, lengths (300,260), (1,260), (300,1), (0,10), (17,0), NaN in the padding."""
    lengths1, lengths2 = [300, 1, 300, 0, 17], [260, 260, 1, 10, 0]
    x, y = clouds(300, 260, 1000.0, seed=77, batch=5)
    for i, (a, b) in enumerate(zip(lengths1, lengths2)):
        x[i, a:] = np.nan
        y[i, b:] = np.nan
    return x, y, lengths1, lengths2


def run(x, y, alpha, n_lambda, ratio, device, lengths1=None, lengths2=None):
    """density_aware_chamfer on `device` through autograd with an upstream gradient of 1 per cloud: (value [B] fp32,
    raw dict, gradxyz1, gradxyz2), all NumPy."""
    import torch

    from sparenet_amd.cuda.dcd import density_aware_chamfer

    xt = torch.tensor(x, device=device).requires_grad_(True)
    yt = torch.tensor(y, device=device).requires_grad_(True)
    value, raw = density_aware_chamfer(xt, yt, alpha, n_lambda, ratio, lengths1, lengths2, return_raw=True)
    value.sum().backward()
    return (value.detach().cpu().numpy(), {k: v.cpu().numpy() for k, v in raw.items()}, xt.grad.cpu().numpy(),
            yt.grad.cpu().numpy())


def check_shape_against_ref(n, m, n_lambda, ratio, device):
    """One shape of SHAPES under one rule on `device` against dcd_ref, cloud by cloud; returns run()'s outputs."""
    x, y, alpha, found = case(n, m)
    value, raw, g1, g2 = run(x, y, alpha, n_lambda, ratio, device)
    for i in range(len(x)):
        dist1, idx1, dist2, idx2 = found[i]
        # the search's outputs are the Chamfer op's, and those the reference's, bit for bit
        assert np.array_equal(raw["idx1"][i], idx1) and np.array_equal(raw["idx2"][i], idx2)
        assert np.array_equal(raw["dist1"][i], dist1) and np.array_equal(raw["dist2"][i], dist2)
        want = ref.dcd(x[i], y[i], alpha, n_lambda, ratio, found=found[i])
        check_cloud((raw["sides"][i], raw["count1"][i], raw["count2"][i], g1[i], g2[i]), want,
                    f"{n}x{m} cloud {i} n_lambda {n_lambda} ratio {ratio}")
        # the double value is rounded once
        assert value[i] == np.float32(0.5 * (raw["sides"][i, 0] + raw["sides"][i, 1]))
    return value, raw, g1, g2


def check_ragged(device):
    """Every cloud of the ragged batch equals the dense call on its slice bit for bit; shared with the GPU test."""
    x, y, lengths1, lengths2 = ragged_batch()
    for n_lambda, ratio in ((1.0, "none"), (0.5, "size")):
        value, raw, g1, g2 = run(x, y, 1000.0, n_lambda, ratio, device, lengths1, lengths2)
        assert not np.isnan(value).any() and not np.isnan(raw["sides"]).any()
        assert not np.isnan(g1).any() and not np.isnan(g2).any()
        for i, (a, b) in enumerate(zip(lengths1, lengths2)):
            assert (g1[i, a:] == 0.0).all() and (g2[i, b:] == 0.0).all(), "padding gradients"
            assert (raw["count1"][i, a:] == 0).all() and (raw["count2"][i, b:] == 0).all()
            assert (raw["idx1"][i, a:] == -1).all() and (raw["idx2"][i, b:] == -1).all()
            if a == 0 or b == 0:
                assert value[i] == 0.0 and (raw["sides"][i] == 0.0).all()
                assert (g1[i] == 0.0).all() and (g2[i] == 0.0).all()
                assert (raw["count1"][i] == 0).all() and (raw["count2"][i] == 0).all()
                continue
            dv, draw, dg1, dg2 = run(x[i:i + 1, :a], y[i:i + 1, :b], 1000.0, n_lambda, ratio, device)
            assert value[i] == dv[0] and np.array_equal(raw["sides"][i], draw["sides"][0])
            assert np.array_equal(g1[i, :a], dg1[0]) and np.array_equal(g2[i, :b], dg2[0])
            for key, cut in (("count1", a), ("dist1", a), ("idx1", a), ("count2", b), ("dist2", b), ("idx2", b)):
                assert np.array_equal(raw[key][i, :cut], draw[key][0]), key
