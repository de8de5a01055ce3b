"""Recipes and float64 references shared by tests/golden/gen_fpd.py and the FPD tests.

A full PointNetCls(k=16) is 14 MB, too large for a fixture, and the pretrained classifier is not available, so the
weights are a RECIPE: every tensor of the state dict, in sorted key order, from np.random.RandomState(seed) (the
legacy generator: its stream is frozen across numpy versions).  Running means and variances are non-trivial and about
a quarter of the batch-norm weights are NEGATIVE, so a mistake in folding batch norm or in the order of max and ReLU
shows.  The fixtures hold only results; generator and tests both build weights and clouds here.
"""
import numpy as np

# state_dict() of the reference's PointNetCls(k=16), recorded from the reference class (key -> shape)
_BN = lambda p, c: {f"{p}.weight": (c,), f"{p}.bias": (c,), f"{p}.running_mean": (c,), f"{p}.running_var": (c,),  # noqa: E731
                    f"{p}.num_batches_tracked": ()}
_LAYER = lambda p, shape: {f"{p}.weight": shape, f"{p}.bias": shape[:1]}  # noqa: E731
STATE_SHAPES = {}
for _p in ("feat.stn.", "feat."):
    STATE_SHAPES.update(_LAYER(_p + "conv1", (64, 3, 1)))
    STATE_SHAPES.update(_LAYER(_p + "conv2", (128, 64, 1)))
    STATE_SHAPES.update(_LAYER(_p + "conv3", (1024, 128, 1)))
    STATE_SHAPES.update(_BN(_p + "bn1", 64))
    STATE_SHAPES.update(_BN(_p + "bn2", 128))
    STATE_SHAPES.update(_BN(_p + "bn3", 1024))
STATE_SHAPES.update(_LAYER("feat.stn.fc1", (512, 1024)))
STATE_SHAPES.update(_LAYER("feat.stn.fc2", (256, 512)))
STATE_SHAPES.update(_LAYER("feat.stn.fc3", (9, 256)))
STATE_SHAPES.update(_BN("feat.stn.bn4", 512))
STATE_SHAPES.update(_BN("feat.stn.bn5", 256))
STATE_SHAPES.update(_LAYER("fc1", (512, 1024)))
STATE_SHAPES.update(_LAYER("fc2", (256, 512)))
STATE_SHAPES.update(_LAYER("fc3", (16, 256)))
STATE_SHAPES.update(_BN("bn1", 512))
STATE_SHAPES.update(_BN("bn2", 256))

WEIGHT_SEED = 20240521


def recipe_state_dict(seed=WEIGHT_SEED):
    """{key: numpy array} for every key of STATE_SHAPES, in sorted key order from one RandomState(seed)."""
    rs = np.random.RandomState(seed)
    out = {}
    for key in sorted(STATE_SHAPES):
        shape = STATE_SHAPES[key]
        leaf = key.rsplit(".", 1)[1]
        is_bn = ".bn" in "." + key
        if leaf == "num_batches_tracked":
            v = np.array(1 + rs.randint(0, 1000), np.int64)
        elif leaf == "running_mean":
            v = (0.2 * rs.standard_normal(shape)).astype(np.float32)
        elif leaf == "running_var":
            v = rs.uniform(0.5, 2.0, shape).astype(np.float32)
        elif is_bn and leaf == "weight":
            v = (rs.uniform(0.5, 1.5, shape) * np.where(rs.uniform(size=shape) < 0.25, -1.0, 1.0)).astype(np.float32)
        elif leaf == "bias":
            v = (0.1 * rs.standard_normal(shape)).astype(np.float32)
        else:   # conv / linear weight: unit gain (fc3 of the transform net small, so trans stays near identity + noise)
            fan_in = int(np.prod(shape[1:]))
            gain = 0.3 if key == "feat.stn.fc3.weight" else 1.4
            v = (gain / np.sqrt(fan_in) * rs.standard_normal(shape)).astype(np.float32)
        out[key] = v
    return out


def load_recipe(model, seed=WEIGHT_SEED):
    """load the recipe into a PointNetCls (the reference's or the package's), strict; returns the model in eval mode"""
    import torch

    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in recipe_state_dict(seed).items()}, strict=True)
    return model.eval()


def clouds(kind, count, n, seed):
    """[count, n, 3] float32.  'cube': uniform in [-0.5, 0.5]^3; 'slab': an anisotropic noisy slab
    (0.9 x 0.5 x 0.06, rotated, with 5 % far outliers) -- two distributions whose FPD is far from zero."""
    rs = np.random.RandomState(seed)
    if kind == "cube":
        return (rs.uniform(-0.5, 0.5, (count, n, 3))).astype(np.float32)
    assert kind == "slab"
    p = rs.uniform(-0.5, 0.5, (count, n, 3)) * np.array([0.9, 0.5, 0.06])
    p += 0.01 * rs.standard_normal((count, n, 3))
    far = rs.uniform(size=(count, n, 1)) < 0.05
    p = np.where(far, rs.uniform(-0.6, 0.6, (count, n, 3)), p)
    c, s = np.cos(0.6), np.sin(0.6)
    rot = np.array([[c, -s, 0.0], [s, c * 0.8, -0.6], [0.0, 0.6, 0.8]])
    return (p @ rot).astype(np.float32)


# the fixture cases: name -> (set1 kind, set2 kind or None, clouds per set, points, batch_size, seed)
CASES = {
    "a": ("cube", "slab", 50, 1000, 15, 11),    # 45 used: pins the dropped remainder; 1000 is no multiple of a tile
    "b": ("cube", "slab", 24, 2048, 12, 12),
    "c": ("slab", None, 4, 16384, 4, 13),       # activations only
}


def case_clouds(name):
    k1, k2, count, n, _, seed = CASES[name]
    return clouds(k1, count, n, seed), (clouds(k2, count, n, seed + 100) if k2 else None)


# ---------------------------------------------------------------- the fused op in float64, with its error bound
U = 2.0 ** -24


def gamma(k):
    return k * U / (1 - k * U)


def op_inputs(b, n, seed, with_trans):
    """xyz [b,n,3], trans [b,3,3] or None, folded-style weights (some rows negated), all float32"""
    rs = np.random.RandomState(seed)
    f = lambda *s: rs.standard_normal(s).astype(np.float32)  # noqa: E731
    xyz = rs.uniform(-0.5, 0.5, (b, n, 3)).astype(np.float32)
    trans = (np.eye(3, dtype=np.float32) + 0.3 * f(b, 3, 3)) if with_trans else None
    w = (1.5 * f(64, 3), 0.2 * f(64), 1.4 / 8 * f(128, 64), 0.2 * f(128), 1.4 / np.sqrt(128).astype(np.float32) * f(1024, 128),
         0.2 * f(1024))
    return xyz, trans, tuple(np.ascontiguousarray(a, np.float32) for a in w)


def pool_ref64(xyz, trans, w, relu_last, chunk=2048):
    """float64 value of sn_pointnet_pool_forward and the worst-case forward error bound of its fp32 fma chains:
    gamma_k = k u / (1 - k u), u = 2^-24, propagated through the layers from |W| |h|;
    |max_i a_i - max_i b_i| <= max_i |a_i - b_i| carries it through the pool (ReLU is 1-Lipschitz).
    Returns (out64 [b,1024], err [b,1024])."""
    w1, b1, w2, b2, w3, b3 = (np.asarray(a, np.float64) for a in w)
    bsz, n, _ = xyz.shape
    out = np.full((bsz, 1024), -np.inf)
    err = np.zeros((bsz, 1024))
    for c in range(bsz):
        for p0 in range(0, n, chunk):
            x = xyz[c, p0:p0 + chunk].astype(np.float64)           # [p, 3]
            if trans is not None:
                t = trans[c].astype(np.float64)
                ex = gamma(3) * (np.abs(x) @ np.abs(t))
                x = x @ t
            else:
                ex = np.zeros_like(x)
            a1 = x @ w1.T + b1
            e1 = gamma(4) * (np.abs(x) @ np.abs(w1).T + np.abs(b1)) + ex @ np.abs(w1).T
            h1 = np.maximum(a1, 0)
            a2 = h1 @ w2.T + b2
            e2 = gamma(65) * (h1 @ np.abs(w2).T + np.abs(b2)) + e1 @ np.abs(w2).T
            h2 = np.maximum(a2, 0)
            a3 = h2 @ w3.T + b3
            e3 = gamma(129) * (h2 @ np.abs(w3).T + np.abs(b3)) + e2 @ np.abs(w3).T
            if relu_last:
                a3 = np.maximum(a3, 0)
            out[c] = np.maximum(out[c], a3.max(axis=0))
            err[c] = np.maximum(err[c], e3.max(axis=0))
    return out, err


def fpd_allowance(act1, act2, d=1808):
    """2 d sqrt(2^-52 |S1|_2 |S2|_2): the reference's sqrtm turns a rounding error eps on a zero eigenvalue of the
    rank-deficient product S1 S2 into sqrt(eps) in the trace."""
    def norm2(a):
        x = (a - a.mean(axis=0)) / np.sqrt(a.shape[0] - 1)
        return np.linalg.norm(x, 2) ** 2
    return 2 * d * np.sqrt(2.0 ** -52 * norm2(np.asarray(act1, np.float64)) * norm2(np.asarray(act2, np.float64)))
