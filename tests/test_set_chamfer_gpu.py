"""sn_set_chamfer_sums (sparenet_amd/csrc/set_chamfer.hip) on the GPU through chamfer_direction_sums / chamfer_matrix /
set_metrics.

Reference for a pair of clouds: what the project already trusts -- ChamferDistanceFunction on the pair (here: every
pair of the two sets expanded into one batch), its dist1 widened to float64 and summed.  The kernel's per-point minima
are bit for bit those dist1, so both sides add the same n non-negative doubles, each in some order: each is within
(n - 1) 2^-53 of the exact sum relative to it, hence |got - ref| <= (n - 1) 2^-52 ref.  That bound is the tolerance
(0 for n = 1 and for a zero sum: equality)."""
import os
import re

import numpy as np
import pytest
import torch

import set_metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _strip():
    """The strip length as built: a workgroup walks at most this many target clouds."""
    src = open(os.path.join(ROOT, "sparenet_amd", "csrc", "set_chamfer.hip")).read()
    consts = {k: int(v) for k, v in re.findall(r"constexpr int (kStrip|kFillBlocks) = (\d+);", src)}
    assert set(consts) == {"kStrip", "kFillBlocks"}, consts
    return consts["kStrip"], consts["kFillBlocks"]


S, FILL = _strip()

# (Nx, Ny, n, m)
SHAPES = [
    (1, 1, 1, 1),
    (3, 5, 7, 13),
    (2, 9, 256, 255),            # one short tile, odd chunk tail
    (4, 3, 2048, 2049),          # a full query block; a target tile boundary (two tiles and one point)
    (2, 2, 2049, 300),           # a second query block and the partial-sum kernel
    (2, 3, 1024, 1025),          # the last n of the 4-queries-per-lane instantiation; y -> x: the first n of the wide one
    (1, S + 1, 64, 64),
    (S + 1, 1, 64, 64),
    # small problems take shorter strips (so that the grid still fills the GPU): these two are large enough in pairs
    # of clouds for strips of S and of 2 target clouds, each with a last strip of one cloud
    (FILL * S // (16 * S + 1) + 1, 16 * S + 1, 8, 8),
    (16, FILL * 2 // 16 + 1, 8, 8),
]


def _sets(shape, seed, dev, scale=1.0, shift=0.0):
    nx, ny, n, m = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(nx, n, 3, generator=g) * scale + shift
    y = torch.rand(ny, m, 3, generator=g) * scale + shift
    return x.to(dev), y.to(dev)


def _pair_reference(x, y):
    """(S1, S2) float64 [Nx, Ny]: S1[i, j] = sum of dist1, S2[i, j] = sum of dist2 of ChamferDistanceFunction on
    (x_i, y_j)."""
    from sparenet_amd.cuda.chamfer_distance import ChamferDistanceFunction

    nx, ny = x.size(0), y.size(0)
    xe = x[:, None].expand(nx, ny, -1, -1).reshape(nx * ny, x.size(1), 3)
    ye = y[None, :].expand(nx, ny, -1, -1).reshape(nx * ny, y.size(1), 3)
    d1, d2 = ChamferDistanceFunction.apply(xe, ye)
    return d1.double().sum(dim=1).view(nx, ny), d2.double().sum(dim=1).view(nx, ny)


def _assert_within(got, ref, terms, what):
    got, ref = got.cpu().numpy(), ref.cpu().numpy()
    assert got.shape == ref.shape and got.dtype == np.float64, (what, got.shape, got.dtype)
    err = np.abs(got - ref)
    bound = (terms - 1) * 2.0 ** -52 * ref
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    print(f"{what}: max |got - ref| / ref = {np.max(err / np.maximum(ref, 1e-300)):.3e}, bound {(terms - 1) * 2.0 ** -52:.3e}")
    assert (err <= bound).all(), f"{what}: entry {worst}: got {got[worst]!r}, reference {ref[worst]!r}, bound {bound[worst]!r}"


_CASES = {}


def _case(shape, dev):
    """Sets and pair reference of a shape: computed once, shared by the tests, not modified."""
    if shape not in _CASES:
        x, y = _sets(shape, 1000 + SHAPES.index(shape), dev)
        _CASES[shape] = (x, y) + _pair_reference(x, y)
    return _CASES[shape]


def test_the_strip_cases_take_the_strips_they_are_meant_for():
    """Condition of SHAPES' last two rows, against the rule in set_chamfer.hip: strip = clamp(units / kFillBlocks, 1,
    kStrip), units = x clouds * query blocks * y clouds."""
    (nx, ny, _, _), (nx2, ny2, _, _) = SHAPES[-2:]
    assert S >= 2 and nx * ny // FILL >= S and ny % S == 1
    assert nx2 * ny2 // FILL == 2 and ny2 % 2 == 1


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_direction_sums_match_the_pairwise_chamfer(dev, shape):
    from sparenet_amd.cuda.set_distance import chamfer_direction_sums

    x, y, s1, s2 = _case(shape, dev)
    _assert_within(chamfer_direction_sums(x, y), s1, shape[2], f"{shape} x -> y")
    _assert_within(chamfer_direction_sums(y, x), s2.t(), shape[3], f"{shape} y -> x")


@pytest.mark.parametrize("shape", [(3, 5, 7, 13), (2, 2, 2049, 300)], ids=lambda s: "x".join(map(str, s)))
def test_chamfer_matrix_combines_both_directions(dev, shape):
    from sparenet_amd.cuda.set_distance import chamfer_direction_sums, chamfer_matrix

    x, y, _, _ = _case(shape, dev)
    # the quotients as numpy takes them on the host: correctly rounded float64 divisions
    want = chamfer_direction_sums(x, y).cpu().numpy() / shape[2] + chamfer_direction_sums(y, x).cpu().numpy().T / shape[3]
    got = chamfer_matrix(x, y)
    assert got.dtype == torch.float64 and np.array_equal(got.cpu().numpy(), want)


def test_coordinates_far_outside_the_unit_cube(dev):
    from sparenet_amd.cuda.set_distance import chamfer_direction_sums

    shape = (3, 4, 300, 257)
    x, y = _sets(shape, 7, dev, scale=100.0, shift=-50.0)
    s1, s2 = _pair_reference(x, y)
    _assert_within(chamfer_direction_sums(x, y), s1, 300, "[-50, 50] x -> y")
    _assert_within(chamfer_direction_sums(y, x), s2.t(), 257, "[-50, 50] y -> x")


def test_duplicated_points_and_duplicated_clouds(dev):
    from sparenet_amd.cuda.set_distance import chamfer_direction_sums

    x, y = _sets((4, 5, 100, 100), 8, dev)
    x[:, 50:] = x[:, :50]         # every point twice
    x[3] = x[0]                   # a cloud twice
    y[:, 7] = y[:, 3]
    y[4] = y[1]
    y[2] = x[0]                   # a cloud of the other set
    s1, s2 = _pair_reference(x, y)
    got = chamfer_direction_sums(x, y)
    _assert_within(got, s1, 100, "duplicates x -> y")
    _assert_within(chamfer_direction_sums(y, x), s2.t(), 100, "duplicates y -> x")
    assert torch.equal(got[0], got[3]) and torch.equal(got[:, 4], got[:, 1])
    assert got[0, 2].item() == 0.0 and got[3, 2].item() == 0.0


def test_a_set_against_itself(dev, monkeypatch):
    from sparenet_amd import _lib
    from sparenet_amd.cuda.set_distance import chamfer_direction_sums, chamfer_matrix

    x, _ = _sets((7, 1, 300, 1), 9, dev)
    sums = chamfer_direction_sums(x, x)
    assert (sums.diagonal() == 0.0).all() and (sums > 0).sum().item() == 7 * 6
    launched = []
    real = _lib.ext_call
    monkeypatch.setattr(_lib, "ext_call", lambda name, *a: (launched.append(name), real(name, *a))[1])
    cd = chamfer_matrix(x, x)
    assert launched.count("sn_set_chamfer_sums") == 1
    assert torch.equal(cd, cd.t()) and (cd.diagonal() == 0.0).all()
    assert np.array_equal(cd.cpu().numpy(), sums.cpu().numpy() / 300 + sums.cpu().numpy().T / 300)
    del launched[:]
    assert torch.equal(chamfer_matrix(x, x.clone()), cd)       # two kernel calls, the same numbers
    assert launched.count("sn_set_chamfer_sums") == 2


def test_two_calls_are_bit_identical_and_every_entry_is_its_own_1x1_call(dev):
    from sparenet_amd.cuda.set_distance import chamfer_direction_sums

    x, y = _sets((4, 3, 2049, 300), 10, dev)
    first = chamfer_direction_sums(x, y)
    assert torch.equal(first, chamfer_direction_sums(x, y))
    for i in range(4):
        for j in range(3):
            alone = chamfer_direction_sums(x[i:i + 1].contiguous(), y[j:j + 1].contiguous())
            assert alone.shape == (1, 1) and alone[0, 0].item() == first[i, j].item(), (i, j)
    # ... also where the set call walks strips of several clouds: the first, a middle and the last (one-cloud) strip
    shape = SHAPES[-2]
    x, y, _, _ = _case(shape, dev)
    full = chamfer_direction_sums(x, y)
    assert torch.equal(full, chamfer_direction_sums(x, y))
    for i, j in ((0, 0), (1, S - 1), (shape[0] - 1, S), (5, shape[1] // 2), (shape[0] - 1, shape[1] - 1)):
        alone = chamfer_direction_sums(x[i:i + 1].contiguous(), y[j:j + 1].contiguous())
        assert alone[0, 0].item() == full[i, j].item(), (i, j)


def test_set_metrics_end_to_end(dev):
    from sparenet_amd.cuda.set_distance import chamfer_matrix
    from sparenet_amd.utils.metrics import set_metrics

    G, Rn, n = 6, 5, 128
    gen, ref = _sets((G, Rn, n, n), 2024, dev)

    def reference_matrix(a, b):
        s1, s2 = _pair_reference(a, b)
        return (s1 / a.size(1) + s2 / b.size(1)).cpu().numpy()

    gg, gr, rr = reference_matrix(gen, gen), reference_matrix(gen, ref), reference_matrix(ref, ref)
    # the condition under which no summation order can flip a decision: every arg-min is won by far more than the
    # matrices' rounding ((n - 1) 2^-52 = 2.8e-14 relative).  The seed was picked with the reference alone.
    gaps = R.argmin_gaps(gg, gr, rr)
    assert gaps.min() > 1e-9, gaps.min()
    got = set_metrics(gen, ref)
    assert set(got) == {"MMD-CD", "COV-CD", "1-NNA-CD"}
    assert all(v.dtype == torch.float64 and v.dim() == 0 for v in got.values())
    assert got["COV-CD"].item() == R.cov(gr)
    assert got["1-NNA-CD"].item() == R.one_nna(gg, gr, rr)
    want = R.mmd(gr)
    print(f"MMD-CD: got {got['MMD-CD'].item()!r}, reference {want!r}")
    assert abs(got["MMD-CD"].item() - want) <= (n - 1) * 2.0 ** -52 * want
    # the reference set's own matrix, computed before
    again = set_metrics(gen, ref, cd_rr=chamfer_matrix(ref, ref))
    assert all(again[k].item() == got[k].item() for k in got)


def test_refusals_name_the_argument(dev):
    from sparenet_amd import SparenetHipError
    from sparenet_amd.cuda.set_distance import chamfer_direction_sums, chamfer_matrix

    x = torch.rand(2, 8, 3, device=dev)
    with pytest.raises(SparenetHipError, match="^y: .*no CPU path"):
        chamfer_direction_sums(x, x.cpu())                      # a CPU tensor, and two devices
    with pytest.raises(SparenetHipError, match="^x: .*no CPU path"):
        chamfer_matrix(x.cpu(), x)
    with pytest.raises(ValueError, match="^y: "):
        chamfer_direction_sums(x, torch.rand(2, 8, 2, device=dev))
    with pytest.raises(ValueError, match="^x: "):
        chamfer_matrix(torch.rand(2, 8, 2, device=dev), x)
    with pytest.raises(TypeError, match="^x: "):
        chamfer_direction_sums(x.double(), x)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="^y is on cuda:1"):
            chamfer_direction_sums(x, x.to("cuda:1"))
