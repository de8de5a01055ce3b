"""sn_set_emd_sums (sparenet_amd/csrc/set_emd.hip) on the GPU through emd_direction_sums / emd_matrix / set_metrics.

Oracle for a pair of clouds: tests/emd_general_ref.py, the NumPy restatement of sn_emd_forward_general.  The kernel's
assignment must equal the oracle's exactly; dist is then the same fp32 expression on the same operands and its square
root the same correctly rounded fp32 number, so both sides add the same n non-negative doubles, each in some order:
each is within (n - 1) 2^-53 of the exact sum relative to it, hence |got - want| <= n 2^-52 want.  That bound is the
tolerance (a zero sum: equality).  want[i, j] = sum of np.sqrt(dist).astype(float64).

Measured on an MI355X: the difference was 0 in every entry of every case below, the emd_general loop beyond 2048
points included ("Set-level EMD matrix")."""
import numpy as np
import pytest
import torch

import emd_general_ref as E
import set_metrics_ref as R

pytestmark = pytest.mark.gpu

EPS = 0.005


def _uniform(shape, seed):
    """(x [nx, n, 3], y [ny, m, 3]) uniform in the unit cube, on the host."""
    nx, ny, n, m = shape
    g = torch.Generator().manual_seed(seed)
    return torch.rand(nx, n, 3, generator=g), torch.rand(ny, m, 3, generator=g)


def _contested(shape, seed):
    """Targets on a sphere of radius 0.5, bidders = targets + uniform noise in [-1, 1]^3 (smoke()'s construction):
    hundreds of bidders per near-side target -- evictions, the window, stale window winners."""
    nx, ny, n, m = shape
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(ny, m, 3, generator=g)
    y = 0.5 * y / y.norm(dim=2, keepdim=True)
    base = y[torch.arange(nx) % ny, :n]
    x = (base + 2 * torch.rand(nx, n, 3, generator=g) - 1).contiguous()
    return x, y.contiguous()


def _oracle(x, y, eps, iters):
    """{k: (want [nx, ny] float64, assignment [nx, ny, n] int32)} for every k of `iters`, from one pass of the
    restatement over all pairs."""
    x, y = x.numpy(), y.numpy()
    nx, n, _ = x.shape
    ny, m, _ = y.shape
    xe = np.repeat(x, ny, axis=0)
    ye = np.tile(y, (nx, 1, 1))
    res = E.emd_general(xe, ye, eps, list(iters))
    return {k: (np.sqrt(d).astype(np.float64).sum(axis=1).reshape(nx, ny), a.reshape(nx, ny, n))
            for k, (d, a, _) in res.items()}


def _assert_pairs(got_sums, got_assign, want, want_assign, n, what):
    got, asg = got_sums.cpu().numpy(), got_assign.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == want.shape, (what, got.dtype, got.shape)
    assert asg.dtype == np.int32 and asg.shape == want_assign.shape, (what, asg.dtype, asg.shape)
    wrong = np.argwhere(asg != want_assign)
    assert wrong.size == 0, f"{what}: {len(wrong)} assignments differ, first at (i, j, bidder) = {tuple(wrong[0])}: " \
                            f"got {asg[tuple(wrong[0])]}, oracle {want_assign[tuple(wrong[0])]}"
    err = np.abs(got - want)
    bound = n * 2.0 ** -52 * want
    print(f"{what}: max |got - want| / want = {np.max(err / np.maximum(want, 1e-300)):.3e}, bound {n * 2.0 ** -52:.3e}")
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    assert (err <= bound).all(), f"{what}: entry {worst}: got {got[worst]!r}, want {want[worst]!r}, bound {bound[worst]!r}"


def _check(dev, x, y, eps, iters, what):
    from sparenet_amd.cuda.set_distance import emd_direction_sums

    want = _oracle(x, y, eps, iters)
    xd, yd = x.to(dev), y.to(dev)
    for k in iters:
        sums, assignment = emd_direction_sums(xd, yd, eps, k, return_assignment=True)
        _assert_pairs(sums, assignment, want[k][0], want[k][1], x.size(1), f"{what}, {k} iterations")
        # the metrics' call, without the assignment: the same bits
        assert torch.equal(emd_direction_sums(xd, yd, eps, k), sums), (what, k)


# ------------------------------------------------------------------------------------------ case 1: small shapes
@pytest.mark.parametrize("n,m", [(1, 1), (1, 5), (5, 5), (63, 64), (64, 200)], ids=lambda v: str(v))
def test_small_shapes(dev, n, m):
    x, y = _uniform((3, 4, n, m), 100 + n + m)
    _check(dev, x, y, EPS, [0, 1, 2, 50], f"3 x 4 of ({n}, {m})")


def test_negative_eps(dev):
    x, y = _uniform((3, 4, 64, 200), 7)
    _check(dev, x, y, -0.001, [3], "3 x 4 of (64, 200), eps -0.001")


def test_no_iterations_leave_every_bidder_unassigned(dev):
    from sparenet_amd.cuda.set_distance import emd_direction_sums

    x, y = _uniform((3, 4, 63, 64), 8)
    sums, assignment = emd_direction_sums(x.to(dev), y.to(dev), EPS, 0, return_assignment=True)
    assert (assignment == -1).all() and (sums == 0.0).all()


# --------------------------------------------------------------------- case 2: tie geometry and the LDS cap
BIG = [(1024, 1024), (1025, 1500), (2047, 2048), (2048, 2048)]


@pytest.mark.parametrize("n,m", BIG, ids=lambda v: str(v))
def test_tie_geometry_and_lds_cap_against_the_oracle(dev, n, m):
    x, y = _uniform((2, 2, n, m), 200 + n)
    _check(dev, x, y, EPS, [10], f"2 x 2 of ({n}, {m})")


@pytest.mark.parametrize("n,m", BIG, ids=lambda v: str(v))
def test_tie_geometry_and_lds_cap_against_emd_general(dev, n, m):
    """50 iterations against the op the project already has, one b = 1 call per pair."""
    from sparenet_amd.cuda.emd.emd_general import emd_general
    from sparenet_amd.cuda.set_distance import emd_direction_sums

    x, y = _uniform((2, 2, n, m), 200 + n)
    xd, yd = x.to(dev), y.to(dev)
    sums, assignment = emd_direction_sums(xd, yd, EPS, 50, return_assignment=True)
    want = np.empty((2, 2), np.float64)
    want_assign = np.empty((2, 2, n), np.int32)
    for i in range(2):
        for j in range(2):
            dist, a = emd_general(xd[i:i + 1], yd[j:j + 1], EPS, 50)
            want[i, j] = np.sqrt(dist.cpu().numpy()).astype(np.float64).sum()
            want_assign[i, j] = a.cpu().numpy()[0]
    _assert_pairs(sums, assignment, want, want_assign, n, f"2 x 2 of ({n}, {m}) against emd_general, 50 iterations")


# ------------------------------------------------------------------------------------ case 3: contested auction
@pytest.mark.parametrize("n,m", [(600, 1500), (2048, 2048)], ids=lambda v: str(v))
def test_contested_auction(dev, n, m):
    x, y = _contested((2, 2, n, m), 300 + n)
    _check(dev, x, y, EPS, [20], f"contested 2 x 2 of ({n}, {m})")


# ------------------------------------------------------------------------------------------- case 4: exact ties
def test_every_target_duplicated(dev):
    x, y = _uniform((2, 2, 256, 512), 400)
    y[:, 256:] = y[:, :256]
    _check(dev, x, y, EPS, [2, 50], "duplicated targets 2 x 2 of (256, 512)")


def test_a_set_against_itself(dev):
    """The diagonal is 0; [i, j] and [j, i] are two auctions, each matched against its own oracle -- nothing here
    asks them to be equal."""
    from sparenet_amd.cuda.set_distance import emd_direction_sums, emd_matrix

    x, _ = _uniform((3, 1, 512, 1), 401)
    _check(dev, x, x.clone(), EPS, [50], "3 x 3 of 512 against itself")
    xd = x.to(dev)
    sums = emd_direction_sums(xd, xd, EPS, 50)
    assert (sums.diagonal() == 0.0).all() and (sums > 0).sum().item() == 6
    assert (emd_matrix(xd, xd).diagonal() == 0.0).all()


# ----------------------------------------------------------------------- case 5: bit-equality, no oracle involved
def test_every_entry_is_its_own_1x1_call_and_two_calls_agree(dev):
    from sparenet_amd.cuda.set_distance import emd_direction_sums

    x, y = _uniform((5, 7, 300, 700), 500)
    xd, yd = x.to(dev), y.to(dev)
    first, first_assign = emd_direction_sums(xd, yd, EPS, 50, return_assignment=True)
    again, again_assign = emd_direction_sums(xd, yd, EPS, 50, return_assignment=True)
    assert torch.equal(first, again) and torch.equal(first_assign, again_assign)
    for i in range(5):
        for j in range(7):
            alone, a = emd_direction_sums(xd[i:i + 1].contiguous(), yd[j:j + 1].contiguous(), EPS, 50,
                                          return_assignment=True)
            assert alone.shape == (1, 1) and alone[0, 0].item() == first[i, j].item(), (i, j)
            assert torch.equal(a[0, 0], first_assign[i, j]), (i, j)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        other, other_assign = emd_direction_sums(xd, yd, EPS, 50, return_assignment=True)
    side.synchronize()
    assert torch.equal(first, other) and torch.equal(first_assign, other_assign)


# -------------------------------------------------------------------------- case 6: emd_matrix and the metrics
def test_emd_matrix_swaps_and_transposes(dev):
    from sparenet_amd.cuda.set_distance import emd_direction_sums, emd_matrix

    x, y = _uniform((3, 2, 400, 150), 600)
    xd, yd = x.to(dev), y.to(dev)
    got = emd_matrix(xd, yd, EPS, 50)
    assert got.shape == (3, 2) and got.dtype == torch.float64
    # the quotient as numpy takes it on the host: a correctly rounded float64 division
    assert np.array_equal(got.cpu().numpy(), emd_direction_sums(yd, xd, EPS, 50).cpu().numpy().T / 150)
    assert np.array_equal(emd_matrix(yd, xd, EPS, 50).cpu().numpy(), got.cpu().numpy().T)


def test_emd_matrix_beyond_the_kernel_takes_the_loop(dev):
    from sparenet_amd.cuda.set_distance import emd_direction_sums, emd_matrix

    n, m = 700, 2304
    x, y = _uniform((2, 2, n, m), 601)
    want, want_assign = _oracle(x, y, EPS, [50])[50]
    xd, yd = x.to(dev), y.to(dev)
    sums, assignment = emd_direction_sums(xd, yd, EPS, 50, return_assignment=True)
    _assert_pairs(sums, assignment, want, want_assign, n, f"loop 2 x 2 of ({n}, {m})")
    got = emd_matrix(xd, yd, EPS, 50).cpu().numpy()
    assert (np.abs(got - want / n) <= n * 2.0 ** -52 * (want / n) + 2.0 ** -53 * (want / n)).all()      # + the division


def test_set_metrics_with_emd(dev):
    from sparenet_amd.utils import set_metrics as M

    G, Rn, n = 6, 5, 256
    gen, ref = _uniform((G, Rn, n, n), 2025)
    gen = gen * (0.6 + 0.08 * torch.arange(G).view(G, 1, 1))       # clouds of different extent: distinct distances
    ref = ref * (0.62 + 0.09 * torch.arange(Rn).view(Rn, 1, 1))

    def oracle_matrix(a, b):
        return _oracle(a, b, EPS, [50])[50][0] / n

    gg, gr, rr = oracle_matrix(gen, gen), oracle_matrix(gen, ref), oracle_matrix(ref, ref)
    # the condition under which no summation order can flip a decision: every arg-min is won by far more than the
    # matrices' rounding (n 2^-52 = 5.7e-14 relative).  Checked on the oracle's matrices alone.
    gaps = R.argmin_gaps(gg, gr, rr)
    assert gaps.min() > 1e-9, gaps.min()
    got = M.set_metrics(gen.to(dev), ref.to(dev), with_emd=True)
    assert list(got) == ["MMD-CD", "COV-CD", "1-NNA-CD", "MMD-EMD", "COV-EMD", "1-NNA-EMD"]
    assert all(v.dtype == torch.float64 and v.dim() == 0 and v.device.type == "cuda" for v in got.values())
    t = torch.from_numpy
    assert got["COV-EMD"].item() == M.coverage(t(gr)).item() == R.cov(gr)
    assert got["1-NNA-EMD"].item() == M.one_nn_accuracy(t(gg), t(gr), t(rr)).item() == R.one_nna(gg, gr, rr)
    want = M.minimum_matching_distance(t(gr)).item()
    print(f"MMD-EMD: got {got['MMD-EMD'].item()!r}, oracle {want!r}")
    assert abs(got["MMD-EMD"].item() - want) <= 1e-12 * want
    # the reference set's own matrix, computed before; other auction parameters reach the kernel
    from sparenet_amd.cuda.set_distance import emd_matrix
    again = M.set_metrics(gen.to(dev), ref.to(dev), with_emd=True, emd_rr=emd_matrix(ref.to(dev), ref.to(dev)))
    assert all(again[k].item() == got[k].item() for k in got)
    few = M.set_metrics(gen.to(dev), ref.to(dev), with_emd=True, emd_iters=1)
    assert few["MMD-EMD"].item() != got["MMD-EMD"].item()


def test_refusals_name_the_argument(dev):
    from sparenet_amd import SparenetHipError
    from sparenet_amd.cuda.set_distance import emd_direction_sums, emd_matrix

    x = torch.rand(2, 8, 3, device=dev)
    with pytest.raises(SparenetHipError, match="^y: .*no CPU path"):
        emd_direction_sums(x, x.cpu())
    with pytest.raises(SparenetHipError, match="^x: .*no CPU path"):
        emd_matrix(x.cpu(), x)
    with pytest.raises(ValueError, match="^y: "):
        emd_matrix(x, torch.rand(2, 8, 2, device=dev))
    with pytest.raises(TypeError, match="^x: "):
        emd_direction_sums(x.double(), x)
    with pytest.raises(ValueError, match="pass the smaller clouds first"):
        emd_direction_sums(torch.rand(2, 9, 3, device=dev), x)
