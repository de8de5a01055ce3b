"""The occupancy grid on the GPU: the kernel against the NumPy reference (tests/occupancy_ref.py) and against the host
entry point, in EXACT equality of cells, counts and occupied on every case of tests/occupancy_cases.py -- the rule of
include/ops/occupancy.h is integer and fully specified -- for several launch sizes, and the Jensen-Shannon divergence
built on it end to end.  Every comparison prints its figures (`pytest -s`).

Measured on an MI355X ("Occupancy grid and JSD"): zero differing cells in every case, device against the
reference and against the host entry point; jensen_shannon_divergence on the device within 1.4e-4 of the derived bound
of occupancy_cases.jsd_bound.  Timings (tools/jsd_time.py, two sets of 1024 x 2048, res 28): sn_occupancy_grid 0.165 ms
per set on uniform balls, 0.455 ms on shells touching the sphere; jsd_between_sets 0.90 / 1.49 ms; the torch composite
237 / 239 ms."""
import warnings

import numpy as np
import pytest
import torch

import occupancy_cases as cases
import occupancy_ref as ref

pytestmark = pytest.mark.gpu

CPU = torch.device("cpu")


# ------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("name", cases.CLOUD_CASES)
def test_device_case_and_host_bits(dev, name):
    out = cases.check_case(name, dev)
    cases.check_case_details(name, dev, out)
    xyz, res, sphere, lengths = cases.case(name)
    assert cases.same(out, cases.run(xyz, res, sphere, CPU, lengths)), f"{name}: device against host"


def test_device_zero_is_a_midpoint_at_res_28(dev):
    cases.check_zero_points(dev)


@pytest.mark.parametrize("blocks", [1, 3, 64])
def test_device_any_number_of_workgroups(dev, blocks):
    """One workgroup for the whole set, three, and 64: the outputs do not depend on the launch."""
    for name in ("many", "cube28", "ragged", "wide"):
        xyz, res, sphere, lengths = cases.case(name)
        out = cases.with_blocks(blocks, lambda: cases.run(xyz, res, sphere, dev, lengths))
        cases.check(out, xyz, res, sphere, cases.reference(name), lengths, f"{name}, {blocks} workgroups")
        assert cases.same(out, cases.run(xyz, res, sphere, dev, lengths))


def test_device_permutation_and_null_outputs(dev):
    cases.check_permutation("many", dev)
    cases.check_permutation("ball28", dev)
    cases.check_null_outputs(dev)
    xyz, res, sphere, lengths = cases.case("ragged")
    want = cases.run(xyz, res, sphere, dev, lengths)
    assert cases.same(cases.run(xyz, res, sphere, dev, torch.tensor(lengths, device=dev)), want)      # not read on the host


def test_device_every_resolution(dev):
    """Every res of the header on one set that leaves the sphere: the list of in-sphere cells the device builds for
    itself, the LDS carve at every size, against the host entry point."""
    rng = np.random.default_rng(77)
    xyz = ((rng.random((3, 130, 3)) - 0.5) * 1.2).astype(np.float32)
    for res in range(2, 33):
        for sphere in ((False,) if res == 2 else (True, False)):
            assert cases.same(cases.run(xyz, res, sphere, dev), cases.run(xyz, res, sphere, CPU)), f"res {res} sphere {sphere}"
    out = cases.run(xyz, 31, True, dev)
    cases.check(out, xyz, 31, True, ref.occupancy_grid(xyz, 31, True), None, "res 31")


def test_device_refusals_carry_the_librarys_text(dev):
    from sparenet_amd import SparenetHipError, _lib
    from sparenet_amd.cuda.occupancy import occupancy_grid

    x = torch.zeros(2, 8, 3, device=dev)
    with pytest.raises(SparenetHipError, match="no cell of the grid lies in the sphere at res = 2"):
        occupancy_grid(x, 2)
    counts = torch.zeros(28 ** 3, dtype=torch.int64, device=dev)
    ws = _lib.op_workspace("occupancy", "sn_occupancy_grid_workspace_bytes", x, 2, 8, 28, 1)
    small = _lib.Workspace(ws.tensor, ws.nbytes - 1)
    for args, text in (((x, None, 2, 8, 40, 1, counts, None, None, ws), "res must be in 2..32"),
                       ((x, None, 0, 8, 28, 1, counts, None, None, ws), ">= 1"),
                       ((x, None, 2, 0, 28, 1, counts, None, None, ws), ">= 1"),
                       ((x, None, 1 << 16, 1 << 15, 28, 1, counts, None, None, ws), "too large"),
                       ((None, None, 2, 8, 28, 1, counts, None, None, ws), "null pointer"),
                       ((x, None, 2, 8, 28, 1, None, None, None, ws), "no output"),
                       ((x, None, 2, 8, 28, 1, counts, None, None, small), "workspace too small"),
                       ((x, None, 2, 8, 28, 1, counts, None, None, None), "workspace too small")):
        with pytest.raises(SparenetHipError, match=text):
            _lib.op_call("occupancy", "sn_occupancy_grid", *args)
    assert int(counts.sum()) == 0, "a refused call writes nothing"


# ------------------------------------------------------------------------------------------ end to end
def _sets(dev):
    rng = np.random.default_rng(9)
    return torch.tensor(cases.ball(rng, 5, 257), device=dev), torch.tensor(cases.ball(rng, 7, 257, radius=0.4), device=dev)


def test_jsd_between_sets(dev):
    from sparenet_amd.cuda.occupancy import occupancy_grid
    from sparenet_amd.utils import metrics
    from sparenet_amd.utils.set_metrics import jensen_shannon_divergence, jsd_between_sets

    gen, gt = _sets(dev)
    with warnings.catch_warnings():
        warnings.simplefilter("error")      # both sets lie inside the sphere: no warning
        value = jsd_between_sets(gen, gt)
        grid = occupancy_grid(gt)[0]
        assert value.is_cuda and value.dtype == torch.float64
        assert value.item() == jensen_shannon_divergence(occupancy_grid(gen)[0], grid).item()
        assert jsd_between_sets(gen, None, ref_counts=grid).item() == value.item(), "ref_counts against recomputing"
        assert metrics.jsd(gen, gt).item() == value.item() and metrics.jsd(gen, gt, gt_counts=grid).item() == value.item()
        assert jsd_between_sets(gen, gen).item() == 0.0
    # the grids are the host's bits; the metric on the device against NumPy at the derived bound
    p, q = occupancy_grid(gen)[0], grid
    assert torch.equal(p.cpu(), occupancy_grid(gen.cpu())[0]) and torch.equal(q.cpu(), occupancy_grid(gt.cpu())[0])
    worst = 0.0
    pairs = [(p.cpu().numpy(), q.cpu().numpy())] + [(cases.reference(a)["counts"], cases.reference(b)["counts"])
                                                    for a, b in (("ball28", "cube28"), ("many", "wide"), ("many", "onecell"))]
    for a, b in pairs:
        ta, tb = torch.tensor(a, device=dev), torch.tensor(b, device=dev)
        got, want, bound = jensen_shannon_divergence(ta, tb).item(), ref.jsd(a, b), cases.jsd_bound(a, b)
        worst = max(worst, abs(got - want) / bound)
        print(f"JSD on the device {got:.17g} ref {want:.17g} err {abs(got - want):.3g} bound {bound:.3g}")
        assert abs(got - want) <= bound
        assert got == jensen_shannon_divergence(tb, ta).item() and jensen_shannon_divergence(ta * 2, tb * 4).item() == got
        assert jensen_shannon_divergence(ta, ta).item() == 0.0
    print(f"worst fraction of the derived bound on the device: {worst:.3g}")
    with pytest.warns(UserWarning, match="outside the unit sphere"):
        jsd_between_sets(gen * 2, gt)


def test_set_metrics_with_jsd(dev):
    from sparenet_amd.cuda.occupancy import occupancy_grid
    from sparenet_amd.utils.set_metrics import jsd_between_sets, set_metrics

    gen, gt = _sets(dev)
    plain = set_metrics(gen, gt)
    off = set_metrics(gen, gt, with_jsd=False, jsd_resolution=9, ref_counts=None)
    flagged = set_metrics(gen, gt, with_jsd=True)
    assert sorted(plain) == sorted(off) == ["1-NNA-CD", "COV-CD", "MMD-CD"]
    assert sorted(flagged) == ["1-NNA-CD", "COV-CD", "JSD", "MMD-CD"]
    for key in plain:
        assert torch.equal(plain[key], off[key]) and torch.equal(plain[key], flagged[key]), key
    assert flagged["JSD"].item() == jsd_between_sets(gen, gt).item()
    given = set_metrics(gen, gt, with_jsd=True, ref_counts=occupancy_grid(gt)[0])
    assert given["JSD"].item() == flagged["JSD"].item()
    coarse = set_metrics(gen, gt, with_jsd=True, jsd_resolution=9)
    assert coarse["JSD"].item() == jsd_between_sets(gen, gt, 9).item() != flagged["JSD"].item()
