"""The occupancy grid and the Jensen-Shannon divergence without a GPU: the header and its binding, every refusal, the
host entry point (sn_occupancy_grid_host, through occupancy_grid on CPU tensors) against the NumPy reference
(tests/occupancy_ref.py) in EXACT equality on the cases of tests/occupancy_cases.py, and the float64 metric functions of
sparenet_amd.utils.set_metrics.  tests/test_occupancy_gpu.py runs the kernel on the same cases and compares it with
this host path bit for bit.

Measured ("Occupancy grid and JSD"): jensen_shannon_divergence on CPU tensors stays within 4.4e-3 of the
derived bound of occupancy_cases.jsd_bound over every pair of grids below (3.6e-4 on the 28^3 grids)."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

import occupancy_cases as cases
import occupancy_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ops", "occupancy.h")
NAMES = ["sn_occupancy_grid", "sn_occupancy_grid_host", "sn_occupancy_grid_workspace_bytes"]
DATA = ["xyz", "lengths", "s", "n", "res", "in_sphere", "counts", "occupied", "cells"]
CPU = torch.device("cpu")


# ------------------------------------------------------------------------------------------ header and binding
def test_header_and_exports():
    from sparenet_amd import _lib

    protos = _lib.prototypes(HEADER)
    assert sorted(protos) == NAMES
    assert [p.name for p in protos["sn_occupancy_grid"][1]] == DATA + ["workspace", "workspace_bytes", "stream"]
    assert protos["sn_occupancy_grid"][1][-1] == _lib.Param("stream", "void", True, False)
    assert _lib.Param("counts", "long long", True, False) in protos["sn_occupancy_grid"][1]
    assert [p.name for p in protos["sn_occupancy_grid_host"][1]] == DATA + ["threads"]
    assert protos["sn_occupancy_grid_workspace_bytes"][0] == "size_t"
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name), f"{name} declared in include/ops/occupancy.h but not exported"
    assert _lib.op_headers()["occupancy"] == HEADER
    assert sorted(_lib._op_calls["occupancy"]) == NAMES
    assert _lib.signature("sn_occupancy_grid") == DATA + ["workspace"]
    assert L.sn_abi_version() == 4
    size = lambda *shape: _lib.op_call("occupancy", "sn_occupancy_grid_workspace_bytes", *shape)  # noqa: E731
    assert size(1024, 2048, 28, 1) == (10144 * 4 + 255) // 256 * 256
    assert size(1024, 2048, 28, 0) == 0 and size(1, 1, 2, 1) == 0 and size(1, 1, 0, 1) == 0 and size(1, 1, 33, 1) == 0
    import sparenet_amd

    assert sparenet_amd.occupancy_grid is __import__("sparenet_amd.cuda.occupancy", fromlist=["x"]).occupancy_grid


def test_library_refuses_bad_arguments():
    import sparenet_amd

    L = sparenet_amd.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(8)      # `one` is never dereferenced: validation fails first

    def data(s=2, n=8, res=28, in_sphere=1, **pointers):
        p = {"xyz": one, "lengths": null, "counts": one, "occupied": one, "cells": one}
        p.update(pointers)
        return (p["xyz"], p["lengths"], s, n, res, in_sphere, p["counts"], p["occupied"], p["cells"])

    def device(**kw):
        return L.sn_occupancy_grid(*data(**kw), null, ctypes.c_size_t(0), null)

    def host(**kw):
        return L.sn_occupancy_grid_host(*data(**kw), 1)

    for fn in (device, host):
        def refused(text, **kw):
            assert fn(**kw) == -22
            assert text in L.sn_last_error(), L.sn_last_error()

        for res in (1, 0, -5, 33, 1 << 20):
            refused(b"res must be in 2..32", res=res)
            refused(b"res must be in 2..32", res=res, in_sphere=0)
        refused(b"no cell of the grid lies in the sphere", res=2)
        for size in ("s", "n"):
            refused(b">= 1", **{size: 0})
            refused(b">= 1", **{size: -3})
        refused(b"too large", s=1 << 16, n=1 << 15)
        refused(b"null pointer", xyz=null)
        refused(b"no output", counts=null, occupied=null, cells=null)
    # the device entry point alone has a workspace: with the sphere it holds the list of in-sphere cells
    assert L.sn_occupancy_grid(*data(), null, ctypes.c_size_t(0), null) == -22
    assert b"workspace too small" in L.sn_last_error()
    assert L.sn_occupancy_grid(*data(), one, ctypes.c_size_t(10144 * 4 - 1), null) == -22
    assert b"workspace too small" in L.sn_last_error()


def test_wrapper_refusals_and_the_bindings_error_text():
    from sparenet_amd import SparenetHipError, _lib
    from sparenet_amd.cuda.occupancy import occupancy_grid

    x = torch.zeros(2, 8, 3)
    with pytest.raises(SparenetHipError, match="no cell of the grid lies in the sphere at res = 2"):
        occupancy_grid(x, 2)
    assert int(occupancy_grid(x, 2, in_sphere=False)[0].sum()) == 16
    for res in (1, 33, 2.5):
        with pytest.raises(ValueError, match="resolution"):
            occupancy_grid(x, res)
    for bad in (torch.zeros(8, 3), torch.zeros(2, 8, 2), torch.zeros(0, 8, 3), torch.zeros(2, 0, 3)):
        with pytest.raises(ValueError, match=r"\[S, n, 3\]"):
            occupancy_grid(bad)
    with pytest.raises(TypeError, match="floating-point"):
        occupancy_grid(torch.zeros(2, 8, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="lengths must be in"):
        occupancy_grid(x, lengths=[1, 9])
    with pytest.raises(ValueError, match="expected 2 lengths"):
        occupancy_grid(x, lengths=[1])
    # every SN_EINVAL reaches Python as the binding's error with the library's text
    counts = torch.zeros(28 ** 3, dtype=torch.int64)
    for args, text in (((x, None, 2, 8, 40, 1, counts, None, None, 0), "res must be in 2..32"),
                       ((x, None, 0, 8, 28, 1, counts, None, None, 0), ">= 1"),
                       ((x, None, 2, 0, 28, 1, counts, None, None, 0), ">= 1"),
                       ((x, None, 1 << 16, 1 << 15, 28, 1, counts, None, None, 0), "too large"),
                       ((None, None, 2, 8, 28, 1, counts, None, None, 0), "null pointer"),
                       ((x, None, 2, 8, 28, 1, None, None, None, 0), "no output")):
        with pytest.raises(SparenetHipError, match=text):
            _lib.op_call("occupancy", "sn_occupancy_grid_host", *args, host=True)
    # double and half inputs are read as fp32; a gradient does not pass
    y = (torch.rand(2, 8, 3) - 0.5).requires_grad_(True)
    out = occupancy_grid(y.double(), return_cells=True)
    assert all(not t.requires_grad for t in out) and torch.equal(out[2], occupancy_grid(y.detach(), return_cells=True)[2])


# ------------------------------------------------------------------------------------------ the host entry point
def test_reference_agrees_with_a_plain_brute_force():
    """The reference itself: Rule 1 + Rule 2 against the nearest in-sphere centre in plain float64, wherever that is
    unique -- uniform in the ball and in a cube of side 1.3, at res 5 and 28."""
    rng = np.random.default_rng(1)
    pts = np.concatenate([cases.ball(rng, 1, 400)[0], ((rng.random((300, 3)) - 0.5) * 1.3).astype(np.float32)])
    for res in (5, 28):
        got, rule2 = ref.cells_of(pts, res, True)
        want, unique = ref.brute_force_cells(pts, res)
        print(f"res {res}: {int(unique.sum())} of {len(pts)} points have a unique nearest centre; Rule 2 decided {int(rule2.sum())}")
        assert unique.sum() >= 0.95 * len(pts) and rule2.sum() >= 100
        assert np.array_equal(got[unique], want[unique])


@pytest.mark.parametrize("name", cases.CLOUD_CASES)
def test_host_case(name):
    out = cases.check_case(name, CPU)
    cases.check_case_details(name, CPU, out)


def test_host_zero_is_a_midpoint_at_res_28():
    cases.check_zero_points(CPU)


def test_host_rule_2_is_ordinary_traffic():
    assert 0.01 <= cases.reference("ball28")["rule2"] <= 0.08 and cases.reference("ball32")["rule2"] >= 0.01
    assert cases.reference("cube28")["rule2"] >= 0.5 and cases.reference("cube5")["rule2"] >= 0.3
    assert cases.reference("ball28cube")["rule2"] == 0


def test_host_permutation_threads_and_null_outputs():
    cases.check_permutation("many", CPU)
    cases.check_permutation("ball28", CPU)
    cases.check_null_outputs(CPU)
    xyz, res, sphere, lengths = cases.case("ragged")
    want = cases.run(xyz, res, sphere, CPU, lengths)
    assert cases.same(cases.run(xyz, res, sphere, CPU, torch.tensor(lengths)), want)      # lengths as a tensor
    assert cases.same(cases.run(xyz, res, sphere, CPU, torch.tensor(lengths, dtype=torch.int32)), want)


# ------------------------------------------------------------------------------------------ the metric functions
def test_in_sphere_cells():
    from sparenet_amd.utils.set_metrics import in_sphere_cells

    assert in_sphere_cells(28) == 10144
    assert in_sphere_cells(2) == 0 and in_sphere_cells(3) == 7 and in_sphere_cells(32) == int(ref.sphere_mask(32).sum())
    for res in cases.BOUNDARY_RES:
        assert in_sphere_cells(res) == int(ref.sphere_mask(res).sum())
        assert len(cases.boundary_cells(res)[1]) == 6
    a = 2 * np.arange(28) - 27
    assert not (a[:, None, None] ** 2 + a[None, :, None] ** 2 + a[None, None, :] ** 2 == 729).any()
    with pytest.raises(ValueError):
        in_sphere_cells(1)


def _grids():
    """Pairs of count grids: the cases' own, random sparse ones, and small hand-made ones."""
    rng = np.random.default_rng(3)
    pairs = [(cases.reference("ball28")["counts"], cases.reference("cube28")["counts"]),
             (cases.reference("many")["counts"], cases.reference("wide")["counts"]),
             (cases.reference("many")["counts"], cases.reference("onecell")["counts"])]
    for cells, fill, top in ((28 ** 3, 0.4, 50), (28 ** 3, 0.02, 5), (125, 0.9, 100000), (8, 1.0, 3)):
        p = rng.integers(1, top + 1, cells) * (rng.random(cells) < fill)
        q = rng.integers(1, top + 1, cells) * (rng.random(cells) < fill)
        p[0] += 1
        q[-1] += 1
        pairs.append((p.astype(np.int64), q.astype(np.int64)))
    return pairs


def test_jensen_shannon_divergence():
    from sparenet_amd.utils.set_metrics import jensen_shannon_divergence as jsd

    worst = 0.0
    for p, q in _grids():
        tp, tq = torch.tensor(p), torch.tensor(q)
        got = jsd(tp, tq)
        assert got.dtype == torch.float64 and got.dim() == 0 and 0.0 <= got.item() <= 1.0
        want, bound = ref.jsd(p, q), cases.jsd_bound(p, q)
        err = abs(got.item() - want)
        worst = max(worst, err / bound)
        print(f"JSD {got.item():.17g} ref {want:.17g} err {err:.3g} bound {bound:.3g} ({err / bound:.3g} of it)")
        assert err <= bound
        assert got.item() == jsd(tq, tp).item(), "symmetric bit for bit"
        for scale in (2, 4):
            assert jsd(tp * scale, tq).item() == got.item() and jsd(tp, tq * scale).item() == got.item()
        assert jsd(tp, tp).item() == 0.0 and jsd(tq, tq * 4).item() == 0.0
        assert jsd(tp.reshape(-1, 1), tq.reshape(-1, 1)).item() == got.item() and jsd(tp.double(), tq.float()).item() == got.item()
    print(f"worst fraction of the derived bound: {worst:.3g}")
    # disjoint supports: one bit
    p = torch.tensor([3, 0, 5, 0, 0, 1])
    q = torch.tensor([0, 2, 0, 7, 9, 0])
    assert abs(jsd(p, q).item() - 1.0) <= cases.jsd_bound(p.numpy(), q.numpy())
    assert jsd(torch.tensor([4, 0]), torch.tensor([0, 9])).item() == 1.0
    with pytest.raises(ValueError, match="positive total"):
        jsd(torch.zeros(5), p[:5])
    with pytest.raises(ValueError, match="shapes differ"):
        jsd(p, q[:5])


def test_occupancy_entropy():
    from sparenet_amd.utils.set_metrics import in_sphere_cells, occupancy_entropy

    ln2 = float(np.log(2.0))
    half = occupancy_entropy(torch.full((5, 5, 5), 4, dtype=torch.int32), 8, 125)
    assert half.dtype == torch.float64 and abs(half.item() - ln2) <= 130 * 2.0 ** -53 * ln2      # a sum of 125 equal terms
    assert occupancy_entropy(torch.tensor([0, 8, 8, 0]), 8, 4).item() == 0.0
    assert abs(occupancy_entropy(torch.tensor([4, 0, 8, 0]), 8, 4).item() - ln2 / 4) <= 2.0 ** -53      # one term, one log
    quarter = -(0.25 * np.log(0.25) + 0.75 * np.log(0.75))
    assert abs(occupancy_entropy(torch.tensor([2, 6]), 8, 2).item() - quarter) <= 8 * 2.0 ** -53
    occupied = torch.tensor(cases.reference("many")["occupied"])
    got = occupancy_entropy(occupied, 700, in_sphere_cells(28)).item()
    want = ref.occupancy_entropy(occupied.numpy(), 700, 10144)
    assert want > 0 and abs(got - want) <= (10144 + 10) * 2.0 ** -53 * want      # a sum of at most 10144 positive terms
    with pytest.raises(ValueError):
        occupancy_entropy(torch.tensor([9]), 8, 1)
    with pytest.raises(ValueError):
        occupancy_entropy(torch.tensor([1]), 0, 1)


def test_jsd_between_sets_on_cpu_tensors():
    """The whole path on CPU tensors (the host entry point): equal to the metric of two grids, ref_counts, the warning."""
    from sparenet_amd.cuda.occupancy import occupancy_grid
    from sparenet_amd.utils import metrics
    from sparenet_amd.utils.set_metrics import jensen_shannon_divergence, jsd_between_sets

    rng = np.random.default_rng(9)
    gen, gt = torch.tensor(cases.ball(rng, 5, 257)), torch.tensor(cases.ball(rng, 7, 257, radius=0.4))
    with warnings.catch_warnings():
        warnings.simplefilter("error")      # nothing leaves the sphere: no warning
        value = jsd_between_sets(gen, gt)
        grid = occupancy_grid(gt)[0]
        assert value.item() == jensen_shannon_divergence(occupancy_grid(gen)[0], grid).item()
        assert jsd_between_sets(gen, None, ref_counts=grid).item() == value.item()
        assert metrics.jsd(gen, gt).item() == value.item() and metrics.jsd(gen, gt, gt_counts=grid).item() == value.item()
        assert jsd_between_sets(gen, gen).item() == 0.0 and 0.0 < value.item() < 1.0
        cube = jsd_between_sets(gen * 0.5, gt * 0.5, resolution=9, in_sphere=False)
        assert cube.item() == jensen_shannon_divergence(occupancy_grid(gen * 0.5, 9, False)[0], occupancy_grid(gt * 0.5, 9, False)[0]).item()
        padded = torch.cat([gen, torch.full((5, 3, 3), float("nan"))], dim=1)
        assert jsd_between_sets(padded, gt, gen_lengths=[257] * 5).item() == value.item()
    with pytest.warns(UserWarning, match="outside the unit sphere"):
        jsd_between_sets(gen * 2, gt)
    with pytest.warns(UserWarning, match="outside the unit sphere"):
        jsd_between_sets(gen, gt * 2)
    with pytest.warns(UserWarning, match="outside the unit cube"):
        jsd_between_sets(gen * 2, gt, in_sphere=False)
    corner = torch.full((1, 4, 3), 0.45)      # inside the cube, outside the sphere
    with pytest.warns(UserWarning, match="outside the unit sphere"):
        jsd_between_sets(corner, gt)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        jsd_between_sets(corner, gt, in_sphere=False)
