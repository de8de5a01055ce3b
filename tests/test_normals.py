"""Normal estimation without a GPU: the header and its binding, every refusal, the host entry point
(sn_local_pca_host, through local_pca on CPU tensors) against the NumPy reference (tests/local_pca_ref.py) at the
derived tolerances of tests/local_pca_cases.py, and the torch-level metrics on CPU tensors.  tests/test_normals_gpu.py
runs the kernel on the same cases and compares it with this host path."""
import ctypes
import os

import numpy as np
import pytest
import torch

import local_pca_cases as cases
import local_pca_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ops", "local_pca.h")
NAMES = ["sn_local_pca", "sn_local_pca_host", "sn_local_pca_workspace_bytes"]
DATA = ["xyz", "idx", "b", "n", "m", "k", "new_xyz", "viewpoint", "eigenvalues", "frames", "normals"]
CPU = torch.device("cpu")


# ------------------------------------------------------------------------------------------ header and binding
def test_header_and_exports():
    from sparenet_amd import _lib

    protos = _lib.prototypes(HEADER)
    assert sorted(protos) == NAMES
    assert [p.name for p in protos["sn_local_pca"][1]] == DATA + ["workspace", "workspace_bytes", "stream"]
    assert protos["sn_local_pca"][1][-1] == _lib.Param("stream", "void", True, False)
    assert _lib.Param("eigenvalues", "double", True, False) in protos["sn_local_pca"][1]
    assert [p.name for p in protos["sn_local_pca_host"][1]] == DATA + ["threads"]
    assert protos["sn_local_pca_workspace_bytes"][0] == "size_t"
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name), f"{name} declared in include/ops/local_pca.h but not exported"
    assert _lib.op_headers()["local_pca"] == HEADER
    assert sorted(_lib._op_calls["local_pca"]) == NAMES
    assert _lib.signature("sn_local_pca") == DATA + ["workspace"]
    assert _lib.signature("sn_local_pca_host") == DATA + ["threads"]
    assert L.sn_abi_version() == 4
    for shape in ((32, 16384, 16384, 16), (1, 1, 1, 64), (0, 0, 0, 0)):
        assert _lib.op_call("local_pca", "sn_local_pca_workspace_bytes", *shape) == 0


def test_library_refuses_bad_arguments():
    import sparenet_amd

    L = sparenet_amd.lib()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(8)      # `one` is never dereferenced: validation fails first

    def data(b=2, n=8, m=4, k=3, **pointers):
        p = {"xyz": one, "idx": one, "new_xyz": null, "viewpoint": null, "eigenvalues": one, "frames": one, "normals": one}
        p.update(pointers)
        return (p["xyz"], p["idx"], b, n, m, k, p["new_xyz"], p["viewpoint"], p["eigenvalues"], p["frames"], p["normals"])

    def device(**kw):
        return L.sn_local_pca(*data(**kw), null, ctypes.c_size_t(0), null)

    def host(**kw):
        return L.sn_local_pca_host(*data(**kw), 1)

    for fn in (device, host):
        def refused(text, **kw):
            assert fn(**kw) == -22
            assert text in L.sn_last_error(), L.sn_last_error()

        for size in ("b", "n", "m"):
            refused(b">= 1", **{size: 0})
            refused(b">= 1", **{size: -3})
        refused(b"too large", b=1 << 16, m=1 << 15)
        for k in (0, -1, 65, 1 << 20):
            refused(b"k must be in 1..64", k=k)
        refused(b"null pointer", xyz=null)
        refused(b"null pointer", idx=null)
        refused(b"no output", eigenvalues=null, frames=null, normals=null)
        refused(b"a viewpoint needs new_xyz", viewpoint=one)


def test_wrapper_refuses_bad_arguments_before_the_library_is_called(monkeypatch):
    from sparenet_amd import _lib
    from sparenet_amd.cuda import normals
    from sparenet_amd.utils import metrics

    def no_call(*a, **k):
        raise AssertionError("the library was called")

    for name in ("op_call", "op_workspace", "call"):
        monkeypatch.setattr(_lib, name, no_call)
    x, idx = torch.zeros(2, 8, 3), torch.zeros(2, 4, 3, dtype=torch.int32)
    for bad in (torch.zeros(2, 8, 2), torch.zeros(8, 3), torch.zeros(2, 0, 3), torch.zeros(0, 8, 3)):
        with pytest.raises(ValueError, match=r"\[B, N, 3\]"):
            normals.local_pca(bad, idx)
    with pytest.raises(TypeError, match="floating-point"):
        normals.local_pca(x.int(), idx)
    with pytest.raises(TypeError, match="int32 / int64"):
        normals.local_pca(x, idx.float())
    for bad in (torch.zeros(3, 4, 3, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, 0, 3, dtype=torch.int32)):
        with pytest.raises(ValueError, match=r"\[B, M, k\]"):
            normals.local_pca(x, bad)
    for k in (0, 65):
        with pytest.raises(ValueError, match=r"k must be in 1\.\.64"):
            normals.local_pca(x, torch.zeros(2, 4, k, dtype=torch.int32))
    with pytest.raises(ValueError, match="a viewpoint needs new_xyz"):
        normals.local_pca(x, idx, viewpoint=[0.0, 0.0, 1.0])
    with pytest.raises(ValueError, match=r"viewpoint must be \[3\] or \[2, 3\]"):
        normals.local_pca(x, idx, new_xyz=torch.zeros(2, 4, 3), viewpoint=torch.zeros(3, 3))
    with pytest.raises(ValueError, match=r"new_xyz must be a \[2, 4, 3\] tensor"):
        normals.local_pca(x, idx, new_xyz=torch.zeros(2, 5, 3), viewpoint=[0.0, 0.0, 1.0])
    y = torch.zeros(2, 4, 3)
    for fn in (normals.normal_consistency, metrics.normal_consistency, normals.point_to_plane_chamfer):
        rest = (y,) if fn is normals.point_to_plane_chamfer else ()
        with pytest.raises(ValueError, match=r"\[B, N, 3\]"):
            fn(torch.zeros(2, 8, 2), y, *rest)
        with pytest.raises(ValueError, match="batch sizes differ"):
            fn(x, torch.zeros(3, 4, 3), *rest)
    with pytest.raises(ValueError, match="normals2"):
        normals.point_to_plane_chamfer(x, y, None)
    with pytest.raises(ValueError, match="normals2 must be a floating-point tensor of its cloud's shape"):
        normals.point_to_plane_chamfer(x, y, torch.zeros(2, 5, 3))
    with pytest.raises(ValueError, match="normals1 must be"):
        normals.normal_consistency(x, y, torch.zeros(2, 7, 3), y)


def test_cpu_tensors_raise_where_there_is_no_host_search():
    import sparenet_amd
    from sparenet_amd.cuda.normals import estimate_normals, normal_consistency
    from sparenet_amd.utils.metrics import fused_validation_metrics

    x = torch.rand(1, 32, 3)
    with pytest.raises(sparenet_amd.SparenetHipError, match="expected a CUDA"):
        estimate_normals(x, 8)
    with pytest.raises(sparenet_amd.SparenetHipError, match="expected a CUDA"):
        normal_consistency(x, x)
    with pytest.raises(sparenet_amd.SparenetHipError, match="expected a CUDA"):
        fused_validation_metrics(x, x, with_emd=False, with_normals=True)
    assert sparenet_amd.estimate_normals is estimate_normals


# ------------------------------------------------------------------------------------------ the host entry point
@pytest.mark.parametrize("m", cases.MS)
def test_host_shapes(m):
    cases.check_shapes(m, CPU)


def test_host_named_clouds():
    cases.check_named_clouds(CPU)
    print("worst figures on the host:", cases.WORST)


def test_host_degenerate_geometry():
    cases.check_degenerate(CPU)


def test_host_tables_with_holes():
    cases.check_holes(CPU)


def test_host_skips_out_of_range_indices_without_reading():
    """n and -7 in the empty slots: skipped as -1 is.  Host only: on the device such slots point at nothing we own."""
    x, idx = cases.cloud("a"), cases.holes_table()
    want = cases.run(x, idx, CPU)
    rng = np.random.default_rng(3)
    bad = idx.copy()
    bad[idx < 0] = np.where(rng.random((idx < 0).sum()) < 0.5, len(x), -7)
    bad[0, :4] = [len(x), 1 << 30, -(1 << 31), -2]
    assert cases.same_bits(cases.run(x, bad, CPU), want)
    # the cloud sits at the end of its buffer: a read through the index n would leave it
    assert cases.same_bits(cases.run(x[:1000].copy(), np.where(idx >= 1000, 1000, idx), CPU),
                           cases.run(x[:1000].copy(), np.where(idx >= 1000, -1, idx), CPU))


def test_host_queries_other_than_the_points():
    cases.check_queries_apart(CPU)


def test_host_signs_and_viewpoints():
    cases.check_signs(CPU)


def test_host_threads_and_nullable_outputs():
    from sparenet_amd import _lib

    x, table = cases.batch_of(257)
    idx = np.ascontiguousarray(table[:, :, :16])
    want = cases.run(x, idx, CPU)
    xt, it = torch.tensor(x), torch.tensor(idx)
    for threads in (1, 2, 7):
        for keep in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
            values = torch.full((3, 257, 3), np.nan, dtype=torch.float64) if keep[0] else None
            frames = torch.full((3, 257, 3, 3), np.nan) if keep[1] else None
            normals = torch.full((3, 257, 3), np.nan) if keep[2] else None
            _lib.op_call("local_pca", "sn_local_pca_host", xt, it, 3, 257, 257, 16, None, None, values, frames, normals,
                         threads, host=True)
            assert values is None or np.array_equal(values.numpy().view(np.uint64), want[1].view(np.uint64))
            assert frames is None or np.array_equal(frames.numpy().view(np.uint32), want[2].view(np.uint32))
            assert normals is None or np.array_equal(normals.numpy().view(np.uint32), want[0].view(np.uint32))


def test_int64_tables_and_other_dtypes():
    from sparenet_amd.cuda.normals import local_pca

    x, idx = cases.cloud("d"), cases.self_table("d", 8)
    want = cases.run(x, idx, CPU)
    got = local_pca(torch.tensor(x, dtype=torch.float64)[None].requires_grad_(True), torch.tensor(idx, dtype=torch.int64)[None],
                    return_frames=True)
    assert not any(t.requires_grad for t in got)
    assert cases.same_bits(tuple(t[0].numpy() for t in got), want)
    assert len(local_pca(torch.tensor(x)[None], torch.tensor(idx)[None])) == 2


# ------------------------------------------------------------------------------------------ the metrics on CPU tensors
def test_surface_variation():
    from sparenet_amd.cuda.normals import surface_variation

    values = torch.tensor([[0.0, 0.0, 0.0], [0.0, 1.0, 3.0], [1.0, 1.0, 2.0], [2.0, 2.0, 2.0]], dtype=torch.float64)
    assert torch.equal(surface_variation(values), torch.tensor([0.0, 0.0, 0.25, 1.0 / 3.0], dtype=torch.float64))
    x, idx = cases.cloud("c"), cases.self_table("c", 16)
    w = cases.run(x, idx, CPU)[1]
    assert np.array_equal(surface_variation(torch.tensor(w)).numpy(), ref.surface_variation(w))
    flat, noisy = cases.run(cases.cloud("b"), cases.self_table("b", 16), CPU)[1], w
    assert ref.surface_variation(flat).mean() < ref.surface_variation(noisy).mean()


def _reference_normals(name, k=16):
    return ref.local_pca(cases.cloud(name), cases.self_table(name, k))["normals"].astype(np.float32)


def test_normal_consistency_on_cpu_tensors():
    from sparenet_amd.cuda.normals import normal_consistency
    from sparenet_amd.utils import metrics

    b, inner, d = cases.cloud("b"), cases.cloud("sphere45"), cases.cloud("d")
    nb, ni, nd = _reference_normals("b"), _reference_normals("sphere45"), _reference_normals("d", 8)
    t = lambda a: torch.tensor(a)[None]      # noqa: E731
    same = normal_consistency(t(b), t(b), t(nb), t(nb))
    assert same.dtype == torch.float32 and abs(same.item() - 1.0) <= 2.0 ** -22
    spheres = normal_consistency(t(b), t(inner), t(nb), t(ni)).item()
    idx1, idx2 = ref.chamfer_indices(b, inner)
    want = ref.normal_consistency(nb, ni, idx1, idx2)
    worst = min(np.abs((nb.astype(np.float64) * ni[idx1]).sum(axis=1)).min(), np.abs((ni.astype(np.float64) * nb[idx2]).sum(axis=1)).min())
    print(f"concentric spheres: {spheres:.9g} ref {want:.9g}, cos of the worst angle {worst:.9g}")
    assert spheres == np.float32(want) and spheres >= worst
    plane = metrics.normal_consistency(t(b), t(d), pred_normals=t(nb), gt_normals=t(nd)).item()
    idx1, idx2 = ref.chamfer_indices(b, d)
    assert plane == np.float32(ref.normal_consistency(nb, nd, idx1, idx2)) and plane < spheres
    # the sign of a normal does not enter
    assert normal_consistency(t(b), t(inner), t(-nb), t(ni)).item() == spheres
    # ragged rows equal the per-cloud call; padding may hold NaN; an empty side gives 0
    x = np.full((3, 2048, 3), np.nan, np.float32)
    y, n1, n2 = x.copy(), x.copy(), x.copy()
    lengths1, lengths2 = [2048, 700, 0], [1000, 2048, 5]
    x[0], n1[0], y[0, :1000], n2[0, :1000] = b, nb, d, nd
    x[1, :700], n1[1, :700], y[1], n2[1] = inner[:700], ni[:700], b, nb
    y[2, :5], n2[2, :5] = b[:5], nb[:5]
    got = normal_consistency(torch.tensor(x), torch.tensor(y), torch.tensor(n1), torch.tensor(n2), lengths1=lengths1,
                             lengths2=lengths2)
    assert got[0].item() == plane and got[2].item() == 0.0
    assert got[1].item() == normal_consistency(t(inner[:700]), t(b), t(ni[:700]), t(nb)).item()


def test_point_to_plane_chamfer_on_cpu_tensors():
    cases.check_point_to_plane(CPU)
    from sparenet_amd.cuda.normals import point_to_plane_chamfer

    # ragged: rows past a length may hold NaN, get gradient 0 and do not enter the value
    b, d, nd = cases.cloud("b"), cases.cloud("d"), _reference_normals("d", 8)
    x = torch.full((2, 2048, 3), float("nan"))
    y, n2 = torch.full((2, 1000, 3), float("nan")), torch.full((2, 1000, 3), float("nan"))
    x[0], y[0], n2[0] = torch.tensor(b), torch.tensor(d), torch.tensor(nd)
    x[1, :300], y[1, :50], n2[1, :50] = torch.tensor(b[:300]), torch.tensor(d[:50]), torch.tensor(nd[:50])
    x.requires_grad_(True)
    got = point_to_plane_chamfer(x, y, n2, [2048, 300], [1000, 50])
    got.sum().backward()
    assert torch.isfinite(got).all() and torch.isfinite(x.grad).all() and (x.grad[1, 300:] == 0).all()
    for i, (a, c) in enumerate(((2048, 1000), (300, 50))):
        xi = x.detach()[i:i + 1, :a].clone().requires_grad_(True)
        alone = point_to_plane_chamfer(xi, y[i:i + 1, :c], n2[i:i + 1, :c])
        alone.sum().backward()
        assert abs(alone.item() - got[i].item()) <= 4 * 2.0 ** -24 * alone.item()
        assert torch.allclose(xi.grad[0], x.grad[i, :a], rtol=1e-5, atol=1e-9)
    empty = point_to_plane_chamfer(x.detach(), y, n2, [0, 300], [1000, 0])
    assert (empty == 0).all()
