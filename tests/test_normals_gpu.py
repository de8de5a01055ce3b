"""Normal estimation on the GPU: the kernel against the NumPy reference (tests/local_pca_ref.py) at the derived
tolerances of tests/local_pca_cases.py, against the host entry point, and the metrics built on it.  Every comparison
with the reference prints its figures (`pytest -s`).

Measured on an MI355X ("Normal estimation"), worst over every case in units of the bound: eigenvalues 0.039
of E = 32 (k + 8) u T; residual 0.18 of E + 2^-22 T; the reference's own residual 0.040 of E; orthonormality 0.20 of
2^-21; sin(angle) of the normal 0.19 of 2 E / (l1 - l0) + 2^-22, signs equal in every judged row; the gap rule excludes
at most 0.78 % of a case's rows.  The device equals the host entry point in every bit of every case, so the tests
assert bit equality.  Timings (tools/normals_time.py, 32 x 16384, k = 16): sn_local_pca 0.102 ms, sn_knn_query 4.42 ms,
estimate_normals 4.52 ms, the torch composite 169.6 ms."""
import numpy as np
import pytest
import torch

import local_pca_cases as cases
import local_pca_ref as ref

pytestmark = pytest.mark.gpu

CPU = torch.device("cpu")


def _t(a, dev):
    return torch.tensor(a, device=dev)[None]


# ------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("m", cases.MS)
def test_device_shapes_and_host_bits(dev, m):
    """Every k on three clouds of m points: odd and even row pitch, partial waves and workgroups, batch offsets."""
    cases.check_shapes(m, dev)
    x, table = cases.batch_of(m)
    for k in cases.KS:
        idx = np.ascontiguousarray(table[:, :, :k])
        assert cases.same_bits(cases.run(x, idx, dev), cases.run(x, idx, CPU)), f"m {m} k {k}: device against host"


def test_device_named_clouds_and_host_bits(dev):
    done = cases.check_named_clouds(dev)
    for (name, k), want in done.items():
        assert cases.same_bits(want["out"], cases.run(cases.cloud(name), cases.self_table(name, k), CPU)), f"({name}) k {k}"
    print("worst figures on the device:", cases.WORST)


def test_device_degenerate_geometry(dev):
    cases.check_degenerate(dev)


def test_device_tables_with_holes(dev):
    cases.check_holes(dev)
    x, idx = cases.cloud("a"), cases.holes_table()
    assert cases.same_bits(cases.run(x, idx, dev), cases.run(x, idx, CPU))


def test_device_signs_and_viewpoints(dev):
    cases.check_signs(dev)
    x, idx = cases.cloud("b"), cases.self_table("b", 16)
    assert cases.same_bits(cases.run(x, idx, dev, new_xyz=x, viewpoint=[0.1, 0.2, 3.0]),
                           cases.run(x, idx, CPU, new_xyz=x, viewpoint=[0.1, 0.2, 3.0]))


def test_device_queries_from_fps_and_the_searches(dev):
    """The tables the library's own searches write: knn_query for farthest-point picks, ball_query(pad="none")."""
    from sparenet_amd.cuda.fps import farthest_point_sample
    from sparenet_amd.cuda.neighbors import ball_query, knn_query

    x, q, idx, out = cases.check_queries_apart(dev)
    xt = _t(x, dev)
    picks = farthest_point_sample(xt, 130)
    qt = torch.gather(xt, 1, picks.long()[:, :, None].expand(-1, -1, 3)).contiguous()
    _, table = knn_query(8, xt, qt)
    assert np.array_equal(qt[0].cpu().numpy(), q) and np.array_equal(table[0].cpu().numpy(), idx)
    a = cases.cloud("a")
    at = _t(a, dev)
    ball = ball_query(cases.BALL_RADIUS, 32, at, at, pad="none")[0].cpu().numpy()
    cases.check(cases.run(a, ball, dev), a, ball, "the device's ball_query(pad='none') table")
    assert np.array_equal(ball, cases.ball_table())


def test_estimate_normals_full_width(dev):
    """One full-width row of the workload, 2 x 16384 at k = 16, against the reference on the DEVICE's table."""
    from sparenet_amd.cuda.neighbors import knn_query
    from sparenet_amd.cuda.normals import estimate_normals, local_pca, surface_variation

    rng = np.random.default_rng(16384)
    p = rng.standard_normal((16384, 3))
    sphere = 0.5 * p / np.linalg.norm(p, axis=1, keepdims=True) + 0.002 * rng.standard_normal(p.shape)
    x = np.stack([sphere, rng.random((16384, 3))]).astype(np.float32)
    xt = torch.tensor(x, device=dev)
    normals, curvature = estimate_normals(xt, 16, return_curvature=True)
    _, idx = knn_query(16, xt, xt)
    n2, values, frames = local_pca(xt, idx, return_frames=True)
    assert torch.equal(normals, n2) and curvature.dtype == torch.float32
    assert torch.equal(curvature, surface_variation(values).float())
    idx = idx.cpu().numpy()
    assert (idx[:, :, 0] == np.arange(16384)).all(), "a point is its own first neighbour"
    out = (n2.cpu().numpy(), values.cpu().numpy(), frames.cpu().numpy())
    cases.check_batch(out, x, idx, "16384 points, k 16")
    view = torch.tensor([0.0, 0.0, 0.0], device=dev)
    inward = estimate_normals(xt[:1], 16, viewpoint=view)
    assert torch.equal(inward.abs(), normals[:1].abs()) and ((inward * xt[:1]).sum(dim=2) < 0).all()


def test_estimate_normals_ragged(dev):
    from sparenet_amd.cuda.normals import estimate_normals

    x, lengths = cases.ragged_batch()
    xt = torch.tensor(x, device=dev)
    normals, curvature = estimate_normals(xt, 5, lengths=lengths, return_curvature=True)
    assert torch.isfinite(normals).all() and torch.isfinite(curvature).all()
    got = cases.run(x, cases.ragged_table(x, lengths), dev)
    assert np.array_equal(normals.cpu().numpy().view(np.uint32), got[0].view(np.uint32))
    for i, n in enumerate(lengths):
        assert (normals[i, n:] == 0).all() and (curvature[i, n:] == 0).all()
        assert torch.equal(estimate_normals(xt[i:i + 1, :n].contiguous(), 5)[0], normals[i, :n])
    on_device = estimate_normals(xt, 5, lengths=torch.tensor(lengths, device=dev))
    assert torch.equal(on_device, normals)


# ------------------------------------------------------------------------------------------ the metrics
def test_normal_consistency(dev):
    from sparenet_amd.cuda.normals import estimate_normals, normal_consistency
    from sparenet_amd.utils import metrics

    b, inner, d = cases.cloud("b"), cases.cloud("sphere45"), cases.cloud("d")
    same = normal_consistency(_t(b, dev), _t(b, dev))
    print(f"a cloud with itself: 1 - value = {1.0 - same.double().item():.3g}")
    assert same.dtype == torch.float32 and abs(same.double().item() - 1.0) <= 2.0 ** -22
    # two concentric spheres: at least the cosine of the worst angle between the reference's normals at matched points
    nb = ref.local_pca(b, cases.self_table("b", 16))["normals"]
    ni = ref.local_pca(inner, cases.self_table("sphere45", 16))["normals"]
    idx1, idx2 = ref.chamfer_indices(b, inner)
    worst = min(np.abs((nb * ni[idx1]).sum(axis=1)).min(), np.abs((ni * nb[idx2]).sum(axis=1)).min())
    want = ref.normal_consistency(nb, ni, idx1, idx2)
    spheres = normal_consistency(_t(b, dev), _t(inner, dev)).item()
    print(f"concentric spheres: {spheres:.9g} ref {want:.9g}, cos of the worst angle {worst:.9g}")
    assert spheres >= worst and abs(spheres - want) <= 2.0 ** -20
    plane = metrics.normal_consistency(_t(b, dev), _t(d, dev), k=8).item()
    print(f"sphere against the noisy plane: {plane:.9g}")
    assert plane < spheres
    # given normals are used as they are, and the sign of a normal does not enter
    nbt, nit = estimate_normals(_t(b, dev)), estimate_normals(_t(inner, dev))
    assert normal_consistency(_t(b, dev), _t(inner, dev), -nbt, nit).item() == spheres
    # ragged rows equal the per-cloud call; an empty side gives 0
    x = np.full((3, 2048, 3), np.nan, np.float32)
    y = x.copy()
    lengths1, lengths2 = [2048, 700, 0], [1000, 2048, 5]
    x[0], y[0, :1000] = b, d
    x[1, :700], y[1] = inner[:700], b
    y[2, :5] = b[:5]
    got = normal_consistency(torch.tensor(x, device=dev), torch.tensor(y, device=dev), k=8, lengths1=lengths1, lengths2=lengths2)
    assert got[0].item() == plane and got[2].item() == 0.0
    assert got[1].item() == normal_consistency(_t(inner[:700], dev), _t(b, dev), k=8).item()


def test_point_to_plane_chamfer(dev):
    cases.check_point_to_plane(dev)


def test_fused_validation_metrics_with_normals(dev):
    from sparenet_amd.cuda.normals import normal_consistency
    from sparenet_amd.utils.metrics import fused_validation_metrics

    pred, gt = _t(cases.cloud("c"), dev), _t(cases.cloud("b"), dev)
    plain = fused_validation_metrics(pred, gt, with_emd=False)
    flagged = fused_validation_metrics(pred, gt, with_emd=False, with_normals=True, normals_k=8)
    assert sorted(plain) == ["ChamferDistance", "F-Score"]
    assert sorted(flagged) == ["ChamferDistance", "F-Score", "NormalConsistency"]
    for key in plain:
        assert torch.equal(plain[key], flagged[key]), key
    assert torch.equal(flagged["NormalConsistency"], normal_consistency(pred, gt, k=8))
    both = fused_validation_metrics(pred, gt, with_emd=False, with_normals=True, with_dcd=True)
    assert torch.equal(both["NormalConsistency"], normal_consistency(pred, gt)) and torch.equal(both["F-Score"], plain["F-Score"])
    x, lengths = cases.ragged_batch()
    lengths1, lengths2 = lengths, [1, 2, 0, 700]      # gt is the batch reversed: its clouds have 1, 2, 1, 700 points
    xt = torch.tensor(x, device=dev)
    yt = torch.tensor(np.ascontiguousarray(x[::-1]), device=dev)
    plain = fused_validation_metrics(xt, yt, with_emd=False, pred_lengths=lengths1, gt_lengths=lengths2)
    flagged = fused_validation_metrics(xt, yt, with_emd=False, pred_lengths=lengths1, gt_lengths=lengths2, with_normals=True, normals_k=5)
    for key in plain:
        assert torch.equal(plain[key], flagged[key]), key
    assert torch.equal(flagged["NormalConsistency"], normal_consistency(xt, yt, k=5, lengths1=lengths1, lengths2=lengths2))
    assert torch.isfinite(flagged["NormalConsistency"]).all() and flagged["NormalConsistency"][2].item() == 0.0
