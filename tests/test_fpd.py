"""Frechet Point-cloud Distance without a GPU: the module's state dict, the CPU path against the reference's float64
activations (fixtures of tests/golden/gen_fpd.py), the two scipy-free forms of the Frechet term against the reference's
sqrtm scalar, the bookkeeping of calculate_fpd, and the C entry points' argument validation."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fpd_ref  # noqa: E402


def _golden(golden_dir, case, i):
    return np.load(os.path.join(golden_dir, f"fpd_{case}_set{i}.npz"))


@pytest.fixture(scope="module")
def model64():
    from sparenet_amd.Frechet.pointnet import PointNetCls

    return fpd_ref.load_recipe(PointNetCls(k=16)).double()


def test_state_dict_keys_and_shapes_equal_the_reference():
    from sparenet_amd.Frechet.pointnet import PointNetCls

    sd = PointNetCls(k=16).state_dict()
    assert sorted(sd.keys()) == sorted(fpd_ref.STATE_SHAPES.keys())
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(s) for k, s in fpd_ref.STATE_SHAPES.items()}
    assert len(sd) == 74
    fpd_ref.load_recipe(PointNetCls(k=16))     # strict load of every recipe tensor


def test_recipe_has_negative_batch_norm_weights_and_real_statistics():
    sd = fpd_ref.recipe_state_dict()
    for bn in ("feat.bn3", "feat.stn.bn3", "feat.bn2", "bn1"):
        w = sd[bn + ".weight"]
        assert 0.1 < (w < 0).mean() < 0.4
        assert np.abs(sd[bn + ".running_mean"]).max() > 0.3 and np.ptp(sd[bn + ".running_var"]) > 1.0


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_cpu_path_reproduces_the_reference_float64_activations(golden_dir, model64, case):
    """Folding batch norm reorders a handful of float64 operations, nothing more: 1e-12 of the largest activation."""
    from sparenet_amd.Frechet.FPD import get_activations

    bs = fpd_ref.CASES[case][4]
    for i, pc in enumerate(fpd_ref.case_clouds(case), 1):
        if pc is None:
            continue
        want = _golden(golden_dir, case, i)["act64"]
        got = get_activations(torch.from_numpy(pc).double(), model64, bs, 1808, None)
        assert got.shape == want.shape and got.dtype == np.float64
        err = np.abs(got - want).max()
        print(f"case {case} set {i}: max |act - ref64| = {err:.3e}, largest activation {np.abs(want).max():.3e}")
        assert err <= 1e-12 * np.abs(want).max()


def test_cpu_forward_returns_the_reference_triple(model64):
    x = torch.from_numpy(fpd_ref.clouds("cube", 3, 50, 5)).double().transpose(1, 2)
    logp, trans, actv = model64(x)
    assert logp.shape == (3, 16) and trans.shape == (3, 3, 3) and actv.shape == (3, 1808)
    np.testing.assert_allclose(torch.logsumexp(logp, dim=0).numpy(), 0, atol=1e-12)   # log_softmax over dim 0, as the reference
    np.testing.assert_allclose(torch.log_softmax(actv[:, -16:], dim=0).numpy(), logp.numpy(), rtol=0, atol=1e-13)
    assert not actv.requires_grad


def test_training_mode_raises():
    from sparenet_amd.Frechet.pointnet import PointNetCls

    m = PointNetCls(k=16).train()
    with pytest.raises(RuntimeError, match="eval mode"):
        m(torch.rand(2, 3, 10))


@pytest.mark.parametrize("case", ["a", "b"])
def test_frechet_distance_both_forms_against_the_reference_scalar(golden_dir, case):
    """The reference's sqrtm is the noisy side: S1 S2 has hundreds of zero eigenvalues (fewer clouds than dimensions) and
    a rounding error eps on one of them becomes sqrt(eps) in the trace -- allowance 2 d sqrt(2^-52 |S1| |S2|), derived,
    not measured.  The nuclear-norm form has no such term, so the package's two forms must also agree within it."""
    from sparenet_amd.Frechet.FPD import calculate_frechet_distance, frechet_distance_from_activations

    g1, g2 = _golden(golden_dir, case, 1), _golden(golden_dir, case, 2)
    a1, a2, ref = g1["act64"], g2["act64"], float(g1["fpd_ref64"])
    tol = fpd_ref.fpd_allowance(a1, a2)
    nuc = frechet_distance_from_activations(a1, a2)
    sym = calculate_frechet_distance(a1.mean(axis=0), np.cov(a1, rowvar=False), a2.mean(axis=0), np.cov(a2, rowvar=False))
    print(f"case {case}: ref {ref:.12g} nuclear {nuc:.12g} symmetric {sym:.12g} allowance {tol:.3e} "
          f"|nuc-ref| {abs(nuc - ref):.3e} |sym-ref| {abs(sym - ref):.3e} |nuc-sym| {abs(nuc - sym):.3e}")
    assert ref > 1.0                       # the two distributions are far apart
    assert abs(nuc - ref) <= tol
    assert abs(sym - ref) <= tol
    assert abs(nuc - sym) <= tol


def test_frechet_distance_of_a_set_with_itself_is_zero(golden_dir):
    from sparenet_amd.Frechet.FPD import frechet_distance_from_activations

    a = _golden(golden_dir, "b", 1)["act64"]
    assert abs(frechet_distance_from_activations(a, a)) <= fpd_ref.fpd_allowance(a, a)


def test_remainder_is_dropped_and_statistics_round_trip(tmp_path, model64, golden_dir):
    from sparenet_amd.Frechet import FPD

    pc1, pc2 = (torch.from_numpy(p[:8, :300]).double() for p in fpd_ref.case_clouds("a"))
    act = FPD.get_activations(pc1, model64, 3, 1808, None)
    assert act.shape == (6, 1808)                                        # 8 // 3 * 3: clouds 6 and 7 are dropped
    np.testing.assert_array_equal(act, FPD.get_activations(pc1[:6], model64, 3, 1808, None))
    assert FPD.get_activations(pc1, model64, 9, 1808, None).shape == (0, 1808)
    full = FPD.calculate_fpd(pc1, pc2, batch_size=3, model=model64)
    assert full == FPD.calculate_fpd(pc1[:6], pc2[:7], batch_size=3, model=model64)
    # saved statistics: the reference's format (keys m, s), read back through statistic_save_path
    path = str(tmp_path / "stats.npz")
    FPD.save_statistics(pc2, path, model64, 3, 1808, None)
    with np.load(path) as f:
        assert sorted(f.keys()) == ["m", "s"] and f["m"].shape == (1808,) and f["s"].shape == (1808, 1808)
        m, s = f["m"], f["s"]
    m2, s2 = FPD.calculate_activation_statistics(pc2, model64, 3, 1808, None)
    np.testing.assert_array_equal(m, m2)
    np.testing.assert_array_equal(s, s2)
    from_stats = FPD.calculate_fpd(pc1, None, statistic_save_path=path, batch_size=3, model=model64)
    a1, a2 = FPD.get_activations(pc1, model64, 3), FPD.get_activations(pc2, model64, 3)
    assert abs(from_stats - full) <= fpd_ref.fpd_allowance(a1, a2)


def test_weights_argument_and_missing_file(tmp_path, model64):
    from sparenet_amd.Frechet import FPD
    from sparenet_amd.Frechet.pointnet import PointNetCls

    pc1, pc2 = (torch.from_numpy(p[:4, :200]) for p in fpd_ref.case_clouds("a"))
    path = str(tmp_path / "cls.pth")
    m32 = fpd_ref.load_recipe(PointNetCls(k=16))
    torch.save(m32.state_dict(), path)
    assert FPD.calculate_fpd(pc1, pc2, batch_size=2, weights=path) == FPD.calculate_fpd(pc1, pc2, batch_size=2, model=m32)
    with pytest.raises(FileNotFoundError, match="weights="):
        FPD.calculate_fpd(pc1, pc2, batch_size=2, weights=str(tmp_path / "absent.pth"))
    cwd = os.getcwd()
    os.chdir(tmp_path)                      # no ./Frechet/cls_model_39.pth here
    try:
        with pytest.raises(FileNotFoundError, match="cls_model_39.pth"):
            FPD.calculate_fpd(pc1, pc2, batch_size=2)
    finally:
        os.chdir(cwd)


def test_metrics_fpd_on_cpu_tensors_equals_calculate_fpd():
    from sparenet_amd.Frechet import FPD
    from sparenet_amd.Frechet.pointnet import PointNetCls
    from sparenet_amd.utils.metrics import fpd

    m32 = fpd_ref.load_recipe(PointNetCls(k=16))
    pc1, pc2 = (torch.from_numpy(p[:6, :128]) for p in fpd_ref.case_clouds("a"))
    assert fpd(pc1, pc2, m32, batch_size=3) == FPD.calculate_fpd(pc1, pc2, batch_size=3, model=m32)


def test_new_symbols_are_exported_and_validate_arguments_without_a_gpu():
    import sparenet_amd

    lib = sparenet_amd.lib()
    assert lib.sn_abi_version() == 4
    assert lib.sn_pointnet_pool_workspace_bytes.restype is ctypes.c_size_t
    assert lib.sn_pointnet_pool_workspace_bytes(0, 10) == 0 and lib.sn_pointnet_pool_workspace_bytes(1, 0) == 0
    assert lib.sn_pointnet_pool_workspace_bytes(1, (1 << 20) + 1) == 0
    weights = (128 * 1024 + 64 * 128) * 4
    assert lib.sn_pointnet_pool_workspace_bytes(1, 1) == weights + 4096
    assert lib.sn_pointnet_pool_workspace_bytes(30, 16384) == weights + 30 * 128 * 4096
    assert lib.sn_pointnet_pool_workspace_bytes(2, 1000) == weights + 2 * 8 * 4096
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(8)     # never dereferenced: validation fails first
    big = ctypes.c_size_t(1 << 30)

    def call(xyz=one, trans=null, w1=one, out=one, ws=one, relu=0, b=1, n=16, nbytes=big):
        return lib.sn_pointnet_pool_forward(xyz, trans, w1, one, one, one, one, one, relu, b, n, out, ws, nbytes, null)

    for kw in ({"xyz": null}, {"w1": null}, {"out": null}, {"ws": null}):
        assert call(**kw) == -22
        assert b"null pointer" in lib.sn_last_error()
    assert call(n=0) == -22 and b"1 <= n <= 2^20" in lib.sn_last_error()
    assert call(n=(1 << 20) + 1) == -22 and b"1 <= n <= 2^20" in lib.sn_last_error()
    assert call(b=0) == -22 and b"b >= 1" in lib.sn_last_error()
    assert call(nbytes=ctypes.c_size_t(1000)) == -22 and b"workspace too small" in lib.sn_last_error()


def test_cuda_tensors_have_no_torch_path():
    """the fused wrapper refuses what the kernel cannot take instead of falling back"""
    from sparenet_amd import SparenetHipError
    from sparenet_amd.Frechet.pointnet import pool_mlp_fused

    w = tuple((torch.zeros(o, i), torch.zeros(o)) for o, i in ((64, 3), (128, 64), (1024, 128)))
    with pytest.raises((SparenetHipError, RuntimeError)):
        pool_mlp_fused(torch.rand(1, 3, 8), None, w, True)          # CPU tensor handed to the fused op


def test_alias_frechet_modules_resolves_and_restores():
    import sparenet_amd

    names = ("Frechet", "Frechet.FPD", "Frechet.pointnet")
    saved = {n: sys.modules.get(n) for n in names}
    before = {k for k in sys.modules if k == "cuda" or k.startswith(("cuda.", "utils"))}
    try:
        sparenet_amd.alias_frechet_modules()
        from Frechet.FPD import calculate_fpd
        from Frechet.pointnet import PointNetCls
        import sparenet_amd.Frechet.FPD as mine

        assert calculate_fpd is mine.calculate_fpd
        assert PointNetCls is sparenet_amd.Frechet.pointnet.PointNetCls
        # a separate opt-in: the reference's operator modules are not aliased by it
        assert {k for k in sys.modules if k == "cuda" or k.startswith(("cuda.", "utils"))} == before
    finally:
        for n, mod in saved.items():
            if mod is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = mod
    assert all(sys.modules.get(n) is saved[n] for n in names)
