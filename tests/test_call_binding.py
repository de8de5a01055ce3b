"""sparenet_amd._lib.call / workspace: the one path on which Python values become C arguments, driven by the
prototypes of include/sparenet_hip.h.  The CPU tests use the host Chamfer entry points (the only ones that run
without a GPU); the GPU tests cover the device, stream and workspace rules."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tiny(golden_dir):
    z = np.load(os.path.join(golden_dir, "chamfer_tiny_3x1x5.npz"))
    return z, {k: torch.from_numpy(z[k]) for k in z.files if k != "provenance"}


def _forward_outputs(b=3, n=1, m=5):
    return (torch.empty(b, n), torch.empty(b, n, dtype=torch.int32), torch.empty(b, m),
            torch.empty(b, m, dtype=torch.int32))


def test_a_parameter_list_is_prepared_for_every_declared_function():
    from sparenet_amd import _lib

    protos = _lib.prototypes()
    assert len(protos) == 80
    _lib.lib()
    assert sorted(_lib._calls) == sorted(protos)
    for name, (ret, params) in protos.items():
        assert ret in _lib._RETURNS, (name, ret)
        for p in params:
            assert p.ctype in (_lib._POINTEES if p.pointer else _lib._SCALARS), (name, p)
        took = _lib.signature(name)
        stream = bool(params) and params[-1].name == "stream"
        assert len(took) == len(params) - stream - ("workspace_bytes" in [p.name for p in params]), name
        assert "stream" not in took and "workspace_bytes" not in took, name
    # the two workspaces without a size are plain pointers
    assert "workspace32" in _lib.signature("sn_depth_project_backward")
    assert "workspace" in _lib.signature("sn_depth_project_backward_views")
    assert sum(bool(p) and p[-1].name == "stream" for _, p in protos.values()) == 46


def test_host_chamfer_through_call_equals_golden_and_a_direct_ctypes_call(golden_dir):
    from sparenet_amd import _lib

    z, t = _tiny(golden_dir)
    d1, i1, d2, i2 = _forward_outputs()
    assert _lib.call("sn_chamfer_forward_host", t["xyz1"], t["xyz2"], 3, 1, 5, d1, i1, d2, i2, 0, host=True) is None
    g1, g2 = torch.empty(3, 1, 3), torch.empty(3, 5, 3)
    _lib.call("sn_chamfer_backward_host", t["xyz1"], t["xyz2"], t["graddist1"], t["graddist2"], i1, i2, 3, 1, 5,
              g1, g2, 0, host=True)

    def p(x):
        return ctypes.c_void_p(x.data_ptr())

    e1, j1, e2, j2 = _forward_outputs()
    h1, h2 = torch.empty(3, 1, 3), torch.empty(3, 5, 3)
    L = _lib.lib()
    assert L.sn_chamfer_forward_host(p(t["xyz1"]), p(t["xyz2"]), 3, 1, 5, p(e1), p(j1), p(e2), p(j2), 0) == 0
    assert L.sn_chamfer_backward_host(p(t["xyz1"]), p(t["xyz2"]), p(t["graddist1"]), p(t["graddist2"]), p(j1), p(j2),
                                      3, 1, 5, p(h1), p(h2), 0) == 0
    for got, direct, key in ((d1, e1, "dist1"), (i1, j1, "idx1"), (d2, e2, "dist2"), (i2, j2, "idx2"),
                             (g1, h1, "gradxyz1"), (g2, h2, "gradxyz2")):
        assert np.array_equal(got.numpy(), z[key]), key
        assert torch.equal(got, direct), key


def test_refusals_name_the_declared_parameter(golden_dir):
    from sparenet_amd import SparenetHipError, _lib

    _, t = _tiny(golden_dir)
    d1, i1, d2, i2 = _forward_outputs()
    x1, x2 = t["xyz1"], t["xyz2"]
    with pytest.raises(TypeError, match="idx1"):
        _lib.call("sn_chamfer_forward_host", x1, x2, 3, 1, 5, d1, i1.long(), d2, i2, 0, host=True)
    with pytest.raises(TypeError, match="xyz2"):
        _lib.call("sn_chamfer_forward_host", x1, x2.numpy(), 3, 1, 5, d1, i1, d2, i2, 0, host=True)
    with pytest.raises(ValueError, match="xyz1"):
        _lib.call("sn_chamfer_forward_host", torch.rand(3, 3, 2).transpose(1, 2), x2, 3, 2, 5, d1, i1, d2, i2, 0,
                  host=True)
    with pytest.raises(TypeError, match="takes 10 arguments"):
        _lib.call("sn_chamfer_forward_host", x1, x2, 3, 1, 5, d1, i1, d2, i2, host=True)
    with pytest.raises(TypeError, match="takes 10 arguments"):
        _lib.call("sn_chamfer_forward_host", x1, x2, 3, 1, 5, d1, i1, d2, i2, 0, 0, host=True)
    with pytest.raises(TypeError, match=r"\bn\b"):
        _lib.call("sn_chamfer_forward_host", x1, x2, 3, 5.5, 5, d1, i1, d2, i2, 0, host=True)
    with pytest.raises(TypeError, match="c_float"):      # a host array of another element type
        _lib.call("sn_chamfer_forward_host", (ctypes.c_double * 9)(), x2, 3, 1, 5, d1, i1, d2, i2, 0, host=True)
    with pytest.raises(SparenetHipError, match="null pointer"):      # the library's own message still arrives
        _lib.call("sn_chamfer_forward_host", x1, x2, 3, 1, 5, None, i1, d2, i2, 0, host=True)
    with pytest.raises(SparenetHipError, match="sn_no_such_entry"):
        _lib.call("sn_no_such_entry")


def test_a_cpu_tensor_is_refused_by_a_device_entry_point():
    from sparenet_amd import SparenetHipError, _lib

    x = torch.rand(1, 3, 32)
    idx = torch.empty(1, 32, 4, dtype=torch.int64)
    with pytest.raises(SparenetHipError, match="no CPU path"):
        _lib.call("sn_knn", x, 1, 3, 32, 4, idx, None)
    with pytest.raises(SparenetHipError, match="no CPU path"):
        _lib.require_device(x, "x")
    with pytest.raises(TypeError, match="workspace"):      # a workspace is what workspace() returned, or None
        _lib.call("sn_knn", None, 1, 3, 32, 4, None, torch.empty(8, dtype=torch.uint8))


def test_size_exports_and_queries_return_their_number(golden_dir):
    from sparenet_amd import _lib

    rows = json.load(open(os.path.join(golden_dir, "workspace_sizes.json")))["sn_emd_workspace_bytes"]
    (want,) = [r[-1] for r in rows if r[:-1] == [32, 16384]]
    assert _lib.call("sn_emd_workspace_bytes", 32, 16384) == want
    assert _lib.call("sn_abi_version") == _lib.EXPECTED_ABI == 4
    assert _lib.call("sn_device_status") == 0      # a parameterless int function is a query, not a status code


def test_old_helpers_keep_their_behaviour():
    from sparenet_amd import SparenetHipError, _lib

    t = torch.arange(6, dtype=torch.float32)
    assert _lib.hptr(t, torch.float32, "t").value == _lib.ptr(t, torch.float32, "t", host=True).value == t.data_ptr()
    with pytest.raises(SparenetHipError, match="no CPU path"):
        _lib.fptr(t, "t")
    with pytest.raises(TypeError, match="t: expected dtype"):
        _lib.hptr(t, torch.int32, "t")
    assert _lib.cfloat(1.5).value == 1.5


def test_lib_refuses_to_load_without_the_header(monkeypatch, tmp_path):
    from sparenet_amd import SparenetHipError, _lib

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "HEADER_PATH", str(tmp_path / "sparenet_hip.h"))
    with pytest.raises(SparenetHipError, match="sparenet_hip.h not found"):
        _lib.lib()


# ------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_knn_refuses_an_int32_index_buffer(dev):
    from sparenet_amd import _lib

    x = torch.rand(1, 3, 32, device=dev)
    idx = torch.full((1, 32, 4), -7, dtype=torch.int32, device=dev)
    ws = _lib.workspace("sn_knn_workspace_bytes", x, 1, 32)
    with pytest.raises(TypeError, match="idx"):
        _lib.call("sn_knn", x, 1, 3, 32, 4, idx, ws)
    assert (idx == -7).all()      # nothing was launched


@pytest.mark.gpu
def test_chamfer_runs_on_the_current_stream_of_the_tensors_device(dev):
    from sparenet_amd.cuda.chamfer_distance import ChamferDistanceFunction

    g = torch.Generator().manual_seed(5)
    x, y = torch.rand(2, 64, 3, generator=g), torch.rand(2, 48, 3, generator=g)
    w1, w2 = torch.rand(2, 64, generator=g).to(dev), torch.rand(2, 48, generator=g).to(dev)

    def run():
        a, b = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
        d1, d2 = ChamferDistanceFunction.apply(a, b)
        ((d1 * w1).sum() + (d2 * w2).sum()).backward()
        return d1.detach(), d2.detach(), a.grad, b.grad

    want = run()
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        got = run()
    side.synchronize()
    for g_, w_ in zip(got, want):
        assert torch.equal(g_, w_)


@pytest.mark.gpu
def test_sampler_with_an_empty_workspace_matches_the_oracle(dev):
    import oracle
    from sparenet_amd import _lib
    from sparenet_amd.cuda.MDS.MDS_module import minimum_density_sample

    x = torch.rand(1, 256, 3, generator=torch.Generator().manual_seed(6))
    mml = torch.tensor([0.05])
    ws = _lib.workspace("sn_mds_workspace_bytes", x.to(dev), 1, 256)
    assert ws.nbytes == 0 and ws.tensor.numel() == 1 and ws.tensor.device == x.to(dev).device
    idx = minimum_density_sample(x.to(dev), 64, mml.to(dev))
    assert np.array_equal(idx.cpu().numpy(), oracle.mds(x.numpy(), 64, mml.numpy(), exp_mode=1))


@pytest.mark.gpu
def test_ragged_emd_through_workspace_matches_the_restatement(dev):
    from emd_general_ref import emd_general as ref_forward
    from sparenet_amd.cuda.ragged import emd_ragged

    r = np.random.default_rng(9)
    x, y = r.random((2, 64, 3), dtype=np.float32), r.random((2, 64, 3), dtype=np.float32)
    lengths = (64, 40)
    d, a = emd_ragged(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), lengths, lengths, 0.005, 12)
    d, a = d.cpu().numpy(), a.cpu().numpy()
    for i, ln in enumerate(lengths):
        wd, wa, _ = ref_forward(x[i:i + 1, :ln], y[i:i + 1, :ln], 0.005, 12)
        assert np.array_equal(a[i, :ln], wa[0]) and np.array_equal(d[i, :ln], wd[0]), i
        assert (a[i, ln:] == -1).all() and not d[i, ln:].any(), i
