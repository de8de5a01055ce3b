"""bench.py's command line: a plain run measures the headline only (everything else behind --full), --steps sets the
number of timed steps, and --dump-outputs writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRAS = ("no_cpu_baseline", "no_roofline", "no_network_steps", "no_emd_regimes", "no_other_ops", "no_literal_radii",
          "no_other_scaling")


def _parse(monkeypatch, *argv):
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_measures_the_headline_only(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert not a.full and a.steps == 7 and a.warmup == 2 and a.dump_outputs is None
    assert all(getattr(a, k) for k in EXTRAS)
    a = _parse(monkeypatch, "--full", "--no-cpu-baseline")
    assert a.full and a.no_cpu_baseline
    assert not any(getattr(a, k) for k in EXTRAS if k != "no_cpu_baseline")


@pytest.mark.parametrize("argv", [("--steps", "0"), ("--warmup", "-1")])
def test_step_counts_are_checked(monkeypatch, argv):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, *argv)


def _captured(b, n, radii, per_view, seed):
    """What HotPath leaves in `captured` after a step, with random stand-ins of the benched shapes."""
    g = torch.Generator().manual_seed(seed)

    def leaf(*shape):
        t = torch.rand(*shape, generator=g).requires_grad_(True)
        t.grad = torch.rand(*shape, generator=g)
        return t

    maps = torch.rand(8, b, radii, 256, 256, generator=g)
    return dict(losses=torch.rand(4, generator=g), chamfer_dist1=torch.rand(b, n, generator=g),
                chamfer_dist2=torch.rand(b, n, generator=g), chamfer_grad1=leaf(b, n, 3), chamfer_grad2=leaf(b, n, 3),
                emd_dist=torch.rand(b, n, generator=g),
                emd_assignment=torch.randint(0, n, (b, n), generator=g, dtype=torch.int32),
                emd_grad=leaf(b, n, 3), expansion_dist=torch.rand(b, n, generator=g),
                expansion_assignment=torch.randint(0, n, (b, n), generator=g, dtype=torch.int32),
                expansion_mean_mst_length=torch.rand(b, generator=g), expansion_grad=leaf(b, n, 3),
                render_grad=leaf(b, n, 3), depthmaps=list(maps.unbind(0)) if per_view else [maps])


def test_dump_outputs_full_size(tmp_path):
    """The benched sizes (32 clouds of 16384 points, 3 radii): float32 files under 64 MB, indices exact, the depth-map
    sample at the same positions whether the views were rendered in one pass or one by one."""
    import bench

    one, per = tmp_path / "one", tmp_path / "per"
    c = _captured(32, 16384, 3, False, 0)
    shapes = bench.dump_outputs(c, str(one))
    bench.dump_outputs(_captured(32, 16384, 3, True, 0), str(per))
    files = sorted(os.listdir(one))
    assert files == sorted(name + ".npy" for name in shapes)
    assert sum(os.path.getsize(one / f) for f in files) <= 64 << 20
    for f in files:
        a = np.load(one / f)
        assert a.dtype == np.float32 and list(a.shape) == shapes[f[:-4]]
        assert np.array_equal(a, np.load(per / f)), f
    assert np.array_equal(np.load(one / "emd_assignment.npy"), c["emd_assignment"].numpy().astype(np.float32))
    assert np.array_equal(np.load(one / "chamfer_grad_gt.npy"), c["chamfer_grad2"].grad.numpy())
    assert np.load(one / "depthmaps_sample.npy").shape == (bench.DUMP_MAP_PIXELS,)


def test_dump_outputs_refuses_a_missing_gradient(tmp_path):
    import bench

    c = _captured(2, 64, 1, False, 1)
    c["emd_grad"].grad = None
    with pytest.raises(RuntimeError, match="emd_grad_pred"):
        bench.dump_outputs(c, str(tmp_path))


@pytest.mark.gpu
def test_plain_bench_run_dumps_its_last_step(dev, tmp_path):
    """`bench.py --steps 2 --warmup 1 --dump-outputs DIR` in a fresh process: one result line that counts exactly the
    2 timed steps, no --full blocks, and the dumped losses are the ones the line reports."""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["roofline"] is None and "cpu_baseline" not in line and not line["full"]
    assert set(line["dumped_outputs"]) == {f[:-4] for f in os.listdir(out)}
    assert np.array_equal(np.load(out / "losses.npy"), np.asarray(line["losses"], np.float32))
    for f in os.listdir(out):
        assert np.isfinite(np.load(out / f)).all(), f
    asg = np.load(out / "emd_assignment.npy")
    assert asg.shape == (32, 16384) and asg.min() >= 0 and asg.max() < 16384
