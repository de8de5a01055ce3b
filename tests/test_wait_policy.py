"""Wait policy of the team-waiting ops (sn_set_wait_policy, SN_WAIT_POLICY; include/sparenet_hip.h).

The persistent EMD auction and the density sampler's teams keep workgroups waiting for each other inside one launch.
On a GPU shared with another process a team can give up after its bounded spin:
  * "fail" (default): NaN / -1 rows and SN_ETIMEDOUT at the next call (pinned by test_fullsize's "is loud" tests);
  * "recover": the same call recomputes the abandoned clouds with kernels that wait for nobody and counts them; later
    calls on that device skip the teams (the latch);
  * "nowait": no team-waiting launch at all.
The GPU tests use the kernels' own park knobs (SN_EMD_DIAG=8 / SN_MDS_DIAG=8: one team member never arrives and the
spin limit is short) to make a team give up, and check that every policy computes what the default computes, bit for
bit / index for index.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW_SYMBOLS = ("sn_set_wait_policy", "sn_wait_policy", "sn_wait_report")


@pytest.fixture
def restore_policy():
    import sparenet_amd

    prev = sparenet_amd.wait_policy()
    yield sparenet_amd
    sparenet_amd.set_wait_policy(prev)


# ------------------------------------------------------------------ CPU side
def test_wait_policy_symbols_are_declared_and_exported():
    import sparenet_amd._lib as L

    hdr = open(os.path.join(ROOT, "include", "sparenet_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int\s+%s\s*\(" % name, hdr, re.M), name
        assert getattr(L.lib(), name) is not None
    assert re.search(r"#define SN_ABI_VERSION 4\b", hdr)
    assert L.lib().sn_abi_version() == 4


def test_set_and_get_round_trip(restore_policy):
    sn = restore_policy
    lib = sn.lib()
    for code, name in enumerate(("fail", "recover", "nowait")):
        sn.set_wait_policy(name)
        assert sn.wait_policy() == name
        assert lib.sn_wait_policy() == code
    for code in (2, 0, 1):
        assert lib.sn_set_wait_policy(code) == 0
        assert lib.sn_wait_policy() == code


def test_unknown_policy_is_rejected(restore_policy):
    sn = restore_policy
    lib = sn.lib()
    sn.set_wait_policy("recover")
    for bad in (3, -1, 100):
        assert lib.sn_set_wait_policy(bad) == sn._lib.SN_EINVAL
        assert b"policy" in lib.sn_last_error()
    assert sn.wait_policy() == "recover"          # a rejected value changes nothing
    with pytest.raises(ValueError):
        sn.set_wait_policy("bogus")
    with pytest.raises(ValueError):
        sn.set_wait_policy("RECOVER")
    assert sn.wait_policy() == "recover"


@pytest.mark.parametrize("env,want", [("recover", "recover"), ("nowait", "nowait"), ("fail", "fail")])
def test_environment_gives_the_initial_policy(env, want):
    code = "import sys; sys.path.insert(0, %r); import sparenet_amd as s; print('RESULT', s.wait_policy(), " \
           "s.lib().sn_wait_policy())" % ROOT
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SN_WAIT_POLICY=env), capture_output=True,
                         text=True, timeout=300)
    line = [l for l in out.stdout.splitlines() if l.startswith("RESULT")]
    assert line, out.stderr[-2000:]
    assert line[0].split()[1:] == [want, str(("fail", "recover", "nowait").index(want))]


# ------------------------------------------------------------------ GPU side
_HEAD = r"""
import sys, numpy as np, torch
sys.path.insert(0, %r)
import oracle
import sparenet_amd
import sparenet_amd._lib as L
dev = torch.device("cuda:0")
""" % ROOT


def _run(code, env, timeout=600):
    out = subprocess.run([sys.executable, "-c", _HEAD + code], env=env, capture_output=True, text=True, timeout=timeout)
    line = [l for l in out.stdout.splitlines() if l.startswith("RESULT")]
    assert line, (out.returncode, out.stderr[-3000:])
    return line[0].split()[1:], out


@pytest.mark.gpu
def test_emd_recover_after_a_parked_team_is_exact():
    """SN_EMD_DIAG=8 parks a member of cloud 0's team: under "recover" the call recomputes the abandoned clouds with
    teams of one workgroup behind the launch -- bit-identical to the oracle, no sticky word (status 0, the next call
    succeeds), SN_EMD_CHECK=1 (the conftest's setting) finds no surviving time-out, the report counts the cloud and the
    device is latched; the latched call is exact as well."""
    code = r"""
from sparenet_amd.cuda.emd.emd_module import emd_forward_raw
g = torch.Generator().manual_seed(1)
x, y = torch.rand(2, 1024, 3, generator=g), torch.rand(2, 1024, 3, generator=g)
d0, a0 = oracle.emd_forward(x.numpy(), y.numpy(), 0.005, 10, mt=True)
d, a = emd_forward_raw(x.to(dev), y.to(dev), 0.005, 10)
torch.cuda.synchronize()
exact1 = np.array_equal(d.cpu().numpy(), d0) and np.array_equal(a.cpu().numpy(), a0)
st = L.lib().sn_device_status()
rep = sparenet_amd.wait_report()
d2, a2 = emd_forward_raw(x.to(dev), y.to(dev), 0.005, 10)      # latched: teams of one workgroup
torch.cuda.synchronize()
exact2 = np.array_equal(d2.cpu().numpy(), d0) and np.array_equal(a2.cpu().numpy(), a0)
print("RESULT", int(exact1), st, int(rep["emd_recovered"] >= 1), int(rep["latched"]), int(exact2),
      sparenet_amd.wait_policy())
"""
    env = dict(os.environ, SN_EMD_DIAG="8", SN_WAIT_POLICY="recover", SN_EMD_CHECK="1")
    got, out = _run(code, env)
    assert got == ["1", "0", "1", "1", "1", "recover"], (got, out.stderr[-1000:])


@pytest.mark.gpu
def test_mds_recover_after_a_parked_team_is_exact():
    """SN_MDS_DIAG=8 parks a member of cloud 0's team: under "recover" the one-workgroup kernel behind the team kernel
    samples every row the teams left at -1 -- both rows index-exact against the oracle, finite gathered features,
    status 0, the report counts the cloud(s)."""
    code = r"""
from sparenet_amd.cuda.MDS.MDS_module import minimum_density_sample, gather_operation
g = torch.Generator().manual_seed(2)
x = torch.rand(2, 4096, 3, generator=g)
mml = torch.full((2,), 0.2)                        # cut ball >> the cube: dense regime, both clouds go to teams
want = oracle.mds(x.numpy(), 1024, mml.numpy(), exp_mode=1)
xd = x.to(dev)
idx = minimum_density_sample(xd, 1024, mml.to(dev))
torch.cuda.synchronize()
exact = np.array_equal(idx.cpu().numpy(), want)
feat = gather_operation(xd.transpose(1, 2).contiguous(), idx)
finite = bool(torch.isfinite(feat).all())
st = L.lib().sn_device_status()
rep = sparenet_amd.wait_report()
print("RESULT", int(exact), int(finite), st, int(rep["mds_recovered"] >= 1), int(rep["latched"]))
"""
    env = dict(os.environ, SN_MDS_DIAG="8", SN_WAIT_POLICY="recover")
    got, out = _run(code, env)
    assert got == ["1", "1", "0", "1", "1"], (got, out.stderr[-1000:])


def _emd(x, y, eps, iters, dev):
    from sparenet_amd.cuda.emd.emd_module import emd_forward_raw

    st = torch.zeros(2, dtype=torch.int64, device=dev)
    d, a = emd_forward_raw(torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), eps, iters, st)
    return d.cpu().numpy(), a.cpu().numpy(), st.cpu().numpy()


def _contested(b, n, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(b, n, 3, generator=g)
    y = 0.5 * y / y.norm(dim=2, keepdim=True)
    x = y + (2 * torch.rand(b, n, 3, generator=g) - 1)
    return x.contiguous().numpy(), y.contiguous().numpy()


@pytest.mark.gpu
def test_emd_policies_agree_with_the_default(restore_policy, dev):
    """"nowait" (teams of one workgroup) and "recover" without a time-out (the recovery pass finds nothing) compute
    what the default computes, bit for bit, pair counters included: the EMD goldens, a contested case and 32 x 16384."""
    import glob

    sn = restore_policy
    rng = torch.Generator().manual_seed(77)
    cases = []
    for f in sorted(glob.glob(os.path.join(GOLDEN, "emd_*.npz"))):
        z = np.load(f)
        cases.append((os.path.basename(f), z["xyz1"], z["xyz2"], float(z["eps"]), int(z["iters"])))
    cases.append(("contested",) + _contested(3, 2048, 31) + (0.005, 20))
    cases.append(("uniform 32x16384", torch.rand(32, 16384, 3, generator=rng).numpy(),
                  torch.rand(32, 16384, 3, generator=rng).numpy(), 0.005, 50))
    for name, x, y, eps, iters in cases:
        sn.set_wait_policy("fail")
        d0, a0, s0 = _emd(x, y, eps, iters, dev)
        for pol in ("nowait", "recover"):
            sn.set_wait_policy(pol)
            d, a, s = _emd(x, y, eps, iters, dev)
            assert np.array_equal(a, a0), (name, pol)
            assert np.array_equal(d, d0), (name, pol)
            assert np.array_equal(s, s0), (name, pol)
    assert sn.lib().sn_device_status() == 0


def _sampler_batch(kind, b, n, rng):
    if kind == "dense":
        return rng.random((b, n, 3), dtype=np.float32), np.full(b, 0.09, np.float32)
    v = rng.standard_normal((b, n, 3)).astype(np.float32)
    x = (0.5 * v / np.linalg.norm(v, axis=2, keepdims=True)).astype(np.float32)
    if kind == "surface":
        return x, np.full(b, 0.0085, np.float32)
    x[::2] = rng.random((len(x[::2]), n, 3), dtype=np.float32)      # mixed: cubes and spheres, both regimes
    return x, np.where(np.arange(b) % 2 == 0, 0.09, 0.0085).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["dense", "surface", "mixed"])
def test_mds_policies_agree_with_the_default(kind, restore_policy, dev):
    """The sampler at SpareNet's 19384 -> 16384: "nowait" (one workgroup per cloud) and "recover" without a time-out
    return the default's index rows exactly."""
    from sparenet_amd.cuda.MDS.MDS_module import minimum_density_sample

    sn = restore_policy
    x, mml = _sampler_batch(kind, 4, 19384, np.random.default_rng(len(kind)))
    xd, md = torch.from_numpy(x).to(dev), torch.from_numpy(mml).to(dev)
    sn.set_wait_policy("fail")
    want = minimum_density_sample(xd, 16384, md).cpu().numpy()
    assert (want[:, 0] == 0).all()
    for pol in ("nowait", "recover"):
        sn.set_wait_policy(pol)
        got = minimum_density_sample(xd, 16384, md).cpu().numpy()
        assert np.array_equal(got, want), pol
    assert sn.lib().sn_device_status() == 0


@pytest.mark.gpu
def test_loss_item_is_finite_after_a_recovered_timeout():
    """The drop-in level: emdModule + networks.emd_term + sparenet_amd.loss_item with a parked auction team under
    "recover" returns the undisturbed loss (equal to the oracle's) instead of raising."""
    code = r"""
from sparenet_amd.cuda.emd.emd_module import emdModule
from sparenet_amd.networks import emd_term
g = torch.Generator().manual_seed(1)
x = torch.rand(2, 1024, 3, generator=g)
y = torch.rand(2, 1024, 3, generator=g)
d0, _ = oracle.emd_forward(x.numpy(), y.numpy(), 0.005, 10, mt=True)
xd = x.to(dev).requires_grad_(True)
dist, _ = emdModule()(xd, y.to(dev), eps=0.005, iters=10)
loss = emd_term(dist)
try:
    v = sparenet_amd.loss_item(loss)
    raised = 0
except sparenet_amd.SparenetHipError:
    v, raised = float("nan"), 1
want = emd_term(torch.from_numpy(d0).to(dev)).item()
print("RESULT", raised, int(np.isfinite(v)), int(v == want), int(sparenet_amd.wait_report()["emd_recovered"] >= 1))
"""
    env = dict(os.environ, SN_EMD_DIAG="8", SN_WAIT_POLICY="recover")
    env.pop("SN_EMD_CHECK", None)
    got, out = _run(code, env)
    assert got == ["0", "1", "1", "1"], (got, out.stderr[-1000:])


_CONCURRENT = r"""
from sparenet_amd.cuda.emd.emd_module import emd_forward_raw
from sparenet_amd.cuda.MDS.MDS_module import minimum_density_sample
g = torch.Generator().manual_seed(int(sys.argv[2]))
x, y = torch.rand(8, 4096, 3, generator=g), torch.rand(8, 4096, 3, generator=g)
p = torch.rand(4, 19384, 3, generator=g)
mml = torch.full((4,), 0.0085)
outs = {}
for rep in range(3):
    d, a = emd_forward_raw(x.to(dev), y.to(dev), 0.005, 30)
    idx = minimum_density_sample(p.to(dev), 4096, mml.to(dev))
    torch.cuda.synchronize()
    if rep == 0:
        outs = dict(d=d.cpu().numpy(), a=a.cpu().numpy(), idx=idx.cpu().numpy())
    else:
        assert np.array_equal(d.cpu().numpy(), outs["d"]) and np.array_equal(idx.cpu().numpy(), outs["idx"])
np.savez(sys.argv[1], **outs)
print("RESULT", sparenet_amd.wait_policy(), L.lib().sn_device_status())
"""


@pytest.mark.gpu
def test_two_processes_share_the_gpu_under_nowait(tmp_path, restore_policy, dev):
    """Two processes on one GPU at the same time, both "nowait" (no workgroup waits for another, so neither can starve
    the other's teams): both finish, under a time limit each, and match a single-process default run bit for bit."""
    from sparenet_amd.cuda.emd.emd_module import emd_forward_raw
    from sparenet_amd.cuda.MDS.MDS_module import minimum_density_sample

    env = dict(os.environ, SN_WAIT_POLICY="nowait")
    env.pop("SN_EMD_DIAG", None)
    env.pop("SN_MDS_DIAG", None)
    procs = []
    for i in range(2):
        path = str(tmp_path / ("out%d.npz" % i))
        procs.append((path, subprocess.Popen([sys.executable, "-c", _HEAD + _CONCURRENT, path, str(100 + i)], env=env,
                                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
    results = []
    for path, pr in procs:
        try:
            so, se = pr.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for _, q in procs:
                q.kill()
            raise
        assert pr.returncode == 0, se[-3000:]
        line = [l for l in so.splitlines() if l.startswith("RESULT")]
        assert line and line[0].split()[1:] == ["nowait", "0"], (so, se[-1000:])
        results.append(np.load(path))
    sn = restore_policy
    sn.set_wait_policy("fail")
    for i, z in enumerate(results):
        g = torch.Generator().manual_seed(100 + i)
        x, y = torch.rand(8, 4096, 3, generator=g), torch.rand(8, 4096, 3, generator=g)
        p = torch.rand(4, 19384, 3, generator=g)
        d, a = emd_forward_raw(x.to(dev), y.to(dev), 0.005, 30)
        idx = minimum_density_sample(p.to(dev), 4096, torch.full((4,), 0.0085, device=dev))
        assert np.array_equal(z["d"], d.cpu().numpy()), i
        assert np.array_equal(z["a"], a.cpu().numpy()), i
        assert np.array_equal(z["idx"], idx.cpu().numpy()), i
