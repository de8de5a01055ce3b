"""The sampler's dispatch (sn_mds_plan, include/ops/mds_plan.h) without a GPU: the header and its binding, the
invariants the kernels rely on over a sweep of batch sizes, cloud sizes, team caps and compute-unit counts, and the
coverage of tests/mds_plan_cases.py -- the table tests/test_mds.py runs on the GPU -- over every compiled instance and
both sides of every switch-over.  Each bound below is read off the kernel it protects (sparenet_amd/csrc/mds.hip), not
off the plan function."""
import ctypes
import os

import numpy as np
import pytest

import mds_plan_cases as mc

NAMES = ["sn_mds_plan"]
KIB = 1024


# ------------------------------------------------------------------------------------------ header and binding
def test_header_and_exports():
    from sparenet_amd import _lib

    protos = _lib.prototypes(mc.HEADER)
    assert sorted(protos) == NAMES
    assert [p.name for p in protos["sn_mds_plan"][1]] == ["b", "n", "cus", "g_cap", "ratio_given", "solo", "plan",
                                                          "plan_words"]
    assert protos["sn_mds_plan"][1][6] == _lib.Param("plan", "int", True, False)
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name), f"{name} declared in include/ops/mds_plan.h but not exported"
    assert _lib.op_headers()["mds_plan"] == mc.HEADER
    assert sorted(_lib._op_calls["mds_plan"]) == NAMES
    assert _lib.signature("sn_mds_plan") == [p.name for p in protos["sn_mds_plan"][1]]
    assert L.sn_abi_version() == 4
    # the words are numbered 0 .. WORDS - 1 without a gap, and the helper reads all of them
    assert sorted(mc.FIELDS.values()) == list(range(mc.WORDS))
    assert (mc.REGISTERS, mc.GENERIC, mc.CLUSTERED) == (0, 1, 2)


def test_library_refuses_bad_arguments():
    from sparenet_amd import _lib

    L = _lib.lib()
    out = (ctypes.c_int * mc.WORDS)()

    def refused(text, b=2, n=4096, plan=out, words=mc.WORDS):
        assert L.sn_mds_plan(b, n, 256, 32, 0, 0, plan, words) == -22
        assert text in L.sn_last_error(), L.sn_last_error()

    refused(b"null pointer", plan=None)
    refused(b"plan needs", words=mc.WORDS - 1)
    refused(b">= 1", b=0)
    refused(b">= 1", n=0)
    refused(b">= 1", n=-5)
    refused(b"too large", n=1 << 22)
    with pytest.raises(TypeError, match="host array of c_int"):
        _lib.op_call("mds_plan", "sn_mds_plan", 1, 1, 256, 32, 0, 0, (ctypes.c_float * mc.WORDS)(), mc.WORDS)


def test_knob_values_outside_their_range_mean_the_default():
    for n in (2048, 8192, 19384):
        want = mc.plan(3, n, 256, 32)
        for g in (0, -1, 33, 1 << 20):
            assert mc.plan(3, n, 256, g) == want


# ------------------------------------------------------------------------------------------ the sweep
BATCHES = list(range(1, 131)) + [256, 512]
# every n up to 2100, then steps (odd, so that the residues mod 64 and mod 1024 vary) through 30000, then both sides
# of every switch-over and slot-table edge
SIZES = sorted(set(range(1, 2101)) | set(range(2100, 30001, 61)) | {30000}
               | {n + d for n in mc.BOUNDARIES + (1023,) for d in (0, 1)})
CAPS = [1, 2, 4, 8, 16, 32]
UNITS = [64, 80, 104, 256, 304, 1024]


def _sweep(cus, g_cap, ratio_given=0, solo=0, batches=BATCHES, sizes=SIZES):
    """Every plan of batches x sizes as one int array [len(batches), len(sizes), WORDS] (the raw export, word by word:
    the sweep is millions of calls), and b, n as arrays that broadcast against its words."""
    from sparenet_amd import _lib

    fn = _lib.lib().sn_mds_plan
    plans = np.full((len(batches), len(sizes), mc.WORDS), -1, np.int32)
    base, row, step = plans.ctypes.data, plans.strides[0], plans.strides[1]
    for i, b in enumerate(batches):
        at = base + i * row
        for j, n in enumerate(sizes):
            if fn(b, n, cus, g_cap, ratio_given, solo, at + j * step, mc.WORDS):
                raise AssertionError(f"sn_mds_plan({b}, {n}, {cus}, {g_cap}) refused: {_lib.lib().sn_last_error()}")
    return plans, np.array(batches)[:, None], np.array(sizes)[None, :]


def _check(plans, b, n, cus, g_cap, every_regime_allowed=True):
    w = {name: plans[:, :, i].astype(np.int64) for name, i in mc.FIELDS.items()}
    b, n = np.broadcast_arrays(b, n)

    def holds(cond, what, where=None):
        bad = ~cond if where is None else where & ~cond
        assert not bad.any(), (f"{what}: cus={cus} g_cap={g_cap} first at b={b[bad][0]} n={n[bad][0]} "
                               f"({int(bad.sum())} plans)")

    pow2_threads = 1 << np.floor(np.log2(np.minimum(n, 1024))).astype(np.int64)
    holds(w["threads"] == pow2_threads, "the workgroup is the largest power of two <= min(n, 1024)")
    holds(w["ppt"] == -(-n // w["threads"]), "points per lane")
    holds(np.isin(w["family"], (mc.REGISTERS, mc.GENERIC, mc.CLUSTERED)), "family")

    # ---- teams (mds_dense_team_kernel<P>: member g owns groups [g P nw, (g + 1) P nw) of 64 sorted points, keeps
    # P slots per lane in registers -- lane i < P also keeps slot i's box -- and [P][64 nw][2] floats in LDS)
    clustered = w["family"] == mc.CLUSTERED
    team = w["team_g"] >= 2
    G, P, pg, nw, slots = w["team_g"], w["team_instance"], w["team_pg"], w["team_nw"], w["team_slots"]
    holds(clustered, "teams only in front of the clustered kernel", team)
    holds(w["team_g"] >= 1, "team size >= 1")
    holds((G & (G - 1)) == 0, "team size is a power of two")
    holds(G <= g_cap, "team size within its cap")
    holds(pg <= 10, "pg <= 10", team)
    holds((nw >= 1) & (nw <= 16), "1 <= nw <= 16", team)
    holds(np.isin(P, mc.TEAM_INSTANCES), "a compiled team instance", team)
    holds(P >= pg, "team instance >= pg", team)
    holds(G * P * nw >= -(-n // 64), "every point has an owner", team)
    holds(G * pg * nw >= -(-n // 64), "the slots a member needs cover its share", team)
    holds(slots >= b, "every cloud has a team", team)
    holds(slots % 8 == 0, "as many teams on every XCD", team)
    holds(slots * G <= 1024, "team_slots * G <= 1024 (the control block's exchange lines)", team)
    holds(slots * G <= cus, "the team grid is resident", team)
    holds(w["team_ctl_bytes"] == 128 + 128 * 3 * slots * G, "control block bytes", team)
    holds(w["team_lds_bytes"] == P * nw * 64 * 8, "team LDS = [P][64 nw] (y, z) pairs", team)
    holds(w["team_lds_bytes"] <= w["team_lds_opt_in"], "team LDS within its opt-in", team)
    holds(w["team_lds_opt_in"] <= 160 * KIB - 4096, "team LDS opt-in <= 160 KiB - 4096", team)
    every = w["team_every_regime"] == 1
    holds(np.isin(w["team_every_regime"], (0, 1)), "every-regime flag")
    holds(team & (G >= 8) & (n >= 8192), "every regime only for clouds >= 8192 on teams >= 8", every)
    if not every_regime_allowed:
        holds(~every, "a given SN_MDS_RATIO turns the every-regime override off")
    for name in ("team_slots", "team_pg", "team_nw", "team_instance", "team_lds_bytes", "team_lds_opt_in",
                 "team_every_regime", "team_ctl_bytes"):
        holds(w[name] == 0, f"{name} is 0 without a team launch", ~team)

    # ---- mds_clustered_kernel<P>: 1024 lanes, slot i of a lane is sorted position i * 1024 + ...; the kernel
    # initialises all P (y, z) slots of every lane in LDS, padding included, beside 1 KiB of static hand-off storage
    inst, lds, opt = w["instance"], w["lds_bytes"], w["lds_opt_in"]
    holds(w["threads"] == 1024, "clustered: 1024 lanes", clustered)
    holds(np.isin(inst, mc.CLUSTERED_INSTANCES), "a compiled clustered instance", clustered)
    holds(inst >= w["ppt"], "clustered instance >= ppt", clustered)
    holds(lds >= inst * 1024 * 8, "clustered LDS holds every slot the kernel writes", clustered)
    holds(lds <= opt, "clustered LDS within its opt-in", clustered)
    holds(opt <= 160 * KIB - 1024, "clustered LDS opt-in <= 160 KiB - 1024", clustered)
    holds((w["zlds"] == 0) & (w["static_bs"] == 0), "clustered: no register-kernel words", clustered)

    # ---- mds_kernel<PPT, ZLDS, BS>: lane t owns points t, t + bs, ...; ZLDS coordinates of every point in LDS
    regs = w["family"] == mc.REGISTERS
    variant = np.zeros_like(regs)
    for ppt, zlds, bs in mc.REGISTER_VARIANTS:
        variant |= (inst == ppt) & (w["zlds"] == zlds) & (w["static_bs"] == bs)
    holds(variant, "a compiled mds_kernel variant", regs)
    holds(inst * w["threads"] >= n, "mds_kernel: PPT slots per lane hold the cloud", regs)
    holds((w["static_bs"] == 0) | (w["static_bs"] == w["threads"]), "mds_kernel: compile-time size = launch size", regs)
    holds(lds == w["zlds"] * n * 4, "mds_kernel: LDS = ZLDS coordinates per point", regs)
    holds(lds <= np.where(opt > 0, opt, 64 * KIB), "mds_kernel: LDS within the limit it opts in to", regs)
    holds(opt <= 160 * KIB - 512, "<20,2>: opt-in leaves the 256 B of static hand-off storage", regs & (w["zlds"] == 2))
    holds(opt <= 100 * KIB, "<24,1>: opt-in", regs & (w["zlds"] == 1))
    holds(opt == 0, "no opt-in without LDS", regs & (w["zlds"] == 0))

    # ---- mds_kernel_generic: any number of points per lane, densities in the workspace
    generic = w["family"] == mc.GENERIC
    holds((inst == 0) & (lds == 0) & (opt == 0) & (w["zlds"] == 0), "generic: no instance words", generic)
    holds(~team, "no team outside the clustered family", ~clustered)
    return w


@pytest.fixture(scope="module")
def exported_workspace():
    """sn_mds_workspace_bytes over the sweep's batches x sizes."""
    from sparenet_amd import _lib

    fn = _lib.lib().sn_mds_workspace_bytes
    return np.array([[fn(b, n) for n in SIZES] for b in BATCHES], np.int64)


@pytest.mark.parametrize("cus", UNITS)
def test_invariants_over_the_sweep(cus, exported_workspace):
    for g_cap in CAPS:
        plans, b, n = _sweep(cus, g_cap)
        w = _check(plans, b, n, cus, g_cap)
        need = (w["workspace_hi"] << 32) | (w["workspace_lo"] & 0xffffffff)
        assert (exported_workspace >= need).all() and ((exported_workspace == 0) == (need == 0)).all()
        bb, nn = np.broadcast_arrays(b, n)
        clustered, generic = w["family"] == mc.CLUSTERED, w["family"] == mc.GENERIC
        # what the kernels index: the sort's permutation and scratch (2 ints per point) + the teams' control block;
        # the generic kernel's density per point
        assert (need[clustered] >= (bb * nn * 8)[clustered] + 128 + 128 * 3 * 1024).all()
        assert (need[generic] >= (bb * nn * 4)[generic]).all()
        assert (need[w["family"] == mc.REGISTERS] == 0).all()


def test_invariants_with_a_given_ratio_and_with_one_workgroup_forced():
    some_b = [1, 2, 7, 8, 9, 32, 33, 64, 65, 130, 512]
    some_n = [n for n in SIZES if n >= 2040 or n % 97 == 0]
    for cus in UNITS:
        plans, b, n = _sweep(cus, 32, ratio_given=1, batches=some_b, sizes=some_n)
        _check(plans, b, n, cus, 32, every_regime_allowed=False)
        free, _, _ = _sweep(cus, 32, batches=some_b, sizes=some_n)
        plans[:, :, mc.FIELDS["team_every_regime"]] = free[:, :, mc.FIELDS["team_every_regime"]]
        assert np.array_equal(plans, free)          # the ratio changes that one word
        solo, b, n = _sweep(cus, 32, solo=1, batches=some_b, sizes=some_n)
        w = _check(solo, b, n, cus, 32)
        assert (w["team_g"] == 1).all()
        off, _, _ = _sweep(cus, 1, batches=some_b, sizes=some_n)
        assert np.array_equal(solo, off)            # forced = teams capped at one member
    for cus in (8, 63, 100, 255):                   # no XCD share to give: one workgroup per cloud
        plans, b, n = _sweep(cus, 32, batches=some_b, sizes=some_n)
        assert (_check(plans, b, n, cus, 32)["team_g"] == 1).all()


def test_the_dispatch_as_the_design_states_it():
    """The family and instance per range of n (DESIGN.md's table), asserted at both ends of every range."""
    for lo, hi, family, inst, zlds, bs in [
            (1, 1023, mc.REGISTERS, 2, 0, 0), (1024, 2047, mc.REGISTERS, 2, 0, 1024),
            (2048, 2048, mc.CLUSTERED, 2, 0, 0), (2049, 4096, mc.CLUSTERED, 4, 0, 0),
            (4097, 8192, mc.CLUSTERED, 8, 0, 0), (8193, 12288, mc.CLUSTERED, 12, 0, 0),
            (12289, 16384, mc.CLUSTERED, 16, 0, 0), (16385, 17408, mc.CLUSTERED, 17, 0, 0),
            (17409, 18432, mc.CLUSTERED, 18, 0, 0), (18433, 19456, mc.CLUSTERED, 19, 0, 0),
            (19457, 20352, mc.REGISTERS, 20, 2, 1024), (20353, 24576, mc.REGISTERS, 24, 1, 1024),
            (24577, (1 << 22) - 1, mc.GENERIC, 0, 0, 0)]:
        for n in (lo, hi):
            p = mc.plan(4, n)
            assert (p["family"], p["instance"], p["zlds"], p["static_bs"]) == (family, inst, zlds, bs), n
    # team geometry per batch size at SpareNet's n = 19384 on 256 compute units: G, pg, nw, instance
    for lo, hi, geometry in [(1, 8, (32, 1, 10, 1)), (9, 16, (16, 2, 10, 2)), (17, 32, (8, 3, 13, 3)),
                             (33, 64, (4, 5, 16, 5)), (65, 128, (2, 10, 16, 10)), (129, 512, (1, 0, 0, 0))]:
        for b in (lo, hi):
            p = mc.plan(b, 19384)
            assert (p["team_g"], p["team_pg"], p["team_nw"], p["team_instance"]) == geometry, b
            assert p["team_every_regime"] == (p["team_g"] >= 8)


# ------------------------------------------------------------------------------------------ coverage of the GPU table
def _kernel(p):
    return p["family"], p["instance"], p["zlds"], p["static_bs"]


def missing(cases):
    """What the plans of `cases`, for 256 compute units, leave unreached: [] when the table covers the dispatch."""
    plans = [(c, mc.case_plan(c)) for c in cases]
    out = [f"{c.id}: plan {p} is not the {c.expect} it was written for" for c, p in plans
           if any(p[k] != v for k, v in c.expect.items())]
    # teams that sample BOTH clouds of their case (every regime, or a cross-over of ~0), by instance and by slots needed
    whole = [(c, p) for c, p in plans if p["team_g"] >= 2 and (p["team_every_regime"] or float(c.env.get("SN_MDS_RATIO", 1)) < 1e-20)]
    whole += [(c, p) for c, p in plans if p["team_g"] >= 2 and c.b == 1]      # or the one dense cloud of theirs
    for inst in mc.TEAM_INSTANCES:
        if not any(p["team_instance"] == inst for _, p in whole):
            out.append(f"no case runs mds_dense_team_kernel<{inst}>")
    for pg, inst in ((7, 8), (8, 8), (9, 10), (10, 10)):
        if not any((p["team_pg"], p["team_instance"]) == (pg, inst) for _, p in whole):
            out.append(f"no case runs mds_dense_team_kernel<{inst}> with pg = {pg}")
    owned = [(c, mc.members(p, c.n)) for c, p in whole]
    if not any(any(first == last for first, last in own) for _, own in owned):
        out.append("no team with a member that owns no point")
    if not any(c.n % 64 and all(first < last for first, last in own) for c, own in owned):
        out.append("no team whose last member ends in a partial group")
    # the clustered kernel sampling both clouds itself (no team launch in front), and behind a team in one call
    alone = [(c, p) for c, p in plans if p["family"] == mc.CLUSTERED and p["team_g"] == 1]
    for inst in mc.CLUSTERED_INSTANCES:
        if not any(p["instance"] == inst for _, p in alone):
            out.append(f"no case samples with mds_clustered_kernel<{inst}> alone")
    for team, inst in ((4, 16), (5, 19)):
        if not any(p["team_g"] >= 2 and not p["team_every_regime"] and float(c.env.get("SN_MDS_RATIO", 0)) > 1e-3
                   and c.b > 1 and (p["team_instance"], p["instance"]) == (team, inst) for c, p in plans):
            out.append(f"no case hands over from team<{team}> to clustered<{inst}> in one call")
    single = [(c, p) for c, p in plans if p["team_g"] == 1]
    for variant in mc.REGISTER_VARIANTS:
        if not any(_kernel(p) == (mc.REGISTERS,) + variant for _, p in single):
            out.append(f"no case runs mds_kernel<{variant}>")
    if not any(p["family"] == mc.GENERIC for _, p in single):
        out.append("no case runs mds_kernel_generic")
    # both sides of every switch-over, by one-workgroup kernels (a team in front would sample the cloud instead)
    for edge in mc.BOUNDARIES:
        below = {_kernel(p) for c, p in single if c.n == edge}
        above = {_kernel(p) for c, p in single if c.n == edge + 1}
        if not below or not above or below & above:
            out.append(f"no pair of cases on the two sides of {edge} | {edge + 1}")
    return out


def test_the_gpu_table_reaches_every_instance_and_boundary():
    assert missing(mc.CASES) == []


def test_every_case_of_the_table_is_needed():
    """Dropping any one case leaves an instance or a boundary unreached: the table has no case the coverage test
    would not miss."""
    for i, c in enumerate(mc.CASES):
        assert missing(mc.CASES[:i] + mc.CASES[i + 1:]), c.id


def test_case_clouds_and_geometry_helpers():
    c = next(c for c in mc.CASES if c.id.startswith("team8-pg7"))
    x, mml = mc.clouds(c)
    assert x.shape == (2, 12289, 3) and x.dtype == np.float32 and mml.dtype == np.float32
    assert np.allclose(np.linalg.norm(x[1], axis=1), 0.5, atol=1e-6) and 0 <= x[0].min() and x[0].max() < 1
    assert mc.members(mc.case_plan(c), c.n) == [(0, 112), (112, 193)]        # 193 groups, the last holds one point
    c = next(c for c in mc.CASES if "empty-member" in c.id)
    assert mc.members(mc.case_plan(c), c.n)[-2:] == [(30, 33), (33, 33)]
    assert list(mc.tie_rule_row(8, 5)) == [0, 4, 2, 6, 1]
    for c in mc.CASES:
        assert 600 <= c.m <= 1500 and c.m <= c.n
