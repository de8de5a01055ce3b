"""The sampler's GPU cases, by the kernel instance each was written for, and the one place that asks sn_mds_plan.

tests/test_mds.py runs every case on the GPU against the oracle; tests/test_mds_plan.py asserts on the CPU that the
plans of this table, for 256 compute units, contain every compiled instance and both sides of every switch-over -- so a
retuned threshold that moves a case off its instance fails there, without a GPU.

A case: the knobs (SN_MDS_G caps the team size, 1 = no teams; SN_MDS_RATIO = the team cross-over, and giving it turns
the every-regime override off), b clouds of n points, m picks, and the plan words it expects for 256 compute units.
Cloud 0 is a uniform cube at mean MST length 0.09 (dense regime: the cut ball covers the cloud), cloud 1 a point set on
a sphere of radius 0.5 at mean MST length 0.0085 sqrt(19384 / n) (surface regime at every n)."""
import collections
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ops", "mds_plan.h")

_DEFINES = {k: int(v) for k, v in re.findall(r"^#define SN_MDS_(\w+) (\d+)", open(HEADER).read(), re.M)}
WORDS = _DEFINES["PLAN_WORDS"]
FIELDS = {k[len("PLAN_"):].lower(): v for k, v in _DEFINES.items() if k.startswith("PLAN_") and k != "PLAN_WORDS"}
REGISTERS, GENERIC, CLUSTERED = (_DEFINES["FAMILY_" + k] for k in ("REGISTERS", "GENERIC", "CLUSTERED"))

CUS = 256                       # the compute units the table is written for (MI355X)
TEAM_INSTANCES = (1, 2, 3, 4, 5, 6, 8, 10)
CLUSTERED_INSTANCES = (2, 4, 8, 12, 16, 17, 18, 19)
REGISTER_VARIANTS = ((2, 0, 0), (2, 0, 1024), (20, 2, 1024), (24, 1, 1024))     # mds_kernel<PPT, ZLDS, BS>
# n | n + 1 where the dispatch changes kernel, and where a kernel's own slot table changes instance
BOUNDARIES = (2047, 19456, 20352, 24576, 2048, 4096, 8192, 12288, 16384, 17408, 18432)


def plan(b, n, cus=CUS, g_cap=32, ratio_given=False, solo=False):
    """sn_mds_plan's answer as {word name: value}, `workspace` joined from its two words.  cus <= 0 asks the device."""
    from sparenet_amd import _lib

    out = (ctypes.c_int * WORDS)()
    _lib.op_call("mds_plan", "sn_mds_plan", b, n, cus, g_cap, int(ratio_given), int(solo), out, WORDS)
    p = {name: out[i] for name, i in FIELDS.items()}
    p["workspace"] = ((p.pop("workspace_hi") & 0xffffffff) << 32) | (p.pop("workspace_lo") & 0xffffffff)
    return p


Case = collections.namedtuple("Case", "id env b n m expect")


def case_plan(c, cus=CUS):
    """The plan of the call a case makes under its knobs."""
    g = int(c.env.get("SN_MDS_G", 32))
    return plan(c.b, c.n, cus, g, "SN_MDS_RATIO" in c.env)


def _team(g, n, pg, inst, nw, m=1200):
    env = {"SN_MDS_RATIO": "1e-30", "SN_MDS_G": str(g)}     # both clouds on teams
    return Case(f"team{inst}-pg{pg}-g{g}-n{n}", env, 2, n, m,
                dict(family=CLUSTERED, team_g=g, team_pg=pg, team_instance=inst, team_nw=nw, team_every_regime=0))


def _clustered(n, inst, m=1000):
    return Case(f"clustered{inst}-n{n}", {"SN_MDS_G": "1"}, 2, n, m, dict(family=CLUSTERED, instance=inst, team_g=1))


def _handover(n, team, inst, m=1000):
    env = {"SN_MDS_RATIO": "0.075", "SN_MDS_G": "4"}        # the cube to the team, the sphere to the kernel behind it
    return Case(f"handover-team{team}-clustered{inst}-n{n}", env, 2, n, m,
                dict(family=CLUSTERED, instance=inst, team_g=4, team_instance=team, team_every_regime=0))


def _registers(n, ppt, zlds, bs, m=600):
    return Case(f"registers{ppt}-{zlds}-{bs}-n{n}", {}, 2, n, m,
                dict(family=REGISTERS, instance=ppt, zlds=zlds, static_bs=bs, team_g=1))


CASES = [
    _team(4, 16384, 4, 4, 16),
    _team(4, 19384, 5, 5, 16),
    _team(2, 12288, 6, 6, 16),
    _team(2, 12289, 7, 8, 14),      # rounded up: 8 slots compiled, 7 filled; member 1 ends in a partial group
    _team(2, 16384, 8, 8, 16),
    _team(2, 16385, 9, 10, 15),     # rounded up: 10 slots compiled, 9 filled
    _team(2, 19456, 10, 10, 16),
    _team(8, 19384, 3, 3, 13),
    _team(16, 19384, 2, 2, 10),
    # default knobs: 33 groups of 64 dealt out 5 per member to a team of 8 -- member 7 starts behind the cloud.
    # One dense cloud (under the default cross-over a surface cloud of this size stays off the team).
    Case("team1-empty-member-n2049", {}, 1, 2049, 1200,
         dict(family=CLUSTERED, team_g=8, team_pg=1, team_instance=1, team_nw=5, team_every_regime=0)),
    _clustered(2048, 2), _clustered(2049, 4), _clustered(4096, 4), _clustered(4097, 8), _clustered(8192, 8),
    _clustered(8193, 12), _clustered(12288, 12), _clustered(12289, 16), _clustered(16384, 16), _clustered(16385, 17),
    _clustered(17408, 17), _clustered(17409, 18), _clustered(18432, 18), _clustered(18433, 19), _clustered(19456, 19),
    _handover(16384, 4, 16),
    _handover(19384, 5, 19),
    _registers(1023, 2, 0, 0),
    _registers(2047, 2, 0, 1024),
    _registers(19457, 20, 2, 1024), _registers(20352, 20, 2, 1024),
    _registers(20353, 24, 1, 1024), _registers(24576, 24, 1, 1024),
    Case("generic-n24577", {}, 2, 24577, 600, dict(family=GENERIC, team_g=1)),
]
assert len({c.id for c in CASES}) == len(CASES)


def clouds(c):
    """(xyz [b, n, 3], mean MST lengths [b]) of a case: cloud 0 the dense cube, cloud 1 the sphere."""
    rng = np.random.default_rng(c.n * 31 + c.m)
    x = rng.random((c.b, c.n, 3), dtype=np.float32)
    mml = np.full(c.b, 0.09, np.float32)
    if c.b > 1:
        v = rng.standard_normal((c.n, 3)).astype(np.float32)
        x[1] = (0.5 * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
        mml[1] = np.float32(0.0085 * np.sqrt(19384.0 / c.n))
    return x, mml


def tie_rule_row(n, m):
    """The row a cloud gives when every increment underflows to 0: point 0, then argmin (bitrev(k mod bs), k) over and
    over (bs = the reference's thread count) -- such a cloud exercises the tie key and no arithmetic."""
    bs = 1
    while bs * 2 <= n and bs < 1024:
        bs *= 2
    lg = bs.bit_length() - 1
    rev = [int(format(t, f"0{lg}b")[::-1], 2) if lg else 0 for t in range(bs)]
    order = sorted(range(1, n), key=lambda k: (rev[k % bs], k))
    return np.array([0] + order[:m - 1], np.int32)


def members(p, n):
    """[(first, last)] groups of 64 sorted points that each member of a planned team owns (last exclusive, clipped to the
    cloud): a member of instance P owns P x nw consecutive groups."""
    groups = (n + 63) // 64
    own = p["team_instance"] * p["team_nw"]
    return [(min(g * own, groups), min((g + 1) * own, groups)) for g in range(p["team_g"])]
