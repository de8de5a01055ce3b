"""Milliseconds per call of the general-size EMD (sn_emd_forward_general) next to the persistent auction.

    python tools/emd_general_bench.py [--reps R] [--skip-long] [--backward] [--json out.json]

Cases: B=32 n=m=16000 and B=32 3000 -> 16384 at the training setting (eps 0.005, 50 iterations), B=1 n=m=16000 at the
reference's final-test setting (eps 0.002, 10000 iterations), and at B=32 n=m=16384 (0.005, 50) the persistent auction
against the general kernels forced by SN_EMD_GENERAL=1.  Uniform clouds in the unit cube; device-event timing after one
warm-up call per case; median of R calls.  Also prints effective pairs per call (stats[0]) and checks the forced
general run against the persistent one bit for bit.  --backward adds sn_emd_backward_general at B=32 n=m=16384 on random
assignments with 1, 64 and 4096 bidders per target in use (the stable scatter by target), median of 4 R calls."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("SN_KNOBS_PER_CALL", "1")   # SN_EMD_GENERAL is switched inside this process

import torch  # noqa: E402

import sparenet_amd._lib as _L  # noqa: E402

if os.environ.get("AB_LIB"):  # time a saved build (tools/build_variant.sh)
    _L.LIB_PATH = os.path.abspath(os.environ["AB_LIB"])
from sparenet_amd.cuda.emd.emd_general import emd_general_backward_raw, emd_general_forward_raw  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def case(name, b, n, m, eps, iters, reps, general, dev, out):
    g = torch.Generator().manual_seed(b * 7 + n + m)
    x = torch.rand(b, n, 3, generator=g).to(dev)
    y = torch.rand(b, m, 3, generator=g).to(dev)
    os.environ["SN_EMD_GENERAL"] = "1" if general else "0"
    st = torch.zeros(2, dtype=torch.int64, device=dev)
    res = {}

    def call():
        st.zero_()
        res["out"] = emd_general_forward_raw(x, y, eps, iters, st)

    med, lo, hi = timed(call, reps)
    pairs = int(st[0].item())
    row = dict(case=name, b=b, n=n, m=m, eps=eps, iters=iters, path="general" if general else "dispatch",
               ms=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3), pairs=pairs,
               gpairs_per_s=round(pairs / med / 1e6, 1))
    print(json.dumps(row), flush=True)
    out.append(row)
    return res["out"]


def backward_case(name, b, n, m, sharers, reps, dev, out):
    """sn_emd_backward_general with gradients for both inputs; `sharers` bidders per target in use."""
    g = torch.Generator().manual_seed(b * 7 + n + m)
    x = torch.rand(b, n, 3, generator=g).to(dev)
    y = torch.rand(b, m, 3, generator=g).to(dev)
    graddist = torch.rand(b, n, generator=g).to(dev)
    assignment = torch.randint(0, max(1, n // sharers), (b, n), generator=g, dtype=torch.int32).to(dev)
    med, lo, hi = timed(lambda: emd_general_backward_raw(x, y, graddist, assignment), reps)
    row = dict(case=name, b=b, n=n, m=m, sharers=sharers, path="backward", ms=round(med, 3), ms_min=round(lo, 3),
               ms_max=round(hi, 3))
    print(json.dumps(row), flush=True)
    out.append(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-long", action="store_true", help="leave out the 10000-iteration case")
    ap.add_argument("--backward", action="store_true", help="add the backward with 1, 64 and 4096 bidders per target")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("emd_general_bench: no GPU visible")
    dev = torch.device("cuda:0")
    out = []
    d0, a0 = case("persistent_32x16384", 32, 16384, 16384, 0.005, 50, a.reps, False, dev, out)
    d1, a1 = case("general_32x16384", 32, 16384, 16384, 0.005, 50, a.reps, True, dev, out)
    same = bool(torch.equal(a0, a1) and torch.equal(d0, d1))
    print(json.dumps({"forced_general_equals_persistent": same}), flush=True)
    case("general_32x16000", 32, 16000, 16000, 0.005, 50, a.reps, False, dev, out)
    case("general_32x3000_16384", 32, 3000, 16384, 0.005, 50, a.reps, False, dev, out)
    if not a.skip_long:
        case("general_1x16000_it10000", 1, 16000, 16000, 0.002, 10000, max(1, a.reps // 2), False, dev, out)
    if a.backward:
        for sharers in (1, 64, 4096):
            backward_case(f"backward_32x16384_share{sharers}", 32, 16384, 16384, sharers, 4 * a.reps, dev, out)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(rows=out, forced_general_equals_persistent=same), f, indent=1)
    if not same:
        sys.exit("forced general run differs from the persistent auction")


if __name__ == "__main__":
    main()
