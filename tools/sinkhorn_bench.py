"""Sinkhorn transport on one GPU: the softmin kernel against the torch composite a user has without it.

    python tools/sinkhorn_bench.py [--reps 10] [--warmup 3] [--sweep] [--skip-composite] [--out FILE]

Per shape (B clouds of N against M points, uniform in the unit cube) the median, minimum and maximum of `--reps`
synchronised wall-clock passes after `--warmup` untimed ones, including the Python wrapper:
  half       ms per half-iteration: a solve of 10 constant steps at eps = 0.01 (20 launches) divided by 20, split width
             chosen by the library (SN_SINKHORN_SPLIT unset); with `--sweep` also every forced width 1, 2, 4, 8, 16 --
             the measurement the dispatch rule rests on;
  solve      ms per sinkhorn_potentials(x, y, eps=0.01, eps_start=3.0) at the default step count (14 steps, 28 launches);
  backward   ms per barycentre pass (one side of the gradient);
  composite  the same half-iteration and solve in torch: cdist ** 2, then logsumexp over the [B,N,M] matrix per
             half-iteration (34 GB at 32 x 16384 x 16384; there only the half-iteration is tried, and a shape for which
             it cannot be allocated is reported as skipped).  Results are not compared here (tests/test_sinkhorn_gpu.py).
Prints one JSON line per shape, then the table; `--out` also appends the lines to a file.  Clocks are not touched."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("SN_KNOBS_PER_CALL", "1")      # the split width is switched inside this process

SHAPES = [(32, 2048, 2048), (4, 2048, 2048), (32, 16384, 16384)]
SWEEP_SHAPES = [(1, 2048, 2048), (8, 1024, 1024)]      # `--sweep` adds these: the small launches the split path is for
EPS, EPS_START, HALF_STEPS = 0.01, 3.0, 10
COMPOSITE_SOLVE_MAX = 1 << 28      # pairs up to which the composite's whole solve is timed


def composite_half(cost, pot, eps):
    """One softmin over the last axis of cost [B,N,M] with the potential pot [B,M]."""
    import torch

    return -eps * torch.logsumexp((pot[:, None, :] - cost) / eps - math.log(cost.size(2)), dim=2)


def composite_solve(x, y, schedule):
    import torch

    cost = torch.cdist(x, y) ** 2
    g = torch.zeros(y.shape[:2], device=y.device)
    for e in schedule:
        f = composite_half(cost, g, e)
        g = composite_half(cost.transpose(1, 2), f, e)
    return f, g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--skip-composite", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import sparenet_amd
    from sparenet_amd import _lib
    from sparenet_amd.cuda.sinkhorn import schedule, sinkhorn_potentials

    if not torch.cuda.is_available():
        sys.exit("sinkhorn_bench: no GPU visible; a time is measured on the GPU or not at all")
    dev = torch.device("cuda:0")

    def measure(fn, scale=1.0):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(max(a.reps, 1)):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3 * scale)
        return {"ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times)}

    steps = schedule(EPS, None, EPS_START)
    rows = []
    for b, n, m in SHAPES + (SWEEP_SHAPES if a.sweep else []):
        gen = torch.Generator().manual_seed(b * 100003 + n)
        x, y = torch.rand(b, n, 3, generator=gen).to(dev), torch.rand(b, m, 3, generator=gen).to(dev)
        res = {"bench": "sinkhorn", "clouds": b, "n": n, "m": m, "reps": a.reps, "warmup": a.warmup,
               "solve_steps": len(steps), "eps": EPS, "eps_start": EPS_START}
        os.environ.pop("SN_SINKHORN_SPLIT", None)
        res["solve"] = measure(lambda: sinkhorn_potentials(x, y, EPS, eps_start=EPS_START))
        _, g = sinkhorn_potentials(x, y, EPS, eps_start=EPS_START)
        bary = torch.empty(b, n, 3, device=dev)
        res["backward"] = measure(lambda: _lib.op_call("sinkhorn", "sn_sinkhorn_barycenter", x, y, g, b, n, m, None,
                                                       None, EPS, bary, None, None))
        if a.sweep:
            for split in (1, 2, 4, 8, 16):
                os.environ["SN_SINKHORN_SPLIT"] = str(split)
                res[f"split={split}"] = measure(lambda: sinkhorn_potentials(x, y, EPS, iters=HALF_STEPS),
                                                1.0 / (2 * HALF_STEPS))
            os.environ.pop("SN_SINKHORN_SPLIT", None)
        # the library's own width last, so that in a sweep it runs as warm as the forced widths beside it
        res["half"] = measure(lambda: sinkhorn_potentials(x, y, EPS, iters=HALF_STEPS), 1.0 / (2 * HALF_STEPS))
        if not a.skip_composite:
            try:
                cost = torch.cdist(x, y) ** 2
                pot = torch.zeros(b, m, device=dev)
                res["composite_half"] = measure(lambda: composite_half(cost, pot, EPS))
                del cost
                if b * n * m <= COMPOSITE_SOLVE_MAX:
                    res["composite_solve"] = measure(lambda: composite_solve(x, y, steps))
            except torch.OutOfMemoryError:
                res["composite_skipped"] = "the [B,N,M] matrix could not be allocated"
            torch.cuda.empty_cache()
        res["build_id"] = sparenet_amd.lib().sn_build_id().decode()
        res["device"] = torch.cuda.get_device_name(0)
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        rows.append(res)

    columns = ["half", "solve", "backward"] + ([f"split={s}" for s in (1, 2, 4, 8, 16)] if a.sweep else []) + \
        ["composite_half", "composite_solve"]
    print("\n| B | N | M | " + " | ".join(f"{c} ms" for c in columns) + " |")
    print("|" + "---|" * (3 + len(columns)))
    for r in rows:
        cells = []
        for c in columns:
            v = r.get(c)
            cells.append("skipped" if c.startswith("composite") and "composite_skipped" in r and v is None else
                         ("-" if v is None else f"{v['ms']:.3f}"))
        print(f"| {r['clouds']} | {r['n']} | {r['m']} | " + " | ".join(cells) + " |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
