"""Density-aware Chamfer distance on one GPU beside the Chamfer distance of the same build, in the same process.

    python tools/dcd_time.py [--clouds 32] [--reps 20] [--warmup 5] [--alpha 1000] [--n-lambda 1.0]
                             [--regimes uniform,scatter] [--out FILE]

Per regime of bench.py's emd_regime_clouds (`uniform`: two independent uniform cubes; `scatter`: prediction = ground
truth on a sphere + uniform offsets up to +-0.3), B clouds of 16384 against 16384 points.  After `--warmup` untimed
rounds, `--reps` (at least 20) timed rounds ALTERNATE the two, each bracketed by device events, Python wrapper and
autograd included:
  dcd            density_aware_chamfer(x, y, alpha, n_lambda).sum().backward(): search, counts, loss and gradients in
                 the forward call, a scaling in backward
  chamfer        ChamferDistance: (dist1.mean() + dist2.mean()).backward(), with an event between forward and backward
Reported in ms as median [min, max]: dcd, chamfer, chamfer's forward and backward alone, and the excess dcd - chamfer
per round -- the DCD call replaces the Chamfer backward (both build the inverse lists once and gather over them), so the
excess is to be read beside that run's own Chamfer backward and its spread.
Prints one JSON line per regime; `--out` also appends the lines to a file.  Without a GPU it stops: a time is measured
on the GPU or not at all.  Clocks are not touched."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REGIMES = ("uniform", "scatter")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--alpha", type=float, default=1000.0)
    ap.add_argument("--n-lambda", type=float, default=1.0)
    ap.add_argument("--regimes", default=",".join(REGIMES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    reps = max(a.reps, 20)

    import torch

    if not torch.cuda.is_available():
        sys.exit("dcd_time: no GPU visible; a time is measured on the GPU or not at all")
    import bench
    import sparenet_amd
    from sparenet_amd.cuda.chamfer_distance import ChamferDistance
    from sparenet_amd.cuda.dcd import density_aware_chamfer

    dev = torch.device("cuda:0")
    chamfer = ChamferDistance()

    def event():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def summary(values):
        return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}

    for name in a.regimes.split(","):
        x, y = bench.emd_regime_clouds(name, a.clouds, dev)
        x, y = x.requires_grad_(True), y.requires_grad_(True)

        def dcd_round():
            x.grad = y.grad = None
            e0 = event()
            density_aware_chamfer(x, y, a.alpha, a.n_lambda).sum().backward()
            return e0, event()

        def chamfer_round():
            x.grad = y.grad = None
            e0 = event()
            dist1, dist2 = chamfer(x, y)
            e1 = event()
            (dist1.mean() + dist2.mean()).backward()
            return e0, e1, event()

        for _ in range(a.warmup):
            dcd_round()
            chamfer_round()
        torch.cuda.synchronize()
        rounds = [(dcd_round(), chamfer_round()) for _ in range(reps)]
        torch.cuda.synchronize()
        dcd_ms = [d[0].elapsed_time(d[1]) for d, _ in rounds]
        cd_ms = [c[0].elapsed_time(c[2]) for _, c in rounds]
        res = {"bench": "dcd_time", "regime": name, "clouds": a.clouds, "n": x.size(1), "m": y.size(1), "alpha": a.alpha,
               "n_lambda": a.n_lambda, "reps": reps, "warmup": a.warmup,
               "dcd_ms": summary(dcd_ms), "chamfer_ms": summary(cd_ms),
               "chamfer_forward_ms": summary([c[0].elapsed_time(c[1]) for _, c in rounds]),
               "chamfer_backward_ms": summary([c[1].elapsed_time(c[2]) for _, c in rounds]),
               "excess_ms": summary([d - c for d, c in zip(dcd_ms, cd_ms)]),
               "build_id": sparenet_amd.lib().sn_build_id().decode(), "device": torch.cuda.get_device_name(0)}
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
