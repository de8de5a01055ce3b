"""The occupancy grid and the Jensen-Shannon divergence between two sets on one GPU: the kernel, the whole metric, and the
torch composite they replace, in the same process.

    python tools/jsd_time.py [--clouds 1024] [--points 2048] [--resolution 28] [--reps 20] [--warmup 5]
                             [--composite-budget 60] [--out FILE]

Two sets of S clouds of n points (seeded), the grid clipped to the sphere.  Two kinds of data, each timed on its own:
  ball    uniform in the ball of radius 0.5: a few per cent of the points have their cube cell clipped away (Rule 2);
  shell   a thin shell under the sphere's surface, radius 0.49 .. 0.5 -- shapes normalised to touch the sphere: heavy in
          Rule 2.
After `--warmup` untimed rounds, `--reps` (at least 20) timed rounds ALTERNATE, each call bracketed by device events:
  grid       sn_occupancy_grid alone on one set (the library call, no wrapper): counts and occupied
  cells      the same call asked for `cells` only: no histogram in LDS, so no clear and no flush per cloud -- grid minus
             cells bounds what the histogram, its flush and the global atomics cost
  jsd        jsd_between_sets(gen, ref) through the Python wrappers: the range check, two grids, the divergence
and then the torch composite on the same device -- torch.cdist of a chunk of points to the in-sphere centres, argmin,
bincount, for both sets, then the same divergence -- is timed on its own: first on 32 clouds per set; when that time
scaled to S stays inside `--composite-budget` seconds for all its rounds, on the whole sets with 5 rounds, otherwise the
scaled median is reported and marked as extrapolated.  (The composite takes fp32 distances to rounded centres: it is
what a user writes, not the rule of include/ops/occupancy.h, and its cells differ from the kernel's near midpoints.)
`rule2_share` is the share of the points whose cube cell lies outside the sphere.  Reported in ms as median [min, max].
Prints one JSON line per kind of data; `--out` also appends them to a file.  Without a GPU it stops: a time is measured
on the GPU or not at all.  Clocks are not touched."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=1024)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--resolution", type=int, default=28)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--composite-budget", type=float, default=60.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    reps = max(a.reps, 20)

    import torch

    if not torch.cuda.is_available():
        sys.exit("jsd_time: no GPU visible; a time is measured on the GPU or not at all")
    import sparenet_amd
    from sparenet_amd import _lib
    from sparenet_amd.utils.set_metrics import jensen_shannon_divergence, jsd_between_sets

    dev = torch.device("cuda:0")
    s, n, res = a.clouds, a.points, a.resolution
    axis = 2 * torch.arange(res) - (res - 1)
    inside = (axis[:, None, None] ** 2 + axis[None, :, None] ** 2 + axis[None, None, :] ** 2 <= (res - 1) ** 2).to(dev)
    centres = (torch.nonzero(inside).float() / (res - 1) - 0.5).contiguous()      # the published lattice, in linear order
    cell_of_centre = torch.nonzero(inside.reshape(-1))[:, 0]

    def make(kind, seed):
        g = torch.Generator().manual_seed(seed)
        v = torch.randn(s, n, 3, generator=g)
        v = v / v.norm(dim=2, keepdim=True)
        u = torch.rand(s, n, 1, generator=g)
        r = 0.5 * u ** (1.0 / 3.0) if kind == "ball" else 0.49 + 0.01 * u
        return (v * r).to(dev).contiguous()

    def rule2_share(x):
        i = torch.ceil(x.double() * (res - 1) + 0.5 * (res - 1) - 0.5).clamp(0, res - 1).long()
        return 1.0 - inside[i[..., 0], i[..., 1], i[..., 2]].double().mean().item()

    def event():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def timed(fn):
        e0 = event()
        fn()
        return e0, event()

    def summary(values_ms):
        return {"median": round(statistics.median(values_ms), 4), "min": round(min(values_ms), 4),
                "max": round(max(values_ms), 4)}

    def composite_counts(x, chunk=16384):
        pts = x.reshape(-1, 3)
        counts = torch.zeros(res ** 3, dtype=torch.int64, device=dev)
        for start in range(0, pts.size(0), chunk):
            nearest = torch.cdist(pts[start:start + chunk], centres).argmin(dim=1)
            counts += torch.bincount(cell_of_centre[nearest], minlength=res ** 3)
        return counts

    for kind in ("ball", "shell"):
        gen, ref = make(kind, 0), make(kind, 1)
        counts = torch.empty(res ** 3, dtype=torch.int64, device=dev)
        occupied = torch.empty(res ** 3, dtype=torch.int32, device=dev)
        ws = _lib.op_workspace("occupancy", "sn_occupancy_grid_workspace_bytes", gen, s, n, res, 1)

        def grid():
            _lib.op_call("occupancy", "sn_occupancy_grid", gen, None, s, n, res, 1, counts, occupied, None, ws)

        cells = torch.empty(s, n, dtype=torch.int32, device=dev)

        def cells_only():
            _lib.op_call("occupancy", "sn_occupancy_grid", gen, None, s, n, res, 1, None, None, cells, ws)

        def jsd():
            return jsd_between_sets(gen, ref, res)

        def composite(clouds):
            return jensen_shannon_divergence(composite_counts(gen[:clouds]), composite_counts(ref[:clouds]))

        for _ in range(a.warmup):
            grid(), cells_only(), jsd()
        torch.cuda.synchronize()
        rounds = [(timed(grid), timed(jsd), timed(cells_only)) for _ in range(reps)]
        torch.cuda.synchronize()
        ms = [[r[i][0].elapsed_time(r[i][1]) for r in rounds] for i in range(3)]

        def composite_ms(clouds, rounds_):
            for _ in range(2):
                composite(clouds)
            torch.cuda.synchronize()
            pairs = [timed(lambda: composite(clouds)) for _ in range(rounds_)]
            torch.cuda.synchronize()
            return [p0.elapsed_time(p1) for p0, p1 in pairs]

        part = min(32, s)
        one = composite_ms(part, 5)
        whole = statistics.median(one) * s / part
        extrapolated = part < s and whole * 7 > a.composite_budget * 1000.0
        comp = [t * s / part for t in one] if extrapolated or part == s else composite_ms(s, 5)
        out = {"bench": "jsd_time", "data": kind, "clouds": s, "points": n, "resolution": res, "reps": reps,
               "warmup": a.warmup, "rule2_share": round(rule2_share(gen), 4), "grid_ms": summary(ms[0]),
               "cells_ms": summary(ms[2]),
               "jsd_ms": summary(ms[1]), "composite_ms": summary(comp), "composite_extrapolated": extrapolated,
               "jsd": jsd().item(), "composite_jsd": composite(part).item() if part == s else None,
               "build_id": sparenet_amd.lib().sn_build_id().decode(), "device": torch.cuda.get_device_name(0)}
        line = json.dumps(out)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
