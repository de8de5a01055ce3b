"""Farthest point sampling on one GPU: the kernel against the only route a user has without it.

    python tools/fps_bench.py [--reps 9] [--warmup 2] [--loop-reps 2] [--skip-loop] [--skip-mds] [--out FILE]

Times, between device events on the current stream, per shape (B clouds of N points, M picks: 16384 -> 2048 at
B = 1, 4, 32 and 2048 -> 512 at B = 32, 256):
  fps    farthest_point_sample(xyz, M) (sparenet_amd/cuda/fps): one sn_fps launch, one workgroup per cloud;
  loop   the same rule as a loop of torch ops on the same GPU -- per pick (x - x[c]) ** 2, sum, minimum, argmax -- a
         handful of launches per pick, which is what the time is made of (`--loop-reps` passes, it is slow);
  mds    for scale, minimum_density_sample 16384 -> 2048 at the same B with a fixed mean MST length (`--mml`): another
         sampler with another rule, not an alternative implementation.
Uniform clouds from a seed; `--warmup` untimed passes of every shape, then `--reps` timed passes; medians with minimum
and maximum, us per pick = the median over M.  The loop's picks are compared with the kernel's (torch's sum may round
differently from the kernel's order, so a differing pick is counted and reported, not asserted).  Prints one JSON line
per shape; `--out` also appends them to a file.  Clocks are not touched."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1, 16384, 2048), (4, 16384, 2048), (32, 16384, 2048), (32, 2048, 512), (256, 2048, 512)]


def torch_loop(x, m):
    """The rule of include/ops/fps.h in torch ops: [B, m] picks (int64)."""
    import torch

    b, n, _ = x.shape
    rows = torch.arange(b, device=x.device)
    mind = torch.full((b, n), float("inf"), device=x.device)
    c = torch.zeros(b, dtype=torch.long, device=x.device)
    picks = torch.empty(b, m, dtype=torch.long, device=x.device)
    for k in range(m):
        picks[:, k] = c
        d = ((x - x[rows, c][:, None, :]) ** 2).sum(dim=2)
        mind = torch.minimum(mind, d)
        c = mind.argmax(dim=1)
    return picks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop-reps", type=int, default=2)
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--skip-mds", action="store_true")
    ap.add_argument("--mml", type=float, default=0.0085)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import sparenet_amd
    from sparenet_amd.cuda.fps import farthest_point_sample
    from sparenet_amd.cuda.MDS.MDS_module import minimum_density_sample

    if not torch.cuda.is_available():
        sys.exit("fps_bench: no GPU visible; a time is measured on the GPU or not at all")
    dev = torch.device("cuda:0")

    def timed(fn):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = fn()
        end.record()
        end.synchronize()
        return start.elapsed_time(end), out

    def stats(prefix, times, m):
        med = statistics.median(times)
        return {f"{prefix}_ms": med, f"{prefix}_min_ms": min(times), f"{prefix}_max_ms": max(times),
                f"{prefix}_us_per_pick": med * 1e3 / m}

    for b, n, m in SHAPES:
        x = torch.rand(b, n, 3, generator=torch.Generator().manual_seed(b * 100003 + n)).to(dev)
        for _ in range(a.warmup):
            farthest_point_sample(x, m)
        torch.cuda.synchronize()
        t_fps = []
        for _ in range(a.reps):
            ms, idx = timed(lambda: farthest_point_sample(x, m))
            t_fps.append(ms)
        res = {"bench": "fps", "clouds": b, "points": n, "picks": m, "reps": a.reps, "warmup": a.warmup}
        res.update(stats("fps", t_fps, m))
        if not a.skip_loop:
            torch_loop(x, 8)      # warm-up: the loop's kernels are loaded before it is timed
            torch.cuda.synchronize()
            t_loop = []
            for _ in range(a.loop_reps):
                ms, picks = timed(lambda: torch_loop(x, m))
                t_loop.append(ms)
            res.update(stats("loop", t_loop, m))
            res["loop_reps"] = a.loop_reps
            res["loop_over_fps"] = res["loop_ms"] / res["fps_ms"]
            res["clouds_whose_loop_picks_differ"] = int((picks != idx.long()).any(dim=1).sum())
        if not a.skip_mds and n == 16384:
            mml = torch.full((b,), a.mml, device=dev)
            res["mds_mean_mst_length"] = a.mml
            try:      # its teams of workgroups can time out on a shared GPU: that is reported, not fatal to the rest
                minimum_density_sample(x, m, mml)
                torch.cuda.synchronize()
                t_mds = []
                for _ in range(a.reps):
                    ms, _ = timed(lambda: minimum_density_sample(x, m, mml))
                    t_mds.append(ms)
                sparenet_amd.device_check("fps_bench: minimum_density_sample")
                res.update(stats("mds", t_mds, m))
            except sparenet_amd.SparenetHipError as e:
                res["mds_error"] = str(e)
        res["build_id"] = sparenet_amd.lib().sn_build_id().decode()
        res["device"] = torch.cuda.get_device_name(0)
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
