"""Sliced Wasserstein distance on one GPU, forward plus gradients, beside the two other transport losses.

    python tools/swd_time.py [--clouds 32] [--slices 128] [--p 2] [--reps 20] [--window-ms 250] [--sweep]
                             [--regimes uniform,scatter] [--skip-yardsticks] [--out FILE]

Per regime of bench.py's emd_regime_clouds (`uniform`: two independent uniform cubes; `scatter`: prediction = ground
truth on a sphere + uniform offsets up to +-0.3), B clouds of 16384 against 16384 points, each measured with device
events around at least `--reps` calls and at least `--window-ms` of work, after as much untimed work (the first calls
load code and the clock follows the load), ms per call, Python wrapper and autograd included:
  swd            sliced_wasserstein(x, y, directions=<L fixed unit vectors>, p).sum().backward()
  project_sort   sorted_projections(x, dirs) alone: the sort launch of ONE side for all L slices (the forward runs it for
                 both sides, in chunks) -- what is left of `swd` after twice this is the transport, the accumulation and
                 the wrapper
  sinkhorn       sinkhorn_divergence(x, y, eps=0.01) at its defaults (20 iterations), .sum().backward()
  emd            emdModule()(x, y, 0.005, 50): dist.mean().backward()
  chunk=<c>      with `--sweep`: `swd` again with SN_SWD_CHUNK forced to 2 ... 64 slices per launch (the library's own
                 choice is max(1, 512 / B)) -- the measurement the default rests on
Prints one JSON line per regime; `--out` also appends the lines to a file.  Without a GPU it stops: a time is measured
on the GPU or not at all.  Clocks are not touched."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("SN_KNOBS_PER_CALL", "1")      # the chunk width is switched inside this process

REGIMES = ("uniform", "scatter")
SINKHORN_EPS, EMD_EPS, EMD_ITERS = 0.01, 0.005, 50


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=32)
    ap.add_argument("--slices", type=int, default=128)
    ap.add_argument("--p", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--window-ms", type=float, default=250.0)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--regimes", default=",".join(REGIMES))
    ap.add_argument("--skip-yardsticks", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("swd_time: no GPU visible; a time is measured on the GPU or not at all")
    import bench
    import sparenet_amd
    from sparenet_amd.cuda.emd.emd_module import emdModule
    from sparenet_amd.cuda.sinkhorn import sinkhorn_divergence
    from sparenet_amd.cuda.swd import random_directions, sliced_wasserstein, sorted_projections

    dev = torch.device("cuda:0")

    def measure(fn):
        fn()      # code objects, allocator
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        reps = max(a.reps, 1, int(a.window_ms / max(e0.elapsed_time(e1), 1e-3)) + 1)
        for _ in range(reps):      # as much untimed work as the window holds
            fn()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    dirs = random_directions(a.slices, dev, torch.Generator().manual_seed(99))
    emd = emdModule()
    for name in a.regimes.split(","):
        x, y = bench.emd_regime_clouds(name, a.clouds, dev)
        x, y = x.requires_grad_(True), y.requires_grad_(True)

        def step(loss):
            x.grad = y.grad = None
            loss().backward()

        res = {"bench": "swd_time", "regime": name, "clouds": a.clouds, "n": x.size(1), "m": y.size(1),
               "slices": a.slices, "p": a.p, "min_reps": a.reps, "window_ms": a.window_ms}
        res["swd_ms"] = measure(lambda: step(lambda: sliced_wasserstein(x, y, p=a.p, directions=dirs).sum()))
        res["project_sort_ms"] = measure(lambda: sorted_projections(x, dirs))
        if a.sweep:
            for c in (2, 4, 8, 16, 32, 64):
                os.environ["SN_SWD_CHUNK"] = str(c)
                res[f"chunk={c}"] = measure(lambda: step(lambda: sliced_wasserstein(x, y, p=a.p, directions=dirs).sum()))
            os.environ.pop("SN_SWD_CHUNK", None)
        if not a.skip_yardsticks:
            res["sinkhorn_ms"] = measure(lambda: step(lambda: sinkhorn_divergence(x, y, SINKHORN_EPS).sum()))
            res["emd_ms"] = measure(lambda: step(lambda: emd(x, y, EMD_EPS, EMD_ITERS)[0].mean()))
        res["build_id"] = sparenet_amd.lib().sn_build_id().decode()
        res["device"] = torch.cuda.get_device_name(0)
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
