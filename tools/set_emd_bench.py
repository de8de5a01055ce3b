"""The EMD matrix between two sets of clouds: the set-level kernel against the only route without it, on one GPU.

    python tools/set_emd_bench.py [--clouds 64] [--points 2048] [--geometry uniform|contested] [--eps 0.005]
                                  [--iters 50] [--reps 9] [--warmup 3] [--out FILE]

Times, between device events on the current stream,
  matrix  emd_matrix(gen, ref) as the package routes it (sparenet_amd/cuda/set_distance.py) -- `route` in the result
          says where: "kernel" is one sn_set_emd_sums launch, one workgroup per pair with the auction in LDS;
  kernel  the same through the kernel whatever the routing says (equal to `matrix` where the route is the kernel);
  loop    per generated cloud one emd_general call against the whole reference set, the cloud expanded to a batch, the
          per-pair means of sqrt(dist) taken in torch -- G calls (for n a multiple of 1024 the persistent auction).
All on the same data, after `--warmup` untimed passes of each, `--reps` timed passes alternating between them; the
medians are reported with the minimum and maximum of each, which is the run-to-run spread a routing decision must
exceed.  Geometry: `uniform` clouds in a cube, or `contested` -- targets on a sphere of radius 0.5, bidders = targets
plus uniform noise in [-1, 1]^3, hundreds of bidders per near-side target.  The matrices are compared (the same
per-bidder distances, two float64 summation orders).  Prints one JSON line; `--out` also writes it to a file.
Clocks are not touched."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=64)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--geometry", choices=("uniform", "contested"), default="uniform")
    ap.add_argument("--eps", type=float, default=0.005)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import sparenet_amd
    from sparenet_amd import _lib
    from sparenet_amd.cuda import set_distance
    from sparenet_amd.cuda.emd.emd_general import emd_general

    if not torch.cuda.is_available():
        sys.exit("set_emd_bench: no GPU visible; a time is measured on the GPU or not at all")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    G = R = a.clouds
    n = m = a.points
    if a.geometry == "uniform":
        gen = (torch.rand(G, n, 3, generator=g) - 0.5).to(dev)
        ref = (torch.rand(R, m, 3, generator=g) - 0.5).to(dev)
    else:
        ref = torch.randn(R, m, 3, generator=g)
        ref = 0.5 * ref / ref.norm(dim=2, keepdim=True)
        gen = (ref[torch.arange(G) % R] + 2 * torch.rand(G, n, 3, generator=g) - 1).contiguous().to(dev)
        ref = ref.contiguous().to(dev)
    per_n = torch.full((), float(n), dtype=torch.float64, device=dev)

    def matrix():
        return set_distance.emd_matrix(gen, ref, a.eps, a.iters)

    def kernel():
        sums = torch.empty(G, R, dtype=torch.float64, device=dev)
        _lib.topic_call("set_emd", "sn_set_emd_sums", gen, ref, G, n, R, m, a.eps, a.iters, sums, None)
        return sums / per_n

    def loop():
        rows = []
        for i in range(G):
            dist, _ = emd_general(gen[i:i + 1].expand(R, n, 3), ref, a.eps, a.iters)
            rows.append(dist.sqrt().double().sum(dim=1) / per_n)
        return torch.stack(rows)

    def timed(fn):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = fn()
        end.record()
        end.synchronize()
        return start.elapsed_time(end), out

    routed = set_distance._uses_emd_kernel(n, m)
    legs = {"matrix": matrix, "loop": loop}
    if not routed:
        legs["kernel"] = kernel
    for _ in range(a.warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    times, outs = {k: [] for k in legs}, {}
    for _ in range(a.reps):
        for k, fn in legs.items():
            ms, outs[k] = timed(fn)
            times[k].append(ms)
    if routed:
        times["kernel"], outs["kernel"] = times["matrix"], outs["matrix"]
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"bench": "set_emd", "clouds": [G, R], "points": [n, m], "geometry": a.geometry, "eps": a.eps,
           "iters": a.iters, "reps": a.reps, "warmup": a.warmup, "route": "kernel" if routed else "loop"}
    for k in ("matrix", "kernel", "loop"):
        res.update({f"{k}_ms": med[k], f"{k}_min_ms": min(times[k]), f"{k}_max_ms": max(times[k])})
    res.update({"loop_over_kernel": med["loop"] / med["kernel"], "loop_over_matrix": med["loop"] / med["matrix"],
                "max_rel_diff_kernel_vs_loop": float(((outs["kernel"] - outs["loop"]).abs()
                                                      / outs["loop"].clamp_min(1e-300)).max()),
                "mean_emd": float(outs["matrix"].mean()),
                "build_id": sparenet_amd.lib().sn_build_id().decode(), "device": torch.cuda.get_device_name(0)})
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
