"""Neighbourhood queries on one GPU: the kernels against the torch composite a user has without them.

    python tools/neighbors_bench.py [--reps 20] [--warmup 3] [--sweep] [--skip-composite] [--out FILE]

Per shape (B clouds of N points, M queries, uniform in the unit cube) and op -- knn_query with k = 3 and k = 16,
ball_query with r = 0.1 and nsample = 32 -- the median, minimum and maximum of `--reps` synchronised wall-clock
passes after `--warmup` untimed ones:
  kernel     sparenet_amd.cuda.neighbors, split width chosen by the library (SN_NEIGHBORS_SPLIT unset);
  split=1    at the small shapes (N = 2048, M = 512: B = 1, 4, 32) the same with the split forced off; with `--sweep`
             every forced width 1, 2, 4, 8, 16 at every shape -- the measurement the dispatch rule rests on (a width
             above the k bucket's cap is held to it: k = 16 runs 8 under "16");
  composite  torch.cdist(...) ** 2 + topk for k-NN, a mask over the same matrix + sort for the ball query: the [B,M,N]
             matrix is materialised (4.3 GB at B = 32, N = 16384, M = 2048).  A shape for which it cannot be allocated is
             skipped and reported as such.  The composite's ties are its own: results are not compared here.
Prints one JSON line per shape and op, then the table; `--out` also appends the lines to a file.  Clocks are not
touched."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("SN_KNOBS_PER_CALL", "1")      # the split width is switched inside this process

SHAPES = [(32, 16384, 2048), (1, 2048, 512), (4, 2048, 512), (32, 2048, 512)]
OPS = [("knn k=3", "knn", 3), ("knn k=16", "knn", 16), ("ball r=0.1 nsample=32", "ball", 32)]
RADIUS = 0.1


def composite(kind, arg, x, q):
    import torch

    d2 = torch.cdist(q, x) ** 2                                   # [B, M, N]
    if kind == "knn":
        return torch.topk(d2, arg, dim=2, largest=False)
    n = x.size(1)
    key = torch.where(d2 < RADIUS * RADIUS, torch.arange(n, device=x.device, dtype=torch.int32)[None, None, :], n)
    return torch.sort(key, dim=2).values[:, :, :arg]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--skip-composite", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import sparenet_amd
    from sparenet_amd.cuda.neighbors import ball_query, knn_query

    if not torch.cuda.is_available():
        sys.exit("neighbors_bench: no GPU visible; a time is measured on the GPU or not at all")
    dev = torch.device("cuda:0")

    def measure(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(max(a.reps, 1)):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        return {"ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times)}

    def kernel(kind, arg, x, q):
        return knn_query(arg, x, q) if kind == "knn" else ball_query(RADIUS, arg, x, q)

    rows = []
    for b, n, m in SHAPES:
        gen = torch.Generator().manual_seed(b * 100003 + n)
        x, q = torch.rand(b, n, 3, generator=gen).to(dev), torch.rand(b, m, 3, generator=gen).to(dev)
        for label, kind, arg in OPS:
            res = {"bench": "neighbors", "op": label, "clouds": b, "points": n, "queries": m, "reps": a.reps,
                   "warmup": a.warmup}
            os.environ.pop("SN_NEIGHBORS_SPLIT", None)
            res["kernel"] = measure(lambda: kernel(kind, arg, x, q))
            if n == 2048 or a.sweep:
                for split in [1] + ([2, 4, 8, 16] if a.sweep else []):
                    os.environ["SN_NEIGHBORS_SPLIT"] = str(split)
                    res[f"split={split}"] = measure(lambda: kernel(kind, arg, x, q))
                os.environ.pop("SN_NEIGHBORS_SPLIT", None)
            if not a.skip_composite:
                try:
                    res["composite"] = measure(lambda: composite(kind, arg, x, q))
                except torch.OutOfMemoryError:
                    res["composite"] = None
                    res["composite_skipped"] = "the [B,M,N] matrix could not be allocated"
                torch.cuda.empty_cache()
            res["build_id"] = sparenet_amd.lib().sn_build_id().decode()
            res["device"] = torch.cuda.get_device_name(0)
            line = json.dumps(res)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
            rows.append(res)

    columns = ["kernel", "split=1"] + ([f"split={s}" for s in (2, 4, 8, 16)] if a.sweep else []) + ["composite"]
    print("\n| B | N | M | op | " + " | ".join(f"{c} ms" for c in columns) + " |")
    print("|" + "---|" * (4 + len(columns)))
    for r in rows:
        cells = []
        for c in columns:
            v = r.get(c)
            cells.append("skipped" if c == "composite" and "composite_skipped" in r else
                         ("-" if v is None else f"{v['ms']:.3f}"))
        print(f"| {r['clouds']} | {r['points']} | {r['queries']} | {r['op']} | " + " | ".join(cells) + " |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
