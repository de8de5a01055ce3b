"""Normal estimation on one GPU: the PCA kernel beside the search that feeds it and beside the torch composite it
replaces, in the same process.

    python tools/normals_time.py [--clouds 32] [--points 16384] [--k 16] [--reps 20] [--warmup 5]
                                 [--composite-budget 60] [--out FILE]

B clouds of N points (half of them noisy spheres, half uniform cubes, seeded), each point's k nearest neighbours.
After `--warmup` untimed rounds, `--reps` (at least 20) timed rounds ALTERNATE three calls, each bracketed by device
events:
  pca            sn_local_pca alone on the finished table: normals, eigenvalues and frames (the library call, no wrapper)
  knn            sn_knn_query alone (the library call, no wrapper): the search that wrote the table
  estimate       estimate_normals(xyz, k): search plus PCA through the Python wrappers
and then the torch composite -- xyz gathered to [B,N,k,3] in float64, centred, the covariance by a batched matmul,
torch.linalg.eigh -- is timed on its own (it allocates hundreds of MB and is far slower): first on ONE cloud; when
that time times B stays inside `--composite-budget` seconds for all its rounds, on the whole batch with the same
warm-up and 5 rounds, otherwise the one-cloud median times B is reported and marked as extrapolated.
Reported in ms as median [min, max].  The gate: `pca` must not exceed `knn` (the search is O(n) per query, the PCA O(k));
the JSON line says so and the exit status is 1 when it does not hold.  Prints one JSON line; `--out` also appends it to
a file.  Without a GPU it stops: a time is measured on the GPU or not at all.  Clocks are not touched."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=32)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--composite-budget", type=float, default=60.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    reps = max(a.reps, 20)

    import torch

    if not torch.cuda.is_available():
        sys.exit("normals_time: no GPU visible; a time is measured on the GPU or not at all")
    import sparenet_amd
    from sparenet_amd import _lib
    from sparenet_amd.cuda.normals import estimate_normals

    dev = torch.device("cuda:0")
    b, n, k = a.clouds, a.points, a.k
    g = torch.Generator().manual_seed(0)
    p = torch.randn(b, n, 3, generator=g)
    xyz = 0.5 * p / p.norm(dim=2, keepdim=True) + 0.002 * torch.randn(b, n, 3, generator=g)
    xyz[b // 2:] = torch.rand(b - b // 2, n, 3, generator=g)
    xyz = xyz.to(dev).contiguous()
    idx = torch.empty(b, n, k, dtype=torch.int32, device=dev)
    dist2 = torch.empty(b, n, k, device=dev)
    normals = torch.empty(b, n, 3, device=dev)
    values = torch.empty(b, n, 3, dtype=torch.float64, device=dev)
    frames = torch.empty(b, n, 3, 3, device=dev)

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

    def knn():
        _lib.op_call("neighbors", "sn_knn_query", xyz, xyz, b, n, n, k, None, None, idx, dist2, None)

    def pca():
        _lib.op_call("local_pca", "sn_local_pca", xyz, idx, b, n, n, k, None, None, values, frames, normals, None)

    def estimate():
        estimate_normals(xyz, k)

    def composite(points, table):
        """What a user writes without the op: gather, centre, covariance, a generic batched eigensolver."""
        nb = torch.gather(points.double()[:, None].expand(-1, table.size(1), -1, -1), 2,
                          table.long()[:, :, :, None].expand(-1, -1, -1, 3))
        d = nb - nb.mean(dim=2, keepdim=True)
        w, v = torch.linalg.eigh(d.transpose(2, 3) @ d / table.size(2))
        return v[..., 0].float(), w

    knn()
    for _ in range(a.warmup):
        pca(), knn(), estimate()
    torch.cuda.synchronize()
    rounds = [(timed(pca), timed(knn), timed(estimate)) for _ in range(reps)]
    torch.cuda.synchronize()
    ms = [[r[i][0].elapsed_time(r[i][1]) for r in rounds] for i in range(3)]

    def composite_ms(clouds, rounds_):
        for _ in range(2):
            composite(xyz[:clouds], idx[:clouds])
        torch.cuda.synchronize()
        pairs = [timed(lambda: composite(xyz[:clouds], idx[:clouds])) for _ in range(rounds_)]
        torch.cuda.synchronize()
        return [p0.elapsed_time(p1) for p0, p1 in pairs]

    one = composite_ms(1, 5)
    whole = statistics.median(one) * b
    extrapolated = whole * 7 > a.composite_budget * 1000.0
    comp = [t * b for t in one] if extrapolated else composite_ms(b, 5)

    res = {"bench": "normals_time", "clouds": b, "points": n, "k": k, "reps": reps, "warmup": a.warmup,
           "pca_ms": summary(ms[0]), "knn_ms": summary(ms[1]), "estimate_ms": summary(ms[2]),
           "composite_ms": summary(comp), "composite_one_cloud_ms": summary(one), "composite_extrapolated": extrapolated,
           "gate_pca_not_above_knn": statistics.median(ms[0]) <= statistics.median(ms[1]),
           "build_id": sparenet_amd.lib().sn_build_id().decode(), "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    sys.exit(0 if res["gate_pca_not_above_knn"] else 1)


if __name__ == "__main__":
    main()
