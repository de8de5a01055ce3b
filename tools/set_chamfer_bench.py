"""The Chamfer matrix between two sets of clouds: the set-level kernel against the only route without it, on one GPU.

    python tools/set_chamfer_bench.py [--clouds 128] [--points 2048] [--reps 9] [--warmup 3] [--out FILE]

Times, between device events on the current stream,
  matrix  chamfer_matrix(gen, ref) (sparenet_amd/cuda/set_distance.py): two sn_set_chamfer_sums launches and the
          float64 combination;
  loop    per generated cloud one ChamferDistanceFunction call against the whole reference set, the cloud expanded to
          a batch, the per-pair means taken in torch -- G calls that each write [R, n] distances and indices.
Both on the same data (uniform clouds, the time does not depend on the coordinates beyond the loop's pruned search),
after `--warmup` untimed passes of each, `--reps` timed passes alternating between the two; the medians are reported.
Point pairs per second counts 2 G R n m pairs per matrix (both directions).  The two matrices are compared: the loop
rounds its means to fp32, so they agree to fp32 rounding.  Prints one JSON line; `--out` also writes it to a file.
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
    ap.add_argument("--clouds", type=int, default=128)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import sparenet_amd
    from sparenet_amd.cuda.chamfer_distance import ChamferDistanceFunction
    from sparenet_amd.cuda.set_distance import chamfer_matrix

    if not torch.cuda.is_available():
        sys.exit("set_chamfer_bench: no GPU visible; a time is measured on the GPU or not at all")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    G = R = a.clouds
    n = m = a.points
    gen = (torch.rand(G, n, 3, generator=g) - 0.5).to(dev)
    ref = (torch.rand(R, m, 3, generator=g) - 0.5).to(dev)

    def matrix():
        return chamfer_matrix(gen, ref)

    def loop():
        rows = []
        for i in range(G):
            d1, d2 = ChamferDistanceFunction.apply(gen[i:i + 1].expand(R, n, 3), ref)
            rows.append(d1.mean(dim=1) + d2.mean(dim=1))
        return torch.stack(rows)

    def timed(fn):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        out = fn()
        end.record()
        end.synchronize()
        return start.elapsed_time(end), out

    for _ in range(a.warmup):
        matrix(), loop()
    torch.cuda.synchronize()
    t_matrix, t_loop = [], []
    for _ in range(a.reps):
        ms, cd_new = timed(matrix)
        t_matrix.append(ms)
        ms, cd_old = timed(loop)
        t_loop.append(ms)
    med_matrix, med_loop = statistics.median(t_matrix), statistics.median(t_loop)
    pairs = 2.0 * G * R * n * m
    res = {"bench": "set_chamfer", "clouds": [G, R], "points": [n, m], "reps": a.reps, "warmup": a.warmup,
           "matrix_ms": med_matrix, "matrix_min_ms": min(t_matrix), "matrix_max_ms": max(t_matrix),
           "loop_ms": med_loop, "loop_min_ms": min(t_loop), "loop_max_ms": max(t_loop),
           "loop_over_matrix": med_loop / med_matrix,
           "matrix_point_pairs_per_s": pairs / (med_matrix * 1e-3), "loop_point_pairs_per_s": pairs / (med_loop * 1e-3),
           "max_rel_diff_matrix_vs_loop": float(((cd_new - cd_old.double()).abs() / cd_new).max()),
           "build_id": sparenet_amd.lib().sn_build_id().decode(), "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
