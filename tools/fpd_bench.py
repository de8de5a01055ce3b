"""FPD activations: the fused PointNet kernel against the same module on stock torch layers, on one GPU.

    python tools/fpd_bench.py [--out profiles/fpd_bench.json] [--sizes 16384,2048] [--clouds 30,150]

One parent process that never opens the GPU; every measurement is a fresh child under its own `timeout`, and the
first failing child ends the run.  Per (clouds, points, path): warm-up, then the median of `--reps` timed
get_activations-style passes (batch = 30 clouds, the reference's evaluation batch) between device synchronisations,
torch.cuda.max_memory_allocated for the pass, and for the fused path the share of the fp32 matrix peak (157.3 TFLOP/s)
that the exactly known flop count 2 n (3*3 + 64*3 + 128*64 + 1024*128) per cloud and pass (two passes) amounts to --
on the whole forward, dense layers and transposes included.  `--stock` inside a child forces the module onto the
torch layers (PointNetCls's CPU-path code on CUDA tensors): a switch of this tool, not of the package.
Clocks are not touched; weights are random (time does not depend on them)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 157.3e12
BATCH = 30


def child(clouds, n, stock, reps, warmup):
    import torch

    import sparenet_amd
    from sparenet_amd.Frechet import pointnet

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = pointnet.PointNetCls(k=16)
    for m in model.modules():    # non-trivial batch-norm statistics
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_mean.normal_(0, 0.2)
            m.running_var.uniform_(0.5, 2.0)
    model.eval().to(dev)
    if stock:
        pointnet._PoolMLP.force_torch = True
    pcs = (torch.rand(clouds, n, 3) - 0.5).to(dev)

    def run():
        out = []
        for s in range(0, clouds, BATCH):
            out.append(model(pcs[s:s + BATCH].transpose(1, 2))[2])
        return torch.cat(out)

    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        act = run()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    med = statistics.median(times)
    flop = 2.0 * 2 * n * (3 * 3 + 64 * 3 + 128 * 64 + 1024 * 128) * clouds
    res = {"clouds": clouds, "points": n, "path": "stock" if stock else "fused", "median_ms": med * 1e3,
           "min_ms": min(times) * 1e3, "max_ms": max(times) * 1e3, "reps": reps,
           "peak_mem_mb": (torch.cuda.max_memory_allocated() - base) / 2 ** 20,
           "tflops": flop / med / 1e12, "share_of_fp32_matrix_peak": flop / med / PEAK,
           "checksum": float(act.double().abs().sum()), "build_id": sparenet_amd.lib().sn_build_id().decode(),
           "device": torch.cuda.get_device_name(0)}
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="16384,2048")
    ap.add_argument("--clouds", default="30,150")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-timeout", type=int, default=150)
    ap.add_argument("--child", nargs=3, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(int(a.child[0]), int(a.child[1]), a.child[2] == "stock", a.reps, a.warmup)
        return 0
    results = []
    for n in (int(s) for s in a.sizes.split(",")):
        for clouds in (int(s) for s in a.clouds.split(",")):
            for path in ("fused", "stock"):
                cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--reps",
                       str(a.reps), "--warmup", str(a.warmup), "--child", str(clouds), str(n), path]
                p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                if p.returncode != 0 or not line:
                    print(p.stdout[-2000:])
                    print(f"step {clouds} x {n} {path} ended with status {p.returncode}: stopping", flush=True)
                    if a.out and results:
                        json.dump(results, open(a.out, "w"), indent=1)
                    return 1
                results.append(json.loads(line[0][7:]))
                r = results[-1]
                print(f"{clouds:4d} x {n:6d} {path:5s}: {r['median_ms']:9.3f} ms  {r['tflops']:6.1f} TFLOP/s "
                      f"({100 * r['share_of_fp32_matrix_peak']:.1f} % of peak)  peak memory {r['peak_mem_mb']:8.1f} MB", flush=True)
    if a.out:
        json.dump(results, open(a.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
