"""Voxel-grid subsampling and pooling on one GPU beside the torch composite a user has without them, in one process.

    python tools/voxel_grid_time.py [--reps 20] [--warmup 3] [--scale-reps 5] [--skip-scale] [--out FILE]

Per shape (B clouds of N points: 1 / 4 / 32 x 16384 and 32 x 2048), per kind of cloud (`uniform`: uniform cubes;
`scatter`: the prediction of bench.emd_regime_clouds, a sphere's surface + uniform offsets up to +-0.3) and per target
(about N/8 and about N/2 occupied voxels per cloud: the cell size is found by bisection on cloud 0 through the host entry
point, outside the timed region), `--reps` timed rounds after `--warmup` untimed ones ALTERNATE, each between device
events on the current stream, Python wrapper included:
  grid        voxel_grid(x, size): one sn_voxel_grid call, every output
  composite   the same subsampling from torch ops: cells packed into int64 keys (the cloud's number above them),
              torch.unique(return_inverse=True), index_add_ of the coordinates and of ones, a division
  pool        voxel_pool(features [B,64,N], grid, "mean")
  pool_composite   index_add_ of the transposed features through the composite's inverse, over the counts
and additionally the degenerate cloud whose points all fall into ONE voxel (1 x 16384: one lane adds 16384 terms) and
one shape of the workspace path (4 x 65536, uniform).  For scale only, at the 16384-point shapes on uniform clouds:
farthest_point_sample and minimum_density_sample 16384 -> 2048 (`--scale-reps` rounds).
Reported in ms as median [min, max], and composite / grid of the medians.  The composite's voxel count is compared
with the operator's (they apply the same cell rule in double; a difference is reported, not asserted).  Prints one JSON
line per measurement; `--out` also appends them to a file.  Without a GPU it stops: a time is measured on the GPU or not
at all.  Clocks are not touched."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1, 16384), (4, 16384), (32, 16384), (32, 2048)]
CHANNELS = 64


def composite_grid(x, size):
    """(centroids [V_total, 3], counts [V_total], inverse [B * N], voxels) of the batch from torch ops."""
    import torch

    b, n, _ = x.shape
    cell = torch.floor(x.double() / size).long() + 32768
    key = (cell[..., 0] << 32) | (cell[..., 1] << 16) | cell[..., 2]
    key = key + (torch.arange(b, device=x.device)[:, None] << 48)
    uniq, inverse = torch.unique(key.reshape(-1), return_inverse=True)
    sums = torch.zeros(uniq.numel(), 3, device=x.device).index_add_(0, inverse, x.reshape(-1, 3))
    counts = torch.zeros(uniq.numel(), device=x.device).index_add_(0, inverse, torch.ones(b * n, device=x.device))
    return sums / counts[:, None], counts, inverse, uniq.numel()


def composite_pool(features, counts, inverse):
    """Mean-pooled features [V_total, C] through the composite's inverse."""
    import torch

    b, c, n = features.shape
    rows = features.transpose(1, 2).reshape(b * n, c)
    return torch.zeros(counts.numel(), c, device=features.device).index_add_(0, inverse, rows) / counts[:, None]


def size_for(cloud, target):
    """The cell size at which the one cloud [1, N, 3] (CPU) has about `target` occupied voxels: bisection."""
    from sparenet_amd.cuda.voxel_grid import voxel_grid

    lo, hi = 1e-3, 2.0      # count falls as the size grows
    for _ in range(24):
        mid = (lo * hi) ** 0.5
        if int(voxel_grid(cloud, mid).count[0]) > target:
            lo = mid
        else:
            hi = mid
    return float(hi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale-reps", type=int, default=5)
    ap.add_argument("--skip-scale", action="store_true")
    ap.add_argument("--mml", type=float, default=0.0085)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("voxel_grid_time: no GPU visible; a time is measured on the GPU or not at all")
    import bench
    import sparenet_amd
    from sparenet_amd.cuda.fps import farthest_point_sample
    from sparenet_amd.cuda.MDS.MDS_module import minimum_density_sample
    from sparenet_amd.cuda.voxel_grid import voxel_grid, voxel_pool

    dev = torch.device("cuda:0")

    def event():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def span(fn):
        e0 = event()
        out = fn()
        return (e0, event()), out

    def summary(pairs):
        values = [p[0].elapsed_time(p[1]) for p in pairs]
        return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}

    def emit(res):
        res["build_id"] = sparenet_amd.lib().sn_build_id().decode()
        res["device"] = torch.cuda.get_device_name(0)
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    def measure(x, size, res, with_pool=True):
        b, n, _ = x.shape
        features = torch.rand(b, CHANNELS, n, generator=torch.Generator().manual_seed(n + b)).to(dev) if with_pool else None
        times = {"grid": [], "composite": [], "pool": [], "pool_composite": []}
        for r in range(a.warmup + a.reps):
            keep = r >= a.warmup
            t, grid = span(lambda: voxel_grid(x, size))
            if keep:
                times["grid"].append(t)
            t, (_, counts, inverse, voxels) = span(lambda: composite_grid(x, size))
            if keep:
                times["composite"].append(t)
            if with_pool:
                t, _ = span(lambda: voxel_pool(features, grid, "mean"))
                if keep:
                    times["pool"].append(t)
                t, _ = span(lambda: composite_pool(features, counts, inverse))
                if keep:
                    times["pool_composite"].append(t)
        torch.cuda.synchronize()
        res.update({"clouds": b, "points": n, "size": size, "reps": a.reps, "warmup": a.warmup,
                    "voxels_per_cloud": round(float(grid.count.float().mean()), 1),
                    "composite_voxels_differ_by": int(voxels - int(grid.count.sum()))})
        for name, pairs in times.items():
            if pairs:
                res[f"{name}_ms"] = summary(pairs)
        res["composite_over_grid"] = round(res["composite_ms"]["median"] / res["grid_ms"]["median"], 2)
        if with_pool:
            res["channels"] = CHANNELS
            res["pool_composite_over_pool"] = round(res["pool_composite_ms"]["median"] / res["pool_ms"]["median"], 2)
        emit(res)

    for b, n in SHAPES:
        clouds = {"uniform": torch.rand(b, n, 3, generator=torch.Generator().manual_seed(b * 100003 + n)),
                  "scatter": bench.emd_regime_clouds("scatter", b, torch.device("cpu"))[0][:, :n].contiguous()}
        for kind, x in clouds.items():
            for share in (8, 2):
                size = size_for(x[:1], n // share)
                measure(x.to(dev), size, {"bench": "voxel_grid_time", "cloud": kind, "target": f"n/{share}"})
        if n == 16384 and not a.skip_scale:      # for scale only: the two samplers with chains of picks
            x = clouds["uniform"].to(dev)
            res = {"bench": "voxel_grid_time", "cloud": "uniform", "scale": "16384 -> 2048", "clouds": b, "points": n,
                   "reps": a.scale_reps}
            farthest_point_sample(x, 2048)
            pairs = [span(lambda: farthest_point_sample(x, 2048))[0] for _ in range(a.scale_reps)]
            torch.cuda.synchronize()
            res["fps_ms"] = summary(pairs)
            mml = torch.full((b,), a.mml, device=dev)
            try:      # its teams of workgroups can time out on a shared GPU: that is reported, not fatal to the rest
                minimum_density_sample(x, 2048, mml)
                pairs = [span(lambda: minimum_density_sample(x, 2048, mml))[0] for _ in range(a.scale_reps)]
                torch.cuda.synchronize()
                sparenet_amd.device_check("voxel_grid_time: minimum_density_sample")
                res["mds_ms"], res["mds_mean_mst_length"] = summary(pairs), a.mml
            except sparenet_amd.SparenetHipError as e:
                res["mds_error"] = str(e)
            emit(res)
    # every point in one voxel: one lane adds 16384 terms in sequence
    x = (torch.rand(1, 16384, 3, generator=torch.Generator().manual_seed(5)) * 0.5 + 0.25).to(dev)
    measure(x, 1.0, {"bench": "voxel_grid_time", "cloud": "one voxel", "target": "1"})
    # the workspace path
    x = torch.rand(4, 65536, 3, generator=torch.Generator().manual_seed(6))
    measure(x.to(dev), size_for(x[:1], 65536 // 8), {"bench": "voxel_grid_time", "cloud": "uniform", "target": "n/8",
                                                      "path": "workspace"})
    return 0


if __name__ == "__main__":
    sys.exit(main())
