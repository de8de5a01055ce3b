"""Rigid registration on one GPU beside the torch composite a user has without it, in one process.

    python tools/registration_time.py [--reps 20] [--warmup 3] [--icp-reps 3] [--out FILE]

Per shape (B clouds of N points onto N points: 32 x 16384 and 4 x 2048) and per kind of cloud (`uniform`: uniform cubes;
`scatter`: the prediction and ground truth of bench.emd_regime_clouds), the source is the target's partner moved by 5
degrees about (1,2,3) and (0.05, -0.03, 0.02).  `--reps` timed rounds after `--warmup` untimed ones ALTERNATE, each
between device events on the current stream, Python wrapper included:
  apply        sn_rigid_apply: the transform of the source
  search       chamfer_search_raw(moved, dst): the exact search that feeds the step
  step_point   sn_rigid_step, mode 0 (both launches) on the search's matches
  step_plane   sn_rigid_step, mode 1, with normals estimated outside the timed region
  composite    one point-to-point step from torch ops: gather of the matches, masked float64 einsum sums,
               torch.linalg.svd, determinant fix, composition (no convergence test: that would add a host read)
and `--icp-reps` rounds of a whole icp(iters=30) in point mode.  Reported in ms as median [min, max], composite /
step_point of the medians, and the search's share of one iteration (apply + search + step_point).  The composite's
rotation is compared with the step's (a difference is reported, not asserted).  Prints one JSON line per measurement;
`--out` also appends them to a file.  Without a GPU it stops: a time is measured on the GPU or not at all.  Clocks are
not touched."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(32, 16384), (4, 2048)]


def composite_step(moved, dst, idx, pose):
    """pose' [B,4,4] float64 of one point-to-point step from torch ops (Kabsch by SVD with the determinant fix)."""
    import torch

    valid = idx >= 0
    q = torch.gather(dst, 1, idx.clamp_min(0).long()[:, :, None].expand(-1, -1, 3)).double()
    p = moved.double()
    w = valid.double()
    total = w.sum(dim=1).clamp_min(1.0)
    mp = torch.einsum("bn,bnc->bc", w, p) / total[:, None]
    mq = torch.einsum("bn,bnc->bc", w, q) / total[:, None]
    h = torch.einsum("bn,bni,bnj->bij", w, q - mq[:, None], p - mp[:, None])
    u, _, vt = torch.linalg.svd(h)
    fix = torch.ones(h.size(0), 3, dtype=h.dtype, device=h.device)
    fix[:, 2] = torch.sign(torch.linalg.det(u @ vt))
    r = u @ torch.diag_embed(fix) @ vt
    update = torch.zeros_like(pose)
    update[:, :3, :3], update[:, :3, 3], update[:, 3, 3] = r, mq - torch.einsum("bij,bj->bi", r, mp), 1.0
    return update @ pose


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--icp-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        sys.exit("registration_time: no GPU visible; a time is measured on the GPU or not at all")
    import bench
    import sparenet_amd
    from sparenet_amd.cuda import registration as reg
    from sparenet_amd.cuda.normals import estimate_normals
    from sparenet_amd.cuda.ragged import chamfer_search_raw

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

    axis = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)
    axis = axis / axis.norm()
    k = torch.tensor([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]], dtype=torch.float64)
    angle = math.radians(5.0)
    start = torch.eye(4, dtype=torch.float64)
    start[:3, :3] = torch.eye(3, dtype=torch.float64) + math.sin(angle) * k + (1 - math.cos(angle)) * (k @ k)
    start[:3, 3] = torch.tensor([0.05, -0.03, 0.02], dtype=torch.float64)

    for b, n in SHAPES:
        g = torch.Generator().manual_seed(b * 100003 + n)
        pred, gt = bench.emd_regime_clouds("scatter", b, torch.device("cpu"))[:2]
        pairs_of = {"uniform": (torch.rand(b, n, 3, generator=g), torch.rand(b, n, 3, generator=g)),
                    "scatter": (pred[:, :n].contiguous(), gt[:, :n].contiguous())}
        for kind, (x, y) in pairs_of.items():
            dst = y.to(dev)
            src = reg.transform_points(x.to(dev), start.to(dev))
            normals = estimate_normals(dst, 16)
            eye = torch.eye(4, dtype=torch.float64, device=dev)[None].repeat(b, 1, 1)
            one = torch.ones(b, dtype=torch.float64, device=dev)
            point = reg._Step(dst, None, None, None, n, 0, False, 0.0, 1e-6, 1e-7)
            plane = reg._Step(dst, normals, None, None, n, 1, False, 0.0, 1e-6, 1e-7)
            stats = torch.empty(b, 4, dtype=torch.float64, device=dev)
            times = {"apply": [], "search": [], "step_point": [], "step_plane": [], "composite": []}
            for r in range(a.warmup + a.reps):
                keep = r >= a.warmup
                pose, scale = eye.clone(), one.clone()
                state = torch.zeros(b, 4, dtype=torch.float64, device=dev)
                t_apply, moved = span(lambda: reg._apply(src, pose, scale, None))
                t_search, found = span(lambda: chamfer_search_raw(moved, dst))
                idx = found[2]
                t_point, _ = span(lambda: point(moved, idx, None, 1, pose, scale, state, stats))
                pose2, scale2, state2 = eye.clone(), one.clone(), torch.zeros_like(state)
                t_plane, _ = span(lambda: plane(moved, idx, None, 1, pose2, scale2, state2, stats))
                t_comp, theirs = span(lambda: composite_step(moved, dst, idx, eye))
                if keep:
                    for name, t in (("apply", t_apply), ("search", t_search), ("step_point", t_point),
                                    ("step_plane", t_plane), ("composite", t_comp)):
                        times[name].append(t)
            torch.cuda.synchronize()
            res = {"bench": "registration_time", "cloud": kind, "clouds": b, "points": n, "reps": a.reps, "warmup": a.warmup}
            for name, pairs in times.items():
                res[f"{name}_ms"] = summary(pairs)
            res["composite_over_step_point"] = round(res["composite_ms"]["median"] / res["step_point_ms"]["median"], 2)
            iteration = sum(res[f"{name}_ms"]["median"] for name in ("apply", "search", "step_point"))
            res["search_share_of_iteration"] = round(res["search_ms"]["median"] / iteration, 3)
            res["composite_rotation_differs_by"] = float((theirs[:, :3, :3] - pose[:, :3, :3]).abs().max())
            reg.icp(src, dst, iters=30)
            pairs = [span(lambda: reg.icp(src, dst, iters=30))[0] for _ in range(a.icp_reps)]
            torch.cuda.synchronize()
            res["icp30_ms"] = summary(pairs)
            emit(res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
