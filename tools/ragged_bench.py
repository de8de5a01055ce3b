"""Ragged Chamfer / EMD on one MI355X (sparenet_amd.cuda.ragged): ms per call, medians over alternating repetitions,
HIP events on the stream, after a warm-up of every shape.

  full    B = 32, 16384 x 16384, every length = 16384, forward + backward: the ragged Chamfer kernels next to the dense
          all-pairs kernels (sn_chamfer_forward + sn_chamfer_backward) with the dense kernels' own run-to-run spread,
          and the dense default dispatch (the sorted search at this size)
  ragged  32 clouds with lengths uniform in [2048, 16384] against 16384-point ground truth: ragged Chamfer forward and
          ragged EMD (0.005, 50 iterations) in one call each, next to 32 single-cloud dense calls

The dense side is this library's own dense entry points, not a build of the previous commit: the dense instantiations
of the templated kernels are the instruction streams they were ("Ragged batches"), the dense
entry points and their dispatch are untouched, so they time what the previous commit's library times.

python tools/ragged_bench.py [--reps R] [--json F]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import sparenet_amd  # noqa: E402
from sparenet_amd import _lib  # noqa: E402
from sparenet_amd.cuda.chamfer_distance.chamfer_distance import cd  # noqa: E402
from sparenet_amd.cuda.emd.emd_general import emd_general_forward_raw  # noqa: E402
from sparenet_amd.cuda.ragged import ChamferRaggedFunction, chamfer_ragged_forward_raw, emd_ragged  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(fns, reps, warmup=2):
    """{name: [ms, ...]}: the candidates take turns inside every repetition"""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            out[k].append(timed(f))
    return out


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ragged_bench: no GPU visible (timings are taken on the device only)")
    dev = torch.device("cuda:0")
    lib = sparenet_amd.lib()
    g = torch.Generator().manual_seed(0)
    B, N = 32, 16384
    x = torch.rand(B, N, 3, generator=g).to(dev)
    y = torch.rand(B, N, 3, generator=g).to(dev)
    gd1 = torch.randn(B, N, generator=g).to(dev)
    gd2 = torch.randn(B, N, generator=g).to(dev)
    full = torch.full((B,), N, dtype=torch.int32, device=dev)
    d1, d2 = torch.empty(B, N, device=dev), torch.empty(B, N, device=dev)
    i1, i2 = torch.empty(B, N, dtype=torch.int, device=dev), torch.empty(B, N, dtype=torch.int, device=dev)
    g1, g2 = torch.empty_like(x), torch.empty_like(y)

    def dense_allpairs():
        _lib.check(lib.sn_chamfer_forward(_lib.fptr(x, "x"), _lib.fptr(y, "y"), B, N, N, _lib.fptr(d1, "d"),
                                          _lib.iptr(i1, "i"), _lib.fptr(d2, "d"), _lib.iptr(i2, "i"),
                                          _lib.stream_of(x)), "sn_chamfer_forward")
        cd.backward_cuda(x, y, g1, g2, gd1, gd2, i1, i2)

    def dense_default():
        cd.forward_cuda(x, y, d1, d2, i1, i2)
        cd.backward_cuda(x, y, g1, g2, gd1, gd2, i1, i2)

    class Ctx:
        def save_for_backward(self, *t):
            self.saved_tensors = t

    def ragged_full():
        ctx = Ctx()
        ChamferRaggedFunction.forward(ctx, x, y, full, full)
        ChamferRaggedFunction.backward(ctx, gd1, gd2)

    res = {"build_id": lib.sn_build_id().decode(), "device": torch.cuda.get_device_name(0), "full_length": {}, "ragged": {}}
    t = alternate({"dense_allpairs_fwd_bwd": dense_allpairs, "ragged_fwd_bwd": ragged_full,
                   "dense_default_dispatch_fwd_bwd": dense_default}, args.reps)
    res["full_length"] = {k: summary(v) for k, v in t.items()}
    # same results at full length
    ra = chamfer_ragged_forward_raw(x, y, full, full)
    dense_allpairs()
    res["full_length"]["ragged_equals_dense_bits"] = bool(torch.equal(ra[0], d1) and torch.equal(ra[1], d2) and
                                                          torch.equal(ra[2], i1) and torch.equal(ra[3], i2))

    lengths = torch.randint(2048, N + 1, (B,), generator=g).to(torch.int32)
    lh = lengths.tolist()
    ld = lengths.to(dev)
    singles = [(x[i:i + 1, :n].contiguous(), y[i:i + 1].contiguous()) for i, n in enumerate(lh)]
    outs = [(torch.empty(1, n, device=dev), torch.empty(1, N, device=dev), torch.empty(1, n, dtype=torch.int, device=dev),
             torch.empty(1, N, dtype=torch.int, device=dev)) for n in lh]

    def chamfer_singles():
        for (a, b), (o1, o2, j1, j2) in zip(singles, outs):
            cd.forward_cuda(a, b, o1, o2, j1, j2)

    t = alternate({"chamfer_fwd_ragged_one_call": lambda: chamfer_ragged_forward_raw(x, y, ld, full),
                   "chamfer_fwd_32_single_dense_calls": chamfer_singles}, args.reps)
    res["ragged"].update({k: summary(v) for k, v in t.items()})
    t = alternate({"emd_ragged_one_call": lambda: emd_ragged(x, y, ld, full, 0.005, 50),
                   "emd_32_single_dense_calls": lambda: [emd_general_forward_raw(a, b, 0.005, 50) for a, b in singles]},
                  max(3, args.reps // 3), warmup=1)
    res["ragged"].update({k: summary(v) for k, v in t.items()})
    res["ragged"]["lengths_sum"] = int(sum(lh))
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
