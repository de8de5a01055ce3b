"""Golden vectors for the Frechet Point-cloud Distance: the reference's OWN Frechet/pointnet.py and Frechet/FPD.py,
imported from the reference checkout at run time (nothing of their text is stored in this repository) and executed
on the CPU.  FPD.py imports scipy.misc.imread, which no longer exists; a stand-in for that one name is put into
scipy.misc before the import (the name is never called).  The pretrained classifier is not available: the weights
are the recipe of tests/fpd_ref.py, loaded into the reference's own PointNetCls(k=16).

Per case and set one file  fpd_<case>_set<i>.npz:  act64 [n, 1808] float64 (the reference model run in float64),
act32 [n, 1808] float32 (the reference as shipped), and in set 1 the scalars fpd_ref64 / fpd_ref32 from the
reference's own calculate_frechet_distance (scipy sqrtm) on the float64 / fp32 activations.  Covariances are 26 MB
each and are not stored.  Needs scipy; run:  python tests/golden/gen_fpd.py [reference checkout]"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import fpd_ref  # noqa: E402


def import_reference(ref_root):
    import scipy.misc

    if not hasattr(scipy.misc, "imread"):
        scipy.misc.imread = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("stand-in"))
    sys.modules.setdefault("scipy.misc", scipy.misc)
    sys.path.insert(0, ref_root)
    try:
        import Frechet.FPD as ref_fpd
        import Frechet.pointnet as ref_pointnet
    finally:
        sys.path.remove(ref_root)
    assert os.path.abspath(ref_fpd.__file__).startswith(os.path.abspath(ref_root))
    return ref_pointnet, ref_fpd


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SPARENET_REFERENCE", "/root/reference")
    ref_pointnet, ref_fpd = import_reference(ref_root)
    torch.manual_seed(0)
    m32 = fpd_ref.load_recipe(ref_pointnet.PointNetCls(k=16))
    m64 = fpd_ref.load_recipe(ref_pointnet.PointNetCls(k=16)).double()
    keys = {k: tuple(v.shape) for k, v in m32.state_dict().items()}
    assert keys == {k: tuple(s) for k, s in fpd_ref.STATE_SHAPES.items()}, "fpd_ref.STATE_SHAPES is out of date"
    prov = "reference Frechet/pointnet.py PointNetCls(k=16) + Frechet/FPD.py on the CPU, imported at run time; " \
           f"weights: tests/fpd_ref.py recipe seed {fpd_ref.WEIGHT_SEED}; torch {torch.__version__}, numpy {np.__version__}"
    for name, (k1, k2, count, n, bs, seed) in fpd_ref.CASES.items():
        sets = fpd_ref.case_clouds(name)
        acts = []
        for pc in sets:
            if pc is None:
                continue
            t = torch.from_numpy(pc)
            with torch.no_grad():
                a64 = ref_fpd.get_activations(t.double(), m64, bs, 1808, None)
                a32 = ref_fpd.get_activations(t, m32, bs, 1808, None)
            acts.append((a64, a32.astype(np.float32)))
        extra = {}
        if len(acts) == 2:
            for tag, j in (("fpd_ref64", 0), ("fpd_ref32", 1)):
                a, b = acts[0][j].astype(np.float64), acts[1][j].astype(np.float64)
                extra[tag] = np.float64(ref_fpd.calculate_frechet_distance(
                    np.mean(a, axis=0), np.cov(a, rowvar=False), np.mean(b, axis=0), np.cov(b, rowvar=False)))
        for i, (a64, a32) in enumerate(acts):
            np.savez(os.path.join(HERE, f"fpd_{name}_set{i + 1}.npz"), act64=a64, act32=a32,
                     provenance=np.array(prov), **(extra if i == 0 else {}))
        print(name, [a[0].shape for a in acts], {k: float(v) for k, v in extra.items()}, flush=True)


if __name__ == "__main__":
    main()
