"""Record what every workspace size export of the C ABI returns over a grid of shapes.

    python tools/record_workspace_sizes.py [path/to/libsparenet_hip.so] [out.json]

The size exports are pure host code: no GPU is needed.  The output is the table tests/test_workspace_layout.py
compares the library with -- {export: [[argument, ..., result], ...]}.  It pins the sizes (and sn_emd_diag_offset)
of a KNOWN-GOOD build: record it from the commit before a change of the layout functions, not from the change itself.
A new size export gets its grid here; the test fails until the table has rows for it.
"""
import ctypes
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (1, 3, 32)


def _bnm():
    """(b, n, m) for the ops over two clouds: n != m both ways, sizes that are no multiples of 64, the invalid ones."""
    shapes = [(2048, 2304), (2304, 2048), (1000, 777), (63, 65), (1, 1), (16384, 16384), (3000, 16384), (16000, 16000)]
    rows = [(b, n, m) for b in BATCHES for n, m in shapes]
    return rows + [(0, 1024, 1024), (1, 0, 1024), (1, 1024, 0), (-1, -1, -1)]


def _images():
    return [(32, 1, 224, 224), (2, 3, 32, 32), (1, 1, 7, 9), (3, 4, 100, 60),
            (0, 1, 8, 8), (1, 0, 8, 8), (1, 1, 0, 8), (1, 1, 8, 0)]


def grid():
    """{export: [argument tuples]} -- every branch of every size function."""
    emd = [(b, n) for b in BATCHES for n in (1024, 8192, 16384)]
    g = {
        "sn_emd_workspace_bytes": emd + [(0, 1024), (1, 0), (-1, -1)],
        "sn_emd_diag_offset": emd,
        # persistent shapes (n == m, a multiple of 1024, b <= 512: the larger of the two layouts) and their neighbours
        # (b = 513, n != m, n no multiple of 1024: the stream-ordered auction's own layout); m < n is invalid
        "sn_emd_general_workspace_bytes": _bnm() + [(b, n, n) for b in (1, 32, 512, 513) for n in (1024, 2048, 1025)]
        + [(1, 2048, 1024)],
        "sn_emd_ragged_workspace_bytes": _bnm(),
        "sn_emd_general_backward_workspace_bytes": _bnm(),
        "sn_emd_ragged_backward_workspace_bytes": _bnm(),
        # below the clustered kernel, its range [2048, 19456], the workspace-free kernels up to 24 points per thread,
        # the generic kernel beyond
        "sn_mds_workspace_bytes": [(b, n) for b in BATCHES for n in (1, 100, 1023, 2047, 2048, 19384, 19456, 19457,
                                                                      24 * 1024, 24 * 1024 + 1, 30000)]
        + [(0, 2048), (1, 0)],
        "sn_chamfer_workspace_bytes": _bnm(),
        "sn_chamfer_backward_workspace_bytes": _bnm(),
        "sn_chamfer_backward_ragged_workspace_bytes": _bnm(),
        "sn_expansion_workspace_bytes": [(b, n, p) for b in BATCHES for n, p in ((16384, 512), (1024, 64), (768, 384),
                                                                                 (100, 7), (8, 2))]
        + [(0, 1024, 64), (1, 0, 64), (1, 1024, 0)],
        "sn_p2i_max_workspace_bytes": _images(),
        "sn_p2i_max_backward_workspace_bytes": _images(),
        "sn_p2i_f64_workspace_bytes": _images(),
        # many points on a small image: the tile layout is the larger; few points on a large one: the pixel layout
        "sn_p2i_max_multi_workspace_bytes": [(p,) + im for p, im in itertools.product(
            (0, 1, 512, 100000, 32 * 16384), _images()[:4])] + [(-1, 1, 1, 8, 8), (10, 0, 1, 8, 8), (10, 1, 0, 8, 8),
                                                                 (10, 1, 1, 0, 8), (10, 1, 1, 8, 0)],
        "sn_p2i_max_backward_multi_workspace_bytes": [(p, c) for p in (0, 1, 3, 5, 1023, 32 * 16384) for c in (1, 2, 3)]
        + [(-1, 1), (5, 0)],
        "sn_knn_workspace_bytes": [(b, n) for b in BATCHES for n in (1, 63, 2048, 16384)] + [(0, 8), (8, 0)],
        "sn_graph_feature_backward_workspace_bytes": [(b, n, k) for b in BATCHES for n in (1, 63, 2048) for k in (1, 8, 20)]
        + [(0, 8, 8), (8, 0, 8), (8, 8, 0)],
        # one point, both sides of a tile boundary (128 points), the largest cloud and one point more (invalid)
        "sn_pointnet_pool_workspace_bytes": [(b, n) for b in BATCHES for n in (1, 127, 128, 129, 2048, 16384, 1 << 20,
                                                                                   (1 << 20) + 1)]
        + [(0, 128), (1, 0)],
    }
    return g


def measure(lib_path):
    lib = ctypes.CDLL(lib_path)
    table = {}
    for name, rows in grid().items():
        fn = getattr(lib, name)
        fn.restype = ctypes.c_size_t
        fn.argtypes = [ctypes.c_int] * len(rows[0])
        table[name] = [list(r) + [int(fn(*r))] for r in rows]
    return table


def main():
    lib_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "sparenet_amd", "libsparenet_hip.so")
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "workspace_sizes.json")
    table = measure(lib_path)
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join(f' "{k}": [\n' + ",\n".join("  " + json.dumps(r) for r in v) + "\n ]"
                                   for k, v in table.items()) + "\n}\n")
    print(f"{sum(len(v) for v in table.values())} rows of {len(table)} exports from {lib_path} -> {out}")


if __name__ == "__main__":
    main()
