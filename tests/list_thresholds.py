"""Clouds whose inverse neighbour lists have prescribed lengths, for the tests at the thresholds of sorted_lists.hpp
(tests/test_chamfer.py, tests/test_dcd_gpu.py): a list of up to 16 entries is insertion-sorted, up to 64 heap-sorted by
its lane, up to 16384 sorted in LDS by a workgroup, beyond that in place by one thread."""
import numpy as np

# list lengths on either side of every threshold: (queries, targets) = (165, 6) and (32769, 2)
COUNTS = [(1, 2, 16, 17, 64, 65), (16384, 16385)]


def clouds(counts, seed=0):
    """queries [1, sum(counts), 3], targets [1, len(counts), 3]: target k at (k, 0, 0), counts[k] queries within 0.01 of
    it, the queries in shuffled order."""
    rng = np.random.default_rng(seed + sum(counts))
    targets = np.zeros((1, len(counts), 3), np.float32)
    targets[0, :, 0] = np.arange(len(counts))
    queries = targets[0][np.repeat(np.arange(len(counts)), counts)] + rng.uniform(-0.005, 0.005, (sum(counts), 3))
    return queries[rng.permutation(len(queries))][None].astype(np.float32), targets
