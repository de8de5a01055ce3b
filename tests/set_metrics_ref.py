"""MMD-CD, COV-CD and 1-NNA-CD restated in numpy / float64 as plain loops over distance matrices -- the definitions the
product code (sparenet_amd/utils/set_metrics.py) is tested against -- and the relative gap between the best and the
second-best candidate of every arg-min the metrics take: where that gap is far above the rounding of the matrices, no
summation order can change a decision.

    cd_gr [G, R]  generated x reference      cd_gg [G, G]      cd_rr [R, R]
"""
import numpy as np


def lowest_argmin(values):
    """Index of the minimum of a 1-d sequence; the lowest index among equal minima."""
    best = 0
    for k in range(1, len(values)):
        if values[k] < values[best]:
            best = k
    return best


def mmd(cd_gr):
    cd_gr = np.asarray(cd_gr, np.float64)
    g, r = cd_gr.shape
    total = np.float64(0)
    for j in range(r):
        total += min(cd_gr[i, j] for i in range(g))
    return total / r


def cov(cd_gr):
    cd_gr = np.asarray(cd_gr, np.float64)
    g, r = cd_gr.shape
    matched = set()
    for i in range(g):
        matched.add(lowest_argmin(cd_gr[i]))
    return len(matched) / r


def _leave_one_out_rows(cd_gg, cd_gr, cd_rr):
    """Per cloud of the concatenation (generated first): (its distances to every cloud, its own index)."""
    cd_gg, cd_gr, cd_rr = (np.asarray(a, np.float64) for a in (cd_gg, cd_gr, cd_rr))
    g, r = cd_gr.shape
    assert cd_gg.shape == (g, g) and cd_rr.shape == (r, r)
    for a in range(g + r):
        row = []
        for b in range(g + r):
            if a < g:
                row.append(cd_gg[a, b] if b < g else cd_gr[a, b - g])
            else:
                row.append(cd_gr[b, a - g] if b < g else cd_rr[a - g, b - g])
        yield row, a


def one_nna(cd_gg, cd_gr, cd_rr):
    g, r = np.asarray(cd_gr).shape
    correct = 0
    for row, a in _leave_one_out_rows(cd_gg, cd_gr, cd_rr):
        others = [b for b in range(g + r) if b != a]
        nearest = others[lowest_argmin([row[b] for b in others])]
        correct += (nearest < g) == (a < g)
    return correct / (g + r)


def _gap(values):
    """(second smallest - smallest) / second smallest of a sequence of non-negative numbers; inf for fewer than two
    candidates, 0 for a tie (or for two zeros)."""
    if len(values) < 2:
        return np.inf
    lo, second = sorted(values)[:2]
    return (second - lo) / second if second > 0 else 0.0


def argmin_gaps(cd_gg, cd_gr, cd_rr):
    """The relative gap between the winner and the runner-up of every arg-min COV-CD (one per generated cloud, over the
    reference clouds) and 1-NNA-CD (one per cloud, over all the others) take, as a flat float64 array.  MMD-CD takes
    minima, not arg-minima: a near-tie moves it by no more than the matrices' own rounding."""
    cd_gr = np.asarray(cd_gr, np.float64)
    gaps = [_gap(list(cd_gr[i])) for i in range(cd_gr.shape[0])]
    for row, a in _leave_one_out_rows(cd_gg, cd_gr, cd_rr):
        gaps.append(_gap([v for b, v in enumerate(row) if b != a]))
    return np.array(gaps, np.float64)
