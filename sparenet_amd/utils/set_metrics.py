"""The three set-level metrics published beside FPD for point-cloud generators and completion GANs, with the Chamfer
distance between clouds: minimum matching distance (MMD-CD), coverage (COV-CD) and 1-nearest-neighbour accuracy
(1-NNA-CD).  All three are read off the matrices of Chamfer distances between every generated and every reference
cloud (sparenet_amd.cuda.set_distance.chamfer_matrix); `set_metrics(..., with_emd=True)` adds the same three on the
matrices of auction EMDs (emd_matrix): MMD-EMD, COV-EMD and 1-NNA-EMD.  The fourth number of the same tables, the
Jensen-Shannon divergence between the two sets' occupancy distributions on a 28^3 grid clipped to the unit sphere
(Achlioptas et al. 2018), needs no pairwise distance: `jsd_between_sets` reads it off two occupancy grids
(sparenet_amd.cuda.occupancy), and `set_metrics(..., with_jsd=True)` adds it as "JSD".

The metric functions are plain torch on float64 matrices and work on any device, CPU included; only `set_metrics`
itself, which computes the matrices, needs the GPU (`jsd_between_sets` runs on CPU tensors too, through the library's
host entry point).  Ties are resolved to the LOWEST index, explicitly: torch.argmin
does not promise which of several equal minima it returns.
"""
import warnings

import torch


def _lowest_argmin(mat, dim):
    """Index of the minimum along `dim`; among equal minima the lowest index."""
    size = mat.size(dim)
    lowest = mat.min(dim=dim, keepdim=True).values
    shape = [1] * mat.dim()
    shape[dim] = size
    index = torch.arange(size, device=mat.device).reshape(shape)
    return torch.where(mat == lowest, index, torch.full_like(index, size)).min(dim=dim).values


def _ratio(count, total):
    """count / total as a float64 scalar on count's device.  The divisor is a tensor there: torch divides a CUDA tensor
    by a host number through a multiplication by its reciprocal, which is not the correctly rounded quotient."""
    return count.double() / torch.full((), float(total), dtype=torch.float64, device=count.device)


def _matrix(t, name, rows=None, cols=None):
    if t.dim() != 2 or t.size(0) == 0 or t.size(1) == 0:
        raise ValueError(f"{name}: expected a non-empty distance matrix, got shape {tuple(t.shape)}")
    if (rows is not None and t.size(0) != rows) or (cols is not None and t.size(1) != cols):
        raise ValueError(f"{name}: expected shape ({rows}, {cols}), got {tuple(t.shape)}")
    if bool(torch.isnan(t).any()):      # a NaN is equal to no minimum: no arg-min to take
        raise ValueError(f"{name}: the matrix holds NaN")
    return t.double()


def minimum_matching_distance(cd_gr):
    """cd_gr [G, R] (generated x reference) -> float64 scalar: the mean over the reference clouds of the distance to
    their nearest generated cloud."""
    return _matrix(cd_gr, "cd_gr").min(dim=0).values.mean()


def coverage(cd_gr):
    """cd_gr [G, R] -> float64 scalar: the share of reference clouds that are the nearest reference cloud (lowest index
    among equals) of at least one generated cloud."""
    cd_gr = _matrix(cd_gr, "cd_gr")
    hit = torch.zeros(cd_gr.size(1), dtype=torch.bool, device=cd_gr.device)
    hit[_lowest_argmin(cd_gr, 1)] = True
    return _ratio(hit.sum(), cd_gr.size(1))


def one_nn_accuracy(cd_gg, cd_gr, cd_rr):
    """cd_gg [G, G], cd_gr [G, R], cd_rr [R, R] -> float64 scalar: leave-one-out accuracy of the 1-nearest-neighbour
    classifier "generated or reference?" over the G + R clouds (generated first).  A cloud's own distance is left
    out; among equally near neighbours the one with the lowest index in the concatenation decides.  0.5 is the value
    of two indistinguishable sets."""
    cd_gr = _matrix(cd_gr, "cd_gr")
    g, r = cd_gr.shape
    cd_gg, cd_rr = _matrix(cd_gg, "cd_gg", g, g), _matrix(cd_rr, "cd_rr", r, r)
    full = torch.cat([torch.cat([cd_gg, cd_gr], dim=1), torch.cat([cd_gr.t(), cd_rr], dim=1)], dim=0)
    full.fill_diagonal_(float("inf"))
    nearest = _lowest_argmin(full, 1)
    is_ref = torch.arange(g + r, device=full.device) >= g
    return _ratio((is_ref[nearest] == is_ref).sum(), g + r)


def in_sphere_cells(resolution):
    """The number of cells of the resolution^3 grid whose centre lies in the unit sphere (include/ops/occupancy.h: in
    integers, the boundary included): 10144 at 28."""
    res = int(resolution)
    if res != resolution or res < 2:
        raise ValueError(f"in_sphere_cells: resolution must be an integer >= 2, got {resolution!r}")
    a = 2 * torch.arange(res, dtype=torch.int64) - (res - 1)
    a2 = a * a
    return int((a2[:, None, None] + a2[None, :, None] + a2[None, None, :] <= (res - 1) ** 2).sum())


def _entropy_bits(x):
    """-sum x log2 x over x > 0, float64."""
    x = x[x > 0]
    return -(x * torch.log2(x)).sum()


def jensen_shannon_divergence(p_counts, q_counts):
    """Two grids of counts (any shape, the same for both; integers or floats) -> float64 scalar in [0, 1], in bits:
    H((P + Q) / 2) - (H(P) + H(Q)) / 2 with P = p / sum(p), Q = q / sum(q) and H(x) = -sum x log2 x over x > 0.
    Symmetric in its arguments bit for bit, and exactly 0.0 for equal counts."""
    if tuple(p_counts.shape) != tuple(q_counts.shape):
        raise ValueError(f"jensen_shannon_divergence: shapes differ: {tuple(p_counts.shape)} and {tuple(q_counts.shape)}")
    p, q = p_counts.double().reshape(-1), q_counts.double().reshape(-1)
    sp, sq = p.sum(), q.sum()
    if not (float(sp) > 0 and float(sq) > 0):
        raise ValueError("jensen_shannon_divergence: a grid without a point (the counts must have a positive total)")
    p, q = p / sp, q / sq      # divisions by a tensor: see _ratio.  The halvings below are exact
    # equal counts: (P + P) / 2 is P, the three entropies are one sum evaluated three times, and H - (H + H) / 2 is 0.0
    value = _entropy_bits((p + q) * 0.5) - (_entropy_bits(p) + _entropy_bits(q)) * 0.5
    return value.clamp(0.0, 1.0)      # rounding may leave the interval by an ulp at its ends


def occupancy_entropy(occupied, n_clouds, n_cells):
    """The published `acc_entropy` of a set: occupied (any shape, integers) holds per cell the number g of the set's
    n_clouds clouds with a point there; the result is the sum over the cells of the entropy of Bernoulli(g / n_clouds)
    -- natural logarithm, as published; cells with g = 0 or g = n_clouds contribute 0 -- over n_cells, the number of
    cells of the grid (in_sphere_cells(resolution) for the clipped one).  float64 scalar."""
    if int(n_clouds) < 1 or int(n_cells) < 1:
        raise ValueError("occupancy_entropy: n_clouds and n_cells must be >= 1")
    g = occupied.double().reshape(-1)
    if bool((g < 0).any()) or bool((g > n_clouds).any()):
        raise ValueError(f"occupancy_entropy: occupied must lie in [0, {int(n_clouds)}]")
    g = g[(g > 0) & (g < n_clouds)]
    total = torch.full((), float(n_clouds), dtype=torch.float64, device=g.device)
    p = g / total
    r = (total - g) / total
    cells = torch.full((), float(n_cells), dtype=torch.float64, device=g.device)
    return -(p * torch.log(p) + r * torch.log(r)).sum() / cells


def _out_of_range(clouds, lengths, in_sphere):
    """What the published code warns about: a coordinate beyond 0.5 + 1e-3 in magnitude, or -- on the clipped grid -- a
    point beyond that norm (which covers the coordinates), taken in the clouds' fp32 as published.  Padding rows and
    non-finite points, which no cell counts, are not looked at.  One pass and one number read back."""
    x = clouds.detach().float()
    keep = torch.isfinite(x).all(dim=2)
    if lengths is not None:
        from sparenet_amd.cuda.ragged import valid_mask

        keep = keep & valid_mask(lengths, x.size(1), x.device)
    size = (x * x).sum(dim=2).sqrt() if in_sphere else x.abs().amax(dim=2)
    return torch.where(keep, size, torch.zeros((), device=x.device)).max().item() > 0.5 + 1e-3


def jsd_between_sets(gen, ref, resolution=28, in_sphere=True, gen_lengths=None, ref_lengths=None, ref_counts=None):
    """gen [G, n, 3], ref [R, m, 3] -> float64 scalar on the clouds' device: the Jensen-Shannon divergence (bits, in
    [0, 1]) between the two sets' distributions of points over the resolution^3 grid on [-0.5, 0.5]^3, clipped to the
    unit sphere with in_sphere -- jensen_shannon_divergence of two occupancy_grid calls.  Device tensors run the
    kernel, CPU tensors the library's host entry point.  `gen_lengths` / `ref_lengths` make a set ragged.  `ref_counts`
    takes the reference set's grid (occupancy_grid(ref, resolution, in_sphere)[0]) where it has been computed before:
    it is the same for every checkpoint, and `ref` is then not read.  Warns -- once per call, whichever set it is --
    when a set leaves the unit cube (with in_sphere: the unit sphere) by more than 1e-3, as the published code does;
    such points are still assigned, to the rim."""
    from sparenet_amd.cuda.occupancy import occupancy_grid

    outside = _out_of_range(gen, gen_lengths, in_sphere)
    gen_counts = occupancy_grid(gen, resolution, in_sphere, gen_lengths)[0]
    if ref_counts is None:
        outside = outside or _out_of_range(ref, ref_lengths, in_sphere)
        ref_counts = occupancy_grid(ref, resolution, in_sphere, ref_lengths)[0]
    if outside:
        warnings.warn(f"jsd_between_sets: points outside the unit {'sphere' if in_sphere else 'cube'} (centred at the "
                      "origin, diameter 1): they are assigned to the nearest cell of its rim", stacklevel=2)
    return jensen_shannon_divergence(gen_counts, ref_counts)


def set_metrics(gen, ref, cd_rr=None, with_emd=False, emd_eps=0.005, emd_iters=50, emd_rr=None, with_jsd=False,
                jsd_resolution=28, ref_counts=None):
    """gen [G, n, 3], ref [R, m, 3] (contiguous fp32 CUDA tensors) -> {"MMD-CD", "COV-CD", "1-NNA-CD"}, float64 scalars
    on the clouds' device, from three chamfer_matrix calls.  `cd_rr` takes the reference set's own matrix
    (chamfer_matrix(ref, ref)) where it has been computed before: it is the same for every checkpoint.
    with_emd: also {"MMD-EMD", "COV-EMD", "1-NNA-EMD"}, the same three metrics on the auction EMD between the clouds
    (sparenet_amd.cuda.set_distance.emd_matrix with emd_eps and emd_iters; `emd_rr` takes emd_matrix(ref, ref, ...)).
    An EMD matrix of a set against itself is not symmetric (an auction is directed); the 1-NN classifier reads a
    reference cloud's distances to the generated clouds off the transposed generated x reference matrix, as for CD.
    with_jsd: also {"JSD"}, jsd_between_sets(gen, ref, jsd_resolution) on the grid clipped to the sphere; `ref_counts`
    takes the reference set's grid (occupancy_grid(ref, jsd_resolution)[0]).  The other keys keep their bits."""
    from sparenet_amd.cuda.set_distance import chamfer_matrix, emd_matrix

    cd_gr = chamfer_matrix(gen, ref)
    cd_gg = chamfer_matrix(gen, gen)
    if cd_rr is None:
        cd_rr = chamfer_matrix(ref, ref)
    out = {"MMD-CD": minimum_matching_distance(cd_gr), "COV-CD": coverage(cd_gr),
           "1-NNA-CD": one_nn_accuracy(cd_gg, cd_gr, cd_rr)}
    if with_emd:
        emd_gr = emd_matrix(gen, ref, emd_eps, emd_iters)
        emd_gg = emd_matrix(gen, gen, emd_eps, emd_iters)
        if emd_rr is None:
            emd_rr = emd_matrix(ref, ref, emd_eps, emd_iters)
        out.update({"MMD-EMD": minimum_matching_distance(emd_gr), "COV-EMD": coverage(emd_gr),
                    "1-NNA-EMD": one_nn_accuracy(emd_gg, emd_gr, emd_rr)})
    if with_jsd:
        out["JSD"] = jsd_between_sets(gen, ref, jsd_resolution, True, ref_counts=ref_counts)
    return out
