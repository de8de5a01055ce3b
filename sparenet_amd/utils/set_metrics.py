"""The three set-level metrics published beside FPD for point-cloud generators and completion GANs, with the Chamfer
distance between clouds: minimum matching distance (MMD-CD), coverage (COV-CD) and 1-nearest-neighbour accuracy
(1-NNA-CD).  All three are read off the matrices of Chamfer distances between every generated and every reference
cloud (sparenet_amd.cuda.set_distance.chamfer_matrix); `set_metrics(..., with_emd=True)` adds the same three on the
matrices of auction EMDs (emd_matrix): MMD-EMD, COV-EMD and 1-NNA-EMD.

The metric functions are plain torch on float64 matrices and work on any device, CPU included; only `set_metrics`
itself, which computes the matrices, needs the GPU.  Ties are resolved to the LOWEST index, explicitly: torch.argmin
does not promise which of several equal minima it returns.
"""
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


def set_metrics(gen, ref, cd_rr=None, with_emd=False, emd_eps=0.005, emd_iters=50, emd_rr=None):
    """gen [G, n, 3], ref [R, m, 3] (contiguous fp32 CUDA tensors) -> {"MMD-CD", "COV-CD", "1-NNA-CD"}, float64 scalars
    on the clouds' device, from three chamfer_matrix calls.  `cd_rr` takes the reference set's own matrix
    (chamfer_matrix(ref, ref)) where it has been computed before: it is the same for every checkpoint.
    with_emd: also {"MMD-EMD", "COV-EMD", "1-NNA-EMD"}, the same three metrics on the auction EMD between the clouds
    (sparenet_amd.cuda.set_distance.emd_matrix with emd_eps and emd_iters; `emd_rr` takes emd_matrix(ref, ref, ...)).
    An EMD matrix of a set against itself is not symmetric (an auction is directed); the 1-NN classifier reads a
    reference cloud's distances to the generated clouds off the transposed generated x reference matrix, as for CD."""
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
    return out
