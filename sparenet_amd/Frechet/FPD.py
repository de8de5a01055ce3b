"""Frechet Point-cloud Distance between two sets of point clouds (the reference's Frechet/FPD.py, same function
names, signatures, defaults and statistics file format).

  d^2 = |m1 - m2|^2 + tr S1 + tr S2 - 2 tr sqrt(S1 S2)

on the 1808-wide activations of PointNetCls(k=16).  Differences from the reference, none of them in the value:
  * on a CUDA device the per-point MLPs run as the fused HIP kernel (see pointnet.py);
  * no scipy: with both activation sets at hand, tr sqrt(S1 S2) is the sum of the singular values of X1 X2^T,
    X = (A - mean) / sqrt(n - 1) (`frechet_distance_from_activations`); from saved statistics it is the sum of the
    square roots of the eigenvalues of S1^(1/2) S2 S1^(1/2), negative ones clamped to zero
    (`calculate_frechet_distance`).  Both in float64, neither needs the reference's "singular product" retry;
  * `calculate_fpd` takes `model=` or `weights=`: a library cannot assume ./Frechet/cls_model_39.pth.
As in the reference, the clouds after the last full batch are dropped (n_batches = N // batch_size).
"""
import os

import numpy as np
import torch

from .pointnet import PointNetCls

DEFAULT_WEIGHTS = './Frechet/cls_model_39.pth'
DEFAULT_STATISTICS = './Frechet/pre_statistics_all.npz'


def get_activations(pointclouds, model, batch_size=100, dims=1808, device=None, verbose=False):
    """pointclouds [N, n, 3] (torch) -> float64 numpy [N // batch_size * batch_size, dims]."""
    model.eval()
    n_batches = pointclouds.size(0) // batch_size
    n_used = n_batches * batch_size
    pred_arr = np.empty((n_used, dims))
    pointclouds = pointclouds.transpose(1, 2)
    for i in range(n_batches):
        if verbose:
            print('\rPropagating batch %d/%d' % (i + 1, n_batches), end='', flush=True)
        start, end = i * batch_size, (i + 1) * batch_size
        batch = pointclouds[start:end]
        if device is not None:
            batch = batch.to(device)
        _, _, actv = model(batch)
        pred_arr[start:end] = actv.cpu().numpy().reshape(batch_size, -1)
    if verbose:
        print(' done')
    return pred_arr


def _psd_sqrt(s):
    w, v = np.linalg.eigh(s)
    return (v * np.sqrt(np.clip(w, 0.0, None))) @ v.T


def calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """Frechet distance of N(mu1, sigma1) and N(mu2, sigma2) from the statistics alone, in float64.
    tr sqrt(S1 S2) = sum sqrt(eig(S1^(1/2) S2 S1^(1/2))): a symmetric positive semi-definite matrix, so rank-deficient
    covariances (fewer clouds than dimensions) need no regularisation; `eps` is accepted for the reference's
    signature and not used."""
    mu1, mu2 = np.atleast_1d(np.asarray(mu1, np.float64)), np.atleast_1d(np.asarray(mu2, np.float64))
    sigma1, sigma2 = np.atleast_2d(np.asarray(sigma1, np.float64)), np.atleast_2d(np.asarray(sigma2, np.float64))
    assert mu1.shape == mu2.shape, 'Training and test mean vectors have different lengths'
    assert sigma1.shape == sigma2.shape, 'Training and test covariances have different dimensions'
    diff = mu1 - mu2
    r = _psd_sqrt(sigma1)
    m = r @ sigma2 @ r
    ev = np.linalg.eigvalsh((m + m.T) * 0.5)
    tr_covmean = np.sqrt(np.clip(ev, 0.0, None)).sum()
    return diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * tr_covmean


def frechet_distance_from_activations(act1, act2):
    """The same distance from the activations [n1, d], [n2, d] themselves: with X = (A - mean) / sqrt(n - 1),
    S = X^T X and tr sqrt(S1 S2) is the nuclear norm of the n1 x n2 matrix X1 X2^T.  float64."""
    act1, act2 = np.asarray(act1, np.float64), np.asarray(act2, np.float64)
    if act1.shape[0] < 2 or act2.shape[0] < 2:
        raise ValueError("a covariance needs at least two activations per set "
                         f"(got {act1.shape[0]} and {act2.shape[0]}: is batch_size larger than the set?)")
    m1, m2 = act1.mean(axis=0), act2.mean(axis=0)
    x1 = (act1 - m1) / np.sqrt(act1.shape[0] - 1)
    x2 = (act2 - m2) / np.sqrt(act2.shape[0] - 1)
    diff = m1 - m2
    tr_covmean = np.linalg.svd(x1 @ x2.T, compute_uv=False).sum()
    return diff.dot(diff) + (x1 * x1).sum() + (x2 * x2).sum() - 2 * tr_covmean


def calculate_activation_statistics(pointclouds, model, batch_size=100, dims=1808, device=None, verbose=False):
    """(mean [dims], covariance [dims, dims]) of the activations, float64 (np.cov, rowvar=False)."""
    act = get_activations(pointclouds, model, batch_size, dims, device, verbose)
    return np.mean(act, axis=0), np.cov(act, rowvar=False)


def save_statistics(real_pointclouds, path, model, batch_size, dims, cuda):
    m, s = calculate_activation_statistics(real_pointclouds, model, batch_size, dims, cuda)
    np.savez(path, m=m, s=s)
    print('save done !!!')


def load_model(model=None, weights=None, device=None):
    """The PointNetCls(k=16) to use: `model` as given, else one loaded from `weights`, else from DEFAULT_WEIGHTS."""
    if model is None:
        path = DEFAULT_WEIGHTS if weights is None else weights
        if not os.path.isfile(path):
            raise FileNotFoundError(
                f"PointNet classifier weights not found at {path!r}: pass weights=<path to cls_model_39.pth> or "
                "model=<a loaded PointNetCls(k=16)> to calculate_fpd")
        model = PointNetCls(k=16)
        model.load_state_dict(torch.load(path, map_location='cpu'))
    if device is not None:
        model.to(device)
    return model


def calculate_fpd(pointclouds1, pointclouds2=None, statistic_save_path=None, batch_size=100, dims=1808, device=None,
                  model=None, weights=None):
    """FPD of pointclouds1 [N, n, 3] against pointclouds2, or against saved statistics (.npz with `m`, `s`) when
    pointclouds2 is None."""
    if statistic_save_path is None:
        statistic_save_path = DEFAULT_STATISTICS
    model = load_model(model, weights, device)
    act1 = get_activations(pointclouds1, model, batch_size, dims, device)
    if pointclouds2 is not None:
        act2 = get_activations(pointclouds2, model, batch_size, dims, device)
        return frechet_distance_from_activations(act1, act2)
    with np.load(statistic_save_path) as f:
        m2, s2 = f['m'][:], f['s'][:]
    return calculate_frechet_distance(np.mean(act1, axis=0), np.cov(act1, rowvar=False), m2, s2)
