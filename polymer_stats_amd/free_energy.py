"""Free energy along the extension from force-ensemble histograms (pure numpy, no device).

A run at fixed force F along a component x of the end-to-end vector samples P_F(x) ~ Z(x) exp(F x / kT), Z the fixed-extension
partition function.  So the fixed-extension (Helmholtz) free energy is A(x) = -kT ln P_F(x) + F x + const: one run gives it on
the window it visits (extension_free_energy), a force sweep -- the cases of one handle -- gives it from slack to taut once the
windows are stitched by WHAM (wham_force).  The histograms are those of Ensemble.open_hist / Hist.read or of a .hist file of
tools/run_sweep.py --hist; tails are left out, which is exact for A on the binned range up to the additive constant."""
from __future__ import annotations

import numpy as np


def _centers_and_width(edges, nbins: int):
    e = np.asarray(edges, dtype=np.float64)
    if e.shape != (nbins + 1,) or not np.all(np.diff(e) > 0):
        raise ValueError(f"edges must be {nbins + 1} increasing values")
    return 0.5 * (e[:-1] + e[1:]), np.diff(e)


def _logsumexp(a, axis):
    m = np.max(a, axis=axis, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return np.squeeze(m, axis=axis) + np.log(np.sum(np.exp(a - m), axis=axis))


def extension_free_energy(counts, edges, kT: float, F: float):
    """(A, sigma) at the bin centres from one case's histogram of the component the force F acts on:
    A = -kT ln(density) + F x, shifted so that min A = 0; sigma = kT / sqrt(count), the propagated counting error of
    independent samples.  Empty bins give NaN in both."""
    n = np.asarray(counts, dtype=np.float64)
    x, w = _centers_and_width(edges, n.shape[0])
    total = n.sum()
    if n.ndim != 1 or total <= 0:
        raise ValueError("counts must be one histogram with at least one sample")
    with np.errstate(divide="ignore", invalid="ignore"):
        A = np.where(n > 0, -kT * np.log(n / (total * w)) + F * x, np.nan)
        sigma = np.where(n > 0, kT / np.sqrt(n), np.nan)
    return A - np.nanmin(A), sigma


def wham_force(counts, edges, kT: float, forces, tol: float = 1e-10, max_iter: int = 100000):
    """WHAM over K cases that differ only in the force along the binned component (and in seed): counts[K, nbins], forces[K].
    Iterates, in log space and from f = 0, the standard equations (beta = 1 / kT, x_j the bin centres, N_k = sum_j n_kj)
        P0_j = sum_k n_kj / sum_k N_k exp(f_k + beta F_k x_j),      exp(-f_k) = sum_j P0_j exp(beta F_k x_j)
    until no f_k - f_0 changes by more than `tol`.  Returns (A, sigma, f, iterations, converged): A = -kT ln(P0 / width)
    shifted so that min A = 0 -- the zero-force free energy along x, i.e. the fixed-extension one up to its constant --
    sigma_j = kT / sqrt(sum_k n_kj), NaN in both where no case has a sample; f in the gauge f_0 = 0."""
    n = np.asarray(counts, dtype=np.float64)
    F = np.asarray(forces, dtype=np.float64)
    if n.ndim != 2 or F.shape != (n.shape[0],):
        raise ValueError("counts must be [K, nbins] and forces [K]")
    x, w = _centers_and_width(edges, n.shape[1])
    N = n.sum(axis=1)
    if np.any(N <= 0):
        raise ValueError("every case needs at least one sample inside the binned range")
    beta = 1.0 / kT
    tilt = beta * F[:, None] * x[None, :]                    # [K, nbins]
    col = n.sum(axis=0)
    with np.errstate(divide="ignore"):
        logcol, logN = np.log(col), np.log(N)
    f = np.zeros(len(F))
    converged, it = False, 0
    logP0 = np.full(n.shape[1], -np.inf)
    for it in range(1, int(max_iter) + 1):
        logP0 = logcol - _logsumexp(logN[:, None] + f[:, None] + tilt, axis=0)
        new = -_logsumexp(logP0[None, :] + tilt, axis=1)
        new -= new[0]
        change = np.max(np.abs(new - f))
        f = new
        if change < tol:
            converged = True
            break
    logP0 = logcol - _logsumexp(logN[:, None] + f[:, None] + tilt, axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        A = np.where(col > 0, -kT * (logP0 - np.log(w)), np.nan)
        sigma = np.where(col > 0, kT / np.sqrt(col), np.nan)
    return A - np.nanmin(A), sigma, f, it, converged
