"""The numpy twin of the correlation contract (include/pstat.h, DESIGN.md 3.15, polymer_stats_amd/csrc/pstat_corr.hip): written
from the contract, sharing no code with the library.

Angles come as pstat_chain_state returns them: angles[C, 2n], theta[n] then phi[n], radians (a planar handle's theta is unused).
  3D      n_i = (cos phi sin theta, sin phi sin theta, cos theta), field axis = component 3
          dielectric mu_i = (K1 - K2) E0 cos theta_i n_i + K2 E0 z;  polar mu_i = mu n_i
  planar  n_i = (cos phi, sin phi), field axis = component 2
          dielectric mu_i = (K1 - K2) E0 sin phi_i n_i + (0, K2 E0);  polar mu_i = mu n_i
  per chain and lag k: (1 / (n - k)) sum_{i=0}^{n-1-k} of  nn: n_i . n_{i+k}   zz: n_{i,z} n_{i+k,z}   mm: mu_i . mu_{i+k}
  per case and column (channels in the order nn, zz, mm, each max_lag + 1 wide): sum over chains, and sum of squares."""
import numpy as np

CHANNELS = ("nn", "zz", "mm")


def unit_vectors(angles, planar=False):
    """[C, n, 3] (planar: [C, n, 2]); the field axis is the last component."""
    a = np.asarray(angles, dtype=np.float64)
    n = a.shape[1] // 2
    theta, phi = a[:, :n], a[:, n:]
    if planar:
        return np.stack([np.cos(phi), np.sin(phi)], axis=-1)
    return np.stack([np.cos(phi) * np.sin(theta), np.sin(phi) * np.sin(theta), np.cos(theta)], axis=-1)


def dipoles(nhat, E0=0.0, K1=0.0, K2=0.0, mu=0.0, polar=False):
    """[C, n, dim] from the unit vectors; along the field axis a dielectric monomer's cosine is the last component."""
    if polar:
        return mu * nhat
    m = ((K1 - K2) * E0) * nhat[..., -1:] * nhat
    m[..., -1] += K2 * E0
    return m


def per_chain(angles, max_lag, channels=CHANNELS, planar=False, polar=False, E0=0.0, K1=0.0, K2=0.0, mu=0.0):
    """[C, ncols]: every chain's values, the channels of `channels` (kept in the order nn, zz, mm) side by side."""
    nhat = unit_vectors(angles, planar)
    n = nhat.shape[1]
    m = dipoles(nhat, E0, K1, K2, mu, polar)
    cols = []
    for ch in CHANNELS:
        if ch not in channels:
            continue
        for k in range(max_lag + 1):
            if ch == "nn":
                terms = np.sum(nhat[:, :n - k] * nhat[:, k:], axis=-1)
            elif ch == "zz":
                terms = nhat[:, :n - k, -1] * nhat[:, k:, -1]
            else:
                terms = np.sum(m[:, :n - k] * m[:, k:], axis=-1)
            cols.append(terms.sum(axis=1) / (n - k))
    return np.stack(cols, axis=1)


def totals(values):
    """(sum, sumsq) over the chains of per_chain's [C, ncols]."""
    return values.sum(axis=0), (values * values).sum(axis=0)


def scale(channel, E0=0.0, K1=0.0, K2=0.0, mu=0.0, polar=False):
    """A bound on |term| of the channel: 1 for nn and zz, |mu_i|^2 at most for mm."""
    if channel != "mm":
        return 1.0
    return mu * mu if polar else (abs(K1 - K2) * abs(E0) + abs(K2 * E0)) ** 2
