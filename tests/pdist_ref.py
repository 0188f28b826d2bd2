"""The numpy twin of the pair-distance contract (include/pstat.h, DESIGN.md 3.18, polymer_stats_amd/csrc/pstat_pdist.hip): written
from the contract, sharing no code with the library.

Angles come as pstat_chain_state returns them: angles[C, 2n], theta[n] then phi[n], radians (a planar handle's theta is unused).
  positions   the shape recorder's: x_i = b (sum_{j <= i} n_j - n_i / 2); planar n_i = (cos phi, 0, sin phi)
  pair        i < j: d = x_j - x_i;  r2 = (d_x d_x + d_y d_y) + d_z d_z (planar: d_x d_x + d_z d_z);  r = sqrt(r2)
  columns     msd    s = 1 .. max_sep:  R2(s) = (1 / (n - s)) sum_i r2_{i,i+s}
              rmin   min r_ij over j - i >= min_sep
              hist   nbins + 1 counts (none when nbins = 0) of the pairs with j - i >= min_sep:  t = r * inv, inv = nbins / rmax;
                     bin (int)t if t < nbins, else the last column, "above"
              sq     nq columns:  S(q) = 1 + (2 sum_{i<j} sinc(q r_ij)) / n over ALL pairs; sinc(0) = 1, else sin(x) / x, x = q r
  per case and column: sum over chains, and sum of squares.

THE BOUND on |device - twin| (value_bounds, bounds below), derived, not fitted.  u = 2^-53, L = n |b|, P = n (n - 1) / 2.
  position    shape_ref's: a component of x_i is off by at most eps_x = L u (n + 8).
  d           a component of d = x_j - x_i, |d_a| <= L: the two positions' errors and the subtraction's rounding,
              eps_d = 2 eps_x + u L = L u (2 n + 17).
  r2          a product d_a d_a is off by 2 L eps_d + u L^2 (and eps_d^2, below one u L^2 for n <= 4000); three products and two
              additions of partial sums <= L^2:  eps_r2 = 3 (2 L eps_d + u L^2) + 3 u L^2 = L^2 u (12 n + 108).
  r           the square root is not Lipschitz at 0, so the bound depends on r.  For a computed r^ with r^2 > 4 eps_r2 the exact
              r and any other computed r' have r >= 0.86 r^, r' >= 0.7 r^, so |r' - r| = |r'^2 - r^2| / (r' + r) <= eps_r2 /
              (1.56 r^) and the roots' roundings add u L each:  eps_r(r^) = eps_r2 / r^ + 2 u L.  Otherwise all three are below
              sqrt(6 eps_r2):  eps_r(r^) = 2.5 sqrt(eps_r2) + 2 u L.  eps_r falls with r^: over a set of pairs it is largest at
              the smallest distance, `rfloor`, which the twin reports for the data it was given.
  rmin        |min_i a_i - min_i b_i| <= max_i |a_i - b_i|:  E_rmin = eps_r(rfloor).  V = L.
  R2(s)       the mean of m = n - s values <= L^2, each off by eps_r2, added in any order: m eps_r2 + m (m - 1) u L^2, divided by
              m with one rounding:  E_msd = eps_r2 + n u L^2 = L^2 u (13 n + 108).  V = L^2.
  x = q r     q eps_r + u q L.
  sinc        |sinc'| <= 0.44 everywhere; the sine is < 1 ulp (2 u |sin|) on both sides and the division rounds once (u):
              E_sinc = 0.44 q (eps_r(rfloor) + u L) + 3 u.
  S(q)        P terms of size <= 1 in any order: P E_sinc + P (P - 1) u; times 2 exactly; divided by n (a quotient <= n - 1 rounded
              once) and 1 added (a sum <= n rounded once):  E_S = (n - 1) (E_sinc + P u) + 2 n u.  V = n.
  histogram   counts are integers.  A pair's t = r * inv is off by inv eps_r + u t on either side, so device and twin may put
              it into different columns only if t lies within  w = 2 (inv eps_r(r^) + u t)  of an integer k in 1 .. nbins; such a
              pair is UNDECIDED between columns k - 1 and k (k = nbins: the last bin and "above").  The twin returns the
              decided counts and, per column, how many undecided pairs may fall into it: the device's count lies in
              [decided, decided + undecided], and a chain's columns add up to (n - min_sep)(n - min_sep + 1) / 2 exactly.
              THE CONDITION on the inputs of the GPU tests: every random-angle input has ZERO undecided pairs (w ~ 1e-13 and a few
              thousand pairs); the tests assert it, and the comparison is then an equality of integers, on `sum` and on `sumsq`
              (M n^4 / 4 < 2^53).
  totals      as in shape_ref: device and twin may each be off by E per value; a total of M values bounded by V added in any
              order: 2 M E + M^2 u V on `sum`; on `sumsq` the same with E -> 2 V E + u V^2 and V -> V^2.  A row is one record's
              sum divided by num_chains: its bound is that of M = num_chains, divided by num_chains."""
import numpy as np

U = 2.0 ** -53
CHUNK = 4096


def unit_vectors(angles, planar=False):
    a = np.asarray(angles, dtype=np.float64)
    n = a.shape[1] // 2
    theta, phi = a[:, :n], a[:, n:]
    if planar:
        return np.stack([np.cos(phi), np.zeros_like(phi), np.sin(phi)], axis=-1)
    return np.stack([np.cos(phi) * np.sin(theta), np.sin(phi) * np.sin(theta), np.cos(theta)], axis=-1)


def positions(angles, b=1.0, planar=False):
    nhat = unit_vectors(angles, planar)
    return b * (np.cumsum(nhat, axis=1) - nhat / 2)


def pair_index(n):
    """(I, J): the n (n - 1) / 2 pairs i < j."""
    return np.triu_indices(n, 1)


def pair_distances(x, planar=False):
    """(r2, r), each [C, P], in the order of pair_index."""
    I, J = pair_index(x.shape[1])
    d = x[:, J, :] - x[:, I, :]
    if planar:
        r2 = d[:, :, 0] * d[:, :, 0] + d[:, :, 2] * d[:, :, 2]
    else:
        r2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
    return r2, np.sqrt(r2)


def ncols(max_sep, nbins, nq):
    return max_sep + 1 + (nbins + 1 if nbins else 0) + nq


def columns(max_sep, nbins, nq):
    """The column ranges (msd, rmin, hist, sq) as slices."""
    h0 = max_sep + 1
    h1 = h0 + (nbins + 1 if nbins else 0)
    return slice(0, max_sep), slice(max_sep, h0), slice(h0, h1), slice(h1, h1 + nq)


def eps_r2(n, b):
    L = n * abs(b)
    return L * L * U * (12 * n + 108)


def eps_r(r, n, b):
    """The docstring's eps_r(r^), elementwise."""
    r = np.asarray(r, dtype=np.float64)
    e2, L = eps_r2(n, b), n * abs(b)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(r * r > 4 * e2, e2 / r, 2.5 * np.sqrt(e2)) + 2 * U * L


def sinc(x):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(x == 0.0, 1.0, np.sin(x) / x)


def per_chain(angles, b=1.0, max_sep=-1, min_sep=1, nbins=0, rmax=1.0, q=None, planar=False):
    """(values [C, ncols], undecided [C, nbins + 1 or 0], rfloor): every chain's columns with the histogram's DECIDED counts, how
    many undecided pairs may fall into each histogram column, and the smallest distance between any two monomers of a chain."""
    a = np.asarray(angles, dtype=np.float64)
    n = a.shape[1] // 2
    if max_sep < 0:
        max_sep = n - 1
    qv = np.zeros(0) if q is None else np.asarray(q, dtype=np.float64).reshape(-1)
    I, J = pair_index(n)
    sep = J - I
    far = sep >= min_sep
    nh = nbins + 1 if nbins else 0
    values, undecided, rfloor = [], [], np.inf
    for c0 in range(0, len(a), CHUNK):
        r2, r = pair_distances(positions(a[c0:c0 + CHUNK], b, planar), planar)
        C = len(r)
        rfloor = min(rfloor, float(r.min()))
        cols = [r2[:, sep == s].sum(axis=1) / (n - s) for s in range(1, max_sep + 1)]
        cols.append(r[:, far].min(axis=1))
        und = np.zeros((C, nh))
        if nbins:
            inv = nbins / rmax
            rr = r[:, far]
            t = rr * inv
            w = 2.0 * (inv * eps_r(rr, n, b) + U * t)
            k = np.rint(t)
            open_ = (np.abs(t - k) <= w) & (k >= 1) & (k <= nbins)
            bins = np.where(t < nbins, np.minimum(t, nbins).astype(np.int64), nbins)
            dec = np.zeros((C, nh))
            rows = np.broadcast_to(np.arange(C)[:, None], bins.shape)
            np.add.at(dec, (rows[~open_], bins[~open_]), 1.0)
            kk = k[open_].astype(np.int64)
            np.add.at(und, (rows[open_], kk - 1), 1.0)
            np.add.at(und, (rows[open_], kk), 1.0)
            cols += list(dec.T)
        for qk in qv:
            cols.append(1.0 + (2.0 * sinc(qk * r).sum(axis=1)) / n)
        values.append(np.stack(cols, axis=1))
        undecided.append(und)
    return np.concatenate(values), np.concatenate(undecided), rfloor


def pairs_counted(n, min_sep):
    return (n - min_sep) * (n - min_sep + 1) // 2


def density(counts, pairs, rmax):
    """P(r) from the counts [nbins] of `pairs` pairs: counts / (pairs * bin width); integrates to the share below rmax."""
    counts = np.asarray(counts, dtype=np.float64)
    return counts / (pairs * (rmax / len(counts)))


def value_bounds(n, b, max_sep, nbins, q, rfloor):
    """(E, V), each [ncols]: the per-value error bound of the docstring (0 for the histogram's integers) and the bound on the
    value's size; `rfloor`: the smallest distance in the data (per_chain reports it)."""
    qv = np.zeros(0) if q is None else np.asarray(q, dtype=np.float64).reshape(-1)
    L = n * abs(b)
    P = n * (n - 1) / 2
    er = float(eps_r(rfloor, n, b))
    E = [L * L * U * (13 * n + 108)] * max_sep + [er] + [0.0] * (nbins + 1 if nbins else 0)
    V = [L * L] * max_sep + [L] + [P] * (nbins + 1 if nbins else 0)
    for qk in qv:
        es = 0.44 * qk * (er + U * L) + 3 * U
        E.append((n - 1) * (es + P * U) + 2 * n * U)
        V.append(float(n))
    return np.array(E), np.array(V)


def bounds(n, b, M, max_sep, nbins, q, rfloor):
    """(bound on sum, bound on sumsq), each [ncols], for a total of M values per column; 0 on the histogram's columns, whose
    totals are integers below 2^53 and compared through their intervals."""
    E, V = value_bounds(n, b, max_sep, nbins, q, rfloor)
    E2, V2 = 2 * V * E + U * V * V, V * V
    b1, b2 = 2 * M * E + M * M * U * V, 2 * M * E2 + M * M * U * V2
    _, _, hist, _ = columns(max_sep, nbins, len(E) - max_sep - 1 - (nbins + 1 if nbins else 0))
    b1[hist] = 0.0
    b2[hist] = 0.0
    return b1, b2


def judge_closed_form(name, case, mean, se):
    """The statistical conditions of tests/test_pdist_cpu.py and tests/test_gpu_pdist.py on one record of many chains (`mean`,
    `se`: [ncols], the pooled means and their across-chain standard errors; `case`: a case of
    tests/golden/pdist_closed_form.json with its options and expected columns).  Every column the fixture has lies within 5 of its
    own across-chain standard errors of the closed form; for the msd, rmin and sq columns that error is also at most 2 % of the
    value; histogram columns (mean counts per chain) are judged on |z| <= 5 alone.  A column without variance (S at q = 0; an
    empty bin) is held to exact equality.  Returns (largest |z|, largest relative error among msd, rmin, sq)."""
    o, e = case["options"], case["expect"]
    n = case["params"]["n"]
    max_sep = n - 1 if o["max_sep"] < 0 else o["max_sep"]
    msd, rmin, hist, sq = columns(max_sep, o["nbins"], len(o["q"]))
    worst_z = worst_r = 0.0

    def one(i, want, relative):
        nonlocal worst_z, worst_r
        if se[i] == 0.0:
            assert mean[i] == want, (name, i, mean[i], want)
            return
        z = abs(mean[i] - want) / se[i]
        worst_z = max(worst_z, z)
        assert z <= 5.0, (name, i, z)
        if relative:
            r = se[i] / abs(want)
            worst_r = max(worst_r, r)
            assert r <= 0.02, (name, i, r)

    for s, want in zip(e.get("msd_s", []), e.get("msd", [])):
        one(msd.start + s - 1, want, True)
    if "rmin" in e:
        one(rmin.start, e["rmin"], True)
    if "hist" in e:      # the share of a chain's counted pairs per column, "above" last
        pairs = pairs_counted(n, o["min_sep"])
        for j, share in enumerate(e["hist"]):
            one(hist.start + j, share * pairs, False)
    for j, want in enumerate(e.get("sq", [])):
        one(sq.start + j, want, True)
    return worst_z, worst_r
