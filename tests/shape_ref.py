"""The numpy twin of the shape contract (include/pstat.h, DESIGN.md 3.16, polymer_stats_amd/csrc/pstat_shape.hip): written from
the contract, sharing no code with the library.

Angles come as pstat_chain_state returns them: angles[C, 2n], theta[n] then phi[n], radians (a planar handle's theta is unused).
  3D      n_i = (cos phi sin theta, sin phi sin theta, cos theta)
  planar  n_i = (cos phi, 0, sin phi): the two components sit in the x and z slots, y = 0
  positions   x_i = b (sum_{j <= i} n_j - n_i / 2), the monomers' centres
  gyration    xbar = (1 / n) sum_i x_i;  G_ab = (1 / n) sum_i (x_i - xbar)_a (x_i - xbar)_b, centred first;
              columns gxx, gyy, gzz, gxy, gxz, gyz, rg2 = trace, trg2 = sum_ab G_ab^2 (off-diagonals twice)
  form factor S(q) = (1 / n) [(sum_i cos(q . x_i))^2 + (sum_i sin(q . x_i))^2], one column per row of q[nq, 3] (absolute
              units; q_y is ignored for a planar chain)
  per case and column: sum over chains, and sum of squares.

THE BOUND on |device - twin| (bounds() below), derived, not fitted.  u = 2^-53, L = n b, |q|_1 = |q_x| + |q_y| + |q_z|.
  unit vector   each component is a sincos result (< 1 ulp) or a product of two: off by at most 3 u.
  position      a component of x_i is b times a sum of at most n terms of size <= 1, minus a half term.  Whatever the order,
                the at most n - 1 additions each round a partial sum of size <= n: n (n - 1) u, plus n 3 u from the terms, plus
                the subtraction and the product with b:  eps_x = L u (n + 8).
  phase         three products |q_a| |x_a| <= |q_a| L, each off by |q_a| (eps_x + u L), two additions of partial sums <= |q|_1 L:
                eps_phi = |q|_1 L u (n + 11).
  S             cos and sin of the phase are off by eps_phi + u each.  A = sum cos has n terms of size <= 1: its error is at most
                dA = n (eps_phi + u) + n (n - 1) u.  A^2 + B^2 is off by 2 (2 n dA + u n^2) + 2 u n^2, the division by n makes it
                4 dA + 5 u n <= E_S = 4 n u (|q|_1 L (n + 11) + n + 3).
  G_ab          xbar is off by eps_x + L u (n + 1); d = x_i - xbar, |d| <= L, is off by 2 eps_x + L u (n + 2); a product d_a d_b
                by 2 L times that plus u L^2; the mean of n of them adds (n + 1) u L^2:  (4 (n + 8) + 2 (n + 2) + 1 + n + 1) u L^2
                <= E_G = L^2 u (7 n + 51).
  rg2           three entries and two additions: 3 E_G covers them (the additions' 2 u 3 L^2 are inside E_G's slack for n >= 1).
  trg2          nine products G_ab^2 with |G_ab| <= L^2: each off by 2 L^2 E_G + u L^4; nine of them and their additions:
                18 L^2 E_G + 18 u L^4.
  totals        device and twin may each be off by E per value.  A total of M = num_chains * records values bounded by V, added
                in any order: 2 M E + M^2 u V on `sum`, with V = n for S, L^2 for G and rg2, 3 L^4 for trg2.  On `sumsq` the same
                with E -> 2 V E + u V^2 and V -> V^2.  A row is one record's sum divided by num_chains: its bound is that of
                M = num_chains, divided by num_chains."""
import numpy as np

NAMES = ("gxx", "gyy", "gzz", "gxy", "gxz", "gyz", "rg2", "trg2")
NG = len(NAMES)
U = 2.0 ** -53


def unit_vectors(angles, planar=False):
    """[C, n, 3]; a planar chain's y slot is 0."""
    a = np.asarray(angles, dtype=np.float64)
    n = a.shape[1] // 2
    theta, phi = a[:, :n], a[:, n:]
    if planar:
        return np.stack([np.cos(phi), np.zeros_like(phi), np.sin(phi)], axis=-1)
    return np.stack([np.cos(phi) * np.sin(theta), np.sin(phi) * np.sin(theta), np.cos(theta)], axis=-1)


def positions(angles, b=1.0, planar=False):
    """[C, n, 3]: the monomers' centres."""
    nhat = unit_vectors(angles, planar)
    return b * (np.cumsum(nhat, axis=1) - nhat / 2)


def wave_vectors(q, planar=False):
    """[nq, 3] from None, [nq, 3] or, for a planar chain, [nq, 2] = (q_x, q_z); a planar chain's q_y is set to 0."""
    if q is None or np.size(q) == 0:
        return np.zeros((0, 3))
    q = np.array(q, dtype=np.float64)
    if planar and q.shape[1] == 2:
        q = np.stack([q[:, 0], np.zeros(len(q)), q[:, 1]], axis=1)
    if planar:
        q[:, 1] = 0.0
    return q


def per_chain(angles, b=1.0, q=None, planar=False):
    """[C, 8 + nq]: every chain's values, the gyration block and then S at every wave-vector."""
    x = positions(angles, b, planar)
    n = x.shape[1]
    d = x - x.sum(axis=1, keepdims=True) / n
    g = lambda i, j: (d[:, :, i] * d[:, :, j]).sum(axis=1) / n
    gxx, gyy, gzz, gxy, gxz, gyz = g(0, 0), g(1, 1), g(2, 2), g(0, 1), g(0, 2), g(1, 2)
    rg2 = gxx + gyy + gzz
    trg2 = gxx * gxx + gyy * gyy + gzz * gzz + 2.0 * (gxy * gxy + gxz * gxz + gyz * gyz)
    cols = [gxx, gyy, gzz, gxy, gxz, gyz, rg2, trg2]
    for qv in wave_vectors(q, planar):
        ph = qv[0] * x[:, :, 0] + qv[1] * x[:, :, 1] + qv[2] * x[:, :, 2]
        cols.append((np.cos(ph).sum(axis=1) ** 2 + np.sin(ph).sum(axis=1) ** 2) / n)
    return np.stack(cols, axis=1)


def totals(values):
    """(sum, sumsq) over the chains of per_chain's [C, ncols]."""
    return values.sum(axis=0), (values * values).sum(axis=0)


def value_bounds(n, b, q=None, planar=False):
    """(E, V), each [8 + nq]: the per-value error bound of the docstring and the bound on the value's size."""
    L = n * abs(b)
    EG = L * L * U * (7 * n + 51)
    E = [EG] * 6 + [3 * EG, 18 * L * L * EG + 18 * U * L ** 4]
    V = [L * L] * 7 + [3 * L ** 4]
    for qv in wave_vectors(q, planar):
        q1 = np.abs(qv).sum()
        E.append(4 * n * U * (q1 * L * (n + 11) + n + 3))
        V.append(float(n))
    return np.array(E), np.array(V)


def bounds(n, b, M, q=None, planar=False):
    """(bound on sum, bound on sumsq), each [8 + nq], for a total of M values per column."""
    E, V = value_bounds(n, b, q, planar)
    E2, V2 = 2 * V * E + U * V * V, V * V
    return 2 * M * E + M * M * U * V, 2 * M * E2 + M * M * U * V2


def judge_closed_form(name, case, mean, se):
    """The statistical conditions of tests/test_shape_cpu.py and tests/test_gpu_shape.py on one record of many chains (`mean`,
    `se`: [8 + nq], the pooled means and their across-chain standard errors; `case`: a case of tests/golden/shape_closed_form.json): every column of the fixture within 5 of its own
    across-chain standard errors, and every standard error <= 2 % of the fixture value.  Columns whose closed form is 0 (the
    off-diagonals here; a planar chain's y entries are exact zeros on both sides) have no value to take 2 % of: their standard
    error is held to 2 % of <rg2>, the tensor's own scale.  q = 0 has no variance and is held to exact equality."""
    e = case["expect"]
    want = np.array([e[k] for k in NAMES[:7]] + [np.nan] + list(e["sq"]))
    worst_z = worst_r = 0.0
    for i, w in enumerate(want):
        if i == 7:                                                   # trg2 has no closed form (the generator says why)
            continue
        if i >= 8 and not np.any(case["q"][i - 8]):
            assert mean[i] == w == float(case["params"]["n"]) and se[i] == 0.0
            continue
        if w == 0.0 and se[i] == 0.0:
            assert mean[i] == 0.0, (name, i)
            continue
        z = abs(mean[i] - w) / se[i]
        r = se[i] / (abs(w) if w != 0.0 else e["rg2"])
        worst_z, worst_r = max(worst_z, z), max(worst_r, r)
        assert z <= 5.0, (name, i, z)
        assert r <= 0.02, (name, i, r)
    return worst_z, worst_r
