"""The numpy twin of the energy recorder's contract (include/pstat.h, DESIGN.md 3.19, polymer_stats_amd/csrc/pstat_energy.hip):
written from the contract, sharing no code with the library.

Angles come as pstat_chain_state returns them: angles[C, 2n], theta[n] then phi[n], radians (a planar handle's theta is unused).
`case`: anything with the attributes E0, K1, K2, mu, Fz, Fx, b, bend_mod, bend_angle, chain_type (a pstat_params, or Case below).
  unit vectors  n_i = (cos phi sin theta, sin phi sin theta, cos theta); planar n_i = (cos phi, 0, sin phi)
  dipoles       dielectric mu_i = f n_i + (0, 0, K2 E0) with f = ((K1 - K2) E0) n_{i,z}; polar mu_i = mu n_i
  positions     x_i = b (sum_{j <= i} n_j - n_i / 2)
  pair term     i < j: d = x_j - x_i; r2 = (d_x d_x + d_y d_y) + d_z d_z; r = sqrt(r2); mm = mu_i . mu_j; a = mu_i . d; c = mu_j . d;
                t_ij = (mm - 3 ((a c) / r2)) / (FOURPI (r2 r)), FOURPI = 4.0 * 3.14159265358979323846
  columns       field   sum_i (-E0 / 2) mu_{i,z}
                work    -(Fx R_x + Fz R_z), R = x_{n-1} + (b / 2) n_{n-1}
                bend    sum_{i < n-1} ((kappa / 2)(psi_i - psi0))(psi_i - psi0), psi_i = acos(clamp(n_i . n_{i+1})); 0.0 when kappa = 0
                pair[s] s = 1 .. max_sep: sum_i t_{i,i+s}
                rest    sum over the pairs with j - i > max_sep; 0.0 when there is none
                within  sum over the pairs with r2 <= crad2, crad = cutoff * b, crad2 = crad * crad (only with a cutoff)
  model total   by energy type: 0 field + work + bend | 2 (Ising) that + pair[1] | 1 (interacting) that + every pair column + rest
                | 3 (cutoff) within alone
  per case and column: sum over chains, and sum of squares.
The device adds a separation's terms lane by lane and through a shuffle tree, pairs the separations s and n - s in one pass and folds
the chains of a tile, then the tiles (pstat_energy.hip states the order); the twin adds with numpy's sums.  The device's positions
come from tile_positions' scan in f64; the twin's separations d = x_j - x_i are formed in extended precision (numpy's longdouble,
64 bits of mantissa) and rounded once, so that the cancellation in a close pair's d is the device's alone to answer for.  The
trees differ, so the comparison is through THE BOUND below, never bit for bit.

THE BOUND on |device - twin| (value_bounds, bounds below), derived, not fitted.  u = 2^-53, L = n |b|, P = n (n - 1) / 2,
mumax = |(K1 - K2) E0| + |K2 E0| (polar: |mu|) >= |mu_i|.
  unit vector   two < 1 ulp sincos on either side and one product: a component is off by at most eps_n = 6 u.
  dipole        f = ma n_z, f n_a, + mb: a component is off by at most eps_mu = 16 u mumax.
  position      shape_ref's: a component of x_i is off by at most eps_x = L u (n + 8) on either side (the `work` column).
  separation    d = x_j - x_i.  In exact arithmetic only the unit vectors i .. j enter it, each off by eps_n:  (j - i + 1) b eps_n
                on either side.  The device's two positions each went through tile_positions: with seg = ceil(n / 64), a lane's
                seg - 1 additions, the 6 of wave_scan, seg more, a subtraction and a product, each rounding a number of size
                <= n b:  L u (2 seg + 8) per position.  The twin's d is rounded from extended precision once, and its inputs to
                longdouble are the doubles:  2 u L.  Together, for both sides,
                    eps_d(i, j) = L u (4 seg + 18) + 12 u b (j - i + 1).
  pair term     T(d) = [mu_i . mu_j - 3 (mu_i . dh)(mu_j . dh)] / (4 pi r^3), dh = d / r.  With m_i = |mu_i|, m2 = 1.01 m_i m_j
                (the twin's own moduli, 1 % above what they round to):  |T| <= 4 m2 / (4 pi r^3).
                separation  |grad_d T| <= (3 + 6 + 15) m2 / (4 pi r^4); |delta d| <= sqrt(3) eps_d; while that is below r / 200
                            the gradient along the way is at most 1.1 times the one at r:  46 m2 eps_d / (4 pi r^4), device and
                            twin together.  This is the magnification by ~ 3 n b eps / r of the issue: a relative error of
                            11.5 eps_d / r.  A pair closer than 200 sqrt(3) eps_d has no bound (inf): the tests' inputs have none.
                dipoles     T is bilinear: 4 sqrt(3) eps_mu (m_i + m_j) / (4 pi r^3) <= 112 u mumax (m_i + m_j) / (4 pi r^3).
                roundings   mm, a, c: three products and two additions each (3 u of m2, m_i r, m_j r); a c (7 u), / r2 (r2's own
                            three products and two additions 3 u, the division u), times 3 (u), the subtraction (u of 4 m2):
                            43 u m2; the denominator sqrt (2 u), r2 r (6 u), FOURPI (7 u), the division (8 u of 4 m2):  at most
                            80 u m2 / (4 pi r^3).
                Device and twin are each off by the last two from the exact value:
                    w_ij = [m2 (46 eps_d(i, j) / r + 160 u) + 224 u mumax (m_i + m_j)] / (4 pi r^3).
  pair columns  K terms added in two different orders: (K - 1) u sum|t| each side, K <= P:  E = sum w_ij + 2 P u sum |t_ij| over
                the column's pairs.
  within        as a pair column, and a pair whose r2 lies within 2 (eps_r2 + 4 u crad2) of crad2 (eps_r2 = L^2 u (12 n + 108),
                pdist_ref) may be counted on one side only: its |t_ij| + w_ij is added to E.  Such pairs are UNDECIDED; the twin
                reports how many there are, and the tests' inputs have none.
  field         a term is off by (|E0| / 2)(eps_mu + u mumax) on either side; n terms in two orders:  E = |E0| mumax n u (17 + n).
  work          R_a = x_a + (b / 2) n_a is off by eps_x + 3 u L; two products and one addition:  E = 2 (|Fx| + |Fz|) L u (n + 14).
  bend          the dot product of two unit vectors is off by eps_dot = 48 u (three products of components off by 6 u, two
                additions).  acos is not Lipschitz at +-1, so the bound depends on psi: with s = sin psi^ of the twin's angle,
                s^2 > 16 eps_dot gives |delta psi| <= 2 eps_dot / s, otherwise 3 sqrt(eps_dot); the two arccosines' own errors
                (1.2 ulp, < 1 ulp) add 4 u pi.  A term (kappa / 2) D^2, D = psi - psi0, moves by kappa (|D| + dpsi) dpsi + 3 u of
                itself per side; n - 1 terms in two orders:  E = sum_i [kappa (|D_i| + dpsi_i) dpsi_i] + (6 + 2 n) u sum |term|.
                The two sides' dpsi are one bound on their difference, so it enters once.  kappa = 0: the column is 0.0 on both sides.
  totals        M values v_c per column, each within E_c of the twin's, added in two orders:  on `sum`  sum_c E_c + 2 M u sum |v_c|;
                on `sumsq`  sum_c (2 |v_c| + E_c) E_c + 2 (M + 2) u sum v_c^2.  A row is one record's sum divided by num_chains and
                rounded once.
  model total   the energy the step kernel carries against the twin's model total, per case (model_bound): the bounds of the columns
                involved, their host-side addition, and what the home's own U may be off by after T steps.  Every step kernel sets
                U from a full evaluation at initialisation (pstat_kernels.hip init, `U = usum + upair - (r . F)`); afterwards the
                sweep kernels, the fixed-force all-pairs kernel (pstat_interacting.hip, `U += dU`), the clustering kernels
                (`OU + dU`) and the planar kernel CARRY it by increments, one per accepted move, at most n per step -- and the
                clustering all-pairs kernel (pstat_cluster_wave.hip) RECOMPUTES it in full (total_U) for every proposal it judges.
                An increment is a difference of terms of the chain's scale S (sum of |terms| of the model's columns) with a few roundings, and its addition
                rounds once at the size of U <= S: at most 8 u S per move; a full evaluation is off by 2 P u S like a twin column.
                So per chain  (8 T n + 2 P) u S GROWTH.  S is the larger of the chain's scales at the snapshots the test observes;
                GROWTH = 16 allows for the scale between snapshots having been larger than at them (a close pair that has parted
                since) -- the one allowance here that is an assumption and not a derivation.  THE CONDITION that keeps the test
                meaningful, asserted there: the whole bound stays below 1e-9 times the case's sum over chains of that scale; a
                missing or wrong term is of order 1 on it."""
import collections

import numpy as np

U = 2.0 ** -53
FOURPI = 4.0 * 3.14159265358979323846
GROWTH = 16.0
NONINTERACTING, INTERACTING, ISING, CUTOFF = 0, 1, 2, 3

Case = collections.namedtuple("Case", "E0 K1 K2 mu Fz Fx b bend_mod bend_angle chain_type",
                              defaults=(0.0, 1.0, 0.0, 1e-2, 0.0, 0.0, 1.0, 0.0, 0.0, 0))
Twin = collections.namedtuple("Twin", "values absum weight abscols bend_err within_err undecided rfloor")


def unit_vectors(angles, planar=False):
    a = np.asarray(angles, dtype=np.float64)
    n = a.shape[1] // 2
    theta, phi = a[:, :n], a[:, n:]
    if planar:
        return np.stack([np.cos(phi), np.zeros_like(phi), np.sin(phi)], axis=-1)
    return np.stack([np.cos(phi) * np.sin(theta), np.sin(phi) * np.sin(theta), np.cos(theta)], axis=-1)


def dipoles(nhat, case):
    if int(case.chain_type) == 1:
        return case.mu * nhat
    f = ((case.K1 - case.K2) * case.E0) * nhat[:, :, 2]
    mu = f[:, :, None] * nhat
    mu[:, :, 2] += case.K2 * case.E0
    return mu


def mumax(case):
    return abs(case.mu) if int(case.chain_type) == 1 else abs((case.K1 - case.K2) * case.E0) + abs(case.K2 * case.E0)


def positions(nhat, b):
    return b * (np.cumsum(nhat, axis=1) - nhat / 2)


def separations(nhat, b):
    """d [C, P, 3] = x_j - x_i over the pairs i < j in the order of np.triu_indices(n, 1), formed in extended precision and rounded
    once."""
    assert np.finfo(np.longdouble).eps < 1e-18, "the twin's separations need an extended-precision longdouble"
    wide = np.asarray(nhat, dtype=np.longdouble)
    x = np.longdouble(b) * (np.cumsum(wide, axis=1) - wide / 2)
    I, J = np.triu_indices(nhat.shape[1], 1)
    return (x[:, J, :] - x[:, I, :]).astype(np.float64)


def dot3(p, q):
    return (p[..., 0] * q[..., 0] + p[..., 1] * q[..., 1]) + p[..., 2] * q[..., 2]


def pair_terms(d, mu):
    """(t, r2, r), each [C, P], from the separations d [C, P, 3] and the dipoles mu [C, n, 3]; r = 0 gives a non-finite t."""
    I, J = np.triu_indices(mu.shape[1], 1)
    r2 = dot3(d, d)
    r = np.sqrt(r2)
    mm, a, c = dot3(mu[:, I, :], mu[:, J, :]), dot3(mu[:, I, :], d), dot3(mu[:, J, :], d)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (mm - 3.0 * ((a * c) / r2)) / (FOURPI * (r2 * r))
    return t, r2, r


def ncols(max_sep, cutoff):
    return 3 + max_sep + 1 + (1 if cutoff else 0)


def crad2_of(cutoff, b):
    crad = cutoff * b
    return crad * crad


def model_columns(energy_type, max_sep, cutoff):
    if energy_type == CUTOFF:
        assert cutoff, "a cutoff handle's model total is its `within` column"
        return [4 + max_sep]
    if energy_type == ISING:
        return [0, 1, 2, 3]
    if energy_type == INTERACTING:
        return list(range(0, 4 + max_sep))
    return [0, 1, 2]


def eps_d(n, b, sep):
    """The docstring's eps_d(i, j) for pairs `sep` = j - i apart."""
    return n * abs(b) * U * (4 * ((n + 63) // 64) + 18) + 12 * U * abs(b) * (np.asarray(sep) + 1)


def eps_r2(n, b):
    L = n * abs(b)
    return L * L * U * (12 * n + 108)


def per_chain(angles, case, max_sep=-1, cutoff=0.0, planar=False, nhat=None):
    """A Twin: values [C, ncols], every chain's columns; absum [C], the sum of the absolute values of all its terms (field, work,
    bend and every pair term); weight [C, P], the bound w_ij on a pair term, the conditioning weight of the docstring, in the order
    of np.triu_indices(n, 1); abscols [C, ncols], sum |term| per column; bend_err [C], the bend column's conditioning sum;
    within_err [C], the sum of w_ij over the pairs inside the radius and of |t_ij| + w_ij over the undecided ones; undecided [C],
    the pairs too close to the radius to be decided; rfloor, the smallest distance in the data.  `nhat` [C, n, 3]: unit vectors
    given directly in place of the angles', for configurations no angle in radians reaches (two monomers on one point)."""
    a = np.asarray(angles, dtype=np.float64)
    C, n = a.shape[0], a.shape[1] // 2
    if max_sep < 0:
        max_sep = n - 1
    nc = ncols(max_sep, cutoff)
    b, kappa, psi0, mm = float(case.b), float(case.bend_mod), float(case.bend_angle), mumax(case)
    nhat = unit_vectors(a, planar) if nhat is None else np.asarray(nhat, dtype=np.float64)
    mu = dipoles(nhat, case)
    x = positions(nhat, b)
    values, abscols = np.zeros((C, nc)), np.zeros((C, nc))
    terms = (-0.5 * case.E0) * mu[:, :, 2]
    values[:, 0], abscols[:, 0] = terms.sum(axis=1), np.abs(terms).sum(axis=1)
    R = x[:, n - 1, :] + (b / 2) * nhat[:, n - 1, :]
    values[:, 1] = -(case.Fx * R[:, 0] + case.Fz * R[:, 2])
    abscols[:, 1] = np.abs(case.Fx * R[:, 0]) + np.abs(case.Fz * R[:, 2])
    bend_err = np.zeros(C)
    if kappa != 0.0 and n > 1:
        psi = np.arccos(np.clip(dot3(nhat[:, :-1, :], nhat[:, 1:, :]), -1.0, 1.0))
        D = psi - psi0
        terms = ((kappa / 2) * D) * D
        values[:, 2], abscols[:, 2] = terms.sum(axis=1), np.abs(terms).sum(axis=1)
        e_dot, s = 48 * U, np.sin(psi)
        with np.errstate(divide="ignore"):
            dpsi = np.where(s * s > 16 * e_dot, 2 * e_dot / s, 3 * np.sqrt(e_dot)) + 4 * U * np.pi
        bend_err = (abs(kappa) * (np.abs(D) + dpsi) * dpsi).sum(axis=1)
    I, J = np.triu_indices(n, 1)
    sep = J - I
    t, r2, r = pair_terms(separations(nhat, b), mu) if n > 1 else (np.zeros((C, 0)),) * 3
    ed = eps_d(n, b, sep)[None, :]
    mod = np.sqrt(dot3(mu, mu))
    m2, msum = 1.01 * mod[:, I] * mod[:, J], 1.01 * (mod[:, I] + mod[:, J])
    with np.errstate(divide="ignore", invalid="ignore"):
        weight = (m2 * (46 * ed / r + 160 * U) + 224 * U * mm * msum) / (FOURPI * (r2 * r))
        weight = np.where(r > 200 * np.sqrt(3.0) * ed, weight, np.inf)
    at = np.abs(t)
    for s in range(1, max_sep + 1):
        values[:, 2 + s], abscols[:, 2 + s] = t[:, sep == s].sum(axis=1), at[:, sep == s].sum(axis=1)
    far = sep > max_sep
    if far.any():
        values[:, 3 + max_sep], abscols[:, 3 + max_sep] = t[:, far].sum(axis=1), at[:, far].sum(axis=1)
    undecided, within_err = np.zeros(C, dtype=np.int64), np.zeros(C)
    if cutoff:
        c2 = crad2_of(cutoff, b)
        inside = ~(r2 > c2)
        values[:, 4 + max_sep] = np.where(inside, t, 0.0).sum(axis=1)
        abscols[:, 4 + max_sep] = np.where(inside, at, 0.0).sum(axis=1)
        open_ = np.abs(r2 - c2) <= 2 * (eps_r2(n, b) + 4 * U * c2)
        undecided = open_.sum(axis=1)
        within_err = np.where(inside | open_, weight, 0.0).sum(axis=1) + np.where(open_, at, 0.0).sum(axis=1)
    absum = abscols[:, :3].sum(axis=1) + at.sum(axis=1)
    return Twin(values, absum, weight, abscols, bend_err, within_err, undecided, float(r.min()) if r.size else np.inf)


def value_bounds(tw, case, n, max_sep=-1, cutoff=0.0):
    """E [C, ncols]: the docstring's bound on |device - twin| of every chain's every column, on the data of the Twin `tw`."""
    if max_sep < 0:
        max_sep = n - 1
    C, nc = tw.values.shape
    L, P, mm = n * abs(case.b), n * (n - 1) / 2, mumax(case)
    E = np.zeros((C, nc))
    E[:, 0] = abs(case.E0) * mm * n * U * (17 + n)
    E[:, 1] = 2 * (abs(case.Fx) + abs(case.Fz)) * L * U * (n + 14)
    if case.bend_mod != 0.0:
        E[:, 2] = tw.bend_err + (6 + 2 * n) * U * tw.abscols[:, 2]
    I, J = np.triu_indices(n, 1)
    sep = J - I
    for s in range(1, max_sep + 1):
        E[:, 2 + s] = tw.weight[:, sep == s].sum(axis=1) + 2 * P * U * tw.abscols[:, 2 + s]
    far = sep > max_sep
    if far.any():
        E[:, 3 + max_sep] = tw.weight[:, far].sum(axis=1) + 2 * P * U * tw.abscols[:, 3 + max_sep]
    if cutoff:
        E[:, 4 + max_sep] = tw.within_err + 2 * P * U * tw.abscols[:, 4 + max_sep]
    return E


def bounds(tw, case, n, M, max_sep=-1, cutoff=0.0, E=None):
    """(bound on sum, bound on sumsq), each [ncols], for the total over the C chains of the Twin `tw` (or of several, concatenated
    by the caller) among M values per column."""
    E = value_bounds(tw, case, n, max_sep, cutoff) if E is None else E
    v = np.abs(tw.values)
    b1 = E.sum(axis=0) + 2 * M * U * v.sum(axis=0)
    b2 = ((2 * v + E) * E).sum(axis=0) + 2 * (M + 2) * U * (v * v).sum(axis=0)
    return b1, b2


def row_bound(tw, case, n, max_sep=-1, cutoff=0.0):
    """[ncols]: the bound on a kept row, the mean over the C chains of one record (the Twin `tw`)."""
    C = len(tw.values)
    b1, _ = bounds(tw, case, n, C, max_sep, cutoff)
    return b1 / C + U * np.abs(tw.values.sum(axis=0) / C)


def model_values(tw, energy_type, max_sep, cutoff=0.0):
    """[C]: the twin's model total of every chain."""
    return tw.values[:, model_columns(energy_type, max_sep, cutoff)].sum(axis=1)


def model_bound(snapshots, case, n, T, energy_type, max_sep=-1, cutoff=0.0):
    """(bound, scale): the docstring's bound on |sum over the model columns of the device's `sum` - sum_c U_c of the step kernel|
    for one case after T steps, and the case's sum over chains of the sum of |terms| of the model's columns.  `snapshots`: the Twins of the same chains at the
    moments the test observed, the last one the state that is compared."""
    if max_sep < 0:
        max_sep = n - 1
    tw = snapshots[-1]
    cols = model_columns(energy_type, max_sep, cutoff)
    b1, _ = bounds(tw, case, n, len(tw.values), max_sep, cutoff)
    twin_side = b1[cols].sum() + len(cols) * U * np.abs(tw.values[:, cols]).sum()
    S = np.max([s.abscols[:, cols].sum(axis=1) for s in snapshots], axis=0)
    P = n * (n - 1) / 2
    home = ((8 * T * n + 2 * P) * U * S * GROWTH).sum() + 2 * len(S) * U * S.sum()
    return float(twin_side + home), float(tw.abscols[:, cols].sum())


def judge(name, mean, se, want):
    """The statistical judge of the closed forms (tests/test_energy_cpu.py on sampled chains, tests/test_gpu_energy.py on the
    device's): `mean` within 5 of its across-chain standard errors `se` of `want`, that error at most 2 % of the value.  A column
    without variance is held to equality within 1e-12 relative.  Returns (|z|, relative error)."""
    if se == 0.0 or abs(want) == 0.0:
        assert abs(mean - want) <= 1e-12 * max(1.0, abs(want)), (name, mean, want)
        return 0.0, 0.0
    z, rel = abs(mean - want) / se, se / abs(want)
    assert z <= 5.0, (name, mean, want, se, z)
    assert rel <= 0.02, (name, mean, want, se, rel)
    return z, rel
