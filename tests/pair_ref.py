"""The pair census of the all-pairs kernels (pstat_wave.h: ring_pair_sum, ring_pair_sum_pk): the literal sum over i < j in
long double, configurations that make ONE pair visible, and the bounds the kernels' own sums are held to.  No GPU here;
tests/test_pair_census_cpu.py checks the conditions, tests/test_gpu_pair_census.py runs the kernels.

THE LITERAL SUM.  U = sum_i -E0/2 mu_i,z + sum_{i<j} t_ij - (r_x Fx + r_z Fz), with
    t_ij = (mu_i . mu_j - 3 (mu_i . rhat)(mu_j . rhat)) / (4 pi |r|^3),  r = x_i - x_j        inc/eap_chain.jl:196-211
    x_i = b (sum_{k<=i} n_k - n_i / 2),  n = (cos phi sin theta, sin phi sin theta, cos theta)  inc/eap_chain.jl:49-51
    mu_i = (K1 - K2) E0 cos(theta_i) n_i + K2 E0 z (dielectric),  mu n_i (polar)
and with --energy-type cutoff the functor of inc/eap_chain.jl:171-192: the pair terms with r^2 <= (cutoff-radius b)^2 ALONE --
no field term, no force term (the reference's UCutoff returns the truncated pair sum and nothing else, and so do the
kernels: pstat_cluster_wave.hip, total_U).  Angles enter as the device holds them: f64 in radians, f32 as the stored float
in turns, converted exactly (a float is a long double) and multiplied by the long double 2 pi.  PSTAT_Q16 is rejected for
the all-pairs energies by pstat_create, so there is no lattice case.

HOW A CONFIGURATION REACHES THE KERNEL (set_chain_angles).  pstat_advance(h, 0) returns without a launch, and the zero-step
launch pstat_create uses for its first derivation is not part of the ABI.  So the injected image also sets both proposal
step sizes of every chain to 0 and ONE step is advanced: the proposal of that step is the configuration itself (angle + 0 * s
is exact, theta inside [0, theta_max], phi inside the wrap's range), the trial's pair energy is the ring sum of that same
configuration, and whether the step accepts or not the launch ends with U = sum(u) + ring sum - F.r of the injected angles.
What the census reads is therefore the ring sum instance INSIDE the step loop.  Needs: cluster_prob = 1 (no cluster is
reflected), do_flips = 0, and no adaptation window ending at step 1.

THE BOUNDS.  u = 2^-24 (f32) or 2^-53 (f64).  None of the numbers below was measured on a kernel.
  n-hat      sin and cos carry an absolute error SC = 4 u: f32 is step_judge.SINCOS_ABS (v_sin_f32 / v_cos_f32); f64 is
             sincos_fast_f64's 1.5 ulp of a result <= 1, or 1.5 2^-53 next to a zero (tests/test_gpu_math.py), < 4 u.
             n_z = cos theta: E_Z = SC.  n_x, n_y are products of two: 2 SC + u + SC^2 < E_N = 10 u per component.
  dipole     dielectric a n_z n + k2e z: |d mu| <= |a| (E_Z + sqrt(3) E_N |n_z|) + 4 u |mu| (a itself is rounded to the
             type, two products, one sum); polar: |mu0| sqrt(3) E_N + 2 u |mu|.
  position   x_i = b (prefix_i - n_i / 2).  The i + 1 summands carry E_N each: (i + 1) E_N per component.  The prefix is a tree
             scan over 64 lanes (6 levels) plus M running adds, the subtraction of n_i / 2, the product with b and b's own
             rounding: (M + 10) roundings, each of a partial sum that is a difference of two prefixes, <= 2 PMAX in
             magnitude (PMAX: the largest |component| of any prefix, + 1).  |dx_i| <= sqrt(3) b ((i + 1) E_N + 2 (M + 10) u PMAX).
  pair term  the op-count bound of tests/math_ref.py on exact inputs, K_PAIR u S (S of math_ref.ref_pair: DESIGN 5.3), plus the
             inputs' errors to first order.  With T = |mu_i| |mu_j| / (4 pi r^3), |t| <= 2 T and |grad_r t| <= 12 T / r
             (radial 3 |t| / r <= 6 T / r, the direction of rhat in both projections 6 T / r):
                 12 T (|dx_i| + |dx_j| + sqrt(3) u r) / r      (the last: the rounding of x_i - x_j)
               + 2 (|d mu_i| |mu_j| + |mu_i| |d mu_j|) / (4 pi r^3)      (|u.v - 3 (u.h)(v.h)| <= 2 for unit u, v, h)
  cutoff     a pair whose r^2 lies within a relative CUT_MARGIN of rc^2 is undecided: either verdict is accepted (|t| goes
             into the bound) and the pair is not counted as judged.  The CPU test asserts that the position errors above stay
             inside that margin.
  self       -E0/2 mu_z: |E0|/2 (|a| (2 |n_z| + E_Z) E_Z + 4 u |mu_z|) (dielectric), |E0|/2 (|mu0| E_Z + 2 u |mu_z|) (polar).
  force      r = b sum n: b ((n E_N) + (M + 8) u sum |n_c|) per component, times |F_c|, plus 2 u |F_c r_c|.
  summing    a lane adds its M (M - 1) / 2 own pairs, then per rotation M^2 terms into a fresh accumulator and the L / 2
             accumulators into its sum (packed form: M per partner pair, L M / 4 partner pairs); the butterfly adds 6 more
             and U = sum(u) + pairs - F.r 3.  Every partial sum is at most the sum of the |terms| it holds, so the additions
             err by at most C_SUM u sum |terms|, C_SUM = M^2 + M^2 / 2 + L M / 4 + L / 2 + 16.  (Adding an exact 0 is exact,
             which is why a two-lit chain loses nothing here beyond this.)
"""
from __future__ import annotations

import functools
import math
import struct
from dataclasses import dataclass

import numpy as np

import math_ref as mr
import step_judge as sj

LD = np.longdouble
F32, F64 = sj.F32, sj.F64
DIELECTRIC, POLAR = sj.DIELECTRIC, sj.POLAR
INTERACTING, CUTOFF = sj.INTERACTING, sj.CUTOFF
TWO_PI_LD = 2 * mr.PI_LD

CUT_MARGIN = 1e-3            # relative, on r^2 against rc^2
RESOLVE = 8.0                # a pair is resolved if |t| >= RESOLVE x the bound on |U_device - U_ref|
MIN_DIST_A = 0.3             # b: the smallest |x_a - x_b| any injected two-lit chain may have
MIN_DIST_B = 0.5             # b: family B
TILT = 0.6                   # rad: the two lit monomers stand at theta = pi / 2 +- TILT
ROW = 15                     # dark fold: rows of ROW monomers along +-x joined by single monomers along +y
MAX_CHAINS = 4096

# the ring's edges for every M (the issue's list)
CENSUS_N = (2, 3, 63, 64, 65, 66, 100, 127, 128, 129, 130, 200, 253, 256, 257, 264, 400, 505, 512)


def unit(precision: int) -> float:
    return sj.U if precision == F32 else 2.0 ** -53


def ring(n: int):
    """(M, L) of pstat_wave.h: monomers per lane and lanes in the ring."""
    M = 1 if n <= 64 else 2 if n <= 128 else 4 if n <= 256 else 8
    return M, ((n + M - 1) // M + 1) & ~1


def c_sum(n: int) -> float:
    M, L = ring(n)
    return M * M + M * M / 2 + L * M / 4 + L / 2 + 16


# ------------------------------------------------------------------------------------------------ the literal sum

def stored(theta_rad, phi_rad, precision):
    """Angles in radians -> the arrays the device stores: f64 radians, f32 turns rounded to float (phi wrapped to [0, 1))."""
    theta_rad, phi_rad = np.asarray(theta_rad, dtype=np.float64), np.asarray(phi_rad, dtype=np.float64)
    if precision == F64:
        return theta_rad.copy(), phi_rad.copy()
    th = (theta_rad / (2 * math.pi)).astype(np.float32)
    ph = ((phi_rad / (2 * math.pi)) % 1.0).astype(np.float32)
    ph[ph >= 1.0] = 0.0
    return th, ph


def radians_ld(a, precision):
    a = np.asarray(a).astype(LD)
    return a * TWO_PI_LD if precision == F32 else a


def nhat_ld(theta, phi, precision):
    th, ph = radians_ld(theta, precision), radians_ld(phi, precision)
    st = np.sin(th)
    return np.stack([np.cos(ph) * st, np.sin(ph) * st, np.cos(th)], axis=-1)


def dipoles_ld(p, nh):
    if p["chain_type"] == DIELECTRIC:
        a = LD(p.get("K1", 1.0) - p.get("K2", 0.0)) * LD(p["E0"])
        mu = (a * nh[..., 2])[..., None] * nh
        mu[..., 2] += LD(p.get("K2", 0.0)) * LD(p["E0"])
        return mu
    return LD(p.get("mu", 1e-2)) * nh


def coupling(p):
    """(|a| or |mu0|, |K2 E0| or 0): the coefficients of the dipole."""
    if p["chain_type"] == DIELECTRIC:
        return abs((p.get("K1", 1.0) - p.get("K2", 0.0)) * p["E0"]), abs(p.get("K2", 0.0) * p["E0"])
    return abs(p.get("mu", 1e-2)), 0.0


def rc2_of(p) -> float:
    return (p.get("cutoff_radius", 7.5) * p.get("b", 1.0)) ** 2


@dataclass
class Literal:
    U: float                 # long double, rounded to double at the end
    bound: float
    t: np.ndarray            # float64 [pairs]: the pair terms (all of them, cut or not)
    r2: np.ndarray           # float64 [pairs]
    live: np.ndarray         # bool [pairs]: inside the cutoff (all True without one)
    undecided: np.ndarray    # bool [pairs]: within CUT_MARGIN of rc^2
    dmin: float              # smallest pair distance / b
    pos_rel: float           # largest 2 (|dx_i| + |dx_j|) / r over the pairs within 10 % of rc^2: must stay inside CUT_MARGIN


def literal(p: dict, theta, phi, precision: int) -> Literal:
    """One chain: the literal sum in long double from the STORED angles, and the bound on |U_device - U| derived above."""
    n = len(theta)
    u = unit(precision)
    M, _ = ring(n)
    b = p.get("b", 1.0)
    nh = nhat_ld(theta, phi, precision)
    mu = dipoles_ld(p, nh)
    x = LD(b) * (np.cumsum(nh, axis=0) - nh / 2)
    cut = p["energy_type"] == CUTOFF
    E0 = p["E0"]
    ii, jj = np.triu_indices(n, 1)
    rv = x[ii] - x[jj]
    r2 = (rv * rv).sum(1)
    rm = np.sqrt(r2)
    h = rv / rm[:, None]
    den = LD(4) * mr.PI_LD * r2 * rm
    mi, mj = mu[ii], mu[jj]
    t = ((mi * mj).sum(1) - 3 * (mi * h).sum(1) * (mj * h).sum(1)) / den
    S = ((np.abs(mi * mj).sum(1) + 3 * np.abs(mi * h).sum(1) * np.abs(mj * h).sum(1)) / den).astype(np.float64)
    r2d, rd, td = r2.astype(np.float64), rm.astype(np.float64), t.astype(np.float64)
    rc2 = rc2_of(p) if cut else math.inf
    live = r2d <= rc2
    undecided = np.abs(r2d / rc2 - 1.0) <= CUT_MARGIN if cut else np.zeros(len(td), dtype=bool)
    if cut:
        U = t[live].sum()
    else:
        self_terms = LD(-0.5 * E0) * mu[:, 2]
        r = LD(b) * nh.sum(0)
        U = self_terms.sum() + t.sum() - (r[0] * LD(p.get("Fx", 0.0)) + r[2] * LD(p.get("Fz", 0.0)))
    # ---- the bound (float64 is enough for a bound; every factor is rounded up by the 1.01 at the end)
    nhd, mud = nh.astype(np.float64), mu.astype(np.float64)
    E_Z, E_N = 4 * u, 10 * u
    c1, _ = coupling(p)
    mnorm = np.sqrt((mud * mud).sum(1))
    if p["chain_type"] == DIELECTRIC:
        dmu = c1 * (E_Z + math.sqrt(3) * E_N * np.abs(nhd[:, 2])) + 4 * u * mnorm
        dself = 0.5 * abs(E0) * (c1 * (2 * np.abs(nhd[:, 2]) + E_Z) * E_Z + 4 * u * np.abs(mud[:, 2]))
    else:
        dmu = c1 * math.sqrt(3) * E_N + 2 * u * mnorm
        dself = 0.5 * abs(E0) * (c1 * E_Z + 2 * u * np.abs(mud[:, 2]))
    pmax = float(np.abs(np.cumsum(nhd, axis=0)).max()) + 1.0
    dx = math.sqrt(3) * abs(b) * ((np.arange(n) + 1) * E_N + 2 * (M + 10) * u * pmax)
    T = mnorm[ii] * mnorm[jj] / (4 * math.pi * r2d * rd)
    e_pair = mr.K_PAIR * u * S + 12 * T * (dx[ii] + dx[jj] + math.sqrt(3) * u * rd) / rd \
        + 2 * (dmu[ii] * mnorm[jj] + mnorm[ii] * dmu[jj]) / (4 * math.pi * r2d * rd)
    counted = live | undecided
    bound = e_pair[counted].sum() + np.abs(td[undecided]).sum()
    terms = np.abs(td[counted]).sum()
    if not cut:
        bound += dself.sum()
        terms += np.abs(0.5 * E0 * mud[:, 2]).sum()
        for c, F in ((0, p.get("Fx", 0.0)), (2, p.get("Fz", 0.0))):
            rc_ = abs(b) * np.abs(nhd[:, c]).sum()
            bound += abs(F) * abs(b) * (n * E_N + (M + 8) * u * np.abs(nhd[:, c]).sum()) + 2 * u * abs(F) * rc_
            terms += abs(F) * rc_
    bound += c_sum(n) * u * terms
    near = np.abs(r2d / rc2 - 1.0) <= 0.1 if cut else np.zeros(len(td), dtype=bool)
    pos_rel = float((2 * (dx[ii] + dx[jj]) / rd)[near].max()) if near.any() else 0.0
    return Literal(float(U), 1.01 * float(bound), td, r2d, live, undecided, float(rd.min() / abs(b)) if len(rd) else math.inf,
                   pos_rel)


def literal_mp(p: dict, theta, phi, precision: int):
    """The same sum in 200-bit mpmath (the judge of `literal`), for small n."""
    import mpmath as mp
    mp.mp.prec = 200
    n = len(theta)
    conv = (lambda v: 2 * mp.pi * mp.mpf(float(v))) if precision == F32 else (lambda v: mp.mpf(float(v)))
    th, ph = [conv(v) for v in theta], [conv(v) for v in phi]
    nh = [(mp.cos(ph[i]) * mp.sin(th[i]), mp.sin(ph[i]) * mp.sin(th[i]), mp.cos(th[i])) for i in range(n)]
    E0, b = mp.mpf(p["E0"]), mp.mpf(p.get("b", 1.0))
    if p["chain_type"] == DIELECTRIC:
        K1, K2 = mp.mpf(p.get("K1", 1.0)), mp.mpf(p.get("K2", 0.0))
        mu = [((K1 - K2) * E0 * v[2] * v[0], (K1 - K2) * E0 * v[2] * v[1], (K1 - K2) * E0 * v[2] * v[2] + K2 * E0) for v in nh]
    else:
        mu = [tuple(mp.mpf(p.get("mu", 1e-2)) * c for c in v) for v in nh]
    x, acc = [], [mp.mpf(0)] * 3
    for v in nh:
        acc = [acc[c] + v[c] for c in range(3)]
        x.append([b * (acc[c] - v[c] / 2) for c in range(3)])
    cut = p["energy_type"] == CUTOFF
    rc2 = mp.mpf(p.get("cutoff_radius", 7.5)) * b
    rc2 = rc2 * rc2
    U = mp.mpf(0)
    for i in range(n):
        for j in range(i + 1, n):
            r = [x[i][c] - x[j][c] for c in range(3)]
            r2 = sum(c * c for c in r)
            if cut and r2 > rc2:
                continue
            rm = mp.sqrt(r2)
            dot = lambda a_, b_: sum(a_[c] * b_[c] for c in range(3))
            U += (dot(mu[i], mu[j]) - 3 * dot(mu[i], r) * dot(mu[j], r) / r2) / (4 * mp.pi * r2 * rm)
    if not cut:
        U += sum(-E0 / 2 * m[2] for m in mu)
        U -= b * sum(v[0] for v in nh) * mp.mpf(p.get("Fx", 0.0)) + b * sum(v[2] for v in nh) * mp.mpf(p.get("Fz", 0.0))
    return U


# ------------------------------------------------------------------------------------------------ classes of the ring

def pair_classes(n: int, i, j):
    """For monomers i < j (arrays): (k, own slot, partner slot, order) as four integer arrays.
    k: the rotation that meets the pair (0: inside one lane).  For 1 <= k < L/2 the pair is met once, by the lane `owner` that
    reads ring entry owner + L - k: order 2 if that entry lies in the SECOND copy of the ring (owner is the higher lane),
    order 1 if in the first (owner is the lower lane: the partner is reached around the ring's end).  k = L/2: met from both
    ends at weight 1/2 (order 3; slots of the lower, then the higher lane).  k = 0: order 0, slots of i, then j."""
    M, L = ring(n)
    i, j = np.asarray(i), np.asarray(j)
    la, lb, sa, sb = i // M, j // M, i % M, j % M
    d = lb - la
    k = np.where(d <= L // 2, d, L - d)
    order = np.where(d == 0, 0, np.where(2 * d == L, 3, np.where(d < L // 2, 2, 1)))
    own = np.where(order == 2, sb, sa)
    other = np.where(order == 2, sa, sb)
    return k, own, other, order


def class_key(k, own, other, order):
    return ((np.asarray(k) * 8 + own) * 8 + other) * 4 + order


def required_classes(n: int):
    """Every class that exists among the real monomers with k in {0, 1, 2, L/2 - 1, L/2}: sorted keys."""
    _, L = ring(n)
    ii, jj = np.triu_indices(n, 1)
    k, own, other, order = pair_classes(n, ii, jj)
    want = np.isin(k, [0, 1, 2, L // 2 - 1, L // 2])
    return np.unique(class_key(k, own, other, order)[want])


def class_name(n: int, key: int) -> str:
    order, other, own, k = key % 4, (key // 4) % 8, (key // 32) % 8, key // 256
    _, L = ring(n)
    how = ("inside a lane", "partner in the ring's first copy", "partner in the second copy", "both ends, weight 1/2")[order]
    return f"rotation {k}{' = L/2' if k == L // 2 else ''}, slots ({own}, {other}), {how}"


def census_pairs(n: int, seed: int = 7):
    """The pairs (i < j) of family A at chain length n: every pair for n <= 91; beyond, one per required class, the pairs
    that touch monomer 0, monomer n - 1 and every monomer of a partly filled last lane (against partners in the first, a
    middle and the last lane), then seeded random pairs up to MAX_CHAINS."""
    ii, jj = np.triu_indices(n, 1)
    if len(ii) <= MAX_CHAINS:
        return ii, jj
    M, L = ring(n)
    g = np.random.default_rng(seed + n)
    keys = class_key(*pair_classes(n, ii, jj))
    order = g.permutation(len(ii))
    _, first = np.unique(keys[order], return_index=True)
    chosen = set(order[first][np.isin(keys[order][first], required_classes(n))].tolist())
    index = {(a, b_): q for q, (a, b_) in enumerate(zip(ii.tolist(), jj.tolist()))}
    edge = {0, n - 1}
    if n % M:
        edge |= set(range((n // M) * M, n))
    partners = sorted({0, 1, M, n // 2, n // 2 + 1, n - 2, n - 1} | set(range(min(M, n))) | set(range(max(0, n - M - 1), n)))
    for a in edge:
        for b_ in partners:
            if a != b_:
                chosen.add(index[(min(a, b_), max(a, b_))])
    rest = [q for q in g.permutation(len(ii)).tolist() if q not in chosen]
    sel = np.array(sorted(chosen) + rest[:max(0, MAX_CHAINS - len(chosen))], dtype=np.int64)[:MAX_CHAINS]
    return ii[sel], jj[sel]


# ------------------------------------------------------------------------------------------------ family A: two lit monomers

A_PARAMS = dict(chain_type=DIELECTRIC, E0=1.0, K1=400.0, K2=0.0, Fz=0.0, Fx=0.0, b=1.0, kT=1.0)


def dark_fold(n: int):
    """phi (radians) of the dark fold: rows of ROW monomers along +x / -x, joined by one monomer along +y."""
    phi = np.zeros(n)
    for k in range(n):
        row, col = divmod(k, ROW + 1)
        phi[k] = math.pi / 2 if col == ROW else (0.0 if row % 2 == 0 else math.pi)
    return phi


@dataclass
class FamilyA:
    n: int
    precision: int
    cutoff: bool
    params: dict
    i: np.ndarray            # [K] lit monomers i < j and their tilt signs
    j: np.ndarray
    si: np.ndarray
    sj: np.ndarray
    theta: np.ndarray        # [K, n] stored angles
    phi: np.ndarray
    U: np.ndarray            # [K] reference
    bound: np.ndarray        # [K]
    t: np.ndarray            # [K] the lit pair's term (before the cutoff)
    live: np.ndarray         # [K] the lit pair is inside the cutoff
    undecided: np.ndarray    # [K]
    keys: np.ndarray         # [K] class keys
    dmin: float              # certified lower bound on every pair distance of every chain, / b
    candidates: int          # pairs offered (before the |t| >= RESOLVE x bound filter)
    missing_pairs: int       # offered pairs of which NO sign choice is resolved


def _shift_min_distance(x_fold, shifts, b):
    """min over fold pairs a < b and the given relative shifts s of |x_b - x_a + s|: a lower bound on every distance of every
    two-lit chain (whose monomers sit at fold position + an offset that depends on the side of the lit monomers only)."""
    n = len(x_fold)
    if n < 2:
        return math.inf
    ii, jj = np.triu_indices(n, 1)
    d = x_fold[jj] - x_fold[ii]
    best = math.inf
    for s in shifts:
        v = d + s
        best = min(best, float(np.sqrt((v * v).sum(1)).min()))
    return best / b


@functools.lru_cache(maxsize=4)
def _family_a_chains(n: int, precision: int):
    """The two-lit chains of chain length n and everything about them that does not depend on the energy type.  For every
    offered pair the four tilt sign choices are evaluated; with few enough pairs (4 x pairs <= MAX_CHAINS) each is a chain,
    otherwise the one whose term stands highest above the errors of the pair term and the two self terms."""
    p = dict(A_PARAMS, n=n)
    u = unit(precision)
    M, _ = ring(n)
    b, E0 = p["b"], p["E0"]
    a = (p["K1"] - p["K2"]) * E0
    E_Z, E_N = 4 * u, 10 * u
    # |n_z| of a dark monomer.  f32: v_cos_f32 of exactly 1/4 turn is exactly 0 (asserted by tests/test_gpu_math.py), so a dark
    # monomer's dipole a n_z n is an exact zero and there is no dust; f64: cos(fl(pi / 2)) = 6.1e-17 within SC
    D = 0.0 if precision == F32 else 4 * u
    I, J = census_pairs(n)
    npairs = len(I)
    th_dark, ph_fold = stored(np.full(n, math.pi / 2), dark_fold(n), precision)
    th_lit = {s: stored(np.array([math.pi / 2 + s * TILT]), np.zeros(1), precision)[0][0] for s in (+1, -1)}
    nd = nhat_ld(th_dark, ph_fold, precision)                      # [n, 3] the dark chain
    assert float(np.abs(nd[:, 2]).max()) <= 4 * u                     # the dust is carried in the bound: the reference's dark monomers are dark
    Pd = np.cumsum(nd, axis=0)
    pmax = float(np.abs(Pd).max()) + 2.0
    nl = {s: nhat_ld(np.full(n, th_lit[s]), ph_fold, precision) for s in (+1, -1)}     # [n, 3]: monomer k lit with sign s
    x_fold = (b * (Pd - nd / 2)).astype(np.float64)

    def evaluate(Iq, Jq, SI, SJ):
        o = dict(i=Iq, j=Jq, si=SI, sj=SJ)
        nli = np.where((SI == 1)[:, None], nl[1][Iq], nl[-1][Iq])
        nlj = np.where((SJ == 1)[:, None], nl[1][Jq], nl[-1][Jq])
        di, dj = nli - nd[Iq], nlj - nd[Jq]                       # what lighting a monomer adds to every later prefix
        xi = LD(b) * (Pd[Iq] - nd[Iq] + nli / 2)
        xj = LD(b) * (Pd[Jq] + di - nd[Jq] + nlj / 2)
        mi, mj = (LD(a) * nli[:, 2])[:, None] * nli, (LD(a) * nlj[:, 2])[:, None] * nlj
        rv = xi - xj
        r2 = (rv * rv).sum(1)
        rm = np.sqrt(r2)
        h = rv / rm[:, None]
        den = LD(4) * mr.PI_LD * r2 * rm
        o["t_ld"] = ((mi * mj).sum(1) - 3 * (mi * h).sum(1) * (mj * h).sum(1)) / den
        S = ((np.abs(mi * mj).sum(1) + 3 * np.abs(mi * h).sum(1) * np.abs(mj * h).sum(1)) / den).astype(np.float64)
        o["selfs_ld"] = LD(-0.5 * E0) * (mi[:, 2] + mj[:, 2])
        o["r2"], rd, o["t"] = r2.astype(np.float64), rm.astype(np.float64), o["t_ld"].astype(np.float64)
        nzi, nzj = np.abs(nli[:, 2]).astype(np.float64), np.abs(nlj[:, 2]).astype(np.float64)
        mni, mnj = abs(a) * nzi, abs(a) * nzj                      # |mu| = |a n_z| |n|
        dmi = abs(a) * (E_Z + math.sqrt(3) * E_N * nzi) + 4 * u * mni
        dmj = abs(a) * (E_Z + math.sqrt(3) * E_N * nzj) + 4 * u * mnj
        dxi = math.sqrt(3) * b * ((Iq + 1) * E_N + 2 * (M + 10) * u * pmax)
        dxj = math.sqrt(3) * b * ((Jq + 1) * E_N + 2 * (M + 10) * u * pmax)
        T = mni * mnj / (4 * math.pi * o["r2"] * rd)
        o["e_pair"] = mr.K_PAIR * u * S + 12 * T * (dxi + dxj + math.sqrt(3) * u * rd) / rd \
            + 2 * (dmi * mnj + mni * dmj) / (4 * math.pi * o["r2"] * rd)
        o["pos_rel"] = 2 * (dxi + dxj) / rd
        o["e_self"] = 0.5 * abs(E0) * (abs(a) * (2 * nzi + E_Z) * E_Z + 4 * u * abs(a) * nzi * nzi) \
            + 0.5 * abs(E0) * (abs(a) * (2 * nzj + E_Z) * E_Z + 4 * u * abs(a) * nzj * nzj) \
            + (n - 2) * 0.5 * abs(E0) * abs(a) * D * D
        o["geo"] = (xi.astype(np.float64), xj.astype(np.float64), b * di.astype(np.float64), b * dj.astype(np.float64), mni, mnj)
        return o

    SI, SJ = np.repeat([1, 1, -1, -1], npairs), np.repeat([1, -1, 1, -1], npairs)
    o = evaluate(np.tile(I, 4), np.tile(J, 4), SI, SJ)
    if 4 * npairs > MAX_CHAINS:
        best = (np.abs(o["t"]) / (o["e_pair"] + o["e_self"])).reshape(4, npairs).argmax(0)
        sel = best * npairs + np.arange(npairs)
        o = evaluate(np.tile(I, 4)[sel], np.tile(J, 4)[sel], SI[sel], SJ[sel])
    Iq, Jq = o["i"], o["j"]
    K = len(Iq)
    # dust: lit-dark terms with |mu_dark| <= |a| D, from the true distances; dark-dark from a bound on sum 1 / r^3
    xid, xjd, did, djd, mni, mnj = o.pop("geo")
    inv3 = np.zeros(K)
    ks = np.arange(n)
    for lo in range(0, K, 256):
        sl = slice(lo, lo + 256)
        X = x_fold[None, :, :] + (ks[None, :] > Iq[sl, None])[:, :, None] * did[sl, None, :] \
            + (ks[None, :] > Jq[sl, None])[:, :, None] * djd[sl, None, :]
        dark = (ks[None, :] != Iq[sl, None]) & (ks[None, :] != Jq[sl, None])
        for xl, ml in ((xid[sl], mni[sl]), (xjd[sl], mnj[sl])):
            rr = np.sqrt(((X - xl[:, None, :]) ** 2).sum(2))
            inv3[sl] += ml * np.where(dark, 1.0 / np.maximum(rr, 1e-300) ** 3, 0.0).sum(1)
    e_dust = 2 * abs(a) * D * inv3 / (4 * math.pi)
    dmin = float(np.sqrt(o["r2"]).min() / b)
    if n > 2:
        dirs = np.unique(np.round(np.concatenate([did, djd]), 12), axis=0)
        shifts = [np.zeros(3)] + [f * v for v in dirs for f in (0.5, 1.0)] + \
                 [fa * va + fb * vb for va in dirs for vb in dirs for fa, fb in ((1, .5), (1, 1), (.5, .5), (.5, 1))]
        dmin = _shift_min_distance(x_fold, shifts, b)
        fi, fj = np.triu_indices(n, 1)
        rf = np.sqrt(((x_fold[fi] - x_fold[fj]) ** 2).sum(1))
        smax = max(float(np.sqrt((s * s).sum())) for s in shifts)
        e_dust = e_dust + (a * D) ** 2 * 2 / (4 * math.pi) * float((1.0 / np.maximum(rf - smax, dmin * b) ** 3).sum())
    o["e_dust"] = e_dust
    theta = np.tile(th_dark, (K, 1))
    phi = np.tile(ph_fold, (K, 1))
    rows = np.arange(K)
    theta[rows, Iq] = np.where(o["si"] == 1, th_lit[1], th_lit[-1])
    theta[rows, Jq] = np.where(o["sj"] == 1, th_lit[1], th_lit[-1])
    o.update(theta=theta, phi=phi, dmin=dmin, offered=npairs, keys=class_key(*pair_classes(n, Iq, Jq)),
             pair_id=Iq.astype(np.int64) * n + Jq)
    return o


@dataclass
class FamilyA:
    n: int
    precision: int
    cutoff: bool
    params: dict
    theta: np.ndarray        # [K, n] stored angles of EVERY chain of the length (the same chains with and without a cutoff)
    phi: np.ndarray
    i: np.ndarray            # [K] lit monomers i < j
    j: np.ndarray
    U: np.ndarray            # [K] reference
    bound: np.ndarray        # [K]
    t: np.ndarray            # [K] the lit pair's term (before the cutoff)
    live: np.ndarray         # [K] the lit pair is inside the cutoff
    undecided: np.ndarray    # [K] within CUT_MARGIN of the cutoff: not judged
    judged: np.ndarray       # [K] |t| >= RESOLVE x bound and decided
    keys: np.ndarray         # [K] class keys
    dmin: float              # certified lower bound on every pair distance of every chain, / b
    offered: int             # pairs offered
    pos_rel: float           # largest relative move of r^2 by the position errors among pairs within 10 % of rc^2

    def judged_pairs(self) -> int:
        return len(np.unique((self.i.astype(np.int64) * self.n + self.j)[self.judged]))


def family_a(n: int, precision: int, cutoff: bool = False, cutoff_radius: float | None = None) -> FamilyA:
    o = _family_a_chains(n, precision)
    p = dict(A_PARAMS, n=n, energy_type=CUTOFF if cutoff else INTERACTING)
    u = unit(precision)
    td = o["t"]
    if cutoff:
        p["cutoff_radius"] = cutoff_radius
        rc2 = rc2_of(p)
        live = o["r2"] <= rc2
        undecided = np.abs(o["r2"] / rc2 - 1.0) <= CUT_MARGIN
        U = np.where(live, o["t_ld"], LD(0)).astype(np.float64)
        counted = live | undecided
        bound = np.where(counted, o["e_pair"], 0.0) + np.where(undecided, np.abs(td), 0.0) + o["e_dust"]
        terms = np.where(counted, np.abs(td), 0.0) + o["e_dust"]
        near = np.abs(o["r2"] / rc2 - 1.0) <= 0.1
        pos_rel = float(o["pos_rel"][near].max()) if near.any() else 0.0
    else:
        live, undecided = np.ones(len(td), dtype=bool), np.zeros(len(td), dtype=bool)
        U = (o["selfs_ld"] + o["t_ld"]).astype(np.float64)
        bound = o["e_pair"] + o["e_dust"] + o["e_self"]
        terms = np.abs(td) + o["e_dust"] + np.abs(o["selfs_ld"].astype(np.float64))
        pos_rel = 0.0
    bound = 1.01 * (bound + c_sum(n) * u * terms)
    judged = (np.abs(td) >= RESOLVE * bound) & ~undecided
    return FamilyA(n, precision, cutoff, p, o["theta"], o["phi"], o["i"], o["j"], U, bound, td, live, undecided, judged,
                   o["keys"], o["dmin"], o["offered"], pos_rel)


def choose_cutoff_radius(n: int, precision: int = F32) -> float:
    """cutoff-radius (in b) inside the spread of family A's lit-pair distances: the middle of the widest gap between
    neighbouring distinct distances in the central 40 % of them, so that few pairs fall within CUT_MARGIN of it."""
    d = np.sort(np.sqrt(_family_a_chains(n, precision)["r2"])) / A_PARAMS["b"]
    lo, hi = int(0.3 * len(d)), max(int(0.7 * len(d)), int(0.3 * len(d)) + 2)
    mid = d[max(lo - 1, 0):min(hi + 1, len(d))]
    if len(mid) < 2 or mid[-1] - mid[0] < 1e-9:
        mid = d
    if len(mid) < 2 or mid[-1] - mid[0] < 1e-9:
        return float(d[0] * 1.25)          # one distance only: every pair inside
    gaps = np.diff(mid)
    q = int(np.argmax(gaps))
    return float(0.5 * (mid[q] + mid[q + 1]))


# ------------------------------------------------------------------------------------------------ family B: every monomer lit

B_PARAMS = {
    "diel": dict(chain_type=DIELECTRIC, E0=2.0, K1=0.4, K2=1.0, Fz=0.4, Fx=0.7, b=1.3, kT=1.0),
    "polar": dict(chain_type=POLAR, E0=3.0, mu=0.8, Fz=0.4, Fx=0.7, b=1.3, kT=1.0),
}
B_SHAPES = ("rod", "helix")


def _angles_of(tangents):
    t = tangents / np.sqrt((tangents * tangents).sum(1))[:, None]
    return np.arccos(np.clip(t[:, 2], -1, 1)), np.arctan2(t[:, 1], t[:, 0]) % (2 * math.pi)


def shape_b(shape: str, n: int, g) -> tuple:
    """(theta, phi) in radians of one jittered compact chain.  rod: rows of 12 along +-x, two monomers along +y between
    them (row spacing 2 b).  helix: a rising spiral of growing radius (1.3 b per turn, 0.006 b up per monomer): compact in
    three dimensions, yet no pair direction comes near the zero of 1 - 3 cos^2 for dipoles along z."""
    if shape == "rod":
        t = np.zeros((n, 3))
        for k in range(n):
            row, col = divmod(k, 14)
            t[k] = (0, 1, 0) if col >= 12 else ((1, 0, 0) if row % 2 == 0 else (-1, 0, 0))
    else:
        t = np.zeros((n, 3))
        psi, R = 0.0, 1.6
        for k in range(n):
            t[k] = (-math.sin(psi), math.cos(psi), 0.006)
            psi += 1.0 / R
            R += 1.3 / (2 * math.pi * R)
    th, ph = _angles_of(t)
    return np.clip(th + g.uniform(-0.04, 0.04, n), 0.05, math.pi - 0.05), (ph + g.uniform(-0.06, 0.06, n)) % (2 * math.pi)


def chains_per_shape(n: int) -> int:
    """About 64 per shape; fewer for the long chains, whose literal sum costs n^2 long-double terms each."""
    return 64 if n <= 130 else (16 if n <= 256 else 4)


def family_b(n: int, precision: int, chain: str, cutoff: bool = False, cutoff_radius: float | None = None, seed: int = 11):
    """Returns (params, theta[K, n], phi[K, n] stored, [Literal per chain], [shape name per chain])."""
    p = dict(B_PARAMS[chain], n=n, energy_type=CUTOFF if cutoff else INTERACTING)
    if cutoff:
        p["cutoff_radius"] = cutoff_radius
    th_all, ph_all, lits, names = [], [], [], []
    for s, shape in enumerate(B_SHAPES):
        g = np.random.default_rng([seed, n, s])
        made = tries = 0
        while made < chains_per_shape(n):
            tries += 1
            assert tries < 50 * chains_per_shape(n), "the shape does not keep its monomers apart"
            th, ph = stored(*shape_b(shape, n, g), precision)
            if n > 1 and sj.min_pair_distance(p, radians_ld(ph, precision).astype(np.float64),
                                              radians_ld(th, precision).astype(np.float64)) < MIN_DIST_B + 0.02:
                continue
            th_all.append(th); ph_all.append(ph); names.append(shape)
            lits.append(literal(p, th, ph, precision))
            made += 1
    return p, np.stack(th_all), np.stack(ph_all), lits, names


def resolved_share(lit: Literal) -> float:
    """Share of a chain's live, decided pairs whose own term is at least RESOLVE x the chain's bound."""
    judged = lit.live & ~lit.undecided
    return float((np.abs(lit.t[judged]) >= RESOLVE * lit.bound).mean()) if judged.any() else 1.0


# ------------------------------------------------------------------------------------------------ injection (GPU tests only)

def device_params(ps, p: dict, chains: int, precision: int, cluster: bool):
    kw = {k: v for k, v in p.items()}
    return ps.default_params(num_chains=chains, precision=precision, move_set=ps.MOVES_CLUSTER if cluster else ps.MOVES_SINGLE,
                             rng=ps.RNG_MWC64X, seed=1, do_flips=0, steps_per_adjust=50, adj_scale=1.0,
                             **({"cluster_prob": 1.0} if cluster else {}), **kw)


def set_chain_angles(e, theta, phi):
    """Tests only.  theta, phi: [C, n] arrays as the device stores them (f64 radians / f32 turns).  Overwrites the angle planes
    of the handle's checkpoint image -- the first state buffer after the header and the per-case kT list, [2][n][C], plane 0
    theta, element type by the header's precision -- and the proposal step sizes (third state buffer, [2][C] doubles) with 0,
    restores the image and advances ONE step: see the module text for why that launch reports the ring sum of exactly these
    angles.  Sizes come from the header's fields."""
    blob = bytearray(e.checkpoint())
    header_bytes, = struct.unpack_from("<i", blob, 12)
    n, C, ncases = struct.unpack_from("<qqq", blob, 16)
    precision, = struct.unpack_from("<i", blob, 56)
    dt = np.dtype(np.float32) if precision == F32 else np.dtype(np.float64)
    assert precision in (F32, F64)
    theta, phi = np.asarray(theta), np.asarray(phi)
    assert theta.shape == (C, n) and phi.shape == (C, n) and theta.dtype == dt and phi.dtype == dt, (theta.shape, theta.dtype, C, n)
    off = header_bytes + 8 * ncases
    plane = n * C * dt.itemsize
    blob[off:off + plane] = np.ascontiguousarray(theta.T).tobytes()
    blob[off + plane:off + 2 * plane] = np.ascontiguousarray(phi.T).tobytes()
    steps_off = off + 2 * plane + 4 * C * 4          # past the generator words [4][C] uint32
    blob[steps_off:steps_off + 2 * C * 8] = bytes(2 * C * 8)
    e.restore(bytes(blob))
    e.advance(1)


def read_chain_angles(e):
    """(theta, phi) [C, n] as the handle stores them now, read from its checkpoint image."""
    blob = e.checkpoint()
    header_bytes, = struct.unpack_from("<i", blob, 12)
    n, C, ncases = struct.unpack_from("<qqq", blob, 16)
    precision, = struct.unpack_from("<i", blob, 56)
    dt = np.dtype(np.float32) if precision == F32 else np.dtype(np.float64)
    a = np.frombuffer(blob, dtype=dt, count=2 * n * C, offset=header_bytes + 8 * ncases).reshape(2, n, C)
    return a[0].T.copy(), a[1].T.copy()
