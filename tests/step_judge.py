"""Per-step comparison of an f32 / q16 kernel with the oracle's one-step judge (oracle/eap_oracle.h: eap_step_judge).

For one chain and one step: the device's state before the step (Ensemble.chain_state), the judge's output for that state,
the device's state after.  `compare` gives "agree", "undecided" (left out of the comparison) or "wrong".

Everything the f32 / q16 kernels are held to here is derived below from the unit roundoff of f32 and the documented accuracy
of the instructions they use -- nothing from what a kernel returned.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np

F32, F64, Q16 = 0, 1, 2
DIELECTRIC, POLAR = 0, 1
NONINTERACTING, INTERACTING, ISING, CUTOFF = 0, 1, 2, 3
MWC, XOSHIRO = 0, 1

U = 2.0 ** -24          # unit roundoff of f32 (round to nearest)

# ---------------------------------------------------------------------------------------------------------------- bounds
#
# PROPOSAL ROUNDING, f32 (angles are stored in turns).  trial = fma(step, f, angle - 3 step), f in [2, 4), then the clamp of
# theta to [0, 1/2] or one v_fract on phi.  Every intermediate is below 2 in magnitude (|angle| <= 1, 3 step <= 3/2, the
# sum < 2), so each rounded operation errs by at most half an ulp of a number in [1, 2) = 2^-24 turns:
#   step = (float)(step_rad / 2 pi)           relative 2^-24 of step <= 1/2, times |f - 3| <= 1      <= 2^-25
#   3 step                                     one rounding                                           <= 2^-24
#   angle - 3 step                             one rounding                                           <= 2^-24
#   the fma                                    one rounding                                           <= 2^-24
#   v_fract (phi) / the clamp (theta)          fract of a negative number rounds once; the clamp is exact  <= 2^-25
#   --do-flips: 1/2 - 2 theta, theta + flip    two roundings (2 theta is exact)                       <= 2^-24 together
# The reflection of a cluster member, 1/2 - theta, is one rounding (<= 2^-25).  Sum: < 5 * 2^-24; the judge's own f64
# arithmetic and the conversion turns <-> radians add ~1e-15.  Stated with a factor in hand:
F32_ANGLE_BOUND_TURNS = 8 * U
#
# VERDICT MARGIN  m = C_VERDICT * 2^-24 * mag  on  z = d - log(eps).  The f32 kernels decide
#       (1 + u) sin0 < sin1 * exp2(dU * (-log2(e) / kT)) [* alpha] + sin0
# i.e. log u < -dU/kT + log sin1 - log sin0 [+ log alpha - lag] with every quantity in f32.  Error of the right-hand side against
# the judge's f64 d, in units of u = 2^-24, per unit of mag (mag = 1 + sum |t| over the terms t that d is the signed sum of):
#   (a) roundoff of the term arithmetic.  A term t = coefficient * products of sines and cosines passes through at most
#       ~12 rounded operations (n-hat, dipole, the differences old -> new, the scale by b, E0, F, the sum, the product with
#       -log2(e)/kT whose constant is itself rounded): <= 12 u |t|.  The differences are taken term by term, so the bound is
#       on |old| + |new| -- which is what mag sums -- and not on their difference.                          12
#   (b) v_sin_f32 / v_cos_f32 (arguments in turns).  We know no published absolute bound for them; the derivation takes
#       SINCOS_ABS = 4 u = 2^-22, two units in the last place of 1.0, the top of their range -- twice the "1 ULP" that the ISA
#       manual's transcendental class carries, and no number a kernel returned.  A term A g(theta, phi) with |grad g| <= 2
#       (g a product of at most two sines / cosines) moves by <= 8 u |A|; relative to 1 + |A g| that is <= 8 u max(|A| / kT, 1):
#       with |A| / kT <= 13 in every configuration (MAX_COEFFICIENT_OVER_KT, asserted by tests/test_step_judge_cpu.py),  104
#   (c) the proposal rounding above moves the trial angle by < 5 u turns = 31 u rad.  The strongest terms depend on one
#       angle with |dg / dangle| <= 1 (cos^2 theta, cos theta): <= 31 u |A| / kT,                            400
#   (d) v_exp_f32: 1 ulp = 2 u relative, i.e. 2 u absolute in the logarithm; its argument carries (a);
#       v_rcp_f32 (alpha), v_rsq_f32 (pair terms): 1 ulp each; v_log_f32 is not on the decision path.         6
#       (Measured by tests/test_gpu_math.py, profiles/math/math_probe.txt: v_sin / v_cos 2.1 u absolute over every turn the
#       kernels use, v_exp_f32 1.4 u relative, v_rcp_f32 0.86 ulp, v_rsq_f32 0.83 ulp -- on NORMAL results: v_exp_f32
#       and v_rcp_f32 return 0 for every result below 2^-126.  No decision gets there: exp2 underflows for d < -87, where
#       eps >= 2^-23 has long rejected, and alpha is a ratio of link probabilities nowhere near 2^126.)
#   (d') umbrella sampling: the exponent gains (dw - lag) log2(e), dw = du * wscale, and goes through the same v_exp_f32.  dw is
#       one more term of d: du is the SAME rounded number that enters dU (read in the kernels: `dw = du * wscale`,
#       `dus * wscale`, `(tr.usum - cur.usum) * wscale`), so an error of its sines and cosines moves -du / kT + du wscale by the
#       NET coefficient |1 / kT - wscale| A, which is below A / kT because 0 < wscale kT <= 1 (coefficient_over_kT; the CPU test
#       asserts both): (b) and (c) stand as they are.  Its roundoff -- the product with wscale, the sum with -lag, the
#       product with log2(e) -- is three more rounded operations on |dw|, which mag carries as scale |u_i| of every changed
#       monomer, old and new (and du's own roundoff is already in (a)).                                     3
#   (e) log sin.  The kernels never take it, they compare u sin0 against sin1 e; an absolute SINCOS_ABS on sin(theta) is a
#       relative SINCOS_ABS / sin(theta) = the error of log sin, and (c) moves log sin(theta') by 31 u |cot theta'|.  mag grows
#       only like 1 + |log sin|, so no constant covers the poles: these enter the margin as a term of their own,
#           pole = sum over the changed monomers of SINCOS_ABS (1 / sin theta + 1 / sin theta') + 31 u |cot theta'| (moved one),
#       m = C_VERDICT 2^-24 mag + pole.  Far from a pole it is ~1e-6; it only matters within ~1e-2 rad of one.
# Sum of (a)-(d'): ~525.  The next power of two:
C_VERDICT = 1024.0
SINCOS_ABS = 4 * U
PROPOSAL_RAD = 31 * U          # (c): 5 * 2^-24 turns in radians
MAX_COEFFICIENT_OVER_KT = 13.0
#
# GROWTH TESTS of the clustering main: u <= p, p = (1 + n_a . n_b) / 2.  Each n-hat component is a product of two
# v_sin / v_cos results: error <= 2 * 4 u + u = 9 u; the dot product of two unit vectors <= 2 sqrt(3) * 9 u + 3 u = 34 u,
# halved 17 u, plus one rounding; the moved monomer's trial angle differs from the judge's by <= 50 u rad, which moves its
# n-hat by as much and p by <= 16 u.  Sum < 35 u; with a factor in hand:
GROWTH_MARGIN = 64 * U
#
# CARRIED TOTALS after a launch of f32 steps.  r, p, U are re-derived from the angles when a launch STARTS (f64 sums of n f32
# terms) and then carry one f32 difference per accepted step.  Two kinds of error, bounded separately:
#   absolute, from v_sin / v_cos: a single-monomer term c1 g (g a product of up to three sines / cosines, c1 its
#     coefficient) is off by <= (3 SINCOS_ABS + 2 u) c1 < K_ABS u c1 whatever its size -- once per monomer at the
#     re-derivation, and once more (old and new value) per accepted step: (n + 2 accepted) K_ABS u c1;
#   relative, from rounding: <= 8 u per term at the re-derivation and a handful of rounded operations on numbers up to the
#     total itself per accepted step: (accepted + n) K_TOTALS u sum |terms|, the terms by their value.
K_ABS = 16.0
K_TOTALS = 16.0


def lattice(theta, phi):
    """q16: the lattice indices (k, j) of angles given in radians as pstat_chain_state returns them."""
    k = np.rint(np.asarray(theta) * 65536.0 / math.pi - 0.5).astype(np.int64)
    j = np.rint(np.asarray(phi) * 65536.0 / (2 * math.pi) - 0.5).astype(np.int64)
    return k, j


def lattice_theta(k):
    return math.pi * (k + 0.5) / 65536.0


def lattice_phi(j):
    return 2 * math.pi * (j + 0.5) / 65536.0


def q16_disp(step_rad: float, unit: float, w: int) -> int:
    """The lattice displacement of include/pstat.h's PSTAT_Q16 rule, restated exactly: step (an f32, in lattice cells) times
    s = 2u - 1 (u the top 23 bits of the word: s = (m - 2^22) / 2^22), rounded to the nearest integer, ties to even."""
    step = Fraction(float(np.float32(step_rad / unit)))
    s = Fraction((int(w) >> 9) - (1 << 22), 1 << 22)
    return round(step * s)      # Fraction.__round__: exact, half to even


def _next_word(ob, kind, s):
    return ob.lib().eap_xoshiro128pp_next(s) if kind == XOSHIRO else ob.lib().eap_mwc64x_next(s)


def q16_move(ob, op, pre, cluster):
    """(idx, k1 clamped, j1, inside) of the single move of one PSTAT_Q16 step, in integer arithmetic from the step's words."""
    import ctypes as C
    s = (C.c_uint32 * 4)(*[int(w) for w in pre["rng"]])
    n = op.n
    w_idx = _next_word(ob, op.rng, s)
    w_phi = _next_word(ob, op.rng, s)
    flip = bool(op.do_flips and not cluster and (_next_word(ob, op.rng, s) >> 31))
    w_th = _next_word(ob, op.rng, s)
    idx = (w_idx * n) >> 32
    k, j = lattice(pre["theta"], pre["phi"])
    k0 = int(k[idx])
    if flip:
        k0 = 65535 - k0
    k1 = k0 + q16_disp(pre["theta_step"], math.pi / 65536.0, w_th)
    j1 = (int(j[idx]) + q16_disp(pre["phi_step"], 2 * math.pi / 65536.0, w_phi)) % 65536
    inside = 0 <= k1 < 65536
    return idx, min(max(k1, 0), 65535), j1, inside


def judge(ob, op, pre, precision, cluster):
    """The judge's output for the device state `pre` (a chain_state dict).  Returns (Step, inside): for PSTAT_Q16 the single
    move goes to the lattice point of the integer rule; inside = False when that rule takes theta' off the lattice."""
    moved_to, inside = None, True
    if precision == Q16:
        _, k1, j1, inside = q16_move(ob, op, pre, cluster)
        moved_to = (lattice_phi(j1), lattice_theta(k1))
    J = ob.step_judge(op, pre["phi"], pre["theta"], pre["rng"], pre["phi_step"], pre["theta_step"], cluster=cluster,
                      moved_to=moved_to)
    if precision == F32:
        # theta' clamped to 0 or pi.  In f64 sin(fl(pi)) = 1.2e-16, a density of e^-36.7 that a large enough energy drop can
        # still make acceptable (the reference and the f64 kernels do accept it); in turns the clamp value 1/2 has sin = 0
        # exactly, like the lattice's off-lattice theta': a documented deviation of both (include/pstat.h, run_segment),
        # so a clamped trial is a decided rejection here
        inside = 0.0 < J.theta_trial < math.pi
    return J, inside


@dataclass
class Verdict:
    kind: str                 # "accept" | "reject" | "undecided"
    z: float
    m: float
    ratio: float              # |z| / (2^-24 mag)


def pole_term(J, theta) -> float:
    """(e) of the derivation: what the absolute error of v_sin and the proposal rounding do to log sin, for the monomers the
    trial changes.  theta: the chain's current angles."""
    if not 0.0 < J.theta_trial < math.pi:
        return 0.0          # a clamped trial is decided by rule (see judge), not by its density
    sl = slice(J.lower, J.upper + 1)
    with np.errstate(divide="ignore"):
        t = SINCOS_ABS * (1.0 / np.sin(np.asarray(theta)[sl]) + 1.0 / np.sin(J.trial_theta[sl])).sum()
    t += PROPOSAL_RAD * abs(1.0 / math.tan(J.theta_trial))
    return float(t)


def verdict(J, lag: float = 0.0, inside: bool = True, c: float = C_VERDICT, pole: float = 0.0) -> Verdict:
    """z = d - log eps against m = c 2^-24 mag + pole.  `lag`: the clustering mains' acceptor caches log pi + log alpha of the last
    accepted proposal (inc/acceptance.jl:33-36 -- the oracle and every kernel keep it), so their decision is on d - lag."""
    if not inside:
        return Verdict("reject", -math.inf, 0.0, math.inf)      # theta' off the lattice: rejected whatever the density
    d = J.d - lag
    if math.isnan(d) or d == -math.inf:
        return Verdict("reject", -math.inf, 0.0, math.inf)      # a zero or undefined density is no rounding question
    mag = J.mag + abs(lag)
    z = d - (math.log(J.eps) if J.eps > 0 else -math.inf)
    m = c * U * mag + pole
    if abs(z) <= m:
        return Verdict("undecided", z, m, abs(z) / (U * mag))
    return Verdict("accept" if z > 0 else "reject", z, m, abs(z) / (U * mag))


def growth_undecided(J) -> bool:
    return bool(len(J.grow)) and bool(np.any(np.abs(J.grow[:, 2]) <= GROWTH_MARGIN))


def log_alpha_of_move(pre_theta, post_theta, post_phi, idx: int) -> float:
    """log alpha of an ACCEPTED clustering step whose cluster was reflected, recovered from the states around it: the
    members are the monomers whose theta changed (and idx), the trial chain before the reflection is the state after it with
    the members reflected back, and alpha is the ratio of inc/eap_chain.jl:318-329 over the two boundary links.  Used where
    a growth test lay within its margin, so that the judge's own cluster -- and log alpha -- may not be the device's."""
    pre_theta, th1, ph = np.asarray(pre_theta), np.asarray(post_theta), np.asarray(post_phi)
    n = len(th1)
    ch = np.nonzero(pre_theta != th1)[0]
    lo, hi = min([idx, *ch]), max([idx, *ch])
    th0 = th1.copy()
    th0[lo:hi + 1] = math.pi - th1[lo:hi + 1]

    def nhat(th, i):
        return np.array([math.cos(ph[i]) * math.sin(th[i]), math.sin(ph[i]) * math.sin(th[i]), math.cos(th[i])])

    def link(th, a, b):
        return (1 + float(nhat(th, a) @ nhat(th, b))) / 2

    up = link(th0, hi, hi + 1) if hi < n - 1 else 0.0
    new_up = link(th1, hi, hi + 1) if hi < n - 1 else 0.0
    low = link(th0, lo, lo - 1) if lo > 0 else 0.0
    new_low = link(th1, lo, lo - 1) if lo > 0 else 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.log(np.float64((1 - new_up) * (1 - new_low)) / np.float64((1 - up) * (1 - low))))


def _turn_diff(a, b, circular):
    d = (a - b) / (2 * math.pi)
    if circular:
        d -= np.rint(d)
    return np.abs(d)


@dataclass
class StepResult:
    kind: str                  # "agree" | "undecided" | "wrong"
    why: str = ""
    moved: bool = False
    verdict: Verdict | None = None
    log_alpha: float = 0.0     # of this step's proposal (the next lag if the device moved)


def compare(pre, post, J, inside, precision, lag=0.0, c=C_VERDICT, extra=0.0) -> StepResult:
    """One chain, one step: device state before, judge, device state after.  extra: added to the margin (the lag_error of a
    live re-init lag, see "between the launches")."""
    n = len(pre["theta"])
    V = verdict(J, lag, inside, c, pole_term(J, pre["theta"]) + extra)
    dn = post["nacc_total"] - pre["nacc_total"]
    same = np.array_equal(pre["theta"], post["theta"]) and np.array_equal(pre["phi"], post["phi"])
    res = StepResult("agree", moved=dn == 1, verdict=V, log_alpha=J.log_alpha)

    def wrong(why):
        res.kind, res.why = "wrong", why
        return res

    if growth_undecided(J):
        # a link test within its margin: the device may have grown another cluster and drawn other words.  Left out; the
        # next step starts from the device's own state and words.
        res.kind, res.why = "undecided", "growth test within margin"
        return res
    if not np.array_equal(post["rng"], J.rng):
        return wrong(f"generator words {post['rng']} != judge's {J.rng}")
    if dn not in (0, 1):
        return wrong(f"nacc_total rose by {dn}")
    if dn == 0 and not same:
        return wrong("angles changed but nacc_total did not rise")
    if dn == 1:
        lo, hi = J.lower, J.upper
        out = np.ones(n, dtype=bool)
        out[lo:hi + 1] = False
        if not (np.array_equal(pre["theta"][out], post["theta"][out]) and np.array_equal(pre["phi"][out], post["phi"][out])):
            return wrong(f"an angle outside [{lo}, {hi}] changed")
        if precision == Q16:
            kd, jd = lattice(post["theta"][lo:hi + 1], post["phi"][lo:hi + 1])
            kj, jj = lattice(J.trial_theta[lo:hi + 1], J.trial_phi[lo:hi + 1])
            if not (np.array_equal(kd, kj) and np.array_equal(jd % 65536, jj % 65536)):
                return wrong(f"lattice cells {kd, jd} != rule's {kj, jj} (monomers {lo}..{hi})")
        else:
            eth = _turn_diff(post["theta"][lo:hi + 1], J.trial_theta[lo:hi + 1], False).max()
            eph = _turn_diff(post["phi"][lo:hi + 1], J.trial_phi[lo:hi + 1], True).max()
            if max(eth, eph) > F32_ANGLE_BOUND_TURNS + 1e-13:
                return wrong(f"moved angles off the judge's trial by {eth:.3e} / {eph:.3e} turns (theta / phi), bound "
                             f"{F32_ANGLE_BOUND_TURNS:.3e}; monomer {J.idx}, cluster [{lo}, {hi}]")
    if V.kind == "undecided":
        res.kind, res.why = "undecided", "verdict within margin"
        return res
    if (V.kind == "accept") != (dn == 1):
        return wrong(f"device {'moved' if dn == 1 else 'stayed'}, judge says {V.kind}: monomer {J.idx}, theta' = {J.theta_trial!r}, "
                     f"cluster [{J.lower}, {J.upper}], d = {J.d!r}, lag = {lag!r}, "
                     f"eps = {J.eps!r}, z = {V.z!r}, m = {V.m!r}, mag = {J.mag!r}, U {J.U_cur!r} -> {J.U_trial!r}")
    return res


# ------------------------------------------------------------------------------------------------- the oracle by itself

@dataclass
class Walk:
    accepted: np.ndarray
    phi: np.ndarray
    theta: np.ndarray
    rng: np.ndarray
    phi_step: float
    theta_step: float
    undecided: int = 0
    decided: int = 0
    wrong: int = 0            # against `judge_op`, if one was given
    steps: list = field(default_factory=list)
    recs: list = field(default_factory=list)       # with `rec_params`: the Rec of the chain after every step,
    trials: list = field(default_factory=list)     #   of the step's trial where it was rejected (else None),
    usum0: float = 0.0                             #   and usum of the start
    start: object = None                           #   and the start's Rec
    events: list = field(default_factory=list)     # with `events`: one Event per entry,
    lags: np.ndarray = None                        #   the lag every step was decided with,
    windows: list = field(default_factory=list)    #   (nacc_window, natt_window) after every step,
    post_steps: int = 0                            #   and the tallies of the steps after the first event
    post_undecided: int = 0
    post_wrong: int = 0
    wrong_lag: int = 0                             # with `wrong_lag`: that twin's decided disagreements
    in_contact: int = 0                            # all-pairs rows: post-event steps whose margin carried contact_margin


def walk(ob, op, chain_id, nsteps, cluster, judge_op=None, keep=False, c=C_VERDICT, precision=None, probe=None,
         probe_every=25, rec_params=None, events=None, params=None, wrong_lag=None) -> Walk:
    """The oracle's chain stepped by the judge alone from the seeded start: state -> judge -> accept or not -> state.
    Counts the steps whose verdict lies within the margin.  With `judge_op` (another parameter set, e.g. E0 perturbed) that
    judge's verdicts on the same states are held against the true decisions: `wrong` counts its decided disagreements.
    precision = Q16: the chain lives on the lattice -- the start is the lattice point the device stores (start_twin) and
    every single move goes where the integer rule puts it; an off-lattice theta' is rejected.  precision = F32: the start is
    the f32 start (it differs from the oracle's only under --x0); None: the oracle's own f64 start.
    probe(phi, theta): called on the current configuration every `probe_every` steps and at the end.
    rec_params: the configuration's option dict; the walk then keeps what record_twin needs (Walk.recs, trials, usum0).
    events: what happens BETWEEN the launches (see "between the launches" below) -- a list of (step, kind, *args), applied in
    order once `step` steps are done; it needs `params`, the configuration's option dict.  The walk keeps one Event per entry
    (Walk.events), the lag every step was decided with (Walk.lags) and the step count of every acceptance; `post_*` count
    the steps after the first event.  wrong_lag = "zero" | "no_umbrella": a twin that clears the lag at a re-init, or leaves
    the umbrella weight out of it, judges the same states; `wrong_lag` counts its decided disagreements."""
    q16 = precision == Q16
    if precision is None:
        phi, th, rng = ob.seed_state(op, chain_id)
    else:
        phi, th, rng = start_twin(ob, op, params, chain_id, precision)
    ps, ts = op.phi_step, op.theta_step
    nacc = natt = 0
    lag = lag_w = lag_err = 0.0
    step_in_init = 0
    pending = sorted(events or [], key=lambda ev: ev[0])
    assert not pending or params is not None
    params0, judge_op0 = params, judge_op
    acc = np.zeros(nsteps, dtype=np.uint8)
    W = Walk(acc, phi, th, rng, ps, ts, lags=np.zeros(nsteps))
    last_acc = 0
    if rec_params is not None:
        rec = rec_of(ob, op, rec_params, phi, th, cluster)
        W.usum0 = rec.usum
        W.start = rec
    for t in range(nsteps):
        while pending and pending[0][0] == t:
            _, kind, *args = pending.pop(0)
            if kind in ("reinit_forced", "reinit_metropolis"):
                E = reinit_event(ob, op, params, phi, th, rng, lag, kind == "reinit_forced", precision, acc_last=last_acc)
                E.step = t
                rng = E.J.rng
                if E.J.adopt:
                    phi, th, lag = E.J.fresh_phi, E.J.fresh_theta, E.J.lag_out
                    lag_err = E.lag_error + lag_err      # (a lag still live is inherited through lag_in, and so is its error)
                    lag_w = 0.0 if wrong_lag == "zero" else \
                        (lag - (E.J.usum_cur - E.J.usum_fresh) * umbrella_scale(params) if wrong_lag == "no_umbrella" and params.get("umbrella") else lag)
                step_in_init = 0        # the in-init step counter restarts; the adaptation window stays (mcmc_eap_chain.jl:266-276)
            elif kind == "rung":        # scale_kT + reset_sampler (+ reset_averages): a fresh mcmc() call at kT0 * mult
                params = dict(params0, kT=params0["kT"] * args[0])
                op = oracle_params(ob, params)
                judge_op = None if judge_op0 is None else perturbed(ob, params)
                ps, ts, nacc, natt, lag, lag_w, lag_err, step_in_init = op.phi_step, op.theta_step, 0, 0, 0.0, 0.0, 0.0, 0
                E = Event(kind=kind, step=t)
            elif kind == "x0":          # restart_from_x0(vec, dx0_phi, dx0_theta): EAPChain(pargs) anew, generators reseeded
                base = {k: v for k, v in params.items() if k not in ("use_x0", "x0_phi", "x0_theta", "dx0_phi", "dx0_theta")}
                xop = oracle_params(ob, base, x0_vec=args[0], dx0_phi=args[1], dx0_theta=args[2])
                phi, th, rng = start_twin(ob, xop, None, chain_id, F64 if precision is None else precision)
                ps, ts, nacc, natt, lag, lag_w, lag_err, step_in_init = op.phi_step, op.theta_step, 0, 0, 0.0, 0.0, 0.0, 0
                E = Event(kind=kind, step=t)
            else:
                raise ValueError(kind)
            E.phi, E.theta, E.rng = phi, th, rng
            W.events.append(E)
        pre = dict(phi=phi, theta=th, rng=rng, phi_step=ps, theta_step=ts)
        J, inside = judge(ob, op, pre, Q16, cluster) if q16 else (ob.step_judge(op, phi, th, rng, ps, ts, cluster=cluster), True)
        if precision == F32:
            inside = 0.0 < J.theta_trial < math.pi      # (see judge: a clamped trial is a decided rejection in turns)
        d = J.d - lag
        ok = inside and not math.isnan(d) and ((d >= 0) or (J.eps < math.exp(d)))
        touch = contact_margin(params, phi, th, J.trial_phi, J.trial_theta) if W.events and params["energy_type"] == INTERACTING else 0.0
        W.in_contact += touch > 0
        lag_err0, lag_err = lag_err, lag_err + touch
        V = verdict(J, lag, inside, c, pole_term(J, th) + lag_err)
        W.lags[t] = lag
        after = bool(W.events)
        W.post_steps += after
        if V.kind == "undecided":
            W.undecided += 1
            W.post_undecided += after
        else:
            W.decided += 1
            assert (V.kind == "accept") == ok
        if judge_op is not None:
            Jp = judge(ob, judge_op, pre, Q16, cluster)[0] if q16 else ob.step_judge(judge_op, phi, th, rng, ps, ts, cluster=cluster)
            Vp = verdict(Jp, lag, inside, c, pole_term(Jp, th) + lag_err)
            if Vp.kind != "undecided" and (Vp.kind == "accept") != ok:
                W.wrong += 1
                W.post_wrong += after
        if wrong_lag is not None:
            Vw = verdict(J, lag_w, inside, c, pole_term(J, th) + lag_err)
            if Vw.kind != "undecided" and (Vw.kind == "accept") != ok:
                W.wrong_lag += 1
        if keep:
            W.steps.append(J)
        acc[t] = ok
        last_acc = int(ok)
        lag_err = lag_err0
        if ok:
            phi, th, lag, lag_w, lag_err = J.trial_phi, J.trial_theta, J.log_alpha, J.log_alpha, 0.0
            nacc += 1
        if rec_params is not None:
            tri = rec_of(ob, op, rec_params, J.trial_phi, J.trial_theta, cluster, magnitudes=ok)
            assert abs(tri.usum - J.usum_trial) <= 1e-12 * (1 + tri.lit_us) and abs(rec.usum - J.usum_cur) <= 1e-12 * (1 + rec.lit_us)
            W.trials.append(None if ok else tri)
            rec = tri if ok else rec
            W.recs.append(rec)
        natt += 1
        rng = J.rng
        step_in_init += 1
        ps, ts, nacc, natt = ob.adapt(op, step_in_init, ps, ts, nacc, natt)
        W.windows.append((nacc, natt))
        if probe is not None and ((t + 1) % probe_every == 0 or t + 1 == nsteps):
            probe(phi, th)
    assert not pending, pending
    W.phi, W.theta, W.rng, W.phi_step, W.theta_step = phi, th, rng, ps, ts
    return W


def min_pair_distance(p: dict, phi, theta) -> float:
    """The smallest |x_i - x_j| of a configuration in units of b (x_i = b (sum_{k<=i} n_k - n_i / 2)): the all-pairs
    configurations must keep it above CONTACT_DISTANCE, or the run has reached a 1/r^3 contact."""
    phi, theta = np.asarray(phi), np.asarray(theta)
    nh = np.stack([np.cos(phi) * np.sin(theta), np.sin(phi) * np.sin(theta), np.cos(theta)], axis=1)
    x = np.cumsum(nh, axis=0) - 0.5 * nh
    ii, jj = np.triu_indices(len(phi), 1)
    return float(np.sqrt(((x[ii] - x[jj]) ** 2).sum(axis=1)).min())


# Past a contact the f32 all-pairs kernels' error follows the whole pair sum and the cancellation in x_i - x_j (DESIGN.md
# 5.1), not the terms that change: a configuration whose chains come closer than this is outside what mag can judge.
CONTACT_DISTANCE = 0.2     # (coupling / kT)^(1/3) at the configurations' 7e-3: closer than this one pair outweighs kT


# ------------------------------------------------------------------------------------------------- the configurations

JUDGED = (0, 1, 63, 64, -1)       # a full wave, its neighbour, a partial wave


@dataclass
class Config:
    name: str
    kernel: str                    # substring of launch_info().kernel
    precision: int
    params: dict                   # shared oracle / device options
    chains: int
    T: int
    cluster: bool = False
    env: dict = field(default_factory=dict)
    not_kernel: str = ""           # substring that must NOT be in the kernel name
    cases: list = field(default_factory=list)      # LIFECYCLE only: the option dicts of a packed handle's cases (`chains` each)
    events: list = field(default_factory=list)     # LIFECYCLE only: (step, kind, *args), see walk

    def judged(self):
        if self.cases:
            return [0, 1, 63, 64]      # chains 63 and 64 sit in different workgroups and cases, chain 64 in a partial wave
        return sorted({c % self.chains for c in JUDGED})

    def case_of(self, chain):
        """(option dict, chain id within the case) of a chain of the handle"""
        return (self.cases[chain // self.chains], chain % self.chains) if self.cases else (self.params, chain)


_DIEL = dict(chain_type=DIELECTRIC, E0=6.0, K1=0.5, K2=0.15, Fz=0.8, Fx=0.5, b=1.3)
_POLAR = dict(chain_type=POLAR, E0=20.0, mu=0.4, Fz=0.8, Fx=0.0, b=0.7, do_flips=1)
# Ising: the bond vector b/2 (n_i + n_j) has no lower bound, so the coupling is kept weak -- mu^2 / (4 pi (b/2)^3) < 0.1 kT --
# or chains fall into a 1/r^3 contact, where mag swallows every verdict; the field term carries the decision instead
_DIEL_ISING = dict(_DIEL, E0=12.0, K1=0.06, K2=0.02)
_POLAR_ISING = dict(_POLAR, E0=40.0, mu=0.05, Fx=1.0)   # (Fx tilts the chain off the field axis: a flip then lands far from its neighbour)
_ADAPT = dict(steps_per_adjust=50)                       # default adj_scale
_FIXED = dict(steps_per_adjust=50, adj_scale=1.0)        # no adaptation


def _sweep_configs():
    # (n, energy, chain, generator, kT, adaptive): every n with both energies; chain type, generator, kT and adaptation
    # alternate so that each level meets each n at least once and each other level at least twice
    # T: the issue's 1000, doubled where the judge with E0 off by 2^-8 found fewer than 3 wrong steps in the oracle's own run
    rows = [(1, NONINTERACTING, _DIEL, MWC, 0.7, True, 1000), (1, ISING, _POLAR, XOSHIRO, 2.0, False, 2000),
            (2, NONINTERACTING, _POLAR, XOSHIRO, 0.7, False, 1000), (2, ISING, _DIEL, MWC, 2.0, True, 1000),
            (3, NONINTERACTING, _POLAR, XOSHIRO, 2.0, False, 2000), (3, ISING, _DIEL, MWC, 0.7, True, 1000),
            (33, NONINTERACTING, _POLAR, MWC, 2.0, True, 2000), (33, ISING, _DIEL, XOSHIRO, 0.7, False, 1000),
            (40, NONINTERACTING, _DIEL, MWC, 0.7, False, 1000), (40, ISING, _POLAR, XOSHIRO, 2.0, True, 2000)]
    out = []
    for prec, pname, kern in ((F32, "f32", "sweep_kernel<float>"), (Q16, "q16", "sweep_kernel<float, q16 state>")):
        for n, en, ct, g, kT, ad, T in rows:
            if en == ISING:
                ct = _POLAR_ISING if ct is _POLAR else _DIEL_ISING
            p = dict(n=n, energy_type=en, rng=g, kT=kT, seed=1000 + n, **ct, **(_ADAPT if ad else _FIXED))
            name = f"{pname}-sweep-n{n}-{'ising' if en == ISING else 'ni'}-{'polar' if ct['chain_type'] == POLAR else 'diel'}"
            out.append(Config(name, kern, prec, p, chains=70, T=T))
    return out


def _cluster_configs():
    # (polar Ising chains fall into the 1/r^3 contact of two antiparallel neighbours within a few hundred hits per monomer
    #  unless the coupling is negligible, so at n = 2, 3 the Ising rows are dielectric)
    D, P = DIELECTRIC, POLAR
    # (T: the issue's 600, lengthened like the sweep's)
    rows = [(2, ISING, 0.0, 0.5, True, D, 600), (2, NONINTERACTING, 0.8, 0.0, False, P, 1200),
            (3, NONINTERACTING, 0.0, 1.0, True, P, 2400), (3, ISING, 0.8, 0.0, False, D, 2400),
            (20, ISING, 0.8, 0.5, False, D, 2400), (20, NONINTERACTING, 0.0, 0.0, True, P, 2400),
            (20, ISING, 0.0, 1.0, True, D, 1200)]
    homes = ((F32, "f32lds", "cluster_kernel<float>", {"PSTAT_F32_STATE": "lds"}, "state in memory"),
             (Q16, "q16lds", "cluster_kernel<float, q16 state>", {}, "state in memory"),
             (F32, "f32mem", "cluster_kernel<float, state in memory>", {"PSTAT_F32_STATE": "global"}, ""))
    out = []
    for prec, pname, kern, env, notk in homes:
        for i, (n, en, kappa, cp, ad, chain, T) in enumerate(rows):
            # (polar: a field weak enough that reflecting a cluster, which costs 2 E0 mu sum cos(theta) / 2, is not hopeless)
            ct = (_DIEL_ISING if en == ISING else _DIEL) if chain == DIELECTRIC else \
                dict(_POLAR_ISING if en == ISING else dict(_POLAR, E0=5.0), do_flips=0)
            p = dict(n=n, energy_type=en, rng=MWC if i % 2 else XOSHIRO, kT=1.0 if i % 2 else 0.7, seed=2000 + 10 * n + i,
                     bend_mod=kappa, bend_angle=0.3 if kappa else 0.0, cluster_prob=cp, **ct, **(_ADAPT if ad else _FIXED))
            name = f"{pname}-cluster-n{n}-{'ising' if en == ISING else 'ni'}-{'polar' if chain == POLAR else 'diel'}-cp{cp}-{'bend' if kappa else 'nobend'}"
            out.append(Config(name, kern, prec, p, chains=70, T=T, cluster=True, env=env, not_kernel=notk))
    return out


# The all-pairs energies have no excluded volume: from a random start chains cross themselves, fall into 1/r^3 contacts within
# a few hundred steps (the oracle's own chains: sum |pair terms| of 2e2 ... 1e5 kT after 800-1600 steps at mu^2 / (4 pi b^3)
# = 8e-4 kT), and past a contact the f32 error follows the whole pair sum, which mag does not see.  So these configurations
# START EXTENDED (--x0: every monomer near theta = 1.2, phi = 0, a rod in the x-z plane, + Uniform(0, dx0)), are weakly
# coupled (mu^2 / (4 pi b^3) <= 7e-3 kT) and pulled along the rod by Fx, and run too briefly to crumple: the CPU test and the
# GPU test both assert that no two monomers of a judged chain come within CONTACT_DISTANCE b.  A flip theta -> pi - theta of a
# monomer near theta = pi / 2 lands beside itself, not on its neighbour.
_X0 = dict(use_x0=1, x0_phi=-0.25, x0_theta=1.37, dx0_phi=0.5, dx0_theta=0.4)


def _allpairs_configs():
    out = []
    for i, (n, T) in enumerate(((23, 400), (64, 800), (100, 800), (130, 800))):
        ct = dict(chain_type=DIELECTRIC, E0=30.0, K1=0.0125, K2=0.0025, Fz=0.3, Fx=8.0, b=1.0) if i % 2 == 0 else \
            dict(chain_type=POLAR, E0=100.0, mu=0.1, Fz=0.3, Fx=8.0, b=1.0, do_flips=1)
        p = dict(n=n, energy_type=INTERACTING, rng=MWC if i % 2 else XOSHIRO, kT=1.0, seed=3000 + n, **ct, **_X0,
                 **(_ADAPT if i % 2 else _FIXED))
        out.append(Config(f"f32-allpairs-n{n}", "interacting_kernel<float>", F32, p, chains=6, T=T))
    # UCutoff is the pair sum alone (no field, no force: nothing holds the rod), so its run keeps the rod by small fixed steps,
    # and its dipoles are mostly the K2 E0 z part, side by side along the rod: U is a few kT per monomer and every move counts
    for n, en, phys in ((20, INTERACTING, dict(E0=20.0, K1=0.02, K2=0.005, Fz=0.3, Fx=8.0, **_ADAPT)),
                        (64, CUTOFF, dict(E0=10.0, K1=0.4, K2=0.3, Fz=0.3, Fx=8.0, phi_step=0.15, theta_step=0.15, **_FIXED))):
        p = dict(n=n, energy_type=en, rng=MWC, kT=1.0, seed=3500 + n, chain_type=DIELECTRIC, b=1.0, cluster_prob=0.5,
                 cutoff_radius=3.0, **_X0, **phys)
        out.append(Config(f"f32-allpairs-cluster-n{n}-{'cutoff' if en == CUTOFF else 'interacting'}", "cluster_wave_kernel<float>",
                          F32, p, chains=6, T=600, cluster=True))
    # The packed ring sums (ring_pair_sum_pk<4>, <8>, and its cutoff select) and every M >= 2 form of the clustering kernel: the
    # same recipe at the lengths the reference's phase sweeps use (n = 100, 200, 400) and at partial rings (n = 130: M = 4,
    # L = 34; n = 257: M = 8, L = 34).  A judged step costs the oracle two O(n^2) sums, so the long chains judge fewer
    # chains (`chains`), never fewer steps: T is set by the rule above (test_step_judge_cpu.py: a judge with E0 (1 + 2^-8)
    # is caught at this length).
    for i, (n, T, chains) in enumerate(((200, 800, 3), (257, 800, 2))):
        ct = dict(chain_type=DIELECTRIC, E0=30.0, K1=0.0125, K2=0.0025, Fz=0.3, Fx=8.0, b=1.0) if i % 2 == 0 else \
            dict(chain_type=POLAR, E0=100.0, mu=0.1, Fz=0.3, Fx=8.0, b=1.0, do_flips=1)
        p = dict(n=n, energy_type=INTERACTING, rng=MWC if i % 2 else XOSHIRO, kT=1.0, seed=3000 + n, **ct, **_X0,
                 **(_ADAPT if i % 2 else _FIXED))
        out.append(Config(f"f32-allpairs-n{n}", "interacting_kernel<float>", F32, p, chains=chains, T=T))
    inter = dict(E0=20.0, K1=0.02, K2=0.005, Fz=0.3, Fx=8.0, **_ADAPT)
    cut = dict(E0=10.0, K1=0.4, K2=0.3, Fz=0.3, Fx=8.0, phi_step=0.15, theta_step=0.15, **_FIXED)
    # (the perturbed judge is caught about once in 3000 ... 7000 judged steps of these rows, hence their T; at n = 130 the
    #  seeds 3630 ... 3633 do not meet it within 1200 steps of three chains, 3634 does)
    for n, en, phys, T, chains, seed in ((100, INTERACTING, inter, 1200, 4, 3600), (200, CUTOFF, cut, 1200, 3, 3700),
                                         (400, CUTOFF, cut, 2400, 1, 3900), (130, INTERACTING, inter, 1200, 4, 3634)):
        p = dict(n=n, energy_type=en, rng=MWC, kT=1.0, seed=seed, chain_type=DIELECTRIC, b=1.0, cluster_prob=0.5,
                 cutoff_radius=3.0, **_X0, **phys)
        out.append(Config(f"f32-allpairs-cluster-n{n}-{'cutoff' if en == CUTOFF else 'interacting'}", "cluster_wave_kernel<float>",
                          F32, p, chains=chains, T=T, cluster=True))
    return out


# A gauge rise needs a chain whose later configurations outweigh its first by more than e^30: a cold polar chain started
# AGAINST the field (--x0 with theta near pi), which the field and the force then turn round.  Its log-weight gauged on the
# start, wscale E0 mu / 2 (sum cos theta - sum cos theta_0), cannot exceed wscale E0 mu n: the rows choose E0 mu n so that
# this stays below RISE_MAX = 80 -- inside f32's range, so that the records before the rise still count -- and the
# oracle's own walk of every judged chain reaches RISE_MIN = 35 within T (tests/test_step_judge_cpu.py asserts both): above
# the f32 threshold of 30 by far more than any f32 error of w.
RISE_MIN, RISE_MAX = 35.0, 80.0
_AGAINST = dict(use_x0=1, x0_phi=0.0, x0_theta=2.84, dx0_phi=6.28, dx0_theta=0.2)      # theta in [2.84, 3.04]
_COLD = dict(chain_type=POLAR, E0=24.0, mu=0.4, kT=0.5, Fz=0.7, Fx=0.0, b=0.7)           # wscale kT = 0.2 + 0.8 e^-0.98 = 0.5


# The weight function takes wscale kT = 0.2 ... 1 of the field's pull away (that is its purpose), and an Ising chain that the
# field no longer aligns visits the contact of two antiparallel neighbours far more often: on the oracle's walk of the n = 3 row
# with the force of _DIEL_ISING, sum |pair terms| reaches 1e3 kT, and check (b) misses its bound there (measured: error / bound
# 1.24 on U).  The umbrella Ising rows with bonds are therefore held along the field by a stronger force, Fz b / kT = 5.6 at
# kT = 0.7: sum |pair terms| stays below 25 kT at n = 2, 3.
_HELD_ISING = dict(_DIEL_ISING, Fz=3.0)


def _umbrella_configs():
    out = []
    U1 = dict(umbrella=1)
    # sweep_kernel<float>, <float, q16 state>: n = 1, 3, 20; NI and weak-coupling Ising, both chain types; both generators;
    # adaptive and fixed (T by the rule of _sweep_configs)
    # (A polar Ising chain with bonds -- n = 3, n = 20, either kT, any of the seeds tried, Fx up to 6 -- falls into the 1/r^3
    #  contact of two antiparallel neighbours, |n_i + n_j| / 2 ~ 0.002, U ~ -1e3 ... -1e5 kT, where check (b)'s bound does not
    #  hold (measured: error / bound 1.01 at U = -1799; cf. _cluster_configs).  So the polar Ising row is the one at n = 1, the
    #  Ising rows with bonds are dielectric (_HELD_ISING), and the polar chain with neighbours is the NI row at n = 3.)
    rows = [(1, NONINTERACTING, _DIEL, MWC, 0.7, True, 1000, 4001), (1, ISING, _POLAR_ISING, XOSHIRO, 2.0, False, 2000, 4001),
            (3, NONINTERACTING, _POLAR, XOSHIRO, 2.0, False, 2000, 4003), (3, ISING, _HELD_ISING, MWC, 0.7, True, 2000, 4003),
            (20, NONINTERACTING, _DIEL, MWC, 0.7, False, 1000, 4020), (20, ISING, _HELD_ISING, XOSHIRO, 0.7, True, 2000, 4020)]
    for prec, pname, kern in ((F32, "f32", "sweep_kernel<float>"), (Q16, "q16", "sweep_kernel<float, q16 state>")):
        for n, en, ct, g, kT, ad, T, seed in rows:
            p = dict(n=n, energy_type=en, rng=g, kT=kT, seed=seed, **ct, **(_ADAPT if ad else _FIXED), **U1)
            name = f"{pname}-umb-sweep-n{n}-{'ising' if en == ISING else 'ni'}-{'polar' if ct['chain_type'] == POLAR else 'diel'}"
            out.append(Config(name, kern, prec, p, chains=70, T=T))
    # cluster_kernel<float>, <float, q16 state>, <float, state in memory>: n = 2 and 20, with and without bending,
    # cluster_prob 0.5, both chain types (the polar rows at E0 = 10, twice the field of _cluster_configs: the weight halves its net
    # coefficient, and at E0 = 5 the q16 row at n = 20 did not meet the perturbed judge in 4800 steps of five chains)
    D, P = DIELECTRIC, POLAR
    # (the bending rows are the polar ones: where umbrella sampling lets a dielectric Ising chain at n = 20 put neighbours
    #  antiparallel, psi -> pi, acos' slope 1 / sin psi carries the dot product's f32 error into the bending energy, which
    #  check (b)'s bound does not count -- measured: error / bound 7.3 on U, every other column below 0.002)
    rows = [(2, ISING, 0.0, True, D, 1200), (2, NONINTERACTING, 0.8, False, P, 1200),
            (20, ISING, 0.0, False, D, 2400), (20, NONINTERACTING, 0.8, True, P, 2400)]
    homes = ((F32, "f32lds", "cluster_kernel<float>", {"PSTAT_F32_STATE": "lds"}, "state in memory"),
             (Q16, "q16lds", "cluster_kernel<float, q16 state>", {}, "state in memory"),
             (F32, "f32mem", "cluster_kernel<float, state in memory>", {"PSTAT_F32_STATE": "global"}, ""))
    for prec, pname, kern, env, notk in homes:
        for i, (n, en, kappa, ad, chain, T) in enumerate(rows):
            # (not _HELD_ISING: a cluster reflected out of a chain that the force holds along z leaves antiparallel neighbours at
            #  both its ends, the contact itself)
            ct = _DIEL_ISING if chain == D else dict(_POLAR, E0=10.0, do_flips=0)
            # (seed 4402 starts chain 0 of the n = 20 Ising row inside a repulsive contact, U = 7.2e6: the first launch of check (b)
            #  then carries the half ulp of that number for its 64 steps)
            p = dict(n=n, energy_type=en, rng=MWC if i % 2 else XOSHIRO, kT=1.0 if i % 2 else 0.7,
                     seed=4200 + 10 * n + i + (1000 if (n, en) == (20, ISING) else 0),
                     bend_mod=kappa, bend_angle=0.3 if kappa else 0.0, cluster_prob=0.5, **ct, **(_ADAPT if ad else _FIXED), **U1)
            name = f"{pname}-umb-cluster-n{n}-{'ising' if en == ISING else 'ni'}-{'polar' if chain == P else 'diel'}-{'bend' if kappa else 'nobend'}"
            out.append(Config(name, kern, prec, p, chains=70, T=T, cluster=True, env=env, not_kernel=notk))
    # interacting_kernel<float>: n = 23 (M = 1) and 130 (M = 4, partial ring); the extended start of _allpairs_configs
    for i, (n, T, chains) in enumerate(((23, 400, 6), (130, 800, 3))):
        ct = dict(chain_type=DIELECTRIC, E0=30.0, K1=0.0125, K2=0.0025, Fz=0.3, Fx=8.0, b=1.0) if i % 2 == 0 else \
            dict(chain_type=POLAR, E0=100.0, mu=0.1, Fz=0.3, Fx=8.0, b=1.0, do_flips=1)
        p = dict(n=n, energy_type=INTERACTING, rng=MWC if i % 2 else XOSHIRO, kT=1.0, seed=4300 + n, **ct, **_X0,
                 **(_ADAPT if i % 2 else _FIXED), **U1)
        out.append(Config(f"f32-umb-allpairs-n{n}", "interacting_kernel<float>", F32, p, chains=chains, T=T))
    # cluster_wave_kernel<float>: n = 20 interacting, n = 64 cutoff, n = 130 interacting
    inter = dict(E0=20.0, K1=0.02, K2=0.005, Fz=0.3, Fx=8.0, **_ADAPT)
    cut = dict(E0=10.0, K1=0.4, K2=0.3, Fz=0.3, Fx=8.0, phi_step=0.15, theta_step=0.15, **_FIXED)
    # (UCutoff has no field term, but the weight has: wscale |u_i| of the moved monomer enters mag, old and new, while the pair
    #  terms decide.  With the recipe's E0 = 10 that is 7 and leaves 0.67 % of the steps undecided; the same dipoles
    #  E0 (K1 - K2, K2) = (1, 3) from half the field make u_i half as large: 0.3 %.  The perturbed judge is caught about once
    #  in 5000 steps of this row whatever its E0 -- the pair terms catch it -- hence T = 1200 and the seed: 4564 ... 4567, 4569 and
    #  4571 do not meet it, 4572 does twice.  n = 130: 4630 and 4631 do not, 4632 does.)
    cut = dict(cut, E0=5.0, K1=0.8, K2=0.6)
    for n, en, phys, T, chains, seed in ((20, INTERACTING, inter, 600, 6, 4520), (64, CUTOFF, cut, 1200, 6, 4572),
                                         (130, INTERACTING, inter, 1200, 4, 4632)):
        p = dict(n=n, energy_type=en, rng=MWC, kT=1.0, seed=seed, chain_type=DIELECTRIC, b=1.0, cluster_prob=0.5,
                 cutoff_radius=3.0, **_X0, **phys, **U1)
        out.append(Config(f"f32-umb-allpairs-cluster-n{n}-{'cutoff' if en == CUTOFF else 'interacting'}",
                          "cluster_wave_kernel<float>", F32, p, chains=chains, T=T, cluster=True))
    # one gauge-rise row per kernel family
    ni = dict(n=8, energy_type=NONINTERACTING, rng=MWC, **_COLD, **_AGAINST, **_ADAPT, **U1)
    out.append(Config("f32-rise-sweep-n8", "sweep_kernel<float>", F32, dict(ni, seed=4700, do_flips=1), chains=70, T=2000))
    out.append(Config("q16-rise-sweep-n8", "sweep_kernel<float, q16 state>", Q16, dict(ni, seed=4701, do_flips=1), chains=70, T=1000))
    # The clustering main reflects the whole aligned chain at its first cluster attempt (measured on the oracle's walk: the
    # rise then happens at step 1, before anything is recorded), so its rows start just below the equator, theta in
    # [1.75, 1.95]: the reflection gains less than e^30 and the rise comes later, from the single moves, with records behind it.
    below = dict(x0_theta=1.75)
    cl = dict(ni, cluster_prob=0.5, **{k: v for k, v in _AGAINST.items() if k != "x0_theta"})
    cl = dict({k: v for k, v in cl.items() if k != "x0_theta"}, **below)
    out.append(Config("f32lds-rise-cluster-n8", "cluster_kernel<float>", F32, dict(cl, seed=4706), chains=70, T=1200, cluster=True,
                      env={"PSTAT_F32_STATE": "lds"}, not_kernel="state in memory"))
    out.append(Config("f32mem-rise-cluster-n8", "cluster_kernel<float, state in memory>", F32, dict(cl, seed=4703), chains=70,
                      T=1200, cluster=True, env={"PSTAT_F32_STATE": "global"}))
    # all-pairs: the rod of _X0 pointing down the field (theta in [2.1, 2.4], without --do-flips, which lands a monomer on its
    # neighbour here; [1.6, 1.9] under cluster flips), held along x by
    # Fx as in _allpairs_configs, so that turning round does not fold it onto itself (CONTACT_DISTANCE is asserted as there)
    rod = dict(energy_type=INTERACTING, rng=MWC, kT=1.0, chain_type=POLAR, mu=0.1, Fz=0.3, Fx=8.0, b=1.0, use_x0=1, x0_phi=-0.25,
               dx0_phi=0.5, dx0_theta=0.3, **_ADAPT, **U1)
    out.append(Config("f32-rise-allpairs-n23", "interacting_kernel<float>", F32,
                      dict(rod, n=23, E0=160.0, x0_theta=2.1, seed=4704), chains=6, T=800))
    out.append(Config("f32-rise-allpairs-cluster-n20", "cluster_wave_kernel<float>", F32,
                      dict(rod, n=20, E0=240.0, x0_theta=1.6, cluster_prob=0.5, cutoff_radius=3.0, seed=4705), chains=6, T=1200,
                      cluster=True))
    return out


RISE_IDS = []          # filled below: the names of the gauge-rise rows
CONFIGS = _sweep_configs() + _cluster_configs() + _allpairs_configs() + _umbrella_configs()
CONFIG_IDS = [c.name for c in CONFIGS]
RISE_IDS = [c.name for c in CONFIGS if "-rise-" in c.name]

# the packed sweep: 13 cases x 5 chains of different E0, Fz, kT, n = 12
PACKED_CASES = [dict(E0=3.0 + 0.25 * i, Fz=0.2 * (i % 5), kT=0.5 + 0.12 * i) for i in range(13)]
PACKED_COMMON = dict(n=12, chain_type=DIELECTRIC, K1=1.0, K2=0.3, Fx=0.4, b=1.3, energy_type=NONINTERACTING, rng=MWC,
                     steps_per_adjust=50)
PACKED_T = 600


def device_params(ps, p, chains, precision, cluster, **kw):
    """The device's parameter struct for a configuration's option dict (ps: the polymer_stats_amd package)."""
    return ps.default_params(num_chains=chains, precision=precision,
                             move_set=ps.MOVES_CLUSTER if cluster else ps.MOVES_SINGLE, **p, **kw)


def check_adaptation(oracle, op, pre, post, t1, adaptive):
    """The adaptation rule at a window end (mcmc_eap_chain.jl:301-322), from nacc_window / natt_window; between window ends
    the step sizes stay and the window counts the step.  t1: the in-init step counter after the step (1-based)."""
    dn = post["nacc_total"] - pre["nacc_total"]
    nacc, natt = pre["nacc_window"] + dn, pre["natt_window"] + 1
    ps_, ts_ = pre["phi_step"], pre["theta_step"]
    if adaptive and t1 % op.steps_per_adjust == 0:
        ps_, ts_, nacc, natt = oracle.adapt(op, t1, ps_, ts_, nacc, natt)
    got = (post["phi_step"], post["theta_step"], post["nacc_window"], post["natt_window"])
    assert got == (ps_, ts_, nacc, natt), (t1, got, (ps_, ts_, nacc, natt))


def oracle_params(ob, cfg_params, **kw):
    return ob.make_params(num_steps=0, stepout=0, uniform_bits=23, **cfg_params, **kw)


def perturbed(ob, cfg_params):
    """The same options with E0 multiplied by 1 + 2^-8: the judge that the suite must be able to tell from the true one."""
    p = dict(cfg_params)
    p["E0"] = p["E0"] * (1 + 2.0 ** -8)
    return oracle_params(ob, p)


# ------------------------------------------------------------------------------------------------- totals, term by term

def term_sums(p: dict, phi, theta, conditioning: bool = False):
    """For the bound on the carried totals, f64 numpy: (lit, c1) -- lit: the sum of |terms| of r (3), p (3) and U by their
    value; c1: the single-monomer coefficient of each of the seven (the term with every sine and cosine replaced by 1).
    p: the configuration's options.  (Only magnitudes are taken from here; the reference values of r, p, U themselves come
    from the oracle's eap_chain_energy.)
    conditioning = True: also (cond_sum, cond_max), the sum and the largest of T0 (m + 1) / rho over the pair terms -- T0 =
    |mu_i| |mu_j| / (4 pi r^3), m = j - i, rho = r / b: what PAIR CONDITIONING of the record bound multiplies."""
    phi, theta = np.asarray(phi), np.asarray(theta)
    n = len(phi)
    nh = np.stack([np.cos(phi) * np.sin(theta), np.sin(phi) * np.sin(theta), np.cos(theta)], axis=1)
    E0, b = p["E0"], p.get("b", 1.0)
    if p["chain_type"] == DIELECTRIC:
        a = (p.get("K1", 1.0) - p.get("K2", 0.0)) * E0 * nh[:, 2]
        mu = a[:, None] * nh
        mu[:, 2] += p.get("K2", 0.0) * E0
        mu_c = abs((p.get("K1", 1.0) - p.get("K2", 0.0)) * E0) + abs(p.get("K2", 0.0) * E0)
    else:
        mu = p.get("mu", 1e-2) * nh
        mu_c = abs(p.get("mu", 1e-2))
    r_abs = np.abs(b * nh).sum(axis=0)
    p_abs = np.abs(mu).sum(axis=0)
    en = p["energy_type"]
    u = u_c = cond_sum = cond_max = 0.0
    if en != CUTOFF:
        u += np.abs(0.5 * E0 * mu[:, 2]).sum() + abs(p.get("Fx", 0.0)) * r_abs[0] + abs(p.get("Fz", 0.0)) * r_abs[2]
        u_c = 0.5 * abs(E0) * mu_c + (abs(p.get("Fx", 0.0)) + abs(p.get("Fz", 0.0))) * abs(b)
        if p.get("bend_mod", 0.0) and n > 1:
            psi = np.arccos(np.clip((nh[:-1] * nh[1:]).sum(axis=1), -1, 1))
            u += np.abs(p["bend_mod"] / 2 * (psi - p.get("bend_angle", 0.0)) ** 2).sum()
    if en != NONINTERACTING and n > 1:
        x = b * (np.cumsum(nh, axis=0) - 0.5 * nh)
        if en == ISING:
            ii, jj = np.arange(n - 1), np.arange(1, n)
        else:
            ii, jj = np.triu_indices(n, 1)
        rv = x[ii] - x[jj]
        r2 = (rv * rv).sum(axis=1)
        rm = np.sqrt(r2)
        h = rv / rm[:, None]
        t = ((mu[ii] * mu[jj]).sum(axis=1) - 3 * (mu[ii] * h).sum(axis=1) * (mu[jj] * h).sum(axis=1)) / (4 * math.pi * r2 * rm)
        with np.errstate(divide="ignore", invalid="ignore"):
            cond = np.sqrt((mu[ii] ** 2).sum(axis=1) * (mu[jj] ** 2).sum(axis=1)) / (4 * math.pi * r2 * rm) * (jj - ii + 1) * abs(b) / rm
        if en == CUTOFF:
            inside = r2 <= (p.get("cutoff_radius", 7.5) * b) ** 2
            t, cond = t[inside], cond[inside]
        u += np.abs(t).sum()
        if len(cond):
            cond_sum, cond_max = float(cond.sum()), float(cond.max())
    lit = np.concatenate([r_abs, p_abs, [u]])
    c1 = np.array([abs(b)] * 3 + [mu_c] * 3 + [u_c])
    return (lit, c1, cond_sum, cond_max) if conditioning else (lit, c1)


def umbrella_scale(p: dict) -> float:
    """The scale of AntiDipoleWeightFunction (inc/average.jl:104-124): w = sum(u) scale - gauge.  Restated, not imported."""
    F2 = p.get("Fx", 0.0) ** 2 + p.get("Fz", 0.0) ** 2
    return (0.2 + 0.8 * math.exp(-F2 / p["kT"])) / p["kT"]


def coefficient_over_kT(p: dict) -> float:
    """The largest single-monomer coefficient A / kT of a configuration: field, force.  Under umbrella sampling the field
    term enters d as -du / kT + du wscale with one and the same du (see (d') above): its coefficient is the net one,
    |1 / kT - wscale| A; UCutoff has no field term in U, so there the weight's wscale A stands alone."""
    E0 = abs(p["E0"])
    if p["chain_type"] == DIELECTRIC:
        field = 0.5 * E0 * E0 * (abs(p.get("K1", 1.0) - p.get("K2", 0.0)) + abs(p.get("K2", 0.0)))
    else:
        field = 0.5 * E0 * abs(p.get("mu", 1e-2))
    ws = umbrella_scale(p) if p.get("umbrella") else 0.0
    if p["energy_type"] == CUTOFF:
        return ws * field       # UCutoff is the pair sum alone
    force = max(abs(p.get("Fx", 0.0)), abs(p.get("Fz", 0.0))) * abs(p.get("b", 1.0))
    return max(field * abs(1.0 / p["kT"] - ws), force / p["kT"])


# ------------------------------------------------------------------------------------------------- the record, check (d)
#
# Every step, accepted or not, adds the current r, p, U and their squares (the clustering main also sum cos^2 theta and the
# mean bond angle) to f32 block accumulators; the accumulators are folded into the f64 `sums` when a block of at most
# FLUSH = 128 steps, an adaptation window or the launch ends.  Under umbrella sampling every record carries the weight
# e^wrel, wrel = -(usum - uref) wscale, and the normaliser the sum of the weights; a configuration more than e^30 heavier than
# the gauged one raises the gauge: the accumulators are multiplied by (float) e^-wrel, the f64 sums by the double.
#
# THE TWIN (record_twin) restates record! in numpy f64 on the states of one chain.  Plain: the 16 running sums in ABI order
# (+ 2).  Umbrella: the gauge-free ratios  sum v e^L / sum e^L,  L = -s usum,  and N* = sum e^(L - max L), every prefix with ITS
# maximum factored out, so nothing overflows; s is umbrella_scale (the oracle's weight_make(...).scale, restated).
#
# THE BOUND (record_bound), per prefix and column, in units of u = 2^-24; nothing in it is taken from a kernel's output.
#   Per record, the error of wgt * v:
#     the carried value: the CARRIED TOTALS bound above, e_v = (a + n) K_TOTALS u sum |terms| + (n + 2 a) K_ABS u c1, a = the
#       steps accepted since the launch began (the all-pairs kernels re-derive more often: a bound all the same);
#       a square v^2 errs by 2 |v| e_v + e_v^2, r.r and p.p by the sum of their three squares;
#     PAIR CONDITIONING (found by check (d) on a polar Ising chain inside a 1/r^3 contact, |n_i + n_j| / 2 = 0.002, where U^2
#       was off by 250 u relative against the 128 u of the line above; DESIGN.md 5.1 is the same thing seen in distribution):
#       "by their value" counts a pair term's roundings but not the cancellation inside its separation.  The kernels
#       form x_i - x_j from f32 n-hats -- `hb * (pnx + nix)` in refresh_totals and the step of pstat_kernels.hip, `bond()` of
#       pstat_cluster.hip, the prefix sums behind ring_pair_sum of the all-pairs kernels -- m + 1 = j - i + 1 unit vectors whose
#       components carry 9 u each (GROWTH TESTS), sqrt(3) 9 u < 16 u per vector: |d r| <= 16 (m + 1) u b.  A term
#       (mu_i . mu_j - 3 (mu_i . h)(mu_j . h)) / (4 pi r^3) moves by at most 3 + 2 * 3 = 9 times T0 |d r| / r, T0 = |mu_i| |mu_j| /
#       (4 pi r^3) (the r^-3, and the two projections on h = r / |r|).  So U gains
#           K_COND u (sum over the pair terms of T0 (m + 1) / rho  +  4 a max T0 (m + 1) / rho),  rho = r / b,  K_COND = 9 * 16:
#       the sum for the re-derivation (or the fresh pair sum of the all-pairs kernels), the maximum -- the largest any term
#       has had so far -- for the at most two bonds, old and new, that a chain-per-lane kernel recomputes per accepted step.
#       Away from contacts (rho >= CONTACT_DISTANCE, which the all-pairs rows assert) it is of the order of the line above.
#     the extras: sum cos^2 theta like a total with unit coefficient; a bond angle psi = acos(n_i . n_j) errs by
#       e_psi = min(sqrt(2 D), D / sin psi) + ACOS_ABS, D = 2 GROWTH_MARGIN the error of the dot product (see GROWTH TESTS;
#       acos' slope is 1 / sin psi, and no worse than sqrt(2 D) at its ends), ACOS_ABS = 16 u: acos_r's stated truncation
#       2e-8 (pstat_math.h) plus eight roundings of a number below 4; the sum of n - 1 angles is re-derived when a launch
#       starts and then carries the differences of at most 4 bonds, old and new, per accepted step: sum e_psi + 8 a max e_psi;
#       the same e_psi reaches U through the bending energy kappa / 2 (psi - psi0)^2: kappa |psi - psi0| e_psi per bond, summed for
#       the re-derivation, and 4 a times the largest such sum so far for the carried differences (a bound on any 4 bonds);
#     the weight: its relative error is the absolute error of wrel,
#       e_w = wscale e_usum + 4 u |wrel| + 2 u:  e_usum the f32 sum(u), re-derived at launch start, then one f32 difference per
#       accepted step: e_usum = (2 + a) K_TOTALS u sum |terms| + (n + 2 a) K_ABS u c1 on the terms of sum(u).  The CARRIED
#       TOTALS form with its re-derivation counted as it is made (read in the kernels): <= 8 u on each f32 term, then an f64
#       sum (refresh_totals of the chain-per-lane kernels) or an f32 wave sum of at most 8 partial sums per lane and 6
#       butterfly levels (the all-pairs kernels), then the cast: <= 23 u sum |terms| < 2 K_TOTALS u sum |terms|, not n times
#       that.  (The totals r, p, U keep the (a + n) of check (b): U's pair part is an f32 sum of n^2 / 2 terms.)
#       The difference usum - uref, the product with wscale and the product with log2(e) inside __expf: one rounding each
#       on |wrel|, with one in hand; v_exp_f32 1 ulp = 2 u.
#       |wrel| <= the range of L over the prefix, since the gauge is the L of a configuration of the prefix (or the start);
#     the product wgt * v [* v]: 2 u.
#   Per block: up to `block` f32 additions on numbers no larger than the block's sum |wgt v|: block u sum |wgt v|
#     (block = 128 in a long launch, 64 in launches of 64, 1 in the stepped handle).
#   At the flush: f32 -> f64 is exact; the f64 addition 2^-52 per block; sweep_kernel<float> carries r in units of b and
#     rescales its accumulators by (float) b and (float) b * (float) b: 2 u and 4 u.  Stated for every kernel: RESCALE = 4 u.
#   A gauge rise multiplies what was recorded by e^-wrel: the (float) factor 1 u, the error 4 u |wrel| of its exponent, with
#     one in hand; each rise lifts the gauge by more than 29, so a prefix has seen at most G = floor(range / 29) of them:
#     G (4 u range + 2 u) on everything recorded before.
#   v_exp_f32 returns 0 below 2^-126 (of the gauged weight), and an accumulator times (float) e^-wrel may fall there too:
#     2^-126 e^(gauge - max L) per record, absolute.
#   A ratio num / den with |d num| <= E_num, |d den| <= E_den:  |d (num / den)| <= (E_num + |num / den| E_den) / (den - E_den).
FLUSH = 128
K_COND = 144.0
ACOS_ABS = 16 * U
PSI_DOT = 2 * GROWTH_MARGIN
RESCALE = 4 * U
GAUGE_T = 30.0                # umbrella_logw's threshold for `float` (pstat_math.h)
GAUGE_LIFT = 29.0             # every rise lifts the gauge by more than this
# THE GAUGE CONTRACT: ln(device normaliser / N*) = (heaviest log-weight) - (gauge) <= GAUGE_T + margin.  The margin is derived,
# per step: the error e_w of the wrel that the threshold test itself sees (a configuration may weigh e^(30 + e_w) without a
# rise) plus the relative error of the normaliser, E_den / (den - E_den) of the bound above (ln(1 + x) <= x); record_bound returns
# it.  It must stay far below 1 for the contract to say anything: the CPU test asserts GAUGE_MARGIN_MAX on every gauge-rise
# row, the GPU test on every umbrella row.
GAUGE_MARGIN_MAX = 0.125
COLUMNS = ["r1", "r2", "r3", "r1sq", "r2sq", "r3sq", "rsq", "p1", "p2", "p3", "p1sq", "p2sq", "p3sq", "psq", "U", "Usq",
           "cos2", "psi"]


@dataclass
class Rec:
    """One recorded configuration of one chain: what record! adds, and the magnitudes the bound needs."""
    v: np.ndarray              # r (3), p (3), U: oracle.chain_energy
    ex: np.ndarray             # sum cos^2 theta, sum psi / (n - 1) (zeros for n = 1)
    usum: float                # sum(us): the field terms, and in the clustering main the bending energies
    lit: np.ndarray            # term_sums: sum |terms| of the seven
    c1: np.ndarray             # term_sums: single-monomer coefficients of the seven
    lit_us: float              # sum |terms| of usum
    c1_us: float
    cond_sum: float            # term_sums(conditioning=True)
    cond_max: float
    bend_pole: float           # sum over the bonds of kappa |psi - psi0| e_psi: what acos' slope does to the bending energy
    psi_sum: float             # sum psi
    epsi_sum: float            # sum over the bonds of e_psi
    epsi_max: float


def rec_of(ob, op, p: dict, phi, theta, cluster: bool, magnitudes: bool = True) -> Rec:
    """One oracle.chain_energy call, the rest numpy f64 on the angles.  magnitudes = False leaves out term_sums (lit and c1 are
    zero): enough for a configuration that only a wrong twin records."""
    phi, theta = np.asarray(phi), np.asarray(theta)
    n = len(phi)
    Uv, r, pp = ob.chain_energy(op, phi, theta)
    lit, c1, cond_sum, cond_max = term_sums(p, phi, theta, conditioning=True) if magnitudes else (np.zeros(7), np.zeros(7), 0.0, 0.0)
    ct, st = np.cos(theta), np.sin(theta)
    E0 = p["E0"]
    if p["chain_type"] == DIELECTRIC:
        K1, K2 = p.get("K1", 1.0), p.get("K2", 0.0)
        muz = (K1 - K2) * E0 * ct * ct + K2 * E0
        mu_c = abs((K1 - K2) * E0) + abs(K2 * E0)
    else:
        muz = p.get("mu", 1e-2) * ct
        mu_c = abs(p.get("mu", 1e-2))
    us = -0.5 * E0 * muz
    usum, lit_us = float(us.sum()), float(np.abs(us).sum())
    ex = np.zeros(2)
    psi_sum = epsi_sum = epsi_max = bend_pole = 0.0
    if cluster and n > 1:
        nh = np.stack([np.cos(phi) * st, np.sin(phi) * st, ct], axis=1)
        psi = np.arccos(np.clip((nh[:-1] * nh[1:]).sum(axis=1), -1, 1))
        kappa = p.get("bend_mod", 0.0)
        if kappa:
            bend = kappa / 2 * (psi - p.get("bend_angle", 0.0)) ** 2
            usum += float(bend.sum())
            lit_us += float(np.abs(bend).sum())
        ex[0], ex[1] = float((ct * ct).sum()), float(psi.sum() / (n - 1))
        with np.errstate(divide="ignore"):
            ep = np.minimum(math.sqrt(2 * PSI_DOT), PSI_DOT / np.sin(psi)) + ACOS_ABS
        psi_sum, epsi_sum, epsi_max = float(psi.sum()), float(ep.sum()), float(ep.max())
        bend_pole = float((abs(kappa) * np.abs(psi - p.get("bend_angle", 0.0)) * ep).sum())
    return Rec(np.concatenate([r, pp, [Uv]]), ex, usum, lit, c1, lit_us, 0.5 * abs(E0) * mu_c, cond_sum, cond_max, bend_pole,
               psi_sum, epsi_sum, epsi_max)


def _columns(v7, ex):
    """[T, 18]: the 16 observables in ABI order and the two extras, from [T, 7] and [T, 2]."""
    r, pp, Uv = v7[:, 0:3], v7[:, 3:6], v7[:, 6:7]
    return np.concatenate([r, r * r, (r * r).sum(axis=1, keepdims=True), pp, pp * pp, (pp * pp).sum(axis=1, keepdims=True),
                           Uv, Uv * Uv, ex], axis=1)


def _column_errors(v7, e7, eex):
    sq = 2 * np.abs(v7) * e7 + e7 * e7
    return np.concatenate([e7[:, 0:3], sq[:, 0:3], sq[:, 0:3].sum(axis=1, keepdims=True), e7[:, 3:6], sq[:, 3:6],
                           sq[:, 3:6].sum(axis=1, keepdims=True), e7[:, 6:7], sq[:, 6:7], eex], axis=1)


def _weighted_prefix(L, X):
    """P[t] = sum over tau <= t of X[tau] e^(L[tau] - M[t]), M the running maximum of L: carried with the maximum factored out."""
    out = np.empty_like(X, dtype=np.float64)
    acc = np.zeros(X.shape[1])
    m = -math.inf
    for t in range(len(L)):
        if L[t] > m:
            acc *= math.exp(m - L[t]) if m > -math.inf else 0.0
            m = L[t]
        acc = acc + X[t] * math.exp(L[t] - m)
        out[t] = acc
    return out


def _gauge(L, L0):
    """The rising gauge restated on f64 log-weights: g[t] after record t, starting on the start configuration's L0."""
    g = np.empty(len(L))
    cur = L0
    for t in range(len(L)):
        if L[t] - cur > GAUGE_T:
            cur = L[t]
        g[t] = cur
    return g


@dataclass
class Twin:
    cols: np.ndarray           # [T, 18]: plain the running sums, umbrella the gauge-free ratios
    nstar: np.ndarray | None   # umbrella, [T]: the normaliser over its heaviest record's weight
    top: np.ndarray | None     # umbrella, [T]: the heaviest record's log-weight so far, gauged on the start configuration
    rises: np.ndarray | None   # umbrella, [T]: how often the restated gauge has risen


def record_twin(recs, s=None, usum0=None, wrong=None, trial=None, accepted=None) -> Twin:
    """record! restated on `recs`, the configurations of one chain after each of its steps.  s: None (plain) or the umbrella
    scale; usum0: usum of the start configuration (the device gauges a chain on it).
    wrong: None, or one of the wrong twins that the bound must tell from the right one --
      "W1"  the scale is s (1 + 2^-8);
      "W2"  on a rejected step the trial is recorded (trial[t]: its Rec, accepted[t]: the step's outcome);
      "W3"  the first record of every 128-step block is dropped;
      "W4"  umbrella, clustering main: the two extra columns are not rescaled when the gauge rises."""
    if wrong == "W2":
        recs = [r if accepted[t] else trial[t] for t, r in enumerate(recs)]
    V = _columns(np.array([r.v for r in recs]), np.array([r.ex for r in recs]))
    keep = np.ones(len(recs))
    if wrong == "W3":
        keep[::FLUSH] = 0.0
    if s is None:
        return Twin(np.cumsum(V * keep[:, None], axis=0), None, None, None)
    if wrong == "W1":
        s = s * (1 + 2.0 ** -8)
    L = -s * np.array([r.usum for r in recs])
    P = _weighted_prefix(L, np.concatenate([V, np.ones((len(L), 1))], axis=1) * keep[:, None])
    with np.errstate(invalid="ignore", divide="ignore"):
        cols = P[:, :-1] / P[:, -1:]
    L0 = -s * usum0
    g = _gauge(L, L0)
    M = np.maximum.accumulate(L)
    if wrong == "W4":
        # each record of the extras keeps the weight it had under the gauge of ITS time; the normaliser follows the gauge
        ex = np.cumsum(V[:, 16:18] * np.exp(L - g)[:, None], axis=0)
        with np.errstate(invalid="ignore", divide="ignore"):
            cols[:, 16:18] = ex / (P[:, -1:] * np.exp(M - g)[:, None])
    rises = np.cumsum(np.diff(np.concatenate([[L0], g])) != 0)
    return Twin(cols, P[:, -1], M - L0, rises)


def _launch_max(x0, x, launch):
    """Per step, the largest of x over the states its launch has passed through: the state the launch started from (x0 for the
    first launch) and every state up to the step's own.  x: [T] or [T, k]; launch: steps per launch."""
    x = np.asarray(x, dtype=np.float64)
    full = np.concatenate([np.asarray(x0, dtype=np.float64)[None], x], axis=0)
    out = np.empty_like(x)
    for lo in range(0, len(x), launch):
        hi = min(lo + launch, len(x))
        out[lo:hi] = np.maximum.accumulate(full[lo:hi + 1], axis=0)[1:]
    return out


def record_bound(recs, n: int, acc_since_launch, block: int, s=None, usum0=None, start=None, launch=1):
    """The bound of the derivation above on every prefix and column of record_twin(recs, s, usum0): [T, 18]; under
    umbrella sampling also the margin [T] of the gauge contract (see GAUGE_MARGIN_MAX).  acc_since_launch[t]: the steps
    accepted since the launch that recorded t began, t's own included.  start: the Rec of the configuration before the first
    step; launch: steps per launch.  A carried difference passes through the totals and terms of the states it leaves as well
    as of the state it reaches, so every magnitude of a carried term is the largest its launch has seen, the launch's starting
    state included (found by check (d): a random start inside a repulsive contact, U = 7.2e6, left at step 1 -- the f32 U of
    the next state carries the half ulp of 7.2e6)."""
    start = recs[0] if start is None else start
    a = np.asarray(acc_since_launch, dtype=np.float64)
    T = len(recs)
    v7 = np.array([r.v for r in recs])
    V = _columns(v7, np.array([r.ex for r in recs]))
    A = np.abs(V)
    lit = np.array([r.lit for r in recs])
    e7 = n * K_TOTALS * U * lit + a[:, None] * K_TOTALS * U * _launch_max(start.lit, lit, launch) + \
        (n + 2 * a[:, None]) * K_ABS * U * np.array([r.c1 for r in recs])
    cmax = _launch_max(max(start.cond_max, start.cond_sum), np.array([max(r.cond_max, r.cond_sum) for r in recs]), launch)
    e7[:, 6] += K_COND * U * (np.array([r.cond_sum for r in recs]) + 4 * a * cmax)      # PAIR CONDITIONING
    bp = np.array([r.bend_pole for r in recs])
    e7[:, 6] += bp + 4 * a * _launch_max(start.bend_pole, bp, launch)      # the bending energy through acos (see the extras)
    e_c2 = (a + n) * K_TOTALS * U * V[:, 16] + (n + 2 * a) * K_ABS * U
    emax = _launch_max(start.epsi_max, np.array([r.epsi_max for r in recs]), launch)   # a difference takes the old bond and the new
    e_psi = (np.array([r.epsi_sum for r in recs]) + 8 * a * emax +
             (a + n) * K_TOTALS * U * _launch_max(start.psi_sum, np.array([r.psi_sum for r in recs]), launch)) / max(n - 1, 1)
    EV = _column_errors(v7, e7, np.stack([e_c2, e_psi], axis=1))
    common = block * U + RESCALE + 2.0 ** -52
    if s is None:
        return np.cumsum(EV + 2 * U * A, axis=0) + common * np.cumsum(A, axis=0), None
    L = -s * np.array([r.usum for r in recs])
    L0 = -s * usum0
    M = np.maximum.accumulate(np.maximum(L, -math.inf))
    span = np.maximum(M, L0) - np.minimum(np.minimum.accumulate(L), L0)
    lit_us = np.array([r.lit_us for r in recs])
    e_us = 2 * K_TOTALS * U * lit_us + a * K_TOTALS * U * _launch_max(start.lit_us, lit_us, launch) + \
        (n + 2 * a) * K_ABS * U * np.array([r.c1_us for r in recs])
    ew = s * e_us + 4 * U * span + 2 * U
    X = np.concatenate([A, EV + A * (ew[:, None] + 2 * U), np.ones((T, 1)), (ew + U)[:, None]], axis=1)
    P = _weighted_prefix(L, X)
    Pabs, Perr, den, Pew = P[:, :18], P[:, 18:36], P[:, 36], P[:, 37]
    rises = np.floor(span / GAUGE_LIFT)
    shared = (common + rises * (4 * U * span + 2 * U))[:, None]
    tiny = 2.0 ** -126 * np.exp(np.minimum(_gauge(L, L0) - M, 600.0))
    E_num = Perr + shared * Pabs + (tiny * np.arange(1, T + 1))[:, None] * np.maximum.accumulate(A, axis=0)
    E_den = Pew + shared[:, 0] * den + tiny * np.arange(1, T + 1)
    ratio = record_twin(recs, s, usum0).cols
    with np.errstate(invalid="ignore", divide="ignore"):
        B = (E_num + np.abs(ratio) * E_den[:, None]) / (den - E_den)[:, None]
    return B, E_den / (den - E_den) + np.maximum.accumulate(ew)


def first_violation(got, want, bound, steps=None, first_column=0):
    """(worst error / bound, message or None): the first row at which a column leaves its bound.  steps: the 1-based step of
    every row (default: row + 1); first_column: COLUMNS index of column 0."""
    err = np.abs(got - want)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    q = np.where(np.isfinite(got) & np.isfinite(want), q, np.inf)
    bad = np.argwhere(q > 1.0)
    if len(bad) == 0:
        return float(q.max()) if q.size else 0.0, None
    t, k = bad[0]
    step = t + 1 if steps is None else steps[t]
    return float(q.max()), (f"step {step}, column {COLUMNS[first_column + k]}: got {got[t, k]!r}, twin {want[t, k]!r}, "
                            f"error / bound {q[t, k]:.3g}")


# ------------------------------------------------------------------------------------------------- between the launches
#
# What happens to an f32 / q16 handle BETWEEN step launches, pinned per event against the oracle: the start (init_kernel and
# the store_* helpers of pstat_math.h), pstat_reinit (reinit_kernel<float>, <uint16_t>), and the steps that follow a re-init
# while the acceptor's stale cache -- the `lag` -- is live.  The oracle's side is eap_reinit_judge (oracle/eap_oracle.h), which
# shares its functions with the run loops; tests/test_lifecycle_judge_cpu.py replays those loops with it.
#
# THE START, exactly, from the chain's generator words w (phi draws first, then theta draws), u = (w >> 9) 2^-23:
#   f64: phi = 2 pi u, theta = pi u -- the oracle's own start.
#   f32: phi = (float) u turns, theta = (float) (u / 2) turns; both are exact (23 and 24 significant bits), and read back as
#        radians, 2 pi * (double) raw (load_phi / load_theta), they ARE the oracle's start: 2 pi (u / 2) and pi u round alike.
#   q16: the lattice index w >> 16 for both ((uint32) (u 65536) = (w >> 9) >> 7), read back as (index + 1/2) cells.
#   --x0 (scalar or per monomer), a = x0 + dx0 u in f64 (product and sum rounded separately: pstat_kernels.o and the oracle are
#        both built without contraction): f64 keeps a; f32 stores (float) (t - floor(t)), t = a_phi / 2 pi, and
#        (float) (a_theta / 2 pi); q16 stores (uint32) min(65535, (t - floor(t)) 65536) and
#        (uint32) min(65535, max(0, a_theta / pi 65536)) -- store_phi_rad / store_theta_rad restated operation by operation.
#
# THE RE-INIT VERDICT  z = d - log eps  against m, d and mag from eap_reinit_judge (mag = 1 + sum |t| over EVERY term of both
# configurations over kT + sum |log sin| of both + |lag_in|: a fresh draw changes every monomer).
#   sweep homes.  reinit_kernel draws the fresh angles in storage format and evaluates them, and prod sin(theta) of the stored
#     chain, in f64: against the judge on the same angles that is f64 roundoff.  Each configuration costs ~5 n + 12 rounded
#     operations on numbers that mag sums (n-hat, dipole, field, force, n - 1 bonds, the running sums, the exponent, exp,
#     the two products of sines and their quotient): (10 n + 24) 2^-53 mag <= 2^-44 mag for n <= 40 (424 < 512).  The one
#     f32 quantity is U_old = obs[U], what the f32 step kernel carried out of its last launch: the CARRIED TOTALS bound
#     above, carried(U) = (acc + n) K_TOTALS u sum |terms of U| + (n + 2 acc) K_ABS u c1(U), acc the acceptances of that launch:
#         m = 2^-44 mag + carried(U) / kT  [+ carried(usum) wscale under umbrella sampling: the cached usum enters lp_old].
#   all-pairs home.  interacting_kernel<float> re-derives both configurations in f32 (v_sin / v_cos, the f32 all-pairs sum)
#     and compares in f64: the step verdict's derivation holds term by term with mag over all terms, and log((double) st) of
#     a v_sin_f32 result carries SINCOS_ABS / sin(theta) per monomer, old and new (item (e) above, without a proposal):
#         m = C_VERDICT u mag + SINCOS_ABS sum (1 / sin theta + 1 / sin theta') over all monomers.
#     A fresh draw with two monomers closer than CONTACT_DISTANCE b is outside what mag can judge: undecided.
#
# THE LAG.  While an adopted lag is live the device's differs from the twin's lag_out by at most the same quantity (lp_new is
# f64 on stored angles, lp_old carries obs[U] and obs[usum]): lag_error = 2^-44 mag + carried(U) / kT [+ carried(usum) wscale]
# on the sweep homes; it is added to the step margin m until the next acceptance clears the lag.  A re-init adopted while a lag
# is still live inherits it through lag_in, error included: the errors add up until an acceptance clears both.
#
# A forced re-init is decided ("adopt") whatever d is.  Nothing above comes from what a kernel returned.
REINIT_F64 = 2.0 ** -44


@dataclass
class Event:
    kind: str
    step: int = 0
    J: object = None              # oracle Reinit (re-inits)
    V: Verdict = None
    lag_error: float = 0.0
    outside: bool = False         # all-pairs home: the fresh draw holds a contact
    phi: np.ndarray = None        # the twin's state after the event
    theta: np.ndarray = None
    rng: np.ndarray = None


def _seed_words(ob, op, chain_id):
    import ctypes as C
    s = (C.c_uint32 * 4)()
    if op.rng == XOSHIRO:
        ob.lib().eap_rng_seed(int(op.seed), int(chain_id), s)
    else:
        ob.lib().eap_mwc64x_seed(int(op.seed), int(chain_id), s)
    return s


TWO_PI, PI = 6.28318530717958647692, 3.14159265358979323846      # the literals of pstat_math.h


def stored_uniform(words_phi, words_theta, precision):
    """The uniform start / fresh draw as the device stores it, in radians as load_phi / load_theta give it."""
    wp, wt = np.asarray(words_phi, dtype=np.uint64), np.asarray(words_theta, dtype=np.uint64)
    if precision == Q16:
        return lattice_phi((wp >> np.uint64(16)).astype(np.float64)), lattice_theta((wt >> np.uint64(16)).astype(np.float64))
    up = (wp >> np.uint64(9)).astype(np.float64) * 2.0 ** -23
    ut = (wt >> np.uint64(9)).astype(np.float64) * 2.0 ** -23
    if precision == F32:
        rp, rt = np.float32(up), np.float32(0.5 * ut)
        assert np.array_equal(rp.astype(np.float64), up) and np.array_equal(rt.astype(np.float64), 0.5 * ut)     # exact
        return TWO_PI * rp.astype(np.float64), TWO_PI * rt.astype(np.float64)
    return TWO_PI * up, PI * ut


def start_twin(ob, op, params, chain_id, precision):
    """(phi, theta, rng): the stored start of a chain, stated exactly from its generator words (see THE START above), in radians
    as Ensemble.chain_state returns them, and the generator words after the 2n draws.  Everything is read from `op`, the
    oracle's parameter struct (`params`, the option dict, is not needed)."""
    n = int(op.n)
    s = _seed_words(ob, op, chain_id)
    w = [_next_word(ob, op.rng, s) for _ in range(2 * n)]
    rng = np.array(s[:], dtype=np.uint32)
    wp, wt = np.array(w[:n], dtype=np.uint64), np.array(w[n:], dtype=np.uint64)
    if not op.use_x0:
        phi, th = stored_uniform(wp, wt, precision)
        return phi, th, rng
    up = (wp >> np.uint64(9)).astype(np.float64) * 2.0 ** -23
    ut = (wt >> np.uint64(9)).astype(np.float64) * 2.0 ** -23
    if bool(op.x0_vec) and op.x0_len == 2 * n:
        vec = np.array([op.x0_vec[i] for i in range(2 * n)])
        x0p, x0t = vec[0::2], vec[1::2]
    else:
        x0p, x0t = np.float64(op.x0_phi), np.float64(op.x0_theta)
    ap = x0p + np.float64(op.dx0_phi) * up
    at = x0t + np.float64(op.dx0_theta) * ut
    if precision == F64:
        return ap, at, rng
    t = ap / TWO_PI
    t = t - np.floor(t)
    if precision == F32:
        return TWO_PI * np.float32(t).astype(np.float64), TWO_PI * np.float32(at / TWO_PI).astype(np.float64), rng
    j = np.minimum(65535.0, t * 65536.0).astype(np.uint32)
    k = np.minimum(65535.0, np.maximum(0.0, at / PI * 65536.0)).astype(np.uint32)
    return lattice_phi(j.astype(np.float64)), lattice_theta(k.astype(np.float64)), rng


def usum_terms(p: dict, theta):
    """(sum |terms|, single-monomer coefficient) of sum(us) in the fixed-force main: the field terms."""
    ct = np.cos(np.asarray(theta))
    E0 = p["E0"]
    if p["chain_type"] == DIELECTRIC:
        K1, K2 = p.get("K1", 1.0), p.get("K2", 0.0)
        muz, mu_c = (K1 - K2) * E0 * ct * ct + K2 * E0, abs((K1 - K2) * E0) + abs(K2 * E0)
    else:
        muz, mu_c = p.get("mu", 1e-2) * ct, abs(p.get("mu", 1e-2))
    return float(np.abs(0.5 * E0 * muz).sum()), 0.5 * abs(E0) * mu_c


def carried(n: int, acc: int, lit: float, c1: float) -> float:
    """The CARRIED TOTALS bound on one total after a launch with `acc` acceptances: bound (b) of tests/test_gpu_step_judge.py."""
    return (acc + n) * K_TOTALS * U * lit + (n + 2 * acc) * K_ABS * U * c1


def carried_over_kT(p: dict, phi, theta, acc: int) -> float:
    """carried(U) / kT [+ carried(usum) wscale]: what the f32 step kernel's cached totals add to a re-init's exponent and lag."""
    lit, c1 = term_sums(p, phi, theta)
    e = carried(p["n"], acc, float(lit[6]), float(c1[6])) / abs(p["kT"])
    if p.get("umbrella"):
        e += carried(p["n"], acc, *usum_terms(p, theta)) * umbrella_scale(p)
    return e


def reinit_home(p: dict) -> str:
    return "allpairs" if p["energy_type"] == INTERACTING else "sweep"


def reinit_verdict(J, precision, home, carried=0.0, pole=0.0, outside=False) -> Verdict:
    """z = d - log eps of a re-init against its margin (THE RE-INIT VERDICT above).  `carried`: carried_over_kT of the chain
    before the re-init (sweep homes, f32 / q16; 0 for f64); `pole`: SINCOS_ABS sum (1 / sin theta + 1 / sin theta') (all-pairs
    home); `outside`: the fresh draw holds a contact.  kind: "accept" = adopted."""
    if J.forced:
        return Verdict("accept", math.inf, 0.0, math.inf)
    if home == "allpairs":
        m = C_VERDICT * U * J.mag + pole
    else:
        m = REINIT_F64 * J.mag + (0.0 if precision == F64 else carried)
    if math.isnan(J.d) or outside:
        return Verdict("undecided", math.nan, m, 0.0)
    z = J.d - (math.log(J.eps) if J.eps > 0 else -math.inf)
    if abs(z) <= m:
        return Verdict("undecided", z, m, abs(z) / (U * J.mag))
    return Verdict("accept" if z > 0 else "reject", z, m, abs(z) / (U * J.mag))


def sin_pole(theta_old, theta_new) -> float:
    with np.errstate(divide="ignore"):
        return float(SINCOS_ABS * (1.0 / np.sin(np.asarray(theta_old)) + 1.0 / np.sin(np.asarray(theta_new))).sum())


def lag_error(J, p: dict, home, precision, carried=0.0, pole=0.0, lit_old=0.0, lit_new=0.0, cond=0.0) -> float:
    """How far the device's lag may lie from the twin's lag_out while it is live (THE LAG above)."""
    if precision == F64:
        return REINIT_F64 * J.mag
    if home == "allpairs":
        # C_VERDICT u (lit_old + lit_new) / kT, plus what the margin of the verdict also carries: the log sin of v_sin_f32
        # results; the cast of the lag itself to float (one rounding of |lag_out|); cond: PAIR CONDITIONING of both sums
        return C_VERDICT * U * (lit_old + lit_new) / abs(p["kT"]) + pole + U * abs(J.lag_out) + cond
    return REINIT_F64 * J.mag + carried


def u_error(p: dict, phi, theta, acc: int = 1) -> float:
    """The bound on |U (f32 kernel) - U (f64)| of one configuration over kT: CARRIED TOTALS plus PAIR CONDITIONING of the record
    bound above (the re-derivation's sum and 4 acc times the largest term)."""
    lit, c1, cond_sum, cond_max = term_sums(p, phi, theta, conditioning=True)
    return (carried(p["n"], acc, float(lit[6]), float(c1[6])) + K_COND * U * (cond_sum + 4 * acc * cond_max)) / abs(p["kT"])


def contact_margin(p: dict, phi, theta, trial_phi, trial_theta) -> float:
    """All-pairs rows after a re-init: a uniform fresh draw is a coil, not the rod these rows start from, and may hold two
    monomers closer than CONTACT_DISTANCE b.  There the f32 error of a step's dU follows the whole pair sum and the
    cancellation inside the separations, which mag -- the changed terms -- does not see.  It is bounded by
    the error of U itself on both sides of the step: u_error(current) + u_error(trial).  0 where neither holds a contact."""
    if min(min_pair_distance(p, phi, theta), min_pair_distance(p, trial_phi, trial_theta)) >= CONTACT_DISTANCE:
        return 0.0
    return u_error(p, phi, theta) + u_error(p, trial_phi, trial_theta)


def fresh_words(ob, op, rng):
    """The 2n words of a fresh draw from the generator state `rng` (phi words, theta words)."""
    import ctypes as C
    s = (C.c_uint32 * 4)(*[int(w) for w in rng])
    w = [_next_word(ob, op.rng, s) for _ in range(2 * int(op.n))]
    return np.array(w[:op.n], dtype=np.uint64), np.array(w[op.n:], dtype=np.uint64)


def reinit_event(ob, op, p: dict, phi, theta, rng, lag, forced: bool, precision, acc_last: int = 1) -> Event:
    """One re-init of a chain judged from the state (phi, theta, rng, lag): the oracle's eap_reinit_judge on the fresh draw as
    the device stores it (q16: on the lattice; f32: the oracle's own, see THE START), its verdict and the lag error.
    acc_last: the acceptances of the chain's last launch (the stepped handle: of its last step)."""
    home = reinit_home(p)
    fresh_to = None
    if precision == Q16:
        fresh_to = stored_uniform(*fresh_words(ob, op, rng), Q16)
    J = ob.reinit_judge(op, phi, theta, rng, lag_in=lag, force=forced, fresh_to=fresh_to)
    if precision == F32:        # the f32 fresh draw IS the oracle's
        fp, ft = stored_uniform(*fresh_words(ob, op, rng), F32)
        assert np.array_equal(fp, J.fresh_phi) and np.array_equal(ft, J.fresh_theta)
    car = pole = lo = ln = cond = 0.0
    outside = False
    if precision in (F32, Q16):
        if home == "allpairs":
            pole = sin_pole(theta, J.fresh_theta)
            outside = min_pair_distance(p, J.fresh_phi, J.fresh_theta) < CONTACT_DISTANCE
            to, tn = term_sums(p, phi, theta, conditioning=True), term_sums(p, J.fresh_phi, J.fresh_theta, conditioning=True)
            lo, ln = float(to[0][6]), float(tn[0][6])
            cond = K_COND * U * (to[2] + tn[2]) / abs(p["kT"])
        else:
            car = carried_over_kT(p, phi, theta, acc_last)
    V = reinit_verdict(J, precision if precision is not None else F64, home, car, pole, outside)
    E = Event("reinit_forced" if forced else "reinit_metropolis", J=J, V=V)
    E.lag_error = lag_error(J, p, home, precision if precision is not None else F64, car, pole, lo, ln, cond)
    E.outside = outside
    return E


# THE LIFECYCLE TABLE.  Fixed-force rows: 100 steps, forced re-init; 100 steps, Metropolis re-init; 100 steps, forced then
# Metropolis at once (at large n an equilibrated chain never adopts a fresh draw: only a fresh draw against a fresh draw,
# uniform against uniform, shows both outcomes there); 100 steps.
SEGMENT = 100
FIXED_FORCE_EVENTS = [(SEGMENT, "reinit_forced"), (2 * SEGMENT, "reinit_metropolis"), (3 * SEGMENT, "reinit_forced"),
                      (3 * SEGMENT, "reinit_metropolis")]
LIFECYCLE_T = 4 * SEGMENT


# Where a row of CONFIGS is taken over with another seed or force, the reason is a condition of tests/test_lifecycle_judge_cpu.py
# checked with the judge alone (the issue's rule: change the seed or weaken the field, never the cap):
#   sweep-n1-ising-polar: E0 mu / (2 kT) = 0.5, the lags are below 1 and the twin that clears the lag is caught once in 1500
#     post-event steps at seed 1001; 17 times at 1008.
#   umb-sweep-n3-ising-diel: under _HELD_ISING's force (Fz b / kT = 5.6) a forced re-init leaves lags of 15 ... 40 that freeze every
#     judged chain, and the twin without the umbrella term is never caught (seeds 4003 ... 4014: 0 ... 2 times); under
#     _DIEL_ISING's own Fz = 0.8 the chains thaw: 17 times at seed 4006.  (The held force is there for check (b) over 2000 steps
#     of CONFIGS, which this table does not run.)
_LIFE_OVERRIDES = {"umb-sweep-n3-ising-diel": dict(Fz=0.8)}
# THE SEEDS.  The tally rule "the judge with E0 (1 + 2^-8) is caught" holds per row, and a row is only 4 x 100 steps of five chains,
# most of them frozen after the first re-init at n >= 33: under the seeds of CONFIGS the judge alone meets the perturbed judge
# 0 ... 5 times per row (22 of 41 rows: never).  So every row's seed is the FIRST, counting up from the seed of its CONFIGS row
# (the all-pairs rows: from 5000 + n), at which the judge alone, on the row's own judged chains and schedule, shows ALL of: the
# perturbed judge caught at least twice; at most 0.5 % of the post-event steps undecided; no Metropolis verdict undecided; for
# n <= 3 an adopted and a refused Metropolis re-init, a chain that thaws and the lag-free twin caught at least 5 times; for
# n >= 33 a frozen chain; under umbrella sampling the twin without the umbrella term caught at least twice; at n = 100 no fresh
# draw with a pair term above kT.  tests/test_lifecycle_judge_cpu.py asserts each of these per row.
LIFE_SEEDS = {
    "life-f32-allpairs-n100": 5182,
    "life-f32-allpairs-n2": 5004,
    "life-f32-allpairs-n3": 5122,
    "life-f32-allpairs-n5": 5083,
    "life-f32-sweep-n1-ising-polar": 1015,
    "life-f32-sweep-n1-ni-diel": 1001,
    "life-f32-sweep-n2-ising-diel": 1007,
    "life-f32-sweep-n2-ni-polar": 1002,
    "life-f32-sweep-n3-ising-diel": 1003,
    "life-f32-sweep-n3-ni-polar": 1003,
    "life-f32-sweep-n33-ni-polar": 1209,
    "life-f32-sweep-n40-ising-polar": 1098,
    "life-f32-umb-sweep-n1-ising-polar": 4041,
    "life-f32-umb-sweep-n1-ni-diel": 4001,
    "life-f32-umb-sweep-n3-ising-diel": 4007,
    "life-f32-umb-sweep-n3-ni-polar": 4037,
    "life-f32lds-cluster-n20-ising-diel-cp0.5-bend": 2205,
    "life-f32lds-cluster-n20-ni-polar-cp0.0-nobend": 2206,
    "life-f32lds-cluster-n3-ising-diel-cp0.0-bend": 2040,
    "life-f32lds-cluster-n3-ni-polar-cp1.0-nobend": 2037,
    "life-f32mem-cluster-n20-ising-diel-cp0.5-bend": 2205,
    "life-f32mem-cluster-n20-ni-polar-cp0.0-nobend": 2206,
    "life-f32mem-cluster-n3-ising-diel-cp0.0-bend": 2040,
    "life-f32mem-cluster-n3-ni-polar-cp1.0-nobend": 2037,
    "life-q16-sweep-n1-ising-polar": 1015,
    "life-q16-sweep-n1-ni-diel": 1001,
    "life-q16-sweep-n2-ising-diel": 1007,
    "life-q16-sweep-n2-ni-polar": 1002,
    "life-q16-sweep-n3-ising-diel": 1003,
    "life-q16-sweep-n3-ni-polar": 1003,
    "life-q16-sweep-n33-ni-polar": 1209,
    "life-q16-sweep-n40-ising-polar": 1098,
    "life-q16-umb-sweep-n1-ising-polar": 4041,
    "life-q16-umb-sweep-n1-ni-diel": 4001,
    "life-q16-umb-sweep-n3-ising-diel": 4007,
    "life-q16-umb-sweep-n3-ni-polar": 4042,
    "life-q16lds-cluster-n20-ising-diel-cp0.5-bend": 2205,
    "life-q16lds-cluster-n20-ni-polar-cp0.0-nobend": 2206,
    "life-q16lds-cluster-n3-ising-diel-cp0.0-bend": 2040,
    "life-q16lds-cluster-n3-ni-polar-cp1.0-nobend": 2037,
}
LIFE_PACKED_SEED0 = 600      # the packed handle's cases: seeds 600 ... 612


def cluster_events(n: int):
    """The clustering rows' schedule: 100 steps; a rung at 10 kT; 100 steps; the rung at kT; 100 steps; restart_from_x0 with a
    per-monomer x0 (phi beyond 2 pi and below 0, so that store_phi_rad's fold is used) + Uniform(0, dx0); 100 steps."""
    i = np.arange(n)
    x0 = np.stack([-0.25 + 0.7 * i, 0.6 + 0.11 * (i % 17)], axis=1).ravel()
    return [(SEGMENT, "rung", 10.0), (2 * SEGMENT, "rung", 1.0), (3 * SEGMENT, "x0", x0, 0.5, 0.4)]


def _lifecycle_configs():
    out = []

    def take(cfg):
        p = dict(cfg.params, **_LIFE_OVERRIDES.get(cfg.name.split("-", 1)[1], {}), seed=LIFE_SEEDS["life-" + cfg.name])
        out.append(Config("life-" + cfg.name, cfg.kernel, cfg.precision, p, cfg.chains, LIFECYCLE_T, events=list(FIXED_FORCE_EVENTS)))

    for cfg in CONFIGS:
        n = cfg.params["n"]
        sweep = "-sweep-n" in cfg.name and "-rise-" not in cfg.name and "-umb-" not in cfg.name
        umb = "-umb-sweep-n1-" in cfg.name or "-umb-sweep-n3-" in cfg.name
        if (sweep and n in (1, 2, 3)) or umb:
            take(cfg)
    # n = 33 and 40, one each per state format: the non-interacting polar row at 33, the Ising polar row at 40
    for cfg in CONFIGS:
        if cfg.name in ("f32-sweep-n33-ni-polar", "q16-sweep-n33-ni-polar", "f32-sweep-n40-ising-polar", "q16-sweep-n40-ising-polar"):
            take(cfg)
    # one packed f32 handle: 13 cases x 5 chains (packed handles always carry the lag path)
    cases = [dict(PACKED_COMMON, seed=LIFE_PACKED_SEED0 + i, **c) for i, c in enumerate(PACKED_CASES)]
    out.append(Config("life-f32-packed", "sweep_kernel<float> [packed cases]", F32, cases[0], 5, LIFECYCLE_T, env={"PSTAT_PACK": "1"},
                      cases=cases, events=list(FIXED_FORCE_EVENTS)))
    # interacting_kernel<float>, whose re-init runs inside the step kernel in f32: the extended start and the weak coupling of
    # _allpairs_configs; M = 1 at n = 2, 3, 5, M = 2 at n = 100 (forced re-inits only: a uniform coil of 100 monomers holds
    # about three contacts, so its Metropolis verdict would be undecided every time)
    # (at seeds 5002 and 5005 three of the ten Metropolis draws of the judged chains hold a contact and are undecided by rule: hence
    #  THE SEEDS' condition that no Metropolis verdict be undecided)
    for i, n in enumerate((2, 3, 5, 100)):
        ct = dict(chain_type=DIELECTRIC, E0=30.0, K1=0.0125, K2=0.0025, Fz=0.3, Fx=8.0, b=1.0) if i % 2 == 0 else \
            dict(chain_type=POLAR, E0=100.0, mu=0.1, Fz=0.3, Fx=8.0, b=1.0, do_flips=1)
        p = dict(n=n, energy_type=INTERACTING, rng=MWC if i % 2 else XOSHIRO, kT=1.0, seed=LIFE_SEEDS[f"life-f32-allpairs-n{n}"], **ct, **_X0,
                 **(_ADAPT if i % 2 else _FIXED))
        if n == 3:      # under Fx b / kT = 8 a forced re-init leaves lags of 16 ... 40 and no judged chain thaws within its 100 steps
            p["Fx"] = 2.0    # (seeds 5003 ... 5010); under the weaker force two of five do, and both Metropolis outcomes show
        ev = list(FIXED_FORCE_EVENTS) if n < 100 else [(k * SEGMENT, "reinit_forced") for k in (1, 2, 3)]
        chains = 70
        if n == 100:
            # 70 chains x 3 uniform coils of 100 monomers hold a contact below 0.007 b under every seed (two antiparallel
            # neighbours: 99 bonds x rho^2 per coil), a pair term of 1e3 ... 1e5 kT at mu^2 / (4 pi b^3) = 8e-4 kT -- chain 2 of seed
            # 5100 adopts U = +5.7e4 kT -- and there the carried positions of a 100-step launch and the re-derived ones of a
            # one-step launch decide differently in f32 (found by the long-launch check of the GPU test: nacc_total 86
            # against 87 on that chain).  So this row has the six chains of the other all-pairs rows and a fifth of the dipole
            # at ten times the field (E0 mu / 2 = 10 kT per monomer, coupling 3.2e-5 kT; at 5 kT the judge alone met the perturbed
            # judge at most once under the nine contact-free seeds of 5100 ... 5499), and its seed is one at which no fresh draw of
            # any chain holds a pair term above 1 kT; the CPU test asserts it.
            # WHAT THIS ROW PINS: at 3.2e-5 kT the pair sum lies below the verdict margin, so the row pins the words, the adoption,
            # the lag and the field and force part of the M = 2 re-init and of the steps after it -- not its pair part, which the
            # n = 100 ... 257 rows of CONFIGS judge step by step.  M itself is chosen from n alone (pstat_interacting.hip: M = 2 for
            # 64 < n <= 128); launch_info does not name it, so the CPU test asserts the n.
            p.update(mu=0.02, E0=1000.0)
            chains = 6
        out.append(Config(f"life-f32-allpairs-n{n}", "interacting_kernel<float>", F32, p, chains, LIFECYCLE_T, events=ev))
    # the clustering main, every chain-per-lane home: n = 3 and n = 20, an Ising and a non-interacting row each, on the ladder
    for cfg in CONFIGS:
        tail = cfg.name.split("-cluster-", 1)[-1]
        if cfg.cluster and "-umb-" not in cfg.name and "-rise-" not in cfg.name and "allpairs" not in cfg.name and \
                tail in ("n3-ni-polar-cp1.0-nobend", "n3-ising-diel-cp0.0-bend", "n20-ising-diel-cp0.5-bend", "n20-ni-polar-cp0.0-nobend"):
            out.append(Config("life-" + cfg.name, cfg.kernel, cfg.precision, dict(cfg.params, seed=LIFE_SEEDS["life-" + cfg.name]), cfg.chains,
                              LIFECYCLE_T, cluster=True,
                              env=dict(cfg.env), not_kernel=cfg.not_kernel, events=cluster_events(cfg.params["n"])))
    return out


LIFECYCLE = _lifecycle_configs()
LIFECYCLE_IDS = [c.name for c in LIFECYCLE]


def microstate_ld(p: dict, phi, theta, cluster: bool = False):
    """r (3), p (3), U of a configuration in numpy longdouble, restated from inc/eap_chain.jl and energy.jl:7-23 like term_sums
    (bending only in the clustering main).  The reference of pstat_microstate wherever 1e-13 sum |terms| is asked: the
    oracle's eap_chain_energy takes every separation from the running sums of update_xs, and inside a 1/r^3 contact of two
    neighbours that cancellation alone costs it more (measured on the seeded start of life-*-sweep-n40-ising-polar, chain 57,
    |n_i + n_j| / 2 = 0.0012: the oracle 2.5e-13 sum |terms| from this restatement, the bond vector taken directly 1.2e-14)."""
    LD = np.longdouble
    phi, theta = np.asarray(phi).astype(LD), np.asarray(theta).astype(LD)
    n = len(phi)
    nh = np.stack([np.cos(phi) * np.sin(theta), np.sin(phi) * np.sin(theta), np.cos(theta)], axis=1)
    E0, b = LD(p["E0"]), LD(p.get("b", 1.0))
    if p["chain_type"] == DIELECTRIC:
        K1, K2 = LD(p.get("K1", 1.0)), LD(p.get("K2", 0.0))
        mu = ((K1 - K2) * E0 * nh[:, 2])[:, None] * nh
        mu[:, 2] += K2 * E0
    else:
        mu = LD(p.get("mu", 1e-2)) * nh
    r = b * nh.sum(axis=0)
    en = p["energy_type"]
    Uv = LD(0)
    if en != CUTOFF:
        Uv += (-LD(0.5) * E0 * mu[:, 2]).sum() - (r[0] * LD(p.get("Fx", 0.0)) + r[2] * LD(p.get("Fz", 0.0)))
        if cluster and p.get("bend_mod", 0.0) and n > 1:
            psi = np.arccos(np.clip((nh[:-1] * nh[1:]).sum(axis=1), -1, 1))
            Uv += (LD(p["bend_mod"]) / 2 * (psi - LD(p.get("bend_angle", 0.0))) ** 2).sum()
    if en != NONINTERACTING and n > 1:
        if en == ISING:
            rv = -(b / 2) * (nh[:-1] + nh[1:])        # x_i - x_{i+1}
            mi, mj = mu[:-1], mu[1:]
        else:
            x = b * (np.cumsum(nh, axis=0) - LD(0.5) * nh)
            ii, jj = np.triu_indices(n, 1)
            rv, mi, mj = x[ii] - x[jj], mu[ii], mu[jj]
        r2 = (rv * rv).sum(axis=1)
        rm = np.sqrt(r2)
        h = rv / rm[:, None]
        t = ((mi * mj).sum(axis=1) - 3 * (mi * h).sum(axis=1) * (mj * h).sum(axis=1)) / (4 * LD(np.pi) * r2 * rm)
        if en == CUTOFF:
            t = t[r2 <= (LD(p.get("cutoff_radius", 7.5)) * b) ** 2]
        Uv += t.sum()
    return np.concatenate([r, mu.sum(axis=0), [Uv]])


def check_start(oracle, e, cases, ops, chains, precision, which=None, phi_step=None, theta_step=None, cluster=False):
    """THE START on a handle `e` that has not stepped yet (freshly created, or after restart_from_x0): for every chain (or
    `which`) the stored angles equal start_twin bit for bit, the generator words the oracle's, pstat_microstate the oracle's f64
    energy on those angles (microstate_ld: eap_chain_energy restated in longdouble), and steps, sums and windows are zero.  ops: the oracle's parameters of every case, holding
    the --x0 form the handle started from.  The microstate's bound: init_kernel derives r, p, U in f64 from the stored angles --
    1e-13 sum |terms|; the all-pairs homes then re-derive them in f32 (a launch of zero steps): the CARRIED TOTALS bound with
    no acceptance."""
    for c in (range(chains * len(cases)) if which is None else which):
        k, local = divmod(c, chains)
        st = e.chain_state(c)
        phi, th, rng = start_twin(oracle, ops[k], cases[k], local, precision)
        assert np.array_equal(st["phi"], phi), (c, st["phi"][:3], phi[:3])
        assert np.array_equal(st["theta"], th), (c, st["theta"][:3], th[:3])
        assert np.array_equal(st["rng"], rng), (c, st["rng"], rng)
        assert (st["nacc_total"], st["steps_recorded"], st["nacc_window"], st["natt_window"]) == (0, 0, 0, 0), c
        assert not st["sums"].any() and st["normalizer"] == 0.0, c
        assert st["phi_step"] == (ops[k].phi_step if phi_step is None else phi_step), c
        assert st["theta_step"] == (ops[k].theta_step if theta_step is None else theta_step), c
        lit, c1 = term_sums(cases[k], st["phi"], st["theta"])
        if cases[k]["energy_type"] in (INTERACTING, CUTOFF) and precision != F64:
            tol = carried(cases[k]["n"], 0, lit, c1)
        else:
            tol = 1e-13 * lit + 1e-300
        err = np.abs(e.microstate(c) - microstate_ld(cases[k], st["phi"], st["theta"], cluster)).astype(np.float64)
        assert np.all(err <= tol), (c, err / tol)


def _scale(p):
    return umbrella_scale(p) if p.get("umbrella") else None


def record_check(who, D, p, acc, block, launch, at, dev_sums, dev_norm, ncol, rise=False):
    """(d) for one chain: the device's sums read after the steps `at` (0-based) against the twin's prefixes.  D: the stepped
    handle's record of the chain (recs, usum0, start); acc, launch: record_bound's acc_since_launch and steps per launch.  Returns the worst error / bound of the
    16 columns and of the extras."""
    s = _scale(p)
    at = np.asarray(at)
    tw = record_twin(D["recs"], s, D["usum0"])
    B, margin = record_bound(D["recs"], p["n"], acc, block, s, D["usum0"], D["start"], launch)
    dev_sums, dev_norm = np.asarray(dev_sums)[:, :ncol], np.asarray(dev_norm)
    if s is None:
        assert np.array_equal(dev_norm, at + 1.0), f"{who}: normalizer {dev_norm[:4]} is not the number of steps recorded"
        got = dev_sums
    else:
        assert np.all(np.isfinite(dev_norm) & (dev_norm > 0)) and np.all(np.isfinite(dev_sums)), f"{who}: sums or normalizer not finite"
        got = dev_sums / dev_norm[:, None]
        assert launch > 1 or margin[at].max() <= GAUGE_MARGIN_MAX, (who, margin[at].max())      # (the stepped handle's margin)
        over = np.log(dev_norm / tw.nstar[at]) - (GAUGE_T + margin[at])
        assert np.all(over <= 0), (f"{who}: step {at[np.argmax(over > 0)] + 1}: the heaviest record weighs e^"
                                   f"{GAUGE_T + margin[at][np.argmax(over > 0)] + over.max():.3f} of the gauge")
        if rise:
            assert tw.top.max() >= RISE_MIN and tw.rises[-1] >= 1, (who, tw.top.max())
    worst = []
    for lo, hi in ((0, 16), (16, ncol)):
        q, msg = first_violation(got[:, lo:hi], tw.cols[at][:, lo:hi], B[at][:, lo:hi], at + 1, lo) if hi > lo else (0.0, None)
        assert msg is None, f"{who}: {msg}"
        worst.append(q)
    return worst
