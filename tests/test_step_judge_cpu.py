"""The one-step judge of the oracle (eap_step_judge, eap_step_judge_cluster) by itself, on the CPU:
  * it replays the oracle's runs bit for bit (accepted[], final angles, final generator words, adapted step sizes);
  * its d is the difference of eap_chain_energy plus the Jacobian terms, recomputed in numpy longdouble;
  * for every configuration the GPU tests use (tests/step_judge.py): the share of steps whose verdict lies within the margin
    is at most 0.5 %, and a judge whose E0 is off by 2^-8 is caught;
  * all of this under umbrella sampling too: there the judge replays eap_run_fast and eap_run_cluster, and d gains the weight
    function's difference, restated here;
  * the record twin (step_judge.record_twin) equals the oracle's own averages on the replayed states, and each wrong twin
    (W1 ... W4) leaves the derived record bound on the oracle's walk of every configuration it applies to;
  * the gauge-rise rows reach a start-gauged log-weight between 35 and 80.
"""
import itertools
import math

import numpy as np
import pytest

import step_judge as sj

LD = np.longdouble


def _cases():
    """Both mains x four energies x both chain types x both generators x flips / bending / cluster_prob x n."""
    out = []
    ns = (1, 2, 3, 33)
    k = 0
    for en, ct, g in itertools.product((sj.NONINTERACTING, sj.ISING, sj.INTERACTING), (sj.DIELECTRIC, sj.POLAR),
                                       (sj.MWC, sj.XOSHIRO)):
        n = ns[k % 4]
        k += 1
        phys = dict(E0=1.2, K1=1.0, K2=0.3, mu=0.9, Fz=0.7, Fx=0.4, b=1.1, kT=0.8 + 0.3 * (k % 3))
        out.append(("single", dict(n=n, energy_type=en, chain_type=ct, rng=g, do_flips=k % 2, seed=40 + k,
                                   steps_per_adjust=50, uniform_bits=(23, 0)[k % 2], **phys)))
    k = 0
    for en, ct, cp in itertools.product((sj.NONINTERACTING, sj.ISING, sj.INTERACTING, sj.CUTOFF), (sj.DIELECTRIC, sj.POLAR),
                                        (0.0, 0.5, 1.0)):
        n = ns[1 + k % 3]           # the clustering main needs n >= 2
        k += 1
        phys = dict(E0=1.2, K1=1.0, K2=0.3, mu=0.9, Fz=0.7, Fx=0.4, b=1.1, kT=0.8 + 0.3 * (k % 3))
        out.append(("cluster", dict(n=n, energy_type=en, chain_type=ct, rng=k % 2, cluster_prob=cp, seed=70 + k,
                                    bend_mod=0.6 * (k % 2), bend_angle=0.25, cutoff_radius=3.0, steps_per_adjust=50,
                                    uniform_bits=(23, 0)[k % 2], **phys)))
    # umbrella sampling, both mains: every third case again (each energy, chain type and generator at least once)
    out += [(m, dict(p, umbrella=1, seed=p["seed"] + 100)) for m, p in out[::3]]
    return out


CASES = _cases()
IDS = [f"{m}-{i}" for i, (m, _) in enumerate(CASES)]


def test_cases_cover_what_the_issue_lists():
    singles = [p for m, p in CASES if m == "single"]
    clusters = [p for m, p in CASES if m == "cluster"]
    assert {p["energy_type"] for p in clusters} == {0, 1, 2, 3} and {p["energy_type"] for p in singles} == {0, 1, 2}
    for group in (singles, clusters):
        assert {p["chain_type"] for p in group} == {0, 1} and {p["rng"] for p in group} == {0, 1}
        assert {p["n"] for p in group} >= {2, 3, 33}
    assert {p["n"] for p in singles} == {1, 2, 3, 33}
    assert {p["do_flips"] for p in singles} == {0, 1}
    assert {p["cluster_prob"] for p in clusters} == {0.0, 0.5, 1.0}
    assert {bool(p["bend_mod"]) for p in clusters} == {False, True}


@pytest.mark.parametrize("mode,p", CASES, ids=IDS)
def test_judge_replays_the_oracle_bit_for_bit(oracle, mode, p):
    nsteps = 400
    op = oracle.make_params(num_steps=nsteps, stepout=0, **p)
    run_mode = "cluster" if mode == "cluster" else ("fast" if p.get("umbrella") else "faithful")
    ref = oracle.run(op, chain_id=3, mode=run_mode, trace=True)
    W = sj.walk(oracle, op, 3, nsteps, cluster=mode == "cluster", rec_params=p)
    assert np.array_equal(W.accepted, ref.accepted[:nsteps])
    assert 0 < W.accepted.sum() < nsteps or p["n"] == 1
    assert np.array_equal(W.phi, ref.final_phi) and np.array_equal(W.theta, ref.final_theta)
    assert np.array_equal(W.rng, ref.rng)
    assert W.phi_step == ref.phi_step and W.theta_step == ref.theta_step
    # the record twin on the replayed states against the oracle's own averagers: sum / steps, or value / normaliser
    umb = bool(p.get("umbrella"))
    tw = sj.record_twin(W.recs, sj.umbrella_scale(p) if umb else None, W.usum0)
    ncol = 18 if mode == "cluster" else 16
    want = np.concatenate([ref.sums, ref.extra_sums])[:ncol] / ref.norm
    got = tw.cols[-1, :ncol] if umb else tw.cols[-1, :ncol] / nsteps
    assert umb or ref.norm == nsteps
    if np.isfinite(want).all() and ref.norm > 0:
        scale = np.abs(sj._columns(np.array([r.v for r in W.recs]), np.array([r.ex for r in W.recs]))).max(axis=0)[:ncol]
        assert np.all(np.abs(got - want) <= 1e-12 * np.maximum(np.abs(want), scale)), (got, want)
    else:
        assert umb      # the reference's a-priori gauge underflowed its normaliser; the twin's maximum gauge cannot
    assert not umb or (np.isfinite(tw.cols[-1, :ncol]).all() and 0 < tw.nstar[-1] <= nsteps)


def _log_sin(theta):
    with np.errstate(divide="ignore"):
        return np.log(np.sin(np.asarray(theta, dtype=LD)))


@pytest.mark.parametrize("mode,p", CASES, ids=IDS)
def test_d_is_the_energy_difference_plus_jacobian(oracle, mode, p):
    op = oracle.make_params(num_steps=120, stepout=0, **p)
    W = sj.walk(oracle, op, 5, 120, cluster=mode == "cluster", keep=True)
    phi, th, _ = oracle.seed_state(op, 5)
    seen_cluster = False
    for t, J in enumerate(W.steps):
        U0, _, _ = oracle.chain_energy(op, phi, th)
        U1, _, _ = oracle.chain_energy(op, J.trial_phi, J.trial_theta)
        assert U0 == J.U_cur and U1 == J.U_trial
        changed = np.nonzero((J.trial_phi != phi) | (J.trial_theta != th))[0]
        assert all(J.lower <= i <= J.upper for i in changed), (t, changed, J.lower, J.upper)
        assert J.lower <= J.idx <= J.upper
        sl = slice(J.lower, J.upper + 1)
        jac = (_log_sin(J.trial_theta[sl]) - _log_sin(th[sl])).sum()
        d = -(LD(U1) - LD(U0)) / LD(op.kT) + jac + LD(J.log_alpha)
        if p.get("umbrella"):       # the weight function's difference, on usum restated in numpy (step_judge.rec_of)
            us0 = sj.rec_of(oracle, op, p, phi, th, mode == "cluster", magnitudes=False).usum
            us1 = sj.rec_of(oracle, op, p, J.trial_phi, J.trial_theta, mode == "cluster", magnitudes=False).usum
            assert abs(us0 - J.usum_cur) <= 1e-12 * J.mag / sj.umbrella_scale(p)
            d += LD(sj.umbrella_scale(p)) * (LD(us1) - LD(us0))
        if math.isfinite(J.d):
            assert abs(LD(J.d) - d) <= 1e-12 * J.mag, (t, J.d, d, J.mag)
            assert J.mag >= 1 + abs(J.d) * (1 - 1e-9)          # |a signed sum| <= the sum of the |terms|
        else:
            assert not np.isfinite(d) or d < -700
        assert len(J.grow) == 0 or mode == "cluster"
        if J.flipped:
            seen_cluster = True
            assert np.array_equal(J.trial_theta[sl][np.arange(J.lower, J.upper + 1) != J.idx],
                                  np.clip(th[sl] + (math.pi - 2 * th[sl]), 0, math.pi)[np.arange(J.lower, J.upper + 1) != J.idx])
        assert np.all(J.grow[:, 2] == J.grow[:, 0] - J.grow[:, 1])
        if W.accepted[t]:
            if J.flipped and math.isfinite(J.log_alpha):      # log alpha recovered from the two states = the judge's
                got = sj.log_alpha_of_move(th, J.trial_theta, J.trial_phi, J.idx)
                assert abs(got - J.log_alpha) <= 1e-9 * (1 + abs(J.log_alpha)), (t, got, J.log_alpha)
            phi, th = J.trial_phi, J.trial_theta
    if mode == "cluster":
        assert seen_cluster == (p["cluster_prob"] < 1.0)


def test_moved_to_puts_the_monomer_where_it_is_told(oracle):
    op = oracle.make_params(num_steps=0, stepout=0, n=5, E0=1.0, Fz=0.5, seed=3)
    phi, th, rng = oracle.seed_state(op, 0)
    free = oracle.step_judge(op, phi, th, rng, op.phi_step, op.theta_step)
    J = oracle.step_judge(op, phi, th, rng, op.phi_step, op.theta_step, moved_to=(1.25, 0.75))
    assert J.idx == free.idx and np.array_equal(J.rng, free.rng) and J.eps == free.eps
    assert abs(J.trial_phi[J.idx] - 1.25) < 1e-15 and abs(J.trial_theta[J.idx] - 0.75) < 1e-15


def test_q16_displacement_rule():
    """The integer restatement against the float expression it restates, including the ties at +-1/2 cell."""
    unit = math.pi / 65536.0
    step = 12288.0 * unit                            # the default theta_step: exactly 12288 cells
    for m, want in ((1 << 22, 0), ((1 << 22) + 512, 2), ((1 << 22) - 512, -2), (0, -12288), ((1 << 23) - 1, 12288)):
        assert sj.q16_disp(step, unit, m << 9) == want, m
    # ties: s = +-1/2 exactly, a step of an odd number of cells
    assert sj.q16_disp(1.0 * unit, unit, ((1 << 22) + (1 << 21)) << 9) == 0      # 0.5 -> 0 (even)
    assert sj.q16_disp(3.0 * unit, unit, ((1 << 22) + (1 << 21)) << 9) == 2      # 1.5 -> 2 (even)
    assert sj.q16_disp(1.0 * unit, unit, ((1 << 22) - (1 << 21)) << 9) == 0      # -0.5 -> 0
    assert sj.q16_disp(3.0 * unit, unit, ((1 << 22) - (1 << 21)) << 9) == -2     # -1.5 -> -2
    # against the float expression itself: step (f32) * s is exact in f64 (24 x 23 bits), rint rounds half to even like the fma
    rng = np.random.default_rng(5)
    for w, st in zip(rng.integers(0, 1 << 32, 2000), rng.uniform(0.01, math.pi / 2, 2000)):
        s_ = np.float64(np.float32(np.uint32((int(w) >> 9) | 0x40000000).view(np.float32) - np.float32(3.0)))
        assert sj.q16_disp(st, unit, int(w)) == int(np.rint(np.float64(np.float32(st / unit)) * s_)), (w, st)
    k, j = sj.lattice([sj.lattice_theta(0), sj.lattice_theta(65535)], [sj.lattice_phi(0), sj.lattice_phi(65535)])
    assert list(k) == [0, 65535] and list(j) == [0, 65535]


# ---------------------------------------------------------------- the conditions on the GPU tests' configurations

def test_configurations_stay_inside_the_margin_derivation():
    """C_VERDICT's derivation assumes single-monomer coefficients of at most MAX_COEFFICIENT_OVER_KT kT -- under umbrella
    sampling with wscale c counted in, as the net coefficient |1 / kT - wscale| c that (d') of the derivation states, which
    needs 0 < wscale kT <= 1."""
    packed = [dict(sj.PACKED_COMMON, **c, umbrella=u) for c in sj.PACKED_CASES for u in (0, 1)]
    for name, p in [(cfg.name, cfg.params) for cfg in sj.CONFIGS] + [("packed", p) for p in packed]:
        assert sj.coefficient_over_kT(p) <= sj.MAX_COEFFICIENT_OVER_KT, name
        if p.get("umbrella"):
            assert 0.0 < sj.umbrella_scale(p) * p["kT"] <= 1.0, name
            # (the plain coefficient bounds the net one: counting the weight in never raises it, except for UCutoff)
            assert p["energy_type"] == sj.CUTOFF or sj.coefficient_over_kT(p) <= sj.coefficient_over_kT(dict(p, umbrella=0)), name
    names = " ".join(sj.CONFIG_IDS)
    for must in ("f32-sweep", "q16-sweep", "f32lds-cluster", "q16lds-cluster", "f32mem-cluster", "f32-allpairs-n23",
                 "f32-allpairs-n64", "f32-allpairs-n100", "f32-allpairs-n130", "allpairs-cluster-n20-interacting",
                 "allpairs-cluster-n64-cutoff", "f32-allpairs-n200", "f32-allpairs-n257", "allpairs-cluster-n100-interacting",
                 "allpairs-cluster-n200-cutoff", "allpairs-cluster-n400-cutoff", "allpairs-cluster-n130-interacting"):
        assert must in names
    # the umbrella rows: every kernel family, the listed sizes, one gauge-rise row per family
    umb = [c for c in sj.CONFIGS if c.params.get("umbrella")]
    assert all("-umb-" in c.name or "-rise-" in c.name for c in umb) and len(umb) == sum("-umb-" in n or "-rise-" in n for n in sj.CONFIG_IDS)
    for kern, sizes in (("sweep_kernel<float>", {1, 3, 20}), ("sweep_kernel<float, q16 state>", {1, 3, 20}),
                        ("cluster_kernel<float>", {2, 20}), ("cluster_kernel<float, q16 state>", {2, 20}),
                        ("cluster_kernel<float, state in memory>", {2, 20}), ("interacting_kernel<float>", {23, 130}),
                        ("cluster_wave_kernel<float>", {20, 64, 130})):
        rows = [c for c in umb if c.kernel == kern]
        assert {c.params["n"] for c in rows} >= sizes, kern
    for kern in ("sweep_kernel<float>", "cluster_kernel<float>", "cluster_kernel<float, state in memory>",
                 "interacting_kernel<float>", "cluster_wave_kernel<float>"):
        assert any(c.kernel == kern and c.name in sj.RISE_IDS for c in umb), kern
    for group in ("umb-sweep", "umb-cluster"):
        rows = [c.params for c in umb if group in c.name]
        assert {p["chain_type"] for p in rows} == {0, 1} and {p["rng"] for p in rows} == {0, 1}
        assert {p.get("adj_scale", 1.1) != 1.0 for p in rows} == {False, True}
    assert {bool(c.params["bend_mod"]) for c in umb if "umb-cluster" in c.name} == {False, True}
    assert all(c.params["cluster_prob"] == 0.5 for c in umb if c.cluster)
    assert all(c.chains <= 6 for c in umb if "allpairs" in c.name) and all(c.chains == 70 for c in umb if "allpairs" not in c.name)


_WALKS = {}      # configuration name -> what the oracle's own walk of its judged chains gave (walked once, used by three tests)


def _walk_config(oracle, cfg):
    if cfg.name in _WALKS:
        return _WALKS[cfg.name]
    op = sj.oracle_params(oracle, cfg.params)
    tot = dict(undecided=0, decided=0, wrong=0, steps=0, walks=[])
    all_pairs = cfg.params["energy_type"] in (sj.INTERACTING, sj.CUTOFF)

    def no_contact(phi, theta):
        assert sj.min_pair_distance(cfg.params, phi, theta) >= sj.CONTACT_DISTANCE, cfg.name

    for c in cfg.judged():
        W = sj.walk(oracle, op, c, cfg.T, cfg.cluster, judge_op=sj.perturbed(oracle, cfg.params),
                    precision=cfg.precision if cfg.precision == sj.Q16 else None, probe=no_contact if all_pairs else None,
                    rec_params=cfg.params)
        tot["undecided"] += W.undecided
        tot["decided"] += W.decided
        tot["wrong"] += W.wrong
        tot["steps"] += len(W.accepted)
        tot["walks"].append(W)
    _WALKS[cfg.name] = tot
    return tot


@pytest.mark.parametrize("cfg", sj.CONFIGS, ids=sj.CONFIG_IDS)
def test_reference_alone_undecided_share_and_teeth(oracle, cfg):
    """Judged chains, run length and margin of the GPU test; the judge alone.  (1) at most 0.5 % of the steps are undecided;
    (2) judged by a judge whose E0 is multiplied by 1 + 2^-8, the oracle's own trajectory shows at least one wrong step."""
    tot = _walk_config(oracle, cfg)
    share = tot["undecided"] / tot["steps"]
    print(f"{cfg.name}: steps {tot['steps']}, undecided {tot['undecided']} ({100 * share:.3f} %), "
          f"wrong under E0 (1 + 2^-8): {tot['wrong']}")
    assert share <= 0.005, (cfg.name, share)
    assert tot["wrong"] >= 1, cfg.name


def _launch_accepts(accepted, every):
    """acc_since_launch of record_bound for launches of `every` steps."""
    ca = np.cumsum(accepted)
    return ca - np.concatenate([[0], ca])[(np.arange(len(ca)) // every) * every]


@pytest.mark.parametrize("cfg", sj.CONFIGS, ids=sj.CONFIG_IDS)
def test_wrong_twins_leave_the_record_bound(oracle, cfg):
    """On the oracle's own walk each applicable wrong twin differs from the right one by more than the derived bound in at
    least one column and prefix, on at least one judged chain.  W1 (scale), W2 (trial recorded on a rejected step) and W4
    (extras not rescaled at a gauge rise) against the bound of the stepped handle, at every step; W3 (a block's first record
    dropped) against the bound of the launches of 64, after each launch -- the stepped handle has no blocks."""
    tot = _walk_config(oracle, cfg)
    umb = bool(cfg.params.get("umbrella"))
    s = sj.umbrella_scale(cfg.params) if umb else None
    n = cfg.params["n"]
    kinds = ["W2", "W3"] + (["W1"] if umb else []) + (["W4"] if cfg.cluster and cfg.name in sj.RISE_IDS else [])
    worst = {k: 0.0 for k in kinds}
    for W in tot["walks"]:
        T = len(W.recs)
        right = sj.record_twin(W.recs, s, W.usum0)
        stepped, _ = sj.record_bound(W.recs, n, np.ones(T), 1, s, W.usum0, W.start, 1)
        by64, _ = sj.record_bound(W.recs, n, _launch_accepts(W.accepted, 64), 64, s, W.usum0, W.start, 64)
        ends = np.arange(63, T, 64)
        for k in kinds:
            wrong = sj.record_twin(W.recs, s, W.usum0, wrong=k, trial=W.trials, accepted=W.accepted)
            if k == "W3":
                q, _ = sj.first_violation(wrong.cols[ends], right.cols[ends], by64[ends])
            else:
                q, _ = sj.first_violation(wrong.cols, right.cols, stepped)
            worst[k] = max(worst[k], q)
    print(f"{cfg.name}: largest difference / bound of the wrong twins {worst}")
    for k in kinds:
        assert worst[k] > 1.0, (cfg.name, k, worst[k])


@pytest.mark.parametrize("cfg", [c for c in sj.CONFIGS if c.name in sj.RISE_IDS], ids=sj.RISE_IDS)
def test_gauge_rise_rows_reach_their_limits(oracle, cfg):
    """Every judged chain's heaviest record, gauged on the start configuration, reaches a log-weight of at least RISE_MIN = 35
    and at most RISE_MAX = 80 within T, with records behind it when the gauge first rises; and the margin of the GPU test's
    gauge contract, the derived relative error of the normaliser, stays far below 1."""
    tot = _walk_config(oracle, cfg)
    s = sj.umbrella_scale(cfg.params)
    for W in tot["walks"]:
        tw = sj.record_twin(W.recs, s, W.usum0)
        assert sj.RISE_MIN <= tw.top.max() <= sj.RISE_MAX, (cfg.name, tw.top.max())
        assert tw.rises[-1] >= 1 and tw.rises[0] == 0, (cfg.name, tw.rises[0], tw.rises[-1])
        for acc, block, launch in ((np.ones(cfg.T), 1, 1), (np.cumsum(W.accepted), sj.FLUSH, cfg.T)):
            _, w_err = sj.record_bound(W.recs, cfg.params["n"], acc, block, s, W.usum0, W.start, launch)
            assert w_err.max() <= sj.GAUGE_MARGIN_MAX, (cfg.name, block, w_err.max())


@pytest.mark.parametrize("prec", [None, sj.Q16], ids=["f32", "q16"])
def test_packed_cases_undecided_share_and_teeth(oracle, prec):
    """The packed handle of the GPU test: chains 0, 1, 63, 64 of 13 cases x 5 chains (cases 0 and 12)."""
    _packed_cases(oracle, prec, 0)


def test_packed_cases_under_umbrella_sampling(oracle):
    _packed_cases(oracle, None, 1)


def _packed_cases(oracle, prec, umbrella):
    und = steps = wrong = 0
    worst = {"W2": 0.0, "W3": 0.0, **({"W1": 0.0} if umbrella else {})}
    for c in (0, 1, 63, 64):
        i = c // 5
        p = dict(sj.PACKED_COMMON, seed=500 + i, **sj.PACKED_CASES[i], umbrella=umbrella)
        W = sj.walk(oracle, sj.oracle_params(oracle, p), c % 5, sj.PACKED_T, False, judge_op=sj.perturbed(oracle, p), precision=prec,
                    rec_params=p)
        und += W.undecided
        steps += len(W.accepted)
        wrong += W.wrong
        s = sj.umbrella_scale(p) if umbrella else None
        right = sj.record_twin(W.recs, s, W.usum0)
        stepped, _ = sj.record_bound(W.recs, p["n"], np.ones(sj.PACKED_T), 1, s, W.usum0, W.start, 1)
        by64, _ = sj.record_bound(W.recs, p["n"], _launch_accepts(W.accepted, 64), 64, s, W.usum0, W.start, 64)
        ends = np.arange(63, sj.PACKED_T, 64)
        for k in worst:
            tb = sj.record_twin(W.recs, s, W.usum0, wrong=k, trial=W.trials, accepted=W.accepted)
            q, _ = sj.first_violation(tb.cols[ends], right.cols[ends], by64[ends]) if k == "W3" else \
                sj.first_violation(tb.cols, right.cols, stepped)
            worst[k] = max(worst[k], q)
    print(f"packed: steps {steps}, undecided {und} ({100 * und / steps:.3f} %), wrong under E0 (1 + 2^-8): {wrong}; wrong twins {worst}")
    assert und / steps <= 0.005
    assert wrong >= 1
    assert all(v > 1.0 for v in worst.values()), worst
