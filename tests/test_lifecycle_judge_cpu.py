"""What happens to a handle BETWEEN the launches, with the oracle alone on the CPU (tests/step_judge.py, "between the launches"):
  * replay: the walk with events (eap_reinit_judge between eap_step_judge steps) reproduces oracle.run(num_inits, force_init)
    bit for bit -- accepted[], final angles, generator words, nacc_total, step sizes -- for the options of every fixed-force
    LIFECYCLE row, forced and Metropolis: the new judge is pinned against the C run loops, not against itself;
  * start: start_twin at f64 equals oracle.seed_state bit for bit, the --x0 forms included; the f32 start IS the oracle's
    start without --x0, and lies within one rounding of it with; the q16 start is the lattice cell that holds the oracle's;
  * caps, per LIFECYCLE row with the judge alone: at most 0.5 % of the post-event steps undecided; over the table at most 2 %
    of the re-init verdicts undecided;
  * coverage: adopted and refused Metropolis re-inits and a thawing chain in every n <= 3 row, a frozen chain in every n >= 33
    row, both outcomes of the "forced, then Metropolis at once" pair over the table;
  * teeth: a twin that clears the lag at the re-init is caught in every n <= 3 row, a twin that leaves the umbrella term out
    of the lag in every umbrella row, a judge with E0 (1 + 2^-8) in the post-event steps of the table.
"""
import numpy as np
import pytest

import step_judge as sj

FIXED = [c for c in sj.LIFECYCLE if not c.cluster]
FIXED_IDS = [c.name for c in FIXED]


# ------------------------------------------------------------------------------------------------------------ replay

def _replay_rows():
    """The option dicts of the fixed-force rows, once each (f32 and q16 rows share theirs), plus the packed handle's first
    and last case."""
    seen, out = set(), []
    for cfg in FIXED:
        for p in (cfg.cases[0], cfg.cases[-1]) if cfg.cases else (cfg.params,):
            key = tuple(sorted((k, v) for k, v in p.items()))
            if key not in seen:
                seen.add(key)
                out.append((cfg.name.split("-", 2)[2] + (f"-seed{p['seed']}" if cfg.cases else ""), p))
    return out


REPLAY = _replay_rows()


@pytest.mark.parametrize("forced", [True, False], ids=["forced", "metropolis"])
@pytest.mark.parametrize("name,p", REPLAY, ids=[r[0] for r in REPLAY])
def test_walk_with_events_replays_the_run_loops(oracle, name, p, forced):
    seg, inits = 120, 4
    kind = "reinit_forced" if forced else "reinit_metropolis"
    events = [(k * seg, kind) for k in range(1, inits)]
    allp = p["energy_type"] == sj.INTERACTING
    lags = []
    for bits in (23, 0):
        q = {k: v for k, v in p.items() if not (allp and k in sj._X0)}     # (eap_run_fast has no --x0: the all-pairs rows replay
        op = oracle.make_params(num_steps=seg, num_inits=inits, force_init=int(forced), stepout=0, uniform_bits=bits, **q)  # from the uniform start)
        for chain in (0, 3):
            W = sj.walk(oracle, op, chain, seg * inits, False, events=events, params=q)
            for mode in ("fast",) if p.get("umbrella") else ("faithful", "fast"):      # (eap_run_faithful's weight has an a-priori gauge
                ref = oracle.run(op, chain_id=chain, mode=mode, trace=True)            #  that may underflow; its decisions are eap_run_fast's)
                assert np.array_equal(W.accepted, ref.accepted[:seg * inits]), (mode, np.nonzero(W.accepted != ref.accepted[:seg * inits])[0][:5])
                assert np.array_equal(W.phi, ref.final_phi) and np.array_equal(W.theta, ref.final_theta), mode
                assert np.array_equal(W.rng, ref.rng) and int(W.accepted.sum()) == ref.nacc_total, mode
                assert W.phi_step == ref.phi_step and W.theta_step == ref.theta_step, mode
            assert len(W.events) == inits - 1 and all(E.J.forced == forced for E in W.events)
            lags += [E.J.lag_out for E in W.events if E.J.adopt]
    assert not forced or any(abs(x) > 0.1 for x in lags), name


def test_metropolis_reinits_of_the_replay_rows_show_both_outcomes(oracle):
    """A row by itself may adopt never -- an equilibrated chain rarely takes a uniform draw -- so both outcomes are asserted over
    the replay rows, on walks of this test's own (the schedule of the replay above)."""
    seg, inits = 120, 4
    adopted = refused = 0
    for _, p in REPLAY:
        q = {k: v for k, v in p.items() if not (p["energy_type"] == sj.INTERACTING and k in sj._X0)}
        op = oracle.make_params(num_steps=seg, num_inits=inits, stepout=0, uniform_bits=23, **q)
        for chain in (0, 3):
            W = sj.walk(oracle, op, chain, seg * inits, False, events=[(k * seg, "reinit_metropolis") for k in range(1, inits)], params=q)
            adopted += sum(E.J.adopt for E in W.events)
            refused += sum(not E.J.adopt for E in W.events)
    assert adopted >= 10 and refused >= 10, (adopted, refused)


def test_reinit_judge_fields(oracle):
    """d, lag_out and the words of one judged re-init against their definitions, restated in numpy longdouble."""
    LD = np.longdouble
    for umbrella, force in ((0, 0), (1, 0), (1, 1)):
        p = dict(n=5, energy_type=sj.ISING, chain_type=sj.DIELECTRIC, E0=3.0, K1=0.6, K2=0.2, Fz=0.5, Fx=0.3, b=1.1, kT=0.9, seed=11,
                 umbrella=umbrella)
        op = sj.oracle_params(oracle, p)
        phi, th, rng = oracle.seed_state(op, 2)
        J = oracle.reinit_judge(op, phi, th, rng, lag_in=0.75, force=bool(force))
        fp, ft = sj.stored_uniform(*sj.fresh_words(oracle, op, rng), sj.F64)
        assert np.array_equal(fp, J.fresh_phi) and np.array_equal(ft, J.fresh_theta)
        U0, _, _ = oracle.chain_energy(op, phi, th)
        U1, _, _ = oracle.chain_energy(op, fp, ft)
        assert (U0, U1) == (J.U_cur, J.U_fresh)
        ls0, ls1 = np.log(np.sin(th.astype(LD))).sum(), np.log(np.sin(ft.astype(LD))).sum()
        d = -(LD(U1) - LD(U0)) / LD(p["kT"]) + ls1 - ls0
        assert abs(LD(J.d) - d) <= 1e-13 * J.mag and J.mag >= 1 + abs(J.d) + 0.75 - 1e-9
        s = (sj.umbrella_scale(p) if umbrella else 0.0)
        us0 = sj.rec_of(oracle, op, p, phi, th, False, magnitudes=False).usum
        us1 = sj.rec_of(oracle, op, p, fp, ft, False, magnitudes=False).usum
        assert abs(us0 - J.usum_cur) <= 1e-12 * (1 + abs(us0)) and abs(us1 - J.usum_fresh) <= 1e-12 * (1 + abs(us1))
        lag = (-LD(U0) / LD(p["kT"]) + ls0 + LD(s) * LD(us0) + LD(0.75)) - (-LD(U1) / LD(p["kT"]) + ls1 + LD(s) * LD(us1))
        # the words: 2n draws, one more for eps unless forced
        import ctypes as C
        w = (C.c_uint32 * 4)(*[int(x) for x in rng])
        for _ in range(2 * p["n"] + (0 if force else 1)):
            last = sj._next_word(oracle, op.rng, w)
        assert np.array_equal(np.array(w[:], dtype=np.uint32), J.rng)
        if force:
            assert J.adopt and J.eps == 0.0
        else:
            assert J.eps == (last >> 9) * 2.0 ** -23
            assert abs(d - np.log(LD(J.eps))) < 1e-9 or J.adopt == bool(np.log(LD(J.eps)) <= d)
        assert abs(LD(J.lag_out) - (lag if J.adopt else LD(0.75))) <= 1e-12 * J.mag
    # neither UCutoff nor (through the binding's fixed-force entry) anything but the fixed-force main
    with pytest.raises(RuntimeError):
        oracle.reinit_judge(sj.oracle_params(oracle, dict(p, energy_type=sj.CUTOFF)), phi, th, rng)


# ------------------------------------------------------------------------------------------------------------- start

def _start_rows():
    rows = [(c.name, c.params) for c in FIXED if not c.cases]
    rows += [(c.name, c.params) for c in sj.CONFIGS if c.params.get("use_x0")]        # the scalar --x0 rows
    rng = np.random.default_rng(7)
    for n, g in ((3, sj.MWC), (20, sj.XOSHIRO)):                                      # the per-monomer form
        vec = np.stack([rng.uniform(-7.0, 7.0, n), rng.uniform(-0.2, 3.3, n)], axis=1).ravel()
        rows.append((f"x0-vec-n{n}", dict(n=n, energy_type=sj.NONINTERACTING, chain_type=sj.POLAR, E0=1.0, mu=0.3, kT=1.0, rng=g,
                                          seed=77 + n, x0_vec=vec, dx0_phi=0.7, dx0_theta=0.2)))
    return rows


START = _start_rows()


@pytest.mark.parametrize("name,p", START, ids=[r[0] for r in START])
def test_start_twin_against_the_seeded_start(oracle, name, p):
    op = sj.oracle_params(oracle, p)
    for chain in (0, 1, 64, 69):
        phi, th, rng = oracle.seed_state(op, chain)
        tp, tt, tr = sj.start_twin(oracle, op, p, chain, sj.F64)
        assert np.array_equal(tp, phi) and np.array_equal(tt, th) and np.array_equal(tr, rng)
        fp, ft, fr = sj.start_twin(oracle, op, p, chain, sj.F32)
        qp, qt, qr = sj.start_twin(oracle, op, p, chain, sj.Q16)
        assert np.array_equal(fr, rng) and np.array_equal(qr, rng)
        turns = lambda a, b: np.abs((a - b) / (2 * np.pi) - np.rint((a - b) / (2 * np.pi)))
        if not op.use_x0:
            assert np.array_equal(fp, phi) and np.array_equal(ft, th)          # the f32 start IS the oracle's
            assert np.all(turns(qp, phi) <= 2.0 ** -17 + 1e-15) and np.all(np.abs(qt - th) / np.pi <= 2.0 ** -17 + 1e-15)
        else:
            assert np.all(turns(fp, phi) <= 2.0 ** -25 + 1e-15)               # one rounding of a number below 1
            assert np.all(np.abs(ft - th) / (2 * np.pi) <= 2.0 ** -25 * np.maximum(1.0, np.abs(th) / np.pi) + 1e-15)
            assert np.all(turns(qp, phi) <= 2.0 ** -17 + 1e-12)
            inside = (th >= 0) & (th < np.pi)
            assert np.all(np.abs(qt - th)[inside] / np.pi <= 2.0 ** -17 + 1e-12)
            k, _ = sj.lattice(qt, qp)
            assert np.all(k[th < 0] == 0) and np.all(k[th >= np.pi] == 65535)


# ----------------------------------------------------------------------------------- caps, coverage, teeth: the table

_LIFE = {}


def _walk_row(oracle, cfg):
    if cfg.name in _LIFE:
        return _LIFE[cfg.name]
    tot = dict(post=0, undecided=0, wrong_perturbed=0, wrong_zero=0, wrong_noumb=0, caught=0, events=[], segments=[])
    for c in cfg.judged():
        p, local = cfg.case_of(c)
        op = sj.oracle_params(oracle, p)
        W = sj.walk(oracle, op, local, cfg.T, cfg.cluster, judge_op=sj.perturbed(oracle, p), precision=cfg.precision, params=p,
                    events=cfg.events, wrong_lag="zero")
        tot["post"] += W.post_steps
        tot["undecided"] += W.post_undecided
        tot["wrong_perturbed"] += W.post_wrong
        tot["caught"] += W.wrong
        tot["wrong_zero"] += W.wrong_lag
        if p.get("umbrella"):
            tot["wrong_noumb"] += sj.walk(oracle, op, local, cfg.T, cfg.cluster, precision=cfg.precision, params=p, events=cfg.events,
                                          wrong_lag="no_umbrella").wrong_lag
        tot["events"].append(W.events)
        cuts = [0] + sorted({e[0] for e in cfg.events}) + [cfg.T]
        tot["segments"].append([int(W.accepted[a:b].sum()) for a, b in zip(cuts[:-1], cuts[1:])])
    _LIFE[cfg.name] = tot
    return tot


@pytest.mark.parametrize("cfg", FIXED, ids=FIXED_IDS)
def test_row_caps_coverage_and_lag_teeth(oracle, cfg):
    tot = _walk_row(oracle, cfg)
    n = cfg.params["n"]
    print(f"{cfg.name}: post-event steps {tot['post']}, undecided {tot['undecided']}; wrong under E0 (1 + 2^-8) {tot['wrong_perturbed']}, "
          f"under lag = 0 {tot['wrong_zero']}, without the umbrella term {tot['wrong_noumb']}; accepted per segment {tot['segments']}")
    assert tot["post"] == len(cfg.judged()) * (cfg.T - sj.SEGMENT)
    assert tot["undecided"] <= 0.005 * tot["post"], cfg.name
    assert tot["caught"] >= 2, cfg.name        # the judge with E0 (1 + 2^-8), over the row's whole schedule: THE SEEDS
    metro = [E.V.kind for ev in tot["events"] for E in ev if E.kind == "reinit_metropolis"]
    assert "undecided" not in metro, cfg.name
    after_forced = [s[1] for s in tot["segments"]]          # the segment after the first, forced re-init
    if n <= 3:
        assert "accept" in metro and "reject" in metro, (cfg.name, metro)
        assert max(after_forced) >= 5, (cfg.name, after_forced)
        assert tot["wrong_zero"] >= 5, cfg.name
    if n >= 33:
        assert min(after_forced) == 0, (cfg.name, after_forced)
    if cfg.params.get("umbrella"):
        assert tot["wrong_noumb"] >= 2, cfg.name
    # every forced re-init is adopted, and every event's words moved on by 2n (+ 1) draws: the walk's own bookkeeping
    for ev in tot["events"]:
        assert [E.kind for E in ev] == [e[1] for e in cfg.events]
        assert all(E.J.adopt for E in ev if E.kind == "reinit_forced")


CLUSTER = [c for c in sj.LIFECYCLE if c.cluster]


@pytest.mark.parametrize("cfg", CLUSTER, ids=[c.name for c in CLUSTER])
def test_cluster_row_caps(oracle, cfg):
    """The ladder rows with the judge alone: at most 0.5 % of the post-event steps undecided; the walk went through both rungs
    and the restart (its states after them are the ones the events define)."""
    tot = _walk_row(oracle, cfg)
    print(f"{cfg.name}: post-event steps {tot['post']}, undecided {tot['undecided']}; wrong under E0 (1 + 2^-8) {tot['wrong_perturbed']}; "
          f"accepted per segment {tot['segments']}")
    assert tot["undecided"] <= 0.005 * tot["post"], cfg.name
    assert tot["caught"] >= 2, cfg.name        # the judge with E0 (1 + 2^-8), over the row's whole schedule: THE SEEDS
    op = sj.oracle_params(oracle, cfg.params)
    for c, ev in zip(cfg.judged(), tot["events"]):
        assert [E.kind for E in ev] == ["rung", "rung", "x0"]
        base = {k: v for k, v in cfg.params.items() if k not in ("use_x0", "x0_phi", "x0_theta", "dx0_phi", "dx0_theta")}
        xop = sj.oracle_params(oracle, base, x0_vec=cfg.events[2][2], dx0_phi=cfg.events[2][3], dx0_theta=cfg.events[2][4])
        phi, th, rng = sj.start_twin(oracle, xop, None, c, cfg.precision)
        assert np.array_equal(ev[2].phi, phi) and np.array_equal(ev[2].theta, th) and np.array_equal(ev[2].rng, rng)
    assert all(max(s[k] for s in tot["segments"]) > 0 for k in range(4)), tot["segments"]


@pytest.mark.parametrize("p", [dict(n=3, energy_type=sj.ISING, chain_type=sj.DIELECTRIC, E0=2.0, K1=0.6, K2=0.2, Fz=0.5, kT=0.8, seed=5,
                                    cluster_prob=0.5, bend_mod=0.4, bend_angle=0.2, rng=sj.MWC, steps_per_adjust=50),
                               dict(n=20, energy_type=sj.NONINTERACTING, chain_type=sj.POLAR, E0=4.0, mu=0.5, Fz=0.5, Fx=0.2, kT=1.1, seed=6,
                                    cluster_prob=0.0, rng=sj.XOSHIRO, steps_per_adjust=50, umbrella=1)], ids=["n3-ising", "n20-ni-umbrella"])
def test_walk_with_rungs_replays_the_burn_in_ladder(oracle, p):
    """A rung event is one fresh mcmc() call of the clustering main: the walk with rungs reproduces eap_run_cluster's ladder."""
    burn, steps, sched = 120, 150, [10.0, 3.0]
    op = oracle.make_params(num_steps=steps, burn_in=burn, burn_sched=sched, stepout=0, uniform_bits=23, **p)
    ref = oracle.run(op, chain_id=2, mode="cluster", trace=True)
    T = 2 * burn + steps
    W = sj.walk(oracle, sj.oracle_params(oracle, p), 2, T, True, params=p,
                events=[(0, "rung", sched[0]), (burn, "rung", sched[1]), (2 * burn, "rung", 1.0)])
    assert np.array_equal(W.accepted, ref.accepted[:T])
    assert np.array_equal(W.phi, ref.final_phi) and np.array_equal(W.theta, ref.final_theta) and np.array_equal(W.rng, ref.rng)
    assert (W.phi_step, W.theta_step) == (ref.phi_step, ref.theta_step) and int(W.accepted[2 * burn:].sum()) == ref.nacc_total


def test_table_caps_coverage_and_teeth(oracle):
    verdicts = pair = 0
    undecided = wrong = 0
    both = set()
    for cfg in CLUSTER:
        wrong += _walk_row(oracle, cfg)["wrong_perturbed"]
    for cfg in FIXED:
        tot = _walk_row(oracle, cfg)
        wrong += tot["wrong_perturbed"]
        for ev in tot["events"]:
            metro = [E for E in ev if E.kind == "reinit_metropolis"]
            if not metro:
                continue        # (the n = 100 all-pairs row: forced re-inits only)
            verdicts += len(metro)
            undecided += sum(E.V.kind == "undecided" for E in metro)
            both.add(metro[-1].V.kind)          # the Metropolis re-init that follows a forced one at once
            pair += 1
    print(f"re-init verdicts {verdicts}, undecided {undecided}; the forced-then-Metropolis pair: {sorted(both)} over {pair} chains; "
          f"wrong under E0 (1 + 2^-8) in the post-event steps of the table: {wrong}")
    assert undecided <= 0.02 * verdicts
    assert {"accept", "reject"} <= both
    assert wrong >= 1


def test_no_fresh_draw_of_the_long_all_pairs_row_holds_a_deep_contact(oracle):
    """Every chain's three forced draws at n = 100 (their words depend on the step count alone: 2n for the start, 5 per step
    with --do-flips, 2n per re-init): the largest pair term |mu|^2 / (4 pi r^3) stays below 1 kT, so that the f32 pair sum of a
    long launch and of one-step launches cannot part ways over it."""
    cfg = [c for c in FIXED if c.name == "life-f32-allpairs-n100"][0]
    p, n = cfg.params, cfg.params["n"]
    assert p["chain_type"] == sj.POLAR and p["do_flips"] and cfg.chains == 6
    op = sj.oracle_params(oracle, p)
    for c in range(cfg.chains):
        s = sj._seed_words(oracle, op, c)
        for _ in range(2 * n):
            sj._next_word(oracle, op.rng, s)
        for _ in cfg.events:
            for _ in range(5 * sj.SEGMENT):
                sj._next_word(oracle, op.rng, s)
            w = np.array([sj._next_word(oracle, op.rng, s) for _ in range(2 * n)], dtype=np.uint64)
            phi, th = sj.stored_uniform(w[:n], w[n:], sj.F32)
            r = sj.min_pair_distance(p, phi, th) * p["b"]
            assert p["mu"] ** 2 / (4 * np.pi * r ** 3) <= p["kT"], (c, r)
    # (the judged chains' walk agrees on those words)
    tot = _walk_row(oracle, cfg)
    assert all(E.J.adopt for ev in tot["events"] for E in ev)


def test_lifecycle_table_is_what_the_issue_lists():
    names = " ".join(sj.LIFECYCLE_IDS)
    for prec in ("f32", "q16"):
        for n in (1, 2, 3):
            rows = [c for c in sj.LIFECYCLE if c.name.startswith(f"life-{prec}-sweep-n{n}-")]
            assert {c.params["energy_type"] for c in rows} == {sj.NONINTERACTING, sj.ISING}, (prec, n)
        sweep = [c.params for c in sj.LIFECYCLE if c.name.startswith(f"life-{prec}-sweep-n")]
        assert {p["chain_type"] for p in sweep} == {0, 1} and {p["rng"] for p in sweep} == {0, 1}
        assert {p["n"] for p in sweep} == {1, 2, 3, 33, 40}
        assert f"life-{prec}-umb-sweep-n1-" in names and f"life-{prec}-umb-sweep-n3-" in names
    assert "life-f32-packed" in names
    for home, kern in (("f32lds", "cluster_kernel<float>"), ("q16lds", "cluster_kernel<float, q16 state>"),
                       ("f32mem", "cluster_kernel<float, state in memory>")):
        rows = [c for c in CLUSTER if c.name.startswith(f"life-{home}-cluster-")]
        assert all(c.kernel == kern and c.chains == 70 and c.T == 4 * sj.SEGMENT for c in rows)
        assert {(c.params["n"], c.params["energy_type"]) for c in rows} == {(3, sj.NONINTERACTING), (3, sj.ISING), (20, sj.NONINTERACTING),
                                                                            (20, sj.ISING)}
        assert all([e[1:3] for e in c.events[:2]] == [("rung", 10.0), ("rung", 1.0)] and c.events[2][1] == "x0" for c in rows)
    ap = [c for c in FIXED if c.kernel == "interacting_kernel<float>"]
    assert [c.params["n"] for c in ap] == [2, 3, 5, 100] and all(c.params["use_x0"] for c in ap)
    assert 64 < ap[-1].params["n"] <= 128          # M = 2 (pstat_interacting.hip chooses M from n alone); M = 1 below 65
    assert [e[1] for e in ap[-1].events] == ["reinit_forced"] * 3 and [e[0] for e in ap[-1].events] == [100, 200, 300]
    for c in FIXED:
        assert c.events == sj.FIXED_FORCE_EVENTS or c is ap[-1]
        assert c.T == 4 * sj.SEGMENT
        assert c.chains == (5 if c.cases else 6 if c is ap[-1] else 70) and (len(c.cases) == 13 if c.cases else True)
        assert sj.coefficient_over_kT(c.params) <= sj.MAX_COEFFICIENT_OVER_KT
        assert c.params["n"] <= 40 or c in ap       # the sweep homes' 2^-44 >= (10 n + 24) 2^-53


@pytest.mark.parametrize("name,p", START, ids=[r[0] for r in START])
def test_longdouble_microstate_against_the_oracle(oracle, name, p):
    """step_judge.microstate_ld is eap_chain_energy restated: they agree to 1e-13 sum |terms| on every start whose chain holds no
    contact, and to the oracle's own cancellation (n 2^-53 b / r on the separation, three powers of it in 1 / r^3) inside one."""
    op = sj.oracle_params(oracle, p)
    q = {k: v for k, v in p.items() if k != "x0_vec"}
    for chain in (0, 1, 33, 57, 64, 69):
        phi, th, _ = sj.start_twin(oracle, op, p, chain, sj.F32)
        Uv, r, pp = oracle.chain_energy(op, phi, th)
        lit, _ = sj.term_sums(q, phi, th)
        cond = 1.0
        if p["energy_type"] != sj.NONINTERACTING and p["n"] > 1:
            nh = np.stack([np.cos(phi) * np.sin(th), np.sin(phi) * np.sin(th), np.cos(th)], axis=1)
            rmin = np.linalg.norm(nh[:-1] + nh[1:], axis=1).min() / 2 if p["energy_type"] == sj.ISING else sj.min_pair_distance(q, phi, th)
            cond = max(1.0, 1.0 / rmin)
        err = np.abs(sj.microstate_ld(q, phi, th) - np.concatenate([r, pp, [Uv]])).astype(np.float64)
        assert np.all(err <= 1e-13 * lit * np.array([1, 1, 1, 1, 1, 1, cond])), (chain, err / lit, cond)
