"""What happens to an f32 / q16 handle BETWEEN the launches, judged against the oracle -- run with -m gpu.

tests/step_judge.py ("between the launches") states the start, the re-init verdict, the lag error and the LIFECYCLE table;
tests/test_lifecycle_judge_cpu.py pins the oracle's re-init judge against its run loops and checks caps, coverage and teeth
with the judge alone.  Per row of the table, on the device:
  the start     every chain's stored angles equal start_twin bit for bit, the generator words the oracle's, pstat_microstate
                the oracle's chain_energy on those angles, steps, sums and windows zero (step_judge.check_start); the same
                after restart_from_x0;
  a re-init     (pstat_reinit, every chain) the words after equal the judge's; the angles are all unchanged or all equal to
                the fresh draw as the device stores it; nacc_total, sums, normalizer, steps_recorded, step sizes and window
                counters are unchanged; after an adoption pstat_microstate is the f64 recomputation (1e-13 sum |terms|: the
                kernel derives it in f64; the all-pairs home in f32: its carried-totals bound), otherwise it is unchanged; (judged chains) adopted or not agrees with
                step_judge.reinit_verdict wherever that is decided;
  after it      every step of the judged chains is judged with the twin's lag, its margin widened by the lag error until
                the first acceptance clears both; the adaptation rule holds with the step counter restarted at the re-init;
  a rung        (scale_kT + reset_sampler + reset_averages) angles and words stay, step sizes go back to the defaults, windows,
                sums, nacc_total and steps_recorded to zero; the steps after it are judged at the new kT with lag = 0;
  tallies       0 wrong, at most 0.5 % undecided; the same steps under a judge with E0 (1 + 2^-8) show at least one wrong step
                (every row's seed is one at which the judge alone meets it at least twice);
  the record    (d) of tests/test_gpu_step_judge.py on the stepped handle: after every step the judged chains' `sums` (and
                chain_extras) against step_judge.record_twin under record_bound -- across the re-inits, where the record goes on
                with the adopted draw, and restarted at every rung and at restart_from_x0;
  long launch   a second handle runs the schedule with one launch per segment, the events between: it ends bit-equal in
                angles, words, nacc_total, step sizes and windows, every chain;
  checkpoint    a third handle runs to the first event (clustering rows: into the middle of the first rung), applies it and
                takes an image -- a live lag in it; a fourth restores the image; both advance 64 steps in one launch and
                agree bit for bit in chain_state, pstat_microstate and chain_extras, every chain.
Each row prints one line: profiles/step_judge/lifecycle_judge.txt.
"""
import numpy as np
import pytest

import step_judge as sj

pytestmark = pytest.mark.gpu

ROWS = {}        # row name -> its tallies


@pytest.fixture(scope="module")
def ps():
    import polymer_stats_amd as ps
    assert ps._lib.load().pstat_device_count() >= 1, "no HIP device visible"
    return ps


def _apply(e, ev):
    """One event of a schedule on a handle."""
    kind, args = ev[1], ev[2:]
    if kind == "reinit_forced":
        e.reinit(True)
    elif kind == "reinit_metropolis":
        e.reinit(False)
    elif kind == "rung":
        e.scale_kT(args[0])
        e.reset_sampler()
        e.reset_averages()
    elif kind == "x0":
        e.restart_from_x0(args[0], args[1], args[2])
    else:
        raise ValueError(kind)


def _same_bookkeeping(a, b, c):
    for k in ("nacc_total", "steps_recorded", "nacc_window", "natt_window", "phi_step", "theta_step", "normalizer"):
        assert a[k] == b[k], (c, k, a[k], b[k])
    assert np.array_equal(a["sums"], b["sums"]), c


class _Twin:
    """What the judge carries for one judged chain between its steps."""

    def __init__(self):
        self.lag = 0.0           # the acceptor's stale cache, as the twin states it
        self.lag_err = 0.0
        self.acc_last = 0        # acceptances of the chain's last launch (one step)


def _reinit_on_device(ps, oracle, e, cfg, cases, ops, forced, twins, tally, msgs):
    """pstat_reinit on the stepped handle, every chain held against eap_reinit_judge from its own state before."""
    total = cfg.chains * len(cases)
    before = [e.chain_state(c) for c in range(total)]
    micro = [e.microstate(c) for c in range(total)]
    e.reinit(forced)
    for c in range(total):
        k = c // cfg.chains
        p, op = cases[k], ops[k]
        pre, post = before[c], e.chain_state(c)
        tw = twins.get(c)
        E = sj.reinit_event(oracle, op, p, pre["phi"], pre["theta"], pre["rng"], tw.lag if tw else 0.0, forced, cfg.precision,
                            acc_last=tw.acc_last if tw else 1)
        assert np.array_equal(post["rng"], E.J.rng), (c, post["rng"], E.J.rng)
        _same_bookkeeping(pre, post, c)
        stayed = np.array_equal(post["phi"], pre["phi"]) and np.array_equal(post["theta"], pre["theta"])
        fresh = np.array_equal(post["phi"], E.J.fresh_phi) and np.array_equal(post["theta"], E.J.fresh_theta)
        assert stayed or fresh, f"chain {c}: the angles after a re-init are neither the old ones nor the fresh draw"
        adopted = fresh and not stayed
        assert adopted or not forced, c
        got = e.microstate(c)
        if adopted:
            lit, c1 = sj.term_sums(p, post["phi"], post["theta"])
            if sj.reinit_home(p) == "allpairs":      # re-derived in f32: CARRIED TOTALS with no acceptance + PAIR CONDITIONING on U
                tol = sj.carried(p["n"], 0, lit, c1)
                tol[6] += sj.K_COND * sj.U * sj.term_sums(p, post["phi"], post["theta"], conditioning=True)[2]
            else:                                    # derived in f64 by reinit_kernel
                tol = 1e-13 * lit + 1e-300
            err = np.abs(got - sj.microstate_ld(p, post["phi"], post["theta"])).astype(np.float64)
            tally["micro"] = max(tally["micro"], float((err / tol).max()))
            assert np.all(err <= tol), (c, err / tol)
        else:
            assert sj.reinit_home(p) == "allpairs" or np.array_equal(got, micro[c]), c
        if tw is None:
            continue
        if not forced:
            if E.V.kind == "undecided":
                tally["reinit_undecided"] += 1
            else:
                tally["reinit_decided"] += 1
                if (E.V.kind == "accept") != adopted:
                    tally["reinit_wrong"] += 1
                    msgs.append(f"chain {c}: the device {'adopted' if adopted else 'refused'} the fresh draw, the judge says {E.V.kind}: "
                                f"d = {E.J.d!r}, eps = {E.J.eps!r}, z = {E.V.z!r}, m = {E.V.m!r}, mag = {E.J.mag!r}")
        if adopted:
            # (the twin's lag_out is stated for an adoption whatever its own decision was)
            J = E.J if E.J.adopt else None
            if J is None:       # within the margin the device adopted where the oracle's expression refused: restate the lag
                J = oracle.reinit_judge(op, pre["phi"], pre["theta"], pre["rng"], lag_in=tw.lag, force=True,
                                        fresh_to=(post["phi"], post["theta"]))
            tw.lag, tw.lag_err = J.lag_out, E.lag_error + tw.lag_err      # (a live lag's error is inherited with it)
            tally["lag_max"] = max(tally["lag_max"], abs(tw.lag))
        before[c] = post
    return {c: before[c] for c in twins}


def _stepped(ps, oracle, cfg):
    """The stepped handle: one launch per step, the events between.  Returns the parameters, every chain's final state and
    the tallies."""
    cases = cfg.cases or [cfg.params]
    chains, precision, cluster = cfg.chains, cfg.precision, cfg.cluster
    total = chains * len(cases)
    judged = cfg.judged()
    pps = [sj.device_params(ps, p, chains, precision, cluster) for p in cases]
    ops = [sj.oracle_params(oracle, p) for p in cases]
    pert = [sj.perturbed(oracle, p) for p in cases]
    ops0 = list(ops)
    adaptive = cases[0].get("adj_scale", 1.1) != 1.0
    tally = dict(agree=0, undecided=0, wrong=0, wrong_perturbed=0, wrong_lag0=0, reinit_decided=0, reinit_undecided=0, reinit_wrong=0,
                 micro=0.0, lag_max=0.0, live=0, worst_ratio=0.0, in_contact=0, record=np.zeros(2))
    all_pairs = cases[0]["energy_type"] == sj.INTERACTING
    msgs = []
    pending = sorted(cfg.events, key=lambda ev: ev[0])
    with ps.Ensemble(pps if len(pps) > 1 else pps[0]) as e:
        info = e.launch_info()
        name = info.kernel.decode()
        assert cfg.kernel in name and (not cfg.not_kernel or cfg.not_kernel not in name), name
        if cfg.cases:
            assert info.packed_cases == 1, name
        sj.check_start(oracle, e, cases, ops, chains, precision, cluster=cluster)
        pre = {c: e.chain_state(c) for c in judged}
        twins = {c: _Twin() for c in judged}
        step_in_init = recorded = 0
        ncol = 18 if cluster else 16

        def new_record():
            """(d) restarts: the twin's records of every judged chain from the state the device records from now on"""
            out = {}
            for c in judged:
                cur = sj.rec_of(oracle, ops[c // chains], cases[c // chains], pre[c]["phi"], pre[c]["theta"], cluster)
                out[c] = dict(recs=[], sums=[], norm=[], usum0=cur.usum, cur=cur, start=cur)
            return out

        def close_record(what):
            """(d) on the records since the last reset: the device's sums after every step against the twin's prefixes"""
            for c in judged:
                D = record[c]
                if D["recs"]:
                    T = len(D["recs"])
                    w = sj.record_check(f"{what}, chain {c}", D, cases[c // chains], np.ones(T), 1, 1, np.arange(T), D["sums"], D["norm"], ncol)
                    tally["record"] = np.maximum(tally["record"], w)

        record = new_record()
        for t in range(cfg.T):
            pending_first = len(pending) == len(cfg.events) and pending[0][0] > t      # no event has happened yet
            while pending and pending[0][0] == t:
                ev = pending.pop(0)
                kind = ev[1]
                if kind in ("reinit_forced", "reinit_metropolis"):
                    was = pre
                    pre = _reinit_on_device(ps, oracle, e, cfg, cases, ops, kind == "reinit_forced", twins, tally, msgs)
                    for c in judged:      # the record goes on across a re-init; an adopted draw is what is recorded from now on
                        if not (np.array_equal(was[c]["phi"], pre[c]["phi"]) and np.array_equal(was[c]["theta"], pre[c]["theta"])):
                            record[c]["cur"] = sj.rec_of(oracle, ops[c // chains], cases[c // chains], pre[c]["phi"], pre[c]["theta"], cluster)
                elif kind == "rung":
                    close_record(f"before the rung at step {t}")
                    before = [e.chain_state(c) for c in range(total)]
                    _apply(e, ev)
                    cases = [dict(p0, kT=p0["kT"] * ev[2]) for p0 in (cfg.cases or [cfg.params])]
                    ops = [sj.oracle_params(oracle, p) for p in cases]
                    pert = [sj.perturbed(oracle, p) for p in cases]
                    for c in range(total):
                        st = e.chain_state(c)
                        assert np.array_equal(st["phi"], before[c]["phi"]) and np.array_equal(st["theta"], before[c]["theta"]), c
                        assert np.array_equal(st["rng"], before[c]["rng"]), c
                        assert (st["phi_step"], st["theta_step"]) == (ops0[c // chains].phi_step, ops0[c // chains].theta_step), c
                        assert (st["nacc_total"], st["steps_recorded"], st["nacc_window"], st["natt_window"]) == (0, 0, 0, 0), c
                        assert not st["sums"].any() and st["normalizer"] == 0.0, c
                        assert not cluster or not e.chain_extras(c)["sums"].any(), c
                    pre = {c: e.chain_state(c) for c in judged}
                    twins = {c: _Twin() for c in judged}
                    recorded = 0
                    record = new_record()
                elif kind == "x0":
                    close_record(f"before the restart at step {t}")
                    _apply(e, ev)
                    base = [{k: v for k, v in p.items() if k not in ("use_x0", "x0_phi", "x0_theta", "dx0_phi", "dx0_theta")} for p in cases]
                    xops = [sj.oracle_params(oracle, p, x0_vec=ev[2], dx0_phi=ev[3], dx0_theta=ev[4]) for p in base]
                    sj.check_start(oracle, e, cases, xops, chains, precision, phi_step=ops0[0].phi_step, theta_step=ops0[0].theta_step,
                                   cluster=cluster)
                    pre = {c: e.chain_state(c) for c in judged}
                    twins = {c: _Twin() for c in judged}
                    recorded = 0
                    record = new_record()
                step_in_init = 0
            e.advance(1)
            step_in_init += 1
            recorded += 1
            for c in judged:
                k = c // chains
                tw = twins[c]
                post = e.chain_state(c)
                assert post["steps_recorded"] == recorded
                J, inside = sj.judge(oracle, ops[k], pre[c], precision, cluster)
                touch = 0.0
                if all_pairs and not pending_first:      # a coil after a re-init may hold a contact: step_judge.contact_margin
                    touch = sj.contact_margin(cases[k], pre[c]["phi"], pre[c]["theta"], J.trial_phi, J.trial_theta)
                    tally["in_contact"] += touch > 0
                extra = tw.lag_err + touch
                R = sj.compare(pre[c], post, J, inside, precision, tw.lag, extra=extra)
                tally[R.kind] += 1
                tally["live"] += tw.lag_err > 0
                if R.kind == "wrong" and len(msgs) < 5:
                    msgs.append(f"chain {c} step {t}: {R.why}")
                if R.why == "verdict within margin" and (R.verdict.z > 0) != R.moved:
                    tally["worst_ratio"] = max(tally["worst_ratio"], R.verdict.ratio)
                if R.why != "growth test within margin":
                    pole = sj.pole_term(J, pre[c]["theta"]) + extra
                    Jp, _ = sj.judge(oracle, pert[k], pre[c], precision, cluster)
                    Vp = sj.verdict(Jp, tw.lag, inside, pole=sj.pole_term(Jp, pre[c]["theta"]) + extra)
                    if Vp.kind != "undecided" and (Vp.kind == "accept") != R.moved:
                        tally["wrong_perturbed"] += 1
                    if tw.lag_err > 0:      # a twin that cleared the lag at the re-init, on the same step
                        V0 = sj.verdict(J, 0.0, inside, pole=pole)
                        if V0.kind != "undecided" and (V0.kind == "accept") != R.moved:
                            tally["wrong_lag0"] += 1
                sj.check_adaptation(oracle, ops[k], pre[c], post, step_in_init, adaptive)
                tw.acc_last = int(R.moved)
                D = record[c]
                if R.moved:
                    D["cur"] = sj.rec_of(oracle, ops[k], cases[k], post["phi"], post["theta"], cluster)
                D["recs"].append(D["cur"])
                D["sums"].append(np.concatenate([post["sums"], e.chain_extras(c)["sums"]]) if cluster else post["sums"])
                D["norm"].append(post["normalizer"])
                if R.moved:
                    # what the device's acceptor caches from here on (cf. test_gpu_step_judge._judge_run)
                    tw.lag = J.log_alpha if R.why != "growth test within margin" else \
                        sj.log_alpha_of_move(pre[c]["theta"], post["theta"], post["phi"], J.idx)
                    tw.lag_err = 0.0
                pre[c] = post
        close_record("to the end")
        final = [e.chain_state(c) for c in range(total)]
    return pps, final, tally, msgs, name


def _segments(cfg):
    """[(steps to advance, events applied after them)] of the schedule with one launch per segment."""
    cuts = sorted({ev[0] for ev in cfg.events})
    out, at = [], 0
    for cut in cuts:
        out.append((cut - at, [ev for ev in cfg.events if ev[0] == cut]))
        at = cut
    out.append((cfg.T - at, []))
    return out


def _long_launches_equal_stepped(ps, cfg, pps, final):
    with ps.Ensemble(pps if len(pps) > 1 else pps[0]) as e:
        for steps, events in _segments(cfg):
            e.advance(steps)
            for ev in events:
                _apply(e, ev)
        for c, want in enumerate(final):
            got = e.chain_state(c)
            assert np.array_equal(got["theta"], want["theta"]) and np.array_equal(got["phi"], want["phi"]), c
            assert np.array_equal(got["rng"], want["rng"]) and got["nacc_total"] == want["nacc_total"], c
            assert got["phi_step"] == want["phi_step"] and got["theta_step"] == want["theta_step"], c
            assert (got["nacc_window"], got["natt_window"]) == (want["nacc_window"], want["natt_window"]), c
            assert got["steps_recorded"] == want["steps_recorded"], c


def _checkpoint_carries_the_lag(ps, cfg, pps):
    """An image taken right after the first event (fixed-force rows: a forced re-init, every chain's lag live) or in the
    middle of the first rung (clustering rows) continues bit for bit on a fresh handle."""
    first = min(ev[0] for ev in cfg.events)
    arg = pps if len(pps) > 1 else pps[0]
    with ps.Ensemble(arg) as a, ps.Ensemble(arg) as b:
        a.advance(first)
        for ev in cfg.events:
            if ev[0] == first:
                _apply(a, ev)
        if cfg.cluster:
            a.advance(sj.SEGMENT // 2)
        b.restore(a.checkpoint())
        a.advance(64)
        b.advance(64)
        for c in range(cfg.chains * len(pps)):
            x, y = a.chain_state(c), b.chain_state(c)
            for k in x:
                assert np.array_equal(x[k], y[k]), (c, k)
            assert np.array_equal(a.microstate(c), b.microstate(c)), c
            if cfg.cluster:
                xe, ye = a.chain_extras(c), b.chain_extras(c)
                assert np.array_equal(xe["sums"], ye["sums"]) and np.array_equal(xe["now"], ye["now"]), c


@pytest.mark.parametrize("cfg", sj.LIFECYCLE, ids=sj.LIFECYCLE_IDS)
def test_between_the_launches(ps, oracle, cfg, monkeypatch):
    for k, v in cfg.env.items():
        monkeypatch.setenv(k, v)
    pps, final, tally, msgs, kernel = _stepped(ps, oracle, cfg)
    steps = tally["agree"] + tally["undecided"] + tally["wrong"]
    share = tally["undecided"] / steps
    print(f"\nlifecycle judge {cfg.name} [{kernel}]: agree {tally['agree']}, undecided {tally['undecided']} ({100 * share:.3f} %), "
          f"wrong {tally['wrong']}; re-init verdicts decided {tally['reinit_decided']}, undecided {tally['reinit_undecided']}, wrong "
          f"{tally['reinit_wrong']}; steps under a live lag {tally['live']}, largest |lag| {tally['lag_max']:.2f}, wrong under lag = 0: "
          f"{tally['wrong_lag0']}, under E0 (1 + 2^-8): {tally['wrong_perturbed']}; worst |z| / (2^-24 mag) among undecided "
          f"disagreements {tally['worst_ratio']:.1f}; microstate after an adoption, worst error / bound {tally['micro']:.3g}"
          + f"; the record (d), worst error / bound {tally['record'][0]:.3g}" + (f", extras {tally['record'][1]:.3g}" if cfg.cluster else "")
          + (f"; steps with a contact in the margin {tally['in_contact']}" if tally["in_contact"] else ""))
    ROWS[cfg.name] = tally
    assert tally["wrong"] == 0 and tally["reinit_wrong"] == 0, "\n".join(msgs)
    assert share <= 0.005, share
    assert tally["wrong_perturbed"] >= 1      # (the rows' seeds: at least 2 with the judge alone, tests/test_lifecycle_judge_cpu.py)
    if cfg.params["n"] <= 3 and not cfg.cluster:        # the lags of a short chain are live in chains that move
        assert tally["wrong_lag0"] >= 1
    # the table's cap on undecided re-init verdicts, 2 % of ALL its verdicts, on the rows run so far: whatever rows are selected
    # and in whatever order, the whole table run is held to exactly the cap
    table = sum(len(c.judged()) * sum(ev[1] == "reinit_metropolis" for ev in c.events) for c in sj.LIFECYCLE)
    assert sum(r["reinit_undecided"] for r in ROWS.values()) <= 0.02 * table
    _long_launches_equal_stepped(ps, cfg, pps, final)
    _checkpoint_carries_the_lag(ps, cfg, pps)
