"""Every f32 and q16 step judged against an f64 reference of that step -- run with -m gpu.

A handle is stepped one launch per step; before and after every step the judged chains' state is read
(pstat_chain_state) and held against the oracle's one-step judge (oracle/eap_oracle.h: eap_step_judge) from the same state:
generator words, which angles moved and where to, nacc_total, and the verdict wherever z = d - log eps lies outside the margin
m = c 2^-24 mag.  tests/step_judge.py states the comparison, the margins and their derivation, and the configurations;
tests/test_step_judge_cpu.py checks on the CPU that every configuration leaves at most 0.5 % of its steps undecided with the
judge alone and that a judge whose E0 is off by 2^-8 is caught.

Per configuration, besides the per-step comparison:
  (a) a second handle advanced T steps in ONE launch equals the stepped handle bit for bit (angles, generator words,
      nacc_total, every chain): the verdict on single-step launches is a verdict on the long launch;
  (b) a third handle advanced in launches of 64 steps: after each, r, p, U of pstat_microstate against the oracle's f64
      recomputation from the stored angles, bound (accepted + n) K_TOTALS 2^-24 sum |terms| + (n + 2 accepted) K_ABS 2^-24 c1:
      the terms by their value, plus the absolute error of v_sin / v_cos on one monomer's coefficient c1 (tests/step_judge.py).
      WHAT (b) COVERS depends on where a kernel re-derives its totals (read in the kernels, not measured):
        sweep_kernel<float[, q16 state]>, cluster_kernel<float[, q16 state | state in memory]>: re-derived from the angles when
          a launch STARTS, then carried through every accepted step: (b) checks 64 steps' worth of carried dU, dr, dp;
        interacting_kernel<float>: re-derived at the start AND after every block of at most 128 steps, i.e. at the END of
          every launch: for r, p and sum(u) the check says nothing about the carried differences; U's pair part is the
          fresh all-pairs sum of the last accepted trial, which (b) does check;
        cluster_wave_kernel<float>: the whole trial configuration is re-derived from its angles at every step: (b) checks
          that derivation, not a carried difference.
  (c) the tally agree / undecided / wrong; any wrong step fails, and so does an undecided share above 0.5 %;
  the same recorded steps judged by a judge whose E0 is multiplied by 1 + 2^-8 must show at least one wrong step.
  (d) THE RECORD.  Every step, accepted or not, adds the current r, p, U and their squares (the clustering main also
      sum cos^2 theta and <psi>) to f32 block accumulators that are folded into the f64 `sums`.  step_judge.record_twin restates
      record! in numpy f64 on the stepped handle's own states (one oracle.chain_energy call per judged chain and step);
      step_judge.record_bound is the derived bound (carried-value error, the weight's error, the block's f32 additions, the
      flush and its rescale by b, the gauge rises).  Compared, for every judged chain:
        the stepped handle after every step: `sums` (and chain_extras) against the twin's prefix, normalizer == steps_recorded;
        the long launch of (a), T steps in one launch across FLUSH blocks and adaptation windows: its final sums, under the
          bound with 128-record blocks and every acceptance of the launch carried;
        the handle of (b) after each launch of 64.
      The first step at which a column leaves its bound is reported: chain, step, column, error / bound.
The configurations with umbrella=1 (step_judge._umbrella_configs) go through all of it.  (a) still demands bit-equal angles,
generator words, nacc_total and step sizes: the weight enters a decision through du of the step, not through the carried
usum.  Under (d) the gauge-free ratios sums / normalizer are compared with the twin's, and THE GAUGE CONTRACT is asserted at
every step of the stepped handle: ln(normalizer / N*) <= 30 + margin, N* the twin's normaliser over its heaviest record's
weight, 30 umbrella_logw's threshold for `float`, the margin derived (step_judge.GAUGE_MARGIN_MAX); averages and
normaliser finite and positive throughout.  On the gauge-rise rows the twin's heaviest record, gauged on the start, exceeds
e^35: the contract can only hold there if the kernel raised the gauge, and that the twin says so is asserted too.
Each configuration prints one line with the worst error / bound of (d): profiles/step_judge/record_judge.txt.
The all-pairs configurations start extended (--x0) and must stay out of 1/r^3 contacts: every 25 steps the judged chains'
smallest |x_i - x_j| is asserted to be at least CONTACT_DISTANCE b.
"""
import math

import numpy as np
import pytest

import step_judge as sj

pytestmark = pytest.mark.gpu

TALLY = {}       # kernel name -> [agree, undecided, wrong]


@pytest.fixture(scope="module")
def ps():
    import polymer_stats_amd as ps
    assert ps._lib.load().pstat_device_count() >= 1, "no HIP device visible"
    return ps


_device_params = sj.device_params            # (shared with tests/test_gpu_lifecycle_judge.py)
_check_adaptation = sj.check_adaptation


_record_check = sj.record_check          # (shared with tests/test_gpu_lifecycle_judge.py)


def _launch_accepts(accepted, every):
    ca = np.cumsum(accepted)
    return ca - np.concatenate([[0], ca])[(np.arange(len(ca)) // every) * every]


def _judge_run(ps, oracle, cases, chains, precision, cluster, T, judged, kernel, not_kernel="", packed=None, rise=False):
    """cases: the option dicts of the handle's cases.  Returns the handle's parameters, the stepped handle's final per-chain
    states, its record per judged chain (for (d) on the other handles) and the worst error / bound of (d)."""
    pps = [_device_params(ps, p, chains, precision, cluster) for p in cases]
    ops = [sj.oracle_params(oracle, p) for p in cases]
    pert = [sj.perturbed(oracle, p) for p in cases]
    adaptive = cases[0].get("adj_scale", 1.1) != 1.0
    all_pairs = cases[0]["energy_type"] in (sj.INTERACTING, sj.CUTOFF)
    tally = dict(agree=0, undecided=0, wrong=0, wrong_perturbed=0, worst_ratio=0.0, adapted=0)
    msgs = []
    with ps.Ensemble(pps if len(pps) > 1 else pps[0]) as e:
        info = e.launch_info()
        name = info.kernel.decode()
        assert kernel in name and (not not_kernel or not_kernel not in name), name
        if packed is not None:
            assert info.packed_cases == packed, name
        if all_pairs and cases[0].get("use_x0"):       # the --x0 start itself (store_phi_rad / store_theta_rad), every chain
            sj.check_start(oracle, e, cases, ops, chains, precision, cluster=cluster)
        pre = {c: e.chain_state(c) for c in judged}
        lag = {c: 0.0 for c in judged}
        ncol = 18 if cluster else 16
        data = {}
        for c in judged:
            k = c // chains
            cur = sj.rec_of(oracle, ops[k], cases[k], pre[c]["phi"], pre[c]["theta"], cluster)
            data[c] = dict(recs=[], acc=[], sums=[], norm=[], usum0=cur.usum, cur=cur, start=cur)
        for t in range(T):
            e.advance(1)
            for c in judged:
                k = c // chains
                post = e.chain_state(c)
                assert post["steps_recorded"] == t + 1
                J, inside = sj.judge(oracle, ops[k], pre[c], precision, cluster)
                R = sj.compare(pre[c], post, J, inside, precision, lag[c])
                tally[R.kind] += 1
                if R.kind == "wrong" and len(msgs) < 5:
                    msgs.append(f"chain {c} step {t}: {R.why}")
                if R.why == "verdict within margin" and (R.verdict.z > 0) != R.moved:
                    tally["worst_ratio"] = max(tally["worst_ratio"], R.verdict.ratio)
                if R.why != "growth test within margin":
                    Jp, _ = sj.judge(oracle, pert[k], pre[c], precision, cluster)
                    Vp = sj.verdict(Jp, lag[c], inside, pole=sj.pole_term(Jp, pre[c]["theta"]))
                    if Vp.kind != "undecided" and (Vp.kind == "accept") != R.moved:
                        tally["wrong_perturbed"] += 1
                _check_adaptation(oracle, ops[k], pre[c], post, t + 1, adaptive)
                D = data[c]
                if R.moved:
                    D["cur"] = sj.rec_of(oracle, ops[k], cases[k], post["phi"], post["theta"], cluster)
                D["recs"].append(D["cur"])
                D["acc"].append(R.moved)
                D["sums"].append(np.concatenate([post["sums"], e.chain_extras(c)["sums"]]) if cluster else post["sums"])
                D["norm"].append(post["normalizer"])
                tally["adapted"] += post["phi_step"] != pre[c]["phi_step"]
                if R.moved:
                    # what the device's acceptor caches.  After a growth test within its margin the device may have grown
                    # another cluster than the judge: its log alpha is then recovered from the states themselves
                    lag[c] = J.log_alpha if R.why != "growth test within margin" else \
                        sj.log_alpha_of_move(pre[c]["theta"], post["theta"], post["phi"], J.idx)
                if all_pairs and (t + 1) % 25 == 0:
                    dmin = sj.min_pair_distance(cases[k], post["phi"], post["theta"])
                    assert dmin >= sj.CONTACT_DISTANCE, f"chain {c} step {t}: monomers {dmin:.3f} b apart: the run reached a contact"
                pre[c] = post
        final = [e.chain_state(c) for c in range(chains * len(cases))]
    acc = TALLY.setdefault(name, [0, 0, 0])
    for i, k in enumerate(("agree", "undecided", "wrong")):
        acc[i] += tally[k]
    steps = tally["agree"] + tally["undecided"] + tally["wrong"]
    share = tally["undecided"] / steps
    print(f"\n{name}: agree {tally['agree']}, undecided {tally['undecided']} ({100 * share:.3f} %), wrong {tally['wrong']}; "
          f"decided {tally['agree'] + tally['wrong']}; worst |z| / (2^-24 mag) among undecided disagreements "
          f"{tally['worst_ratio']:.1f}; wrong under E0 (1 + 2^-8): {tally['wrong_perturbed']}; step sizes adapted "
          f"{tally['adapted']} times; kernel total so far (agree, undecided, wrong) {acc}")
    assert tally["wrong"] == 0, "\n".join(msgs)
    assert share <= 0.005, share
    assert tally["wrong_perturbed"] >= 1
    assert adaptive or tally["adapted"] == 0      # (the rule itself is asserted at every window end, above)
    worst = np.zeros(2)
    for c in judged:       # (d), the stepped handle: every launch is one step, one record, at most one acceptance
        D = data[c]
        D["acc"] = np.array(D["acc"], dtype=np.int64)
        worst = np.maximum(worst, _record_check(f"stepped handle, chain {c}", D, cases[c // chains], np.ones(T), 1, 1, np.arange(T),
                                                D["sums"], D["norm"], ncol, rise))
    return pps, final, data, worst


def _long_launch_equals_stepped(ps, pps, final, T, data, cases, chains, cluster):
    """(a), and (d) on the long launch: its final sums against the twin on the stepped handle's states."""
    worst = np.zeros(2)
    with ps.Ensemble(pps if len(pps) > 1 else pps[0]) as e:
        e.advance(T)
        for c, want in enumerate(final):
            got = e.chain_state(c)
            assert np.array_equal(got["theta"], want["theta"]) and np.array_equal(got["phi"], want["phi"]), c
            assert np.array_equal(got["rng"], want["rng"]) and got["nacc_total"] == want["nacc_total"], c
            assert got["phi_step"] == want["phi_step"] and got["theta_step"] == want["theta_step"], c
            if c in data:
                D = data[c]
                sums = np.concatenate([got["sums"], e.chain_extras(c)["sums"]]) if cluster else got["sums"]
                worst = np.maximum(worst, _record_check(f"long launch, chain {c}", D, cases[c // chains], np.cumsum(D["acc"]), sj.FLUSH, T,
                                                        [T - 1], [sums], [got["normalizer"]], 18 if cluster else 16))
    return worst


def _carried_totals(ps, oracle, pps, cases, chains, T, judged, data, cluster):
    """(b), and (d) after each of its launches of 64"""
    ops = [sj.oracle_params(oracle, p) for p in cases]
    worst = 0.0
    read = {c: dict(sums=[], norm=[]) for c in judged}
    with ps.Ensemble(pps if len(pps) > 1 else pps[0]) as e:
        nacc = {c: 0 for c in judged}
        for _ in range(max(1, T // 64)):
            e.advance(64)
            for c in judged:
                k = c // chains
                st = e.chain_state(c)
                read[c]["sums"].append(np.concatenate([st["sums"], e.chain_extras(c)["sums"]]) if cluster else st["sums"])
                read[c]["norm"].append(st["normalizer"])
                got = e.microstate(c)
                U, r, p = oracle.chain_energy(ops[k], st["phi"], st["theta"])
                lit, c1 = sj.term_sums(cases[k], st["phi"], st["theta"])
                acc = st["nacc_total"] - nacc[c]
                nacc[c] = st["nacc_total"]
                want = np.concatenate([r, p, [U]])
                bound = (acc + ops[k].n) * sj.K_TOTALS * sj.U * lit + (ops[k].n + 2 * acc) * sj.K_ABS * sj.U * c1
                err = np.abs(got - want)
                worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
                assert np.all(err <= bound), (c, got, want, err / bound)
    print(f"carried totals: worst error / bound {worst:.3f}")
    wd = np.zeros(2)
    for c in judged:
        D = data[c]
        at = 64 * np.arange(1, len(read[c]["norm"]) + 1) - 1
        wd = np.maximum(wd, _record_check(f"launches of 64, chain {c}", D, cases[c // chains], _launch_accepts(D["acc"], 64), 64, 64, at,
                                          read[c]["sums"], read[c]["norm"], 18 if cluster else 16))
    return wd


def _report(name, umbrella, stepped, long, by64):
    what = "ratios" if umbrella else "sums"
    print(f"\nrecord judge {name}: worst error / bound of the {what} -- stepped {stepped[0]:.3g}, long launch {long[0]:.3g}, "
          f"launches of 64 {by64[0]:.3g}; of the extras -- stepped {stepped[1]:.3g}, long launch {long[1]:.3g}, "
          f"launches of 64 {by64[1]:.3g}")


@pytest.mark.parametrize("cfg", sj.CONFIGS, ids=sj.CONFIG_IDS)
def test_every_step_against_the_judge(ps, oracle, cfg, monkeypatch):
    for k, v in cfg.env.items():
        monkeypatch.setenv(k, v)
    judged = cfg.judged()
    pps, final, data, w1 = _judge_run(ps, oracle, [cfg.params], cfg.chains, cfg.precision, cfg.cluster, cfg.T, judged, cfg.kernel,
                                      cfg.not_kernel, rise=cfg.name in sj.RISE_IDS)
    wl = _long_launch_equals_stepped(ps, pps, final, cfg.T, data, [cfg.params], cfg.chains, cfg.cluster)
    w64 = _carried_totals(ps, oracle, pps, [cfg.params], cfg.chains, cfg.T, judged, data, cfg.cluster)
    _report(cfg.name, cfg.params.get("umbrella"), w1, wl, w64)


@pytest.mark.parametrize("precision,kernel,umbrella", [(sj.F32, "sweep_kernel<float> [packed cases]", 0),
                                                       (sj.Q16, "sweep_kernel<float, q16 state> [packed cases]", 0),
                                                       (sj.F32, "sweep_kernel<float> [packed cases]", 1)],
                         ids=["f32", "q16", "f32-umbrella"])
def test_every_step_against_the_judge_packed(ps, oracle, precision, kernel, umbrella, monkeypatch):
    """13 cases x 5 chains of different E0, Fz, kT in one packed handle: chains 63 and 64 sit in different workgroups and
    cases, chain 64 in a partial wave."""
    monkeypatch.setenv("PSTAT_PACK", "1")
    cases = [dict(sj.PACKED_COMMON, seed=500 + i, **c, **(dict(umbrella=1) if umbrella else {})) for i, c in enumerate(sj.PACKED_CASES)]
    judged = [0, 1, 63, 64]
    pps, final, data, w1 = _judge_run(ps, oracle, cases, 5, precision, False, sj.PACKED_T, judged, kernel, packed=1)
    wl = _long_launch_equals_stepped(ps, pps, final, sj.PACKED_T, data, cases, 5, False)
    w64 = _carried_totals(ps, oracle, pps, cases, 5, sj.PACKED_T, judged, data, False)
    _report("packed-" + ("q16" if precision == sj.Q16 else "f32") + ("-umbrella" if umbrella else ""), umbrella, w1, wl, w64)
