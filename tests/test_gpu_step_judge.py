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


def _device_params(ps, p, chains, precision, cluster, **kw):
    return ps.default_params(num_chains=chains, precision=precision,
                             move_set=ps.MOVES_CLUSTER if cluster else ps.MOVES_SINGLE, **p, **kw)


def _check_adaptation(oracle, op, pre, post, t1, adaptive):
    """The adaptation rule at a window end (mcmc_eap_chain.jl:301-322), from nacc_window / natt_window; between window ends
    the step sizes stay and the window counts the step."""
    dn = post["nacc_total"] - pre["nacc_total"]
    nacc, natt = pre["nacc_window"] + dn, pre["natt_window"] + 1
    ps_, ts_ = pre["phi_step"], pre["theta_step"]
    if adaptive and t1 % op.steps_per_adjust == 0:
        ps_, ts_, nacc, natt = oracle.adapt(op, t1, ps_, ts_, nacc, natt)
    got = (post["phi_step"], post["theta_step"], post["nacc_window"], post["natt_window"])
    assert got == (ps_, ts_, nacc, natt), (t1, got, (ps_, ts_, nacc, natt))


def _judge_run(ps, oracle, cases, chains, precision, cluster, T, judged, kernel, not_kernel="", packed=None):
    """cases: the option dicts of the handle's cases.  Returns the stepped handle's final per-chain states and the tally."""
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
        pre = {c: e.chain_state(c) for c in judged}
        lag = {c: 0.0 for c in judged}
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
    return pps, final


def _long_launch_equals_stepped(ps, pps, final, T):
    """(a)"""
    with ps.Ensemble(pps if len(pps) > 1 else pps[0]) as e:
        e.advance(T)
        for c, want in enumerate(final):
            got = e.chain_state(c)
            assert np.array_equal(got["theta"], want["theta"]) and np.array_equal(got["phi"], want["phi"]), c
            assert np.array_equal(got["rng"], want["rng"]) and got["nacc_total"] == want["nacc_total"], c
            assert got["phi_step"] == want["phi_step"] and got["theta_step"] == want["theta_step"], c


def _carried_totals(ps, oracle, pps, cases, chains, T, judged):
    """(b)"""
    ops = [sj.oracle_params(oracle, p) for p in cases]
    worst = 0.0
    with ps.Ensemble(pps if len(pps) > 1 else pps[0]) as e:
        nacc = {c: 0 for c in judged}
        for _ in range(max(1, T // 64)):
            e.advance(64)
            for c in judged:
                k = c // chains
                st = e.chain_state(c)
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


@pytest.mark.parametrize("cfg", sj.CONFIGS, ids=sj.CONFIG_IDS)
def test_every_step_against_the_judge(ps, oracle, cfg, monkeypatch):
    for k, v in cfg.env.items():
        monkeypatch.setenv(k, v)
    judged = cfg.judged()
    pps, final = _judge_run(ps, oracle, [cfg.params], cfg.chains, cfg.precision, cfg.cluster, cfg.T, judged, cfg.kernel,
                            cfg.not_kernel)
    _long_launch_equals_stepped(ps, pps, final, cfg.T)
    _carried_totals(ps, oracle, pps, [cfg.params], cfg.chains, cfg.T, judged)


@pytest.mark.parametrize("precision,kernel", [(sj.F32, "sweep_kernel<float> [packed cases]"),
                                              (sj.Q16, "sweep_kernel<float, q16 state> [packed cases]")], ids=["f32", "q16"])
def test_every_step_against_the_judge_packed(ps, oracle, precision, kernel, monkeypatch):
    """13 cases x 5 chains of different E0, Fz, kT in one packed handle: chains 63 and 64 sit in different workgroups and
    cases, chain 64 in a partial wave."""
    monkeypatch.setenv("PSTAT_PACK", "1")
    cases = [dict(sj.PACKED_COMMON, seed=500 + i, **c) for i, c in enumerate(sj.PACKED_CASES)]
    judged = [0, 1, 63, 64]
    pps, final = _judge_run(ps, oracle, cases, 5, precision, False, sj.PACKED_T, judged, kernel, packed=1)
    _long_launch_equals_stepped(ps, pps, final, sj.PACKED_T)
    _carried_totals(ps, oracle, pps, cases, 5, sj.PACKED_T, judged)
