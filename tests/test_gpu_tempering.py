"""GPU tests of replica exchange between the cases of a handle (pstat_tempering_*, pstat_exchange.hip) against
the numpy twin tests/tempering_ref.py: one round's decisions and what it moves on every home, the continuation of exchanged
chains against the planar restatement, the energy caches of the 3D homes, the equilibration of a ladder whose cold rungs
single moves cannot equilibrate (with its control), and tools/phase_scan.py --exchange."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import tempering_ref as tw
from helpers import both

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOT = ("sums", "normalizer", "rng", "phi_step", "theta_step", "nacc_window", "natt_window", "nacc_total")   # stay with the case
CONFIG = ("phi", "theta", "micro")                                                                        # travel with a swap


@pytest.fixture(scope="module")
def ps():
    import polymer_stats_amd as ps
    assert ps._lib.load().pstat_device_count() >= 1, "no HIP device visible"
    return ps


@pytest.fixture(scope="module")
def pb():
    from planar import binding
    binding.lib()
    return binding


def bits(x):
    return np.ascontiguousarray(x).tobytes()


def snapshot(e):
    """chain_state and microstate of every chain."""
    return [dict(e.chain_state(c), micro=e.microstate(c)) for c in range(e.ncases * e.num_chains)]


def twin_round(seed, t, ladder, kT, snap, per):
    """Round t on the snapshot: (source chain of every chain's configuration, {lower case: (attempted, accepted)}, the smallest
    distance of a deciding draw from its threshold)."""
    U = np.array([s["micro"][6] for s in snap])
    src = np.arange(len(snap))
    counts, closest = {}, np.inf
    for a, b in tw.pairs(ladder, kT, t):
        acc, margin = tw.decide(seed, t, a, b, kT, U, per)
        closest = min(closest, margin.min())
        counts[a] = (per, int(acc.sum()))
        for k in np.flatnonzero(acc):
            src[a * per + k], src[b * per + k] = b * per + k, a * per + k
    return src, counts, closest


def assert_round(e, before, src, what):
    """Configurations moved as `src` says, bit for bit; everything that belongs to the temperature slot did not move."""
    after = snapshot(e)
    for c, s in enumerate(after):
        for k in CONFIG:
            assert bits(s[k]) == bits(before[src[c]][k]), f"{what}: {k} of chain {c} is not that of chain {src[c]}"
        for k in SLOT:
            assert bits(s[k]) == bits(before[c][k]), f"{what}: {k} of chain {c} moved"
    return after


# ------------------------------------------------------------------------------------------------ the homes
# two ladders of 3 and 4 rungs, given out of order, and one case that takes no part; 70 chains per case: a pair's chains
# straddle a wave boundary, and so do the cases in a wave of consecutive (pair, chain) lanes
LADDER = [0, 1, 0, -1, 1, 1, 0, 1]
KT = [1.3, 0.6, 0.5, 0.9, 1.7, 0.4, 0.8, 1.0]
PER = 70
BASE = dict(E0=1.0, K1=0.5, Fz=0.5, steps_per_adjust=150)
CLUSTER = dict(move_set=1, cluster_prob=0.5, bend_mod=0.3, bend_angle=0.2)
# name: (parameters, precision, planar, environment, the kernel's name has, has not)
HOMES = {
    "f64 sweep in LDS, Ising": (dict(n=9, energy_type=2), 1, False, {}, "sweep_kernel<double>", "state in L2"),
    "f64 sweep in memory": (dict(n=48), 1, False, {}, "sweep_kernel<double, state in L2>", None),
    "f32 sweep": (dict(n=9), 0, False, {}, "sweep_kernel<float>", "q16"),
    "q16 sweep": (dict(n=9), 2, False, {}, "sweep_kernel<float, q16 state>", None),
    "fixed-force all-pairs": (dict(n=16, energy_type=1), 1, False, {}, "interacting_kernel", None),
    "clustering f64 in memory": (dict(n=9, **CLUSTER), 1, False, {"PSTAT_F64_STATE": "global"}, "cluster_kernel<double, state in memory>", None),
    "clustering f64 chain per wavefront": (dict(n=9, **CLUSTER), 1, False, {"PSTAT_F64_STATE": "wave"}, "cluster_chain_wave_kernel", None),
    "clustering f32 in LDS": (dict(n=9, **CLUSTER), 0, False, {"PSTAT_F32_STATE": "lds"}, "cluster_kernel<float>", "state in memory"),
    "clustering all-pairs": (dict(n=16, energy_type=1, **CLUSTER), 1, False, {}, "cluster_wave_kernel", None),
    "planar": (dict(n=9, cluster_prob=0.5), 1, True, {}, "planar_kernel", None),
}
F64_3D = [k for k, v in HOMES.items() if v[1] == 1 and not v[2]]


def open_home(ps, monkeypatch, name, per=PER):
    kw, precision, planar, env, has, has_not = HOMES[name]
    for k in ("PSTAT_F64_STATE", "PSTAT_F32_STATE", "PSTAT_PACK", "PSTAT_LANES"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    make = ps.default_planar_params if planar else ps.default_params
    cases = [make(num_chains=per, precision=precision, kT=kT, seed=300 + i, **{**BASE, **kw}) for i, kT in enumerate(KT)]
    e = ps.Ensemble(cases, planar=planar)
    k = e.launch_info().kernel.decode()
    assert has in k and (has_not is None or has_not not in k), (name, k)
    return e


@pytest.mark.parametrize("home", list(HOMES))
def test_one_round_equals_the_twin_and_only_the_configuration_moves(ps, monkeypatch, home):
    seed = 0x5eed00000000 + 77
    with open_home(ps, monkeypatch, home) as e:
        t = e.open_tempering(LADDER, seed=seed)
        e.advance(400)
        state = snapshot(e)
        want_att, want_acc = np.zeros(8, dtype=np.int64), np.zeros(8, dtype=np.int64)
        moved = kept = 0
        for rnd in range(2):                              # one round of each parity
            src, counts, closest = twin_round(seed, rnd, LADDER, KT, state, PER)
            print(home, "round", rnd, {a: c for a, c in counts.items()}, "closest draw", closest)
            assert closest > 1e-12, "a borderline decision: the device's exp may round the other way"
            t.exchange()
            state = assert_round(e, state, src, f"{home}, round {rnd}")
            for a, (att, acc) in counts.items():
                want_att[a] += att
                want_acc[a] += acc
                moved, kept = moved + acc, kept + att - acc
            paired = {c for p in tw.pairs(LADDER, KT, rnd) for c in p}
            assert 3 not in paired and all(src[c * PER + k] == c * PER + k for c in range(8) if c not in paired for k in range(PER))
        # rungs by kT: ladder 0 = cases 2, 6, 0; ladder 1 = cases 5, 1, 7, 4
        assert sorted(tw.pairs(LADDER, KT, 0)) == [(2, 6), (5, 1), (7, 4)] and tw.pairs(LADDER, KT, 1) == [(6, 0), (1, 7)]
        assert moved > 0 and kept > 0, "the case shows nothing: every exchange went the same way"
        att, acc, rounds = t.stats()
        assert rounds == 2 and np.array_equal(att, want_att) and np.array_equal(acc, want_acc)
        assert att.sum() == 5 * PER
        t.close()


@pytest.mark.parametrize("home", F64_3D)
def test_energy_caches_travel_with_the_angles(ps, oracle, monkeypatch, home):
    """r, p, U of every exchanged chain are those of its new angles, right after the exchange and after further steps."""
    seed = 5
    kw = HOMES[home][0]
    with open_home(ps, monkeypatch, home) as e:
        t = e.open_tempering(LADDER, seed=seed)
        e.advance(400)
        src, _, _ = twin_round(seed, 0, LADDER, KT, snapshot(e), PER)
        swapped = np.flatnonzero(src != np.arange(len(src)))
        assert len(swapped) >= 2
        t.exchange()
        for stage in ("after the exchange", "after 64 further steps"):
            for c in swapped:
                op, _ = both(1, kT=KT[c // PER], **{k: v for k, v in {**BASE, **kw}.items() if k != "move_set"})
                g = e.chain_state(c)
                U, r, p = oracle.chain_energy(op, g["phi"], g["theta"])
                np.testing.assert_allclose(e.microstate(c), np.r_[r, p, U], rtol=1e-9, atol=1e-9, err_msg=f"{home}, chain {c}, {stage}")
            e.advance(64)


# ------------------------------------------------------------------------------------------------ the continuation (planar)

PLANAR_KT = [0.3, 0.6, 1.2, 2.4]
PLANAR = {
    "non-interacting": dict(n=12, E0=0.9, K1=0.8, K2=0.15, Fz=0.4, Fx=0.1, cluster_prob=0.0, adj_scale=1.0, seed=41),
    # the weak coupling of test_bit_parity_ising_weak_coupling (tests/test_gpu_planar.py): bit parity is meaningful before a collapse
    "Ising, weak coupling": dict(n=12, E0=0.02, K1=0.05, K2=0.01, Fz=0.3, Fx=0.25, b=1.2, energy_type=2, cluster_prob=0.0,
                                 adj_scale=1.0, seed=22),
}


@pytest.mark.parametrize("energy", list(PLANAR))
def test_continuation_is_the_restatements_from_the_swapped_chains(ps, pb, energy):
    """A cache (r, p, U, sum u) that did not travel with its angles changes the chain's path or its averages here."""
    kw, per, seed = PLANAR[energy], 3, 2027      # (on the restatement this seed accepts 4 of the 6 exchanges, 2026 only the upper 3)
    cases = [ps.default_planar_params(num_chains=per, kT=kT, **kw) for kT in PLANAR_KT]
    with ps.Ensemble(cases, planar=True) as e:
        assert "planar" in e.launch_info().kernel.decode()
        t = e.open_tempering([0] * 4, seed=seed)
        e.advance(300)
        before = snapshot(e)
        src, counts, closest = twin_round(seed, 0, [0] * 4, PLANAR_KT, before, per)
        accepted = sum(c[1] for c in counts.values())
        print(energy, counts, "closest draw", closest)
        assert closest > 1e-12
        assert 0 < accepted < 2 * per, "pick another seed: this one accepts none or all of the six exchanges"
        t.exchange()
        e.reset_averages()
        e.advance(300)
        for c in range(4 * per):
            o = pb.run(pb.make_params(num_steps=300, kT=PLANAR_KT[c // per], **kw), chain_id=c % per,
                       phi0=before[src[c]]["phi"], rng0=before[c]["rng"])
            g = e.chain_state(c)
            assert bits(g["phi"]) == bits(o.final_phi), f"phi differs, chain {c} (configuration of chain {src[c]})"
            assert bits(g["rng"]) == bits(o.rng), f"rng differs, chain {c}"
            assert g["nacc_total"] == o.nacc_total, c
            np.testing.assert_allclose(e.microstate(c), o.microstate, rtol=1e-9, atol=1e-8)
            np.testing.assert_allclose(g["sums"] / g["normalizer"], o.avg, rtol=1e-9, atol=1e-9)


# ------------------------------------------------------------------------------------------------ refusals that need a handle

def test_open_refuses_bad_ladders(ps):
    lib = ps._lib.load()
    cases = [ps.default_params(n=6, num_chains=4, kT=kT, Fz=Fz) for kT, Fz in ((1.0, 0.1), (2.0, 0.1), (3.0, 0.3))]
    with ps.Ensemble(cases) as e:
        with pytest.raises(ps.PstatError) as err:
            e.open_tempering([0, -2, 0])
        assert err.value.code == -1 and "ladder[1]" in str(err.value)
        with pytest.raises(ps.PstatError) as err:
            e.open_tempering([0, 0, 0])
        assert err.value.code == -1 and "Fz" in str(err.value) and "case 2" in str(err.value)
        with pytest.raises(ValueError):
            e.open_tempering([0, 0])
        t = e.open_tempering([0, 0, 1])             # a ladder of one case is allowed and never exchanges
        with ps.Ensemble(cases[:2]) as other:       # an object of another handle
            assert lib.pstat_tempering_exchange(other._h, t._t) == -1
        e.advance_tempered(t, 25, 10)
        att, acc, rounds = t.stats()
        assert rounds == 2 and att.tolist() == [4, 0, 0] and e.chain_state(0)["steps_recorded"] == 25
    with ps.Ensemble([ps.default_params(n=6, num_chains=4, kT=kT, umbrella=1) for kT in (1.0, 2.0)]) as e:
        with pytest.raises(ps.PstatError) as err:
            e.open_tempering([0, 0])
        assert err.value.code == -4 and "umbrella" in str(err.value)


# ------------------------------------------------------------------------------------------------ equilibration

def _ladder_run(ps, golden, exchange):
    """The ladder of tests/golden/tempering_closed_form.json, 512 chains per rung: z of <r3>, <r3sq>, <p3>, <U> per rung
    against the closed form, and the swap acceptance of every adjacent pair."""
    p = golden["params"]
    cases = [ps.default_params(n=p["n"], E0=p["E0"], K1=p["K1"], K2=p["K2"], Fz=p["Fz"], b=p["b"], kT=kT, num_chains=512,
                               seed=20261018 + i) for i, kT in enumerate(golden["kT"])]
    cols = [ps.OBS_NAMES.index(k) for k in ("r3", "r3sq", "p3", "U")]
    with ps.Ensemble(cases) as e:
        t = e.open_tempering(ps.ladders_by(cases), seed=9)
        run = (lambda nsteps: e.advance_tempered(t, nsteps, 50)) if exchange else e.advance
        run(20000)
        e.reset_averages()
        run(100000)
        z = np.zeros((len(cases), 4))
        for i, rung in enumerate(golden["rungs"]):
            s = e.summary(i)
            eq = np.array([rung["avg"][k] for k in ("r3", "r3sq", "p3", "U")])
            z[i] = (np.array(s.avg)[cols] - eq) / (np.array(s.stderr)[cols] + 1e-12 * (1 + np.abs(eq)))
        att, acc, rounds = t.stats()
    return z, att, acc, rounds


def test_exchange_equilibrates_what_single_moves_cannot(ps):
    """Device figures (MI355X): see DESIGN.md 3.13."""
    with open(os.path.join(ROOT, "tests", "golden", "tempering_closed_form.json")) as f:
        golden = json.load(f)
    assert golden["kT"] == sorted(golden["kT"]) and len(golden["kT"]) == 7
    z, att, acc, rounds = _ladder_run(ps, golden, True)
    swap = acc[:-1] / np.maximum(att[:-1], 1)
    print("with exchange: z(r3, r3sq, p3, U) per rung\n", np.round(z, 2), "\nswap acceptance", np.round(swap, 3))
    zc, attc, _, roundsc = _ladder_run(ps, golden, False)
    print("control, plain advance: z per rung\n", np.round(zc, 2))
    assert rounds == 2400 and roundsc == 0 and attc.sum() == 0
    assert np.array_equal(att[:-1], np.array([1200 * 512] * 6)) and att[-1] == 0      # each adjacent pair: every other round
    assert np.all(np.abs(z) < 5.0), np.round(z, 2)
    assert np.all((swap > 0.05) & (swap < 0.95)), swap
    # the control shows the metastability the exchange removes: without it the coldest rung is nowhere near its closed form
    assert zc[0, 0] < -10.0, np.round(zc, 2)


# ------------------------------------------------------------------------------------------------ the tool

def _scan(tmp_path, name, *extra, points=8):
    out = tmp_path / name
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "phase_scan.py"), "--points", str(points), "--n", "20", "--chains", "4",
                        "--steps", "2000", "--burn-in", "400", "--out", str(out), *extra], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return out.read_text(), r.stderr


@pytest.mark.parametrize("points", [8, 42])
def test_phase_scan_exchange(tmp_path, points):
    """--points 8 (the grid's 8 evenly spread points all differ in E0: ladders of one rung, nothing to exchange) and --points 42
    (ladders of one and of two rungs)."""
    text, err = _scan(tmp_path, "x.csv", "--exchange", "50", points=points)
    rows = [line.split(",") for line in text.strip().split("\n")]
    assert rows[0][-1] == "swap_acceptance" and len(rows) == 1 + points
    col = np.array([float(r[-1]) for r in rows[1:]])
    assert np.all((col >= 0.0) & (col <= 1.0))
    E0 = [float(r[0]) for r in rows[1:]]
    sizes = [E0.count(x) for x in sorted(set(E0))]
    assert (max(sizes) == 1) if points == 8 else (set(sizes) == {1, 2})
    m = re.search(r"# exchange every 50 steps: (\d+) rounds in production, (\d+) exchanges attempted, (\d+) accepted", err)
    assert m, err
    rounds, attempted, accepted = (int(x) for x in m.groups())
    assert rounds == 2000 // 50
    first = 400 // 50                                   # the burn-in rung's rounds come first
    pairs = sum(len(tw.schedule(s, t)) for s in sizes for t in range(first, first + rounds))
    assert attempted == pairs * 4 and 0 <= accepted <= attempted          # counts = rounds x pairs x chains
    alone = [k for k, x in enumerate(E0) if E0.count(x) == 1]
    assert np.all(col[alone] == 0.0)
    if points == 42:
        assert attempted > 0 and accepted == round(float(np.sum(col * [4 * 20 if E0.count(x) == 2 else 0 for x in E0])) / 2)


def test_phase_scan_without_exchange_is_unchanged(tmp_path):
    """--exchange 0 and no --exchange at all: the same bytes, and no swap_acceptance column."""
    a, _ = _scan(tmp_path, "a.csv", "--exchange", "0")
    b, _ = _scan(tmp_path, "b.csv")
    assert a == b and "swap_acceptance" not in a
    assert a.split("\n")[0] == "E0,kT,chains,r3,r3_stderr,rsq,p3,p3_stderr,psq,U,U_stderr,AR"
