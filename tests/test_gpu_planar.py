"""GPU tests of the planar (2D) clustering main (pstat_create_planar, pstat_planar.hip) against its CPU restatement
(tests/planar/planar_ref.c) on the same random stream, against closed-form single-monomer integrals, and of every
accessor on a planar handle: series, checkpoint, the carried burn-in rung, the hosts."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ps():
    import polymer_stats_amd as ps
    assert ps._lib.load().pstat_device_count() >= 1
    return ps


@pytest.fixture(scope="module")
def pb():
    from planar import binding
    binding.lib()
    return binding


SHARED = ("E0", "K1", "K2", "mu", "kT", "Fz", "Fx", "b", "phi_step", "adj_lb", "adj_ub", "adj_scale", "cluster_prob", "n",
          "steps_per_adjust", "seed", "chain_type", "energy_type", "umbrella", "rng", "uniform_bits")


def both(ps, pb, num_steps, num_chains, chain_id0=0, **kw):
    """(restatement params, pstat params) of the same planar ensemble; defaults are the planar main's."""
    assert not set(kw) - set(SHARED), set(kw) - set(SHARED)
    return pb.make_params(num_steps=num_steps, **kw), ps.default_planar_params(num_chains=num_chains, chain_id0=chain_id0, **kw)


def assert_chain_equals(ps, e, c, o, n):
    """Chain c of ensemble e against the restatement's run o: the figures of _bit_parity in tests/test_gpu_cluster.py."""
    g = e.chain_state(c)
    assert np.array_equal(g["phi"], o.final_phi), f"phi differs, chain {c}"
    assert np.array_equal(g["theta"], np.zeros(n)), f"theta plane is not zero, chain {c}"
    assert np.array_equal(g["rng"], o.rng), f"rng differs, chain {c}"
    assert g["nacc_total"] == o.nacc_total, c
    assert g["phi_step"] == o.phi_step and g["theta_step"] == 0.0, c
    assert (g["nacc_window"], g["natt_window"]) == (o.nacc_window, o.natt_window), c
    # value / normalizer: with umbrella sampling the gauge constant of the weights cancels
    np.testing.assert_allclose(g["sums"] / g["normalizer"], o.avg, rtol=1e-9, atol=1e-9)
    micro = e.microstate(c)
    np.testing.assert_allclose(micro, o.microstate, rtol=1e-9, atol=1e-8)
    assert micro[1] == 0.0 and micro[4] == 0.0 and all(g["sums"][k] == 0.0 for k in (1, 4, 8, 11))
    x = e.chain_extras(c)
    assert np.all(x["sums"] == 0.0) and np.all(x["now"] == 0.0)


def bit_parity(ps, pb, nsteps, nchains, lanes=None, **kw):
    op, pp = both(ps, pb, nsteps, nchains, **kw)
    with ps.Ensemble(pp, planar=True) as e:
        info = e.launch_info()
        assert "planar" in info.kernel.decode()
        if lanes is not None:
            assert info.lanes_per_block <= lanes, info.lanes_per_block
        e.advance(nsteps)
        for c in range(nchains):
            assert_chain_equals(ps, e, c, pb.run(op, chain_id=c), kw.get("n", 100))
        return info


# ------------------------------------------------------------------------------------------------ 7. bit parity

@pytest.mark.parametrize("rng", [0, 1], ids=["mwc64x", "xoshiro128pp"])
@pytest.mark.parametrize("bits", [23, 53])
def test_bit_parity_dielectric_noninteracting_fz(ps, pb, rng, bits):
    bit_parity(ps, pb, 6000, 70, n=25, E0=1.2, K1=1.0, K2=0.2, Fz=0.7, kT=1.0, seed=21, rng=rng, uniform_bits=bits,
               cluster_prob=0.5, steps_per_adjust=500)


def test_bit_parity_polar_fx_fz(ps, pb):
    bit_parity(ps, pb, 5000, 64, n=17, E0=0.8, mu=0.9, Fz=0.3, Fx=0.25, kT=0.8, b=1.2, chain_type=1, seed=22, cluster_prob=0.3,
               steps_per_adjust=400)


def test_bit_parity_ising_weak_coupling(ps, pb):
    # The planar inversion n -> -n puts a boundary bond anti-parallel whenever it was nearly parallel, and a single move
    # finds the 1/r^3 well of a pair of opposed neighbours with a probability LINEAR in its width (in 3D: quadratic), so
    # under the reference's Ising energy planar chains fall towards r = x_i - x_{i+1} -> 0 within tens of steps at any
    # coupling worth the name (E0 = K1 = 1, n = 12: |U| ~ 1e8 after 40 steps on the restatement).  There a 1e-12 relative
    # difference in r (the restatement's prefix-sum positions against b/2 (n_i + n_j)) moves accept decisions, so bit
    # parity is meaningful only before the collapse: weak coupling (|mu| <= 1e-3) and a short run; on the restatement the
    # deepest of these 66 chains reaches |U| = 980.
    bit_parity(ps, pb, 1500, 66, n=17, E0=0.02, K1=0.05, K2=0.01, Fz=0.3, Fx=0.25, kT=0.8, b=1.2, energy_type=2, seed=22,
               cluster_prob=0.5, steps_per_adjust=400)


@pytest.mark.parametrize("chain_type,E0,mu", [(0, 1.0, 0.7), (1, 0.3, 0.12)], ids=["dielectric", "polar"])
def test_bit_parity_ising_real_coupling_first_steps(ps, pb, chain_type, E0, mu):
    # Pair energies that decide steps: on the restatement they change the path of 120 (dielectric) and 101 (polar) of these 128
    # chains within 25 steps.  Some chains already sit in or pass through a 1/r^3 contact by then (restatement: 18 / 25 chains
    # beyond |U| = 1e3, the deepest 7e9 / 2e9, final 6e8 / 4e8) -- the polar coupling is the weaker one because polar chains fall
    # faster (E0 = 1, mu = 0.7: 84 chains beyond 1e3, 7e10).  The final U of every chain is compared at rtol 1e-9 like the rest:
    # the kernel re-derives its pair sum at the end of a segment.
    bit_parity(ps, pb, 25, 128, n=12, E0=E0, K1=0.6, K2=0.1, mu=mu, Fz=0.4, energy_type=2, chain_type=chain_type, seed=23,
               cluster_prob=0.5)


@pytest.mark.parametrize("rng", [0, 1], ids=["mwc64x", "xoshiro128pp"])
def test_bit_parity_umbrella(ps, pb, rng):
    bit_parity(ps, pb, 4000, 65, n=20, E0=1.5, K1=1.0, K2=0.1, Fz=0.4, kT=1.0, seed=25, umbrella=1, rng=rng, cluster_prob=0.5,
               steps_per_adjust=500)
    bit_parity(ps, pb, 3000, 64, n=16, E0=1.0, mu=0.8, Fz=0.3, Fx=0.1, chain_type=1, seed=26, umbrella=1, rng=rng,
               cluster_prob=0.5, steps_per_adjust=500)


@pytest.mark.parametrize("cluster_prob", [0.0, 1.0])
def test_bit_parity_never_and_always_flip(ps, pb, cluster_prob):
    bit_parity(ps, pb, 4000, 64, n=25, E0=1.0, Fz=0.5, seed=27, cluster_prob=cluster_prob, steps_per_adjust=300)


@pytest.mark.parametrize("n,lanes", [(2, 64), (100, 64), (400, 32), (1300, 8)])
def test_bit_parity_chain_lengths_and_lane_counts(ps, pb, n, lanes):
    # 8-byte cells: 64 lanes up to n = 320, 32 up to 640, 16 up to 1 280, 8 up to 2 560
    nsteps = 3000 if n <= 100 else 1200
    info = bit_parity(ps, pb, nsteps, 67 if n <= 100 else 40, lanes=lanes, n=n, E0=1.0, K1=0.8, K2=0.1, Fz=0.5, Fx=0.2, seed=28 + n,
                      cluster_prob=0.5, steps_per_adjust=500)
    assert info.lds_bytes == 8 * n * info.lanes_per_block


# ------------------------------------------------------------------------------------------------ 8. several cases

@pytest.mark.parametrize("pack", ["0", "1"])
def test_cases_in_one_handle_equal_the_case_alone(ps, pb, pack, monkeypatch):
    monkeypatch.setenv("PSTAT_PACK", pack)
    nsteps, per = 2500, 5
    grid = [dict(E0=0.4 + 0.3 * i, kT=0.7 + 0.1 * (i % 3), Fz=0.2 * i, cluster_prob=(0.5, 0.25, 1.0)[i % 3], seed=100 + i,
                 chain_id0=7 * i) for i in range(9)]
    common = dict(n=20, K1=0.9, K2=0.1, steps_per_adjust=500)
    cases = [ps.default_planar_params(num_chains=per, **common, **g) for g in grid]
    with ps.Ensemble(cases, planar=True) as e:
        info = e.launch_info()
        assert info.packed_cases == int(pack) and ("packed" in info.kernel.decode()) == (pack == "1")
        e.advance(nsteps)
        for i, g in enumerate(grid):
            g = dict(g)
            id0 = g.pop("chain_id0")
            op = pb.make_params(num_steps=nsteps, **common, **g)
            for k in range(per):
                assert_chain_equals(ps, e, i * per + k, pb.run(op, chain_id=id0 + k), 20)


# ------------------------------------------------------------------------------------------------ 9. closed form

def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "planar_closed_form.json")) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("name", ["n20_E0_0_Fz1", "diel_n25_E0_1_K1_1_Fz05", "diel_n100_E0_1_K2_1_Fx1",
                                  "polar_n25_E0_1_mu09_Fz1_Fx025_kT08_b12"])
def test_closed_form_on_the_device(ps, name):
    c = _golden()[name]
    p = c["params"]
    kw = dict(n=p["n"], E0=p["E0"], K1=p["K1"], K2=p["K2"], mu=p["mu"], kT=p["kT"], Fz=p["Fz"], Fx=p["Fx"], b=p["b"],
              chain_type=0 if p["chain"] == "dielectric" else 1)
    with ps.Ensemble(ps.default_planar_params(num_chains=4096, cluster_prob=0.0, seed=20260508, **kw), planar=True) as e:
        e.advance(400 * p["n"])
        e.reset_averages()
        e.advance(1000 * p["n"])
        s = e.summary()
        micro = np.array([e.microstate(k) for k in (0, 1, 4095)])
    avg, se = np.array(s.avg), np.array(s.stderr)
    eq = c["avg"]
    z = np.array([(avg[k] - eq[nm]) / (se[k] + 1e-12 * (1 + abs(eq[nm]))) for k, nm in enumerate(ps.OBS_NAMES)])
    print(name, dict(zip(ps.OBS_NAMES, np.round(z, 2))))
    assert np.all(np.abs(z) < 5.0), dict(zip(ps.OBS_NAMES, np.round(z, 2)))
    assert all(avg[k] == 0.0 and se[k] == 0.0 for k in (1, 4, 8, 11))         # the y slots, exactly
    assert np.all(micro[:, [1, 4]] == 0.0)
    assert tuple(s.extra_avg) == (0.0, 0.0) and s.nan_rejects == 0 and s.chains_collapsed == 0


# ------------------------------------------------------------------------------------------------ 10. series, checkpoint, rung

KW10 = dict(n=14, E0=0.9, K1=0.8, K2=0.15, Fz=0.4, Fx=0.1, kT=0.9, cluster_prob=0.5, steps_per_adjust=300, seed=41)


def test_series_rows_equal_the_accessors(ps):
    cases = [ps.default_planar_params(num_chains=6, **{**KW10, "Fz": 0.1 * i}) for i in range(3)]
    with ps.Ensemble(cases, planar=True) as a, ps.Ensemble(cases, planar=True) as b:
        s = a.open_series(8, angles=True)
        a.advance_series(s, 8 * 250 + 100, 250)
        steps, red, micro, ang = s.read()
        assert list(steps) == [250 * (r + 1) for r in range(8)]
        for r in range(8):
            b.advance(250)
            for k in range(3):
                assert np.array_equal(red[r, k], b.reduce_host(k))
                assert np.array_equal(micro[r, k], b.microstate(6 * k))
                st = b.chain_state(6 * k)
                assert np.array_equal(ang[r, k], np.concatenate([st["theta"], st["phi"]]))
                assert np.all(ang[r, k, :14] == 0.0)
        b.advance(100)
        for c in range(18):
            ga, gb = a.chain_state(c), b.chain_state(c)
            assert all(np.array_equal(ga[k], gb[k]) for k in ga)


def test_checkpoint_restore_and_foreign_images(ps):
    pp = ps.default_planar_params(num_chains=70, umbrella=1, **KW10)
    with ps.Ensemble(pp, planar=True) as e, ps.Ensemble(pp, planar=True) as ref:
        e.advance(700)
        ref.advance(700)
        blob = e.checkpoint()
        e.advance(900)
        e.restore(blob)
        e.advance(1100)
        ref.advance(1100)
        for c in (0, 1, 63, 64, 69):
            ga, gb = e.chain_state(c), ref.chain_state(c)
            assert all(np.array_equal(ga[k], gb[k]) for k in ga), c
            assert np.array_equal(e.microstate(c), ref.microstate(c))
        # a 3D handle of the same shape refuses the planar image, and the planar handle a 3D image; both stay untouched
        p3 = ps.default_params(num_chains=70, umbrella=1, move_set=ps.MOVES_CLUSTER, adj_ub=0.40,
                               **{k: v for k, v in KW10.items()})
        with ps.Ensemble(p3) as e3:
            e3.advance(50)
            before3, before = e3.chain_state(5), e.chain_state(5)
            blob3 = e3.checkpoint()
            assert len(blob3) == len(blob)
            for handle, image in ((e3, blob), (e, blob3)):
                with pytest.raises(ps.PstatError) as ei:
                    handle.restore(image)
                assert ei.value.code == -6 and "planar" in str(ei.value)
            after3, after = e3.chain_state(5), e.chain_state(5)
            assert all(np.array_equal(before3[k], after3[k]) for k in before3)
            assert all(np.array_equal(before[k], after[k]) for k in before)
        # what the planar main does not have
        for call in (lambda: e.reinit(True), lambda: e.restart_from_x0([0.1, 0.2], 0.1, 0.1)):
            with pytest.raises(ps.PstatError) as ei:
                call()
            assert ei.value.code == -4


def test_carried_rung_equals_the_restatement_from_the_carried_chain(ps, pb):
    """scale_kT + reset_sampler + reset_averages, then advance: one mcmc() call of the reference started from the chain the
    previous rung left -- what --carry-burn-in runs."""
    nch = 66
    op, pp = both(ps, pb, 800, nch, **KW10)
    with ps.Ensemble(pp, planar=True) as e:
        e.scale_kT(10.0)
        e.advance(800)
        hot = [pb.run(pb.make_params(num_steps=800, **{**KW10, "kT": KW10["kT"] * 10.0}), chain_id=c) for c in range(nch)]
        for c in (0, 65):
            assert_chain_equals(ps, e, c, hot[c], 14)
        e.scale_kT(1.0)
        e.reset_sampler()
        e.reset_averages()
        e.advance(1200)
        op2 = pb.make_params(num_steps=1200, **KW10)
        for c in range(nch):
            assert_chain_equals(ps, e, c, pb.run(op2, chain_id=c, phi0=hot[c].final_phi, rng0=hot[c].rng), 14)


# ------------------------------------------------------------------------------------------------ 11. hosts end to end

def _values(text):
    from polymer_stats_amd.aggregate_mcmc import julia_value
    return [julia_value(line.split("=")[1]) for line in text.splitlines() if line.strip()]


def test_host_end_to_end_equals_the_restatement(ps, pb, tmp_path):
    prefix = str(tmp_path / "run")
    argv = ["-n", "25", "-e", "0.1", "-J", "0.04", "-u", "Ising", "-F", "1", "-N", "20000", "--num-chains", "1", "--seed", "7",
            "--prefix", prefix, "-v", "2"]
    res = subprocess.run([sys.executable, "-m", "polymer_stats_amd.mcmc_clustering_eap_chain_2d"] + argv, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    assert "burn-in ladder is not run" in res.stderr                  # said once, at -v 2
    lines = res.stdout.splitlines()
    assert [l.split("=")[0].strip() for l in lines] == ["<r>", "<r/nb>", "<rj2>", "<r2>", "<p>", "<pj2>", "<p2>", "<U>", "<U2>", "AR"]
    o = pb.run(pb.make_params(n=25, E0=0.1, K1=0.04, energy_type=2, Fz=1.0, num_steps=20000, seed=7), chain_id=0)
    a = o.avg
    want = [[a[0], a[2]], [a[0] / 25, a[2] / 25], [a[3], a[5]], [a[6]], [a[7], a[9]], [a[10], a[12]], [a[13]], [a[14]], [a[15]],
            [o.nacc_total / 20000]]
    got = _values(res.stdout)
    assert [len(g) for g in got] == [len(w) for w in want]
    for g, w in zip(got, want):
        np.testing.assert_allclose(g, w, rtol=1e-9, atol=1e-9)
    traj = open(prefix + "_trajectory.csv").read().splitlines()
    roll = open(prefix + "_rolling.csv").read().splitlines()
    assert traj[0] == "step,r1,r3,p1,p3,U" and roll[0] == "step,r1,r3,r1sq,r3sq,rsq,p1,p3,p1sq,p3sq,psq,U,Usq"
    assert len(traj) == len(roll) == 1 + 20000 // 500
    last_t, last_r = [float(x) for x in traj[-1].split(",")], [float(x) for x in roll[-1].split(",")]
    assert last_t[0] == last_r[0] == 20000.0
    np.testing.assert_allclose(last_t[1:], [o.r[0], o.r[1], o.p[0], o.p[1], o.U], rtol=1e-9, atol=1e-8)
    np.testing.assert_allclose(last_r[1:], a[ps.PLANAR_OBS_INDEX], rtol=1e-9, atol=1e-9)
    # --burn-in / --burn-schedule change no output; --carry-burn-in does
    again = subprocess.run([sys.executable, "-m", "polymer_stats_amd.mcmc_clustering_eap_chain_2d"] + argv +
                           ["--burn-in", "300", "--burn-schedule", "[5; 1]", "-v", "0"], cwd=ROOT, capture_output=True, text=True,
                           timeout=600)
    assert again.returncode == 0 and again.stdout == res.stdout and "burn-in ladder" not in again.stderr
    carried = subprocess.run([sys.executable, "-m", "polymer_stats_amd.mcmc_clustering_eap_chain_2d"] + argv +
                             ["--burn-in", "300", "--burn-schedule", "[5; 1]", "--carry-burn-in", "-v", "0"], cwd=ROOT,
                             capture_output=True, text=True, timeout=600)
    assert carried.returncode == 0 and carried.stdout != res.stdout
    # the carried run is the restatement's three mcmc() calls on one chain
    kw = dict(n=25, E0=0.1, K1=0.04, energy_type=2, Fz=1.0, seed=7)
    r1 = pb.run(pb.make_params(num_steps=300, **{**kw, "kT": 5.0}), chain_id=0)
    r2 = pb.run(pb.make_params(num_steps=300, **kw), chain_id=0, phi0=r1.final_phi, rng0=r1.rng)
    r3 = pb.run(pb.make_params(num_steps=20000, **kw), chain_id=0, phi0=r2.final_phi, rng0=r2.rng)
    got = _values(carried.stdout)
    np.testing.assert_allclose(got[0], [r3.avg[0], r3.avg[2]], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(got[7], [r3.avg[14]], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(got[9], [r3.nacc_total / 20000], rtol=1e-12)
    # what the device lacks is refused loudly
    bad = subprocess.run([sys.executable, "-m", "polymer_stats_amd.mcmc_clustering_eap_chain_2d", "-n", "10", "-u", "interacting",
                          "-N", "10", "--num-chains", "2", "--prefix", prefix + "x", "-v", "0"], cwd=ROOT, capture_output=True,
                         text=True, timeout=600)
    assert bad.returncode != 0 and "interacting" in bad.stderr


def test_sweep_of_twelve_cases_writes_files_the_aggregator_reads(ps, pb, tmp_path):
    work = tmp_path / "sweep"
    cmd = [sys.executable, os.path.join(ROOT, "tools", "run_sweep.py"), str(work), "--main", "mcmc_clustering_eap_chain_2d",
           "--num-chains", "1", "--seed", "100", "--axis", "b=1", "--axis", "n=25", "--axis", "Fx=0", "--axis", "Fz=0,1,5",
           "--axis", "kT=1", "--axis", "E0=0.1", "--axis", "K1=0.01,0.04", "--axis", "K2=0", "--axis", "run=1:2",
           "--name", "E0,K1,K2,kT,Fz,Fx,n,b,run:raw", "--aggregate", str(tmp_path / "agg.csv"),
           "--aggregate-args", "*.out,dielectric,false,true",
           "--", "--chain-type", "dielectric", "--energy-type", "Ising", "--num-steps", "4000", "--burn-in", "200", "-v", "0"]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    outs = sorted(f for f in os.listdir(work) if f.endswith(".out"))
    assert len(outs) == 12 and "planar_kernel" in res.stderr
    rows = (tmp_path / "agg.csv").read_text().splitlines()
    assert len(rows) == 13 and rows[0].startswith("E0,K1,K2,kT,Fz,Fx,n,b,r1,r2,lambda1,lambda2,") and rows[0].endswith(",AR")
    # case k of the full list runs chain 0 on seed 100 + k: the restatement gives its lines
    name = "E0-0000100_K1-0000040_K2-0000000_kT-0001000_Fz-0005000_Fx-0000000_n-0025000_b-0001000_run-2.out"
    assert name in outs                       # (Fz, K1, run) = (5, 0.04, 2): position 2 * 4 + 1 * 2 + 1 = 11
    o = pb.run(pb.make_params(n=25, E0=0.1, K1=0.04, energy_type=2, Fz=5.0, num_steps=4000, seed=111), chain_id=0)
    got = _values(open(work / name).read())
    np.testing.assert_allclose(got[0], [o.avg[0], o.avg[2]], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(got[7], [o.avg[14]], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(got[9], [o.nacc_total / 4000], rtol=1e-12)
