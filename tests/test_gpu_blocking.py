"""Blocked standard errors on the device (pstat_blocking.hip) against their numpy twin (tests/blocking_ref.py): the
transform of seeded matrices, Series.error_bars on every kind of handle, the two estimators of the library against each
other, the error codes on a live handle, and the two tools' --error-bars."""
import os
import subprocess
import sys

import numpy as np
import pytest

import blocking_ref as br

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R1, R2, R3 = 0, 1, 2


@pytest.fixture(scope="module")
def ps():
    import polymer_stats_amd as ps
    assert ps._lib.load().pstat_device_count() >= 1
    return ps


# ---------------------------------------------------------------------------------------------- 1. matrices
def test_blocking_device_on_torch_tensors():
    """tests/blocking_device_cases.py in a process of its own: torch brings its own HIP runtime, which has to be the first
    one loaded, and this process has loaded libpstat's already.  Every shape of that file against the twin, the constant
    and the NaN column, and the kernel's limit and limit + 1."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "blocking_device_cases.py")], capture_output=True, text=True,
                       timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "all shapes agree" in r.stdout


# ---------------------------------------------------------------------------------------------- 2. series
def series_check(ps, e, nrows, stepout, min_blocks=32, want_batches=None):
    s = e.open_series(nrows)
    e.advance_series(s, nrows * stepout, stepout)
    got = s.error_bars(min_blocks=min_blocks, levels=True)
    steps, red, _, _ = s.read()
    x = br.batches(steps, red)
    assert got.nbatches == x.shape[0] == (want_batches or nrows)
    assert got.mean.shape == (e.ncases, ps.NQ) and got.levels.shape == (e.ncases, ps.NQ, 24)
    br.compare(got, br.blocking(x, min_blocks), x, min_blocks)
    return s, got, steps, red


def test_series_error_bars_against_the_twin(ps):
    cases = [ps.default_params(n=10, E0=1.0, K1=1.0, Fz=fz, num_chains=5, seed=31 + k) for k, fz in enumerate((0.5, 1.0, 2.0))]
    with ps.Ensemble(cases) as e:
        e.advance(300)
        e.reset_averages()
        s, got, steps, red = series_check(ps, e, 200, 20)           # from empty averages: 200 batches
        assert steps[0] == 20
        np.testing.assert_allclose(got.mean[:, :16], red[-1][:, 1:17] / 5.0, rtol=1e-10, atol=1e-12)
        assert np.all(got.stderr[:, [R1, R3, 14]] > 0)
        # first_row / nrows select what the twin gets on the sliced rows
        for first, nrows in ((0, 100), (37, 64), (150, None), (0, 33)):
            sub = s.error_bars(first_row=first, nrows=nrows, levels=True)
            x = br.batches(steps, red, first, nrows)
            assert sub.nbatches == x.shape[0] == ((nrows or 200 - first) - (0 if first == 0 else 1))
            br.compare(sub, br.blocking(x, 32), x, 32, f"rows {first}+{nrows}")
        s.close()
    with ps.Ensemble(cases) as e:
        e.advance(130)                                              # the first row is the baseline: 199 batches
        s, got, steps, _ = series_check(ps, e, 200, 20, want_batches=199)
        assert steps[0] == 150
        s.close()


def test_series_error_bars_one_chain(ps):
    with ps.Ensemble(ps.default_params(n=10, E0=1.0, Fz=1.0, num_chains=1, seed=5)) as e:
        series_check(ps, e, 128, 25)[0].close()


def test_series_error_bars_planar(ps):
    cases = [ps.default_planar_params(n=12, E0=1.0, K1=0.5, Fz=1.0, energy_type=ps.ISING, num_chains=6, seed=8 + k) for k in range(2)]
    with ps.Ensemble(cases, planar=True) as e:
        s, got, _, _ = series_check(ps, e, 96, 30)
        y = [ps.EB_NAMES.index(k) for k in ("r2", "r2sq", "p2", "p2sq")]
        assert np.all(got.stderr[:, y] == 0) and np.all(got.inefficiency[:, y] == 1) and np.all(got.converged[:, y])
        assert np.all(got.stderr[:, [R1, R3]] > 0)
        s.close()


def test_series_error_bars_clustering_main_group_per_case(ps):
    cases = [ps.default_params(n=16, E0=1.0, K1=0.3, K2=0.02, Fz=0.5, seed=9 + k, bend_mod=0.4, bend_angle=0.2, cluster_prob=0.5,
                               move_set=ps.MOVES_CLUSTER, energy_type=ps.ISING, num_chains=70) for k in range(2)]
    with ps.Ensemble(cases) as e:
        s, got, _, _ = series_check(ps, e, 64, 10)
        assert np.all(got.stderr[:, 17:] > 0)                      # sum cos^2 theta and the bond angle are recorded here
        s.close()


def test_blocked_and_across_chain_estimates_agree(ps):
    """8 cases of equal physics, 64 chains each: median over the cases of blocked stderr(r3) / across-chain stderr(r3) within
    [0.7, 1.3].  The across-chain estimate has 63 degrees of freedom (9 % relative scatter), the blocked one at least 31
    (13 %); a median of 8 has about 7 %, so +-0.3 is about four standard deviations plus the few per cent of blocking bias.
    A missing square root, a missing / chains or an off-by-one in d falls outside."""
    cases = [ps.default_params(n=10, Fz=1.0, num_chains=64, seed=100 + k) for k in range(8)]
    with ps.Ensemble(cases) as e:
        e.advance(5000)
        e.reset_averages()
        s = e.open_series(512)
        e.advance_series(s, 512 * 50, 50)
        eb = s.error_bars()
        ratio = np.array([eb.stderr[k, R3] / e.summary(k).stderr[R3] for k in range(8)])
        print("blocked / across-chain stderr(r3):", np.round(ratio, 3), "median %.3f" % np.median(ratio))
        assert eb.nbatches == 512
        assert 0.7 <= np.median(ratio) <= 1.3
        np.testing.assert_allclose(eb.mean[:, R3], [e.summary(k).avg[R3] for k in range(8)], rtol=1e-10)
        s.close()


def test_error_codes_on_a_live_handle(ps):
    def code(call):
        with pytest.raises(ps.PstatError) as err:
            call()
        return err.value.code, str(err.value)
    p = ps.default_params(n=10, E0=1.0, Fz=1.0, num_chains=4, seed=2)
    with ps.Ensemble(ps.default_params(n=10, E0=1.0, Fz=1.0, num_chains=4, seed=2, umbrella=1)) as u:
        s = u.open_series(40)
        u.advance_series(s, 400, 10)
        assert code(s.error_bars)[0] == -4
    with ps.Ensemble(p) as e, ps.Ensemble(p) as other:
        s = e.open_series(100)
        e.advance_series(s, 400, 10)
        assert s.error_bars().nbatches == 40
        e.advance_series(s, 400, 20)                    # another stepout: row 40 breaks the spacing
        rc, text = code(s.error_bars)
        assert rc == -1 and "row 40" in text
        assert s.error_bars(nrows=40).nbatches == 40 and s.error_bars(first_row=40, min_blocks=8).nbatches == 19
        s.clear()
        e.advance_series(s, 400, 10)
        e.reset_averages()
        e.advance_series(s, 400, 10)                    # the step count starts over at row 40
        rc, text = code(s.error_bars)
        assert rc == -1 and "row 40" in text
        assert s.error_bars(first_row=40).nbatches == 40
        # a series of another handle; rows outside the recorded ones; min_blocks
        foreign = other.open_series(40)
        other.advance_series(foreign, 400, 10)
        lib, dp = ps._lib.load(), __import__("ctypes").POINTER(__import__("ctypes").c_double)
        out = np.zeros((1, ps.NQ, 6))
        assert lib.pstat_series_error_bars(e._h, foreign._s, 0, -1, 0, None, out.ctypes.data_as(dp), None) == -1
        assert code(lambda: s.error_bars(first_row=41, nrows=40))[0] == -1
        assert code(lambda: s.error_bars(first_row=-1))[0] == -1
        assert code(lambda: s.error_bars(first_row=40, min_blocks=1))[0] == -1
        # 10 rows at min_blocks 32: too few, and the count is written back
        import ctypes as C
        nb = C.c_int64(-5)
        assert lib.pstat_series_error_bars(e._h, s._s, 40, 10, 32, C.byref(nb), out.ctypes.data_as(dp), None) == -7
        assert nb.value == 10
        # none of this has disturbed the handle
        assert s.error_bars(first_row=40, levels=True).nbatches == 40


# ---------------------------------------------------------------------------------------------- 3. the tools
def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout + r.stderr


SWEEP_FIXED = ["--num-steps", "6400", "-v", "0"]


@pytest.fixture(scope="module")
def sweeps(tmp_path_factory):
    """tools/run_sweep.py on 4 single-chain cases, without and with --error-bars 64, same seed: the two directories."""
    tmp = tmp_path_factory.mktemp("sweeps")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "run_sweep.py")]
    common = ["--num-chains", "1", "--seed", "17", "--axis", "n=10", "--axis", "E0=1", "--axis", "Fz=0.5,1,2,4"]
    _run(cmd + [str(tmp / "plain"), *common, "--", *SWEEP_FIXED])
    _run(cmd + [str(tmp / "eb"), *common, "--error-bars", "64", "--", *SWEEP_FIXED])
    return tmp / "plain", tmp / "eb"


def _values(path):
    from polymer_stats_amd.aggregate_mcmc import julia_value
    lines = open(path).read().splitlines()          # the consumers' split('=') + eval
    return [l.split("=")[0] for l in lines], {l.split("=")[0].strip(): julia_value(l.split("=")[1]) for l in lines}


def test_run_sweep_error_bars_writes_err_files(ps, sweeps):
    from polymer_stats_amd import sweep as sw
    plain, eb = sweeps
    outs = sorted(os.listdir(plain))
    assert len(outs) == 4 and all(f.endswith(".out") for f in outs)
    assert sorted(os.listdir(eb)) == sorted(outs + [f[:-4] + ".err" for f in outs])
    cases = sw.product_cases([("n", [10]), ("E0", [1]), ("Fz", [0.5, 1, 2, 4])])
    plan = sw.plan("mcmc_eap_chain", SWEEP_FIXED, cases, str(eb), num_chains=1, seed=17)
    with ps.Ensemble([sw.fixed_main.params_from_pargs(p, 1, 0, 0) for p in plan]) as e:
        s = e.open_series(64)
        e.advance_series(s, 6400, 100)
        want = s.error_bars()
    for k, p in enumerate(plan):
        name = p["_name"]
        out_names, outv = _values(eb / (name + ".out"))
        err_names, vals = _values(eb / (name + ".err"))
        assert err_names[:len(out_names)] == out_names
        assert [n.strip() for n in err_names[len(out_names):]] == ["batches", "inefficiency", "converged"]
        for key in outv:
            assert len(vals[key]) == len(outv[key]), key
        for key in ("<r>", "<U>", "AR"):
            assert np.all(np.isfinite(vals[key])) and np.all(np.array(vals[key]) > 0), (name, key, vals[key])
        assert vals["batches"] == [64.0] and len(vals["inefficiency"]) == len(vals["converged"]) == ps.NQ
        np.testing.assert_allclose(vals["<r>"], want.stderr[k, :3], rtol=1e-9)
        np.testing.assert_allclose(vals["<r/nb>"], want.stderr[k, :3] / 10.0, rtol=1e-9)


def test_run_sweep_error_bars_leaves_the_out_files_byte_identical(sweeps):
    """Every .out of the --error-bars run equals, byte for byte, that of the same command without the flag.  (A recorded run
    alone does not give that: 64 launches of 100 steps add the running sums in another order than one launch of 6 400 --
    measured, all 4 files differed in the last digit or two, 7e-16 relative -- so the pool repeats the production run as one
    launch from a checkpoint, _Pool.error_bars.)"""
    plain, eb = sweeps
    different = [f for f in sorted(os.listdir(plain)) if open(plain / f, "rb").read() != open(eb / f, "rb").read()]
    assert not different, f".out files differ from the run without --error-bars: {different}"


def test_phase_scan_error_bars(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "phase_scan.py"), "--points", "4", "--chains", "1", "--steps", "6400"]
    _run(cmd + ["--out", str(tmp_path / "plain.csv")])
    _run(cmd + ["--error-bars", "64", "--out", str(tmp_path / "eb.csv")])
    plain = [l.split(",") for l in open(tmp_path / "plain.csv").read().splitlines()]
    eb = [l.split(",") for l in open(tmp_path / "eb.csv").read().splitlines()]
    assert eb[0] == plain[0] + ["r3_blocked", "p3_blocked", "U_blocked", "r3_ineff", "U_ineff", "converged"]
    assert len(eb) == len(plain) == 5
    for a, b in zip(plain[1:], eb[1:]):
        assert len(b) == len(eb[0]) and np.all(np.isfinite([float(v) for v in b[len(a):]]))
        assert [float(v) for v in b[:len(a)]] == [float(v) for v in a]
        assert b[-1] in ("0", "1")


def test_error_bars_when_the_steps_are_no_multiple_of_the_batches(ps, tmp_path):
    """--num-steps 1000 --error-bars 64: 64 batches of 15 steps, the other 40 steps in none (advance_series alone would record
    66 rows).  Also: a directory swept without error bars first gets its .err files, and the same .out files, afterwards."""
    from polymer_stats_amd import sweep as sw
    fixed = ["--num-steps", "1000", "-v", "0"]
    cases = sw.product_cases([("n", [10]), ("E0", [1]), ("Fz", [0.5, 2])])
    kw = dict(num_chains=2, seed=23)
    work = str(tmp_path / "w")
    first = sw.run_sweep("mcmc_eap_chain", fixed, cases, work, **kw)
    assert len(first["ran"]) == 2 and sorted(os.listdir(work)) == sorted(n + ".out" for n in first["ran"])
    plain = {n: open(os.path.join(work, n + ".out"), "rb").read() for n in first["ran"]}
    again = sw.run_sweep("mcmc_eap_chain", fixed, cases, work, error_bars=64, **kw)
    assert again["ran"] == first["ran"] and not again["skipped"]             # the .err files were missing
    third = sw.run_sweep("mcmc_eap_chain", fixed, cases, work, error_bars=64, **kw)
    assert not third["ran"] and third["skipped"] == first["ran"]
    plan = sw.plan("mcmc_eap_chain", fixed, cases, work, **kw)
    with ps.Ensemble([sw.fixed_main.params_from_pargs(p, 2, 0, 0) for p in plan]) as e:
        s = e.open_series(64)
        e.advance_series(s, 64 * 15, 15)
        want = s.error_bars()
    for k, name in enumerate(first["ran"]):
        assert open(os.path.join(work, name + ".out"), "rb").read() == plain[name], name
        vals = _values(os.path.join(work, name + ".err"))[1]
        assert vals["batches"] == [64.0]
        np.testing.assert_allclose(vals["<r>"], want.stderr[k, :3], rtol=1e-9)
    # the pool itself, on each main's own stage protocol, with a remainder
    for main_name, extra in (("mcmc_clustering_eap_chain", ["--burn-in", "100", "--burn-schedule", "[2; 1]"]),
                             ("mcmc_clustering_eap_chain_2d", [])):
        res = sw.run_sweep(main_name, ["--num-steps", "777", "-v", "0", "--num-monomers", "8", *extra], [dict(E0=1.0, Fz=1.0)],
                           str(tmp_path / main_name), num_chains=3, seed=5, error_bars=33)
        name = res["ran"][0]
        assert _values(os.path.join(str(tmp_path / main_name), name + ".err"))[1]["batches"] == [33.0]


def test_phase_scan_error_bars_with_a_remainder(tmp_path):
    out = tmp_path / "eb.csv"
    _run([sys.executable, os.path.join(ROOT, "tools", "phase_scan.py"), "--points", "3", "--chains", "2", "--n", "20", "--burn-in", "0",
          "--steps", "1000", "--error-bars", "64", "--out", str(out)])
    rows = [l.split(",") for l in open(out).read().splitlines()]
    assert len(rows) == 4 and rows[0][-6:] == ["r3_blocked", "p3_blocked", "U_blocked", "r3_ineff", "U_ineff", "converged"]
    assert all(np.all(np.isfinite([float(v) for v in r])) for r in rows[1:])
