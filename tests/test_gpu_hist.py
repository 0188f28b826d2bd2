"""GPU tests of the per-case histograms (pstat_hist_*, pstat_histogram_device, pstat_hist.hip) against the numpy
twin of the binning formula (tests/hist_ref.py): counts equal AS INTEGERS to the twin on the microstates of an identical second
ensemble, on every mapping of the kernel and on five homes; crafted edge values through a torch tensor; a closed-form density;
recording between exchange rounds; refusals; tools/run_sweep.py --hist and tools/free_energy.py end to end.  The protocol of the
comparison (run_hist_twin), the homes and the tool call are those of tests/recorder_cases.py; the lifecycle rules are asserted
in tests/test_gpu_recorder_lifecycle.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import hist_ref as hr
import recorder_cases as rc
from recorder_cases import ps  # noqa: F401 (the fixture)
from recorder_cases import run_hist_twin as run_exact

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = dict(E0=1.0, K1=0.5, Fz=0.5, steps_per_adjust=150)             # (no K2, unlike the other recorders' rc.BASE)


def component_specs(ps, n, with_magnitudes=True):
    """nbins 1, 2 and 64; ranges that leave samples in both tails of some and in none of others."""
    s = [ps.hist_spec("r1", 64, -0.3 * n, 0.3 * n), ps.hist_spec("r2", 2, -1.0, 1.5), ps.hist_spec("r3", 1, 0.0, 0.5 * n),
         ps.hist_spec("p1", 64, -1.0, 1.0), ps.hist_spec("p2", 2, -50.0, 50.0), ps.hist_spec("p3", 64, 0.0, 0.4 * n),
         ps.hist_spec("U", 64, -1.0 * n, 0.25 * n)]
    if with_magnitudes:
        s += [ps.hist_spec("rmag", 64, 0.0, 1.0 * n), ps.hist_spec("pmag", 64, 0.0, 0.6 * n)]
    return s


# ------------------------------------------------------------------------------------------------ every mapping of the kernel
# chains per case: 1, 5, 64 (one wavefront per case, its last lane), 65 (the LDS kernel), 300, and 1100 > GROUP_SAMPLES = 1024 of
# pstat_hist.hip (two workgroups per case); 1, 3 and 9 cases (9: the last workgroup of the wave kernel is not full)
SHAPES = [(1, 1), (3, 5), (9, 64), (9, 65), (3, 300), (2, 1100)]


@pytest.mark.parametrize("ncases,per", SHAPES)
def test_counts_equal_the_twin_as_integers(ps, ncases, per):
    cases = [ps.default_params(n=12, num_chains=per, precision=ps.F64, kT=0.7 + 0.2 * k, seed=500 + k, **BASE) for k in range(ncases)]
    got = run_exact(ps, cases, [component_specs(ps, 12)])
    assert sum(int(c.sum()) for c in got.counts) > 0
    if ncases * per >= 64:
        assert got.tails[:, 0].sum() > 0 and got.counts[0].sum() > 0, "r1's range shows nothing: no sample in a tail, or none inside"


@pytest.mark.parametrize("ncases,per", [(2, 5), (3, 300)])
def test_a_handle_with_exactly_the_most_bins(ps, ncases, per):
    n = 12
    nb = [4096, 2048, 1024, 512, 256, 128, 128]
    assert sum(nb) == ps._lib.HIST_MAX_BINS
    rng = [(-0.3 * n, 0.3 * n), (-0.3 * n, 0.3 * n), (-0.2 * n, 0.6 * n), (-1.0, 1.0), (-1.0, 1.0), (0.0, 0.4 * n), (-1.0 * n, 0.25 * n)]
    specs = [ps.hist_spec(ch, nb[ch], *rng[ch]) for ch in range(7)]
    cases = [ps.default_params(n=n, num_chains=per, precision=ps.F64, kT=0.7 + 0.2 * k, seed=600 + k, **BASE) for k in range(ncases)]
    got = run_exact(ps, cases, [specs])
    assert got.counts[0].shape == (ncases, 4096) and got.counts[6][:, -1].shape == (ncases,)
    with ps.Ensemble(cases) as e:                                    # one bin more is refused, the handle stays usable
        with pytest.raises(ps.PstatError) as err:
            e.open_hist(specs + [ps.hist_spec("U", 1, 0.0, 1.0)])
        assert err.value.code == -4 and "8193" in str(err.value)
        e.advance(10)
        assert e.chain_state(0)["steps_recorded"] == 10


# ------------------------------------------------------------------------------------------------ the homes
@pytest.mark.parametrize("home", list(rc.HOMES)[:5])                 # the first five, all at 70 chains per case; with BASE above
def test_every_home_and_a_per_case_range(ps, home):
    cases, planar = rc.home_cases(ps, home, seed=700, base=BASE)
    n, E0 = int(cases[0].n), [c.E0 for c in cases]
    # U's range follows E0: only lo and hi differ between the cases
    rows = [component_specs(ps, n)[:6] + [ps.hist_spec("U", 64, -(0.4 + x * x) * n, 0.3 * n)] + component_specs(ps, n)[7:] for x in E0]
    got = run_exact(ps, cases, rows, per_case=True, planar=planar)
    assert not np.array_equal(got.edges(6, 0), got.edges(6, 2)) and np.array_equal(got.edges(0, 0), got.edges(0, 2))
    if planar:      # the y channels (r2, p2): every sample in whichever bin holds 0
        for i in (1, 4):
            sp = rows[0][i]
            zero = np.bincount(hr.slots([0.0], sp.lo, sp.hi, sp.nbins), minlength=sp.nbins)[:sp.nbins] * got.samples
            assert zero.sum() == got.samples and np.array_equal(got.counts[i], np.tile(zero, (3, 1))) and got.tails[:, i].sum() == 0


# ------------------------------------------------------------------------------------------------ crafted values
def test_crafted_values_through_a_torch_tensor():
    """tests/hist_device_cases.py in a process of its own: torch brings its own HIP runtime, which has to be the first one loaded,
    and this process has loaded libpstat's already.  Edge values, +-0, denormals, NaN, +-inf in matrices of 1, 63, 64, 65 and
    100 000 rows with a stride above the column count: all equal to the twin exactly."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "hist_device_cases.py")], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "all matrices agree" in r.stdout


# ------------------------------------------------------------------------------------------------ a closed-form density
def test_closed_form_density_of_the_extension(ps):
    """Device figures (MI355X): see DESIGN.md 3.14."""
    with open(os.path.join(ROOT, "tests", "golden", "hist_closed_form.json")) as f:
        golden = json.load(f)
    N = 16384
    cases = [ps.default_params(n=c["n"], E0=c["E0"], K1=c["K1"], K2=c["K2"], Fz=c["Fz"], kT=golden["kT"], b=golden["b"], num_chains=N,
                               precision=ps.F64, seed=20261019 + i) for i, c in enumerate(golden["cases"])]
    with ps.Ensemble(cases) as e:
        assert "sweep_kernel" in e.launch_info().kernel.decode()
        h = e.open_hist([ps.hist_spec("r3", golden["nbins"], golden["cases"][0]["lo"], golden["cases"][0]["hi"])])
        e.advance(400 * golden["cases"][0]["n"])
        h.record()
        got = h.read()
    assert got.records == 1 and got.samples == N and got.tails.sum() == 0
    for k, c in enumerate(golden["cases"]):
        p = np.array(c["prob"])
        tested = N * p >= 50
        z = (got.counts[0][k] - N * p) / np.sqrt(N * p * (1 - p))
        print(f"case {k} (E0 = {c['E0']}, Fz = {c['Fz']}): {tested.sum()} bins tested holding {p[tested].sum():.4f}, max |z| = {np.abs(z[tested]).max():.2f}")
        assert p[tested].sum() >= 0.99
        assert np.all(np.abs(z[tested]) < 5.0), np.round(z, 2)
        np.testing.assert_allclose(got.density(0, k).sum() * 0.5, 1.0, rtol=1e-12)
        assert np.array_equal(got.centers(0, k), -8.0 + 0.5 * (np.arange(32) + 0.5))


# ------------------------------------------------------------------------------------------------ with tempering
def test_records_between_exchange_rounds(ps):
    cases = rc.ladder_cases(ps)
    rows = [[ps.hist_spec("r3", 32, -8.0, 8.0), ps.hist_spec("U", 64, -40.0, 0.0)]]
    got, micro = rc.records_between_exchange_rounds(ps, cases, lambda e: e.open_hist(rows[0]), rc.micro_of_all)
    want, want_tails = rc.twin_counts(micro, rows, 7)
    for i in range(2):
        assert np.array_equal(got.counts[i], want[i]) and np.array_equal(got.tails[:, i], want_tails[:, i])
        assert np.array_equal(got.counts[i].sum(axis=1) + got.tails[:, i].sum(axis=1), np.full(7, 5 * 64))
    assert got.samples == 5 * 64


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_handle_usable(ps):
    spec = [ps.hist_spec("r3", 8, -6.0, 6.0)]
    with ps.Ensemble([ps.default_params(n=6, num_chains=4, kT=kT, umbrella=1) for kT in (1.0, 2.0)]) as e:
        with pytest.raises(ps.PstatError) as err:
            e.open_hist(spec)
        assert err.value.code == -4 and "umbrella" in str(err.value)
        e.advance(20)
        assert e.chain_state(0)["steps_recorded"] == 20
    cases = [ps.default_params(n=6, num_chains=4, kT=kT, Fz=0.3) for kT in (1.0, 2.0, 3.0)]
    with ps.Ensemble(cases) as e:
        for bad, code, needle in (([ps.hist_spec(9, 8, 0.0, 1.0)], -1, "channel 9"), ([ps.hist_spec("U", 0, 0.0, 1.0)], -1, "nbins"),
                                  ([ps.hist_spec("U", 4, 1.0, 1.0)], -1, "above lo"), ([ps.hist_spec("U", 4, 0.0, float("nan"))], -1, "finite"),
                                  (spec * 17, -1, "nspecs")):
            with pytest.raises(ps.PstatError) as err:
                e.open_hist(bad)
            assert err.value.code == code and needle in str(err.value), str(err.value)
        with pytest.raises(ps.PstatError) as err:                   # per case: channel and nbins must agree
            e.open_hist([spec, [ps.hist_spec("r3", 9, -6.0, 6.0)], spec], per_case=True)
        assert err.value.code == -1 and "case 1" in str(err.value)
        with pytest.raises(ValueError):
            e.open_hist([spec, spec], per_case=True)
        h = e.open_hist(spec)
        e.advance_hist(h, 25, 10)
        got = h.read()
        assert got.records == 2 and e.chain_state(0)["steps_recorded"] == 25
        assert np.array_equal(got.counts[0].sum(axis=1) + got.tails[:, 0].sum(axis=1), [8, 8, 8])
        h.clear()                                                    # clear, then read: zeros
        got = h.read()
        assert got.records == 0 and got.counts[0].sum() == 0 and got.tails.sum() == 0
        h.record()
        assert h.read().counts[0].sum() + h.read().tails.sum() == 12
        e.advance(5)                                                 # the handle still advances
        assert e.chain_state(0)["steps_recorded"] == 30


# ------------------------------------------------------------------------------------------------ the tools
def test_sweep_writes_hist_files_and_free_energy_reads_them(tmp_path):
    axes, fixed = [("n", "8"), ("Fz", "0,0.5,1,1.5,2,2.5")], ["--num-steps", "3000", "--stepout", "100", "-v", "0"]
    with_hist = rc.sweep_tool(tmp_path, "h", "--hist", "r3:-8:8:32", "--hist", "U:-10:2:16", axes=axes, fixed=fixed)
    plain = rc.sweep_tool(tmp_path, "p", axes=axes, fixed=fixed)
    outs, hists = rc.assert_out_files_unchanged(with_hist, plain, ".hist")
    assert len(outs) == 6
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import free_energy as fe
    for f in hists:
        r3, U = fe.read_hist(str(with_hist / f))
        assert (r3["channel"], r3["nbins"], r3["records"], r3["chains"], r3["lo"], r3["hi"]) == ("r3", 32, 30, 64, -8.0, 8.0)
        assert r3["counts"].sum() + sum(r3["tails"].values()) == 30 * 64 and U["counts"].sum() + sum(U["tails"].values()) == 30 * 64
        assert U["channel"] == "U" and len(U["counts"]) == 16 and np.array_equal(r3["edges"], np.linspace(-8, 8, 33))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "free_energy.py"), str(with_hist), "--component", "r3"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    csvs = [f for f in os.listdir(with_hist) if f.endswith(".csv")]
    assert csvs == ["n-0008000_A_r3.csv"], csvs
    lines = (with_hist / csvs[0]).read_text().strip().split("\n")
    assert lines[0] == "x,A,sigma,samples" and len(lines) > 8
    table = np.array([[float(v) for v in line.split(",")] for line in lines[1:]])
    assert np.all(np.isfinite(table)) and table[:, 1].min() == 0.0 and table[:, 3].sum() == 6 * 30 * 64 and np.all(table[:, 3] > 0)
    # the zero-force free energy of a chain of 8 free monomers has its minimum near r_z = 0
    assert abs(table[np.argmin(table[:, 1]), 0]) <= 1.5
