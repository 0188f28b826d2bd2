"""Histograms without a GPU: the seven entry points' declarations, exports and argument errors; the numpy twin
of the binning formula (tests/hist_ref.py); the closed-form fixture and its generator; wham_force and extension_free_energy of
polymer_stats_amd/free_energy.py on synthetic counts drawn from the fixture's densities."""
import ctypes as C
import importlib.util
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import hist_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["pstat_hist_open", "pstat_hist_record", "pstat_advance_hist", "pstat_hist_read", "pstat_hist_clear",
                "pstat_hist_close", "pstat_histogram_device"]


@pytest.fixture(scope="module")
def ps():
    import polymer_stats_amd as ps
    ps._lib.load()
    return ps


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_hist_closed_form", os.path.join(ROOT, "tests", "golden", "make_hist_closed_form.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "hist_closed_form.json")) as f:
        return json.load(f)


# ---------------------------------------------------------------------------------------------- declarations
def test_declared_exported_and_listed(ps):
    with open(os.path.join(ROOT, "include", "pstat.h")) as f:
        header = f.read()
    lib = ps._lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\b(int|void)\s+%s\(" % name, header), name
        assert name in ps._lib.SYMBOLS and getattr(lib, name) is not None
    assert "#define PSTAT_ABI_VERSION 6" in header and lib.pstat_abi_version() == 6 and ps._lib.ABI_VERSION == 6
    assert "#define PSTAT_HIST_MAX_BINS 8192" in header and ps._lib.HIST_MAX_BINS == 8192
    assert "#define PSTAT_HIST_MAX_SPECS 16" in header and ps._lib.HIST_MAX_SPECS == 16
    assert "pstat_series_error_bars, pstat_hist_read) it fails" in header          # the list of synchronising accessors
    assert ps.HC_NAMES == hr.CHANNELS and ps.hist_spec("r3", 4, -1, 1).channel == 2 and ps.hist_spec("pmag", 4, 0, 1).channel == 8
    with pytest.raises(ValueError):
        ps.hist_spec("r4", 4, -1, 1)


BAD_SPECS = {
    "no specs": ([], -1, "nspecs"),
    "17 specs": ([(0, 4, 0.0, 1.0)] * 17, -1, "nspecs"),
    "negative channel": ([(0, 4, 0.0, 1.0), (-1, 4, 0.0, 1.0)], -1, "spec 1"),
    "channel at stride": ([(3, 4, 0.0, 1.0)], -1, "channel 3"),
    "no bins": ([(0, 0, 0.0, 1.0)], -1, "nbins"),
    "lo is NaN": ([(0, 4, float("nan"), 1.0)], -1, "finite"),
    "hi is inf": ([(0, 4, 0.0, float("inf"))], -1, "finite"),
    "hi == lo": ([(0, 4, 1.0, 1.0)], -1, "above lo"),
    "hi < lo": ([(0, 4, 1.0, 0.5)], -1, "above lo"),
    "hi - lo overflows": ([(0, 4, -1e308, 1e308)], -1, "hi - lo"),
    "hi - lo too small": ([(0, 8192, 0.0, 5e-324)], -1, "hi - lo"),
    "too many bins": ([(0, 8192, 0.0, 1.0), (1, 1, 0.0, 1.0)], -4, "8193 bins"),
}


@pytest.mark.parametrize("what", list(BAD_SPECS))
def test_histogram_device_argument_errors_need_no_gpu(ps, what):
    """Raised before the device is touched: the pointer is never read (and this machine may have no GPU at all)."""
    specs, code, needle = BAD_SPECS[what]
    with pytest.raises(ps.PstatError) as err:
        ps.histogram_device(0x1000, 10, 3, [ps.hist_spec(*s) for s in specs])
    assert err.value.code == code and needle in str(err.value), str(err.value)
    assert ps._lib.load().pstat_last_error()


def test_histogram_device_other_argument_errors(ps):
    ok = [ps.hist_spec(0, 4, 0.0, 1.0)]
    for kw, needle in ((dict(ptr=0x1000, nrows=-1, stride=3), "nrows"), (dict(ptr=0, nrows=10, stride=3), "null"),
                       (dict(ptr=0x1000, nrows=10, stride=0), "stride")):
        with pytest.raises(ps.PstatError) as err:
            ps.histogram_device(kw["ptr"], kw["nrows"], kw["stride"], ok)
        assert err.value.code == -1 and needle in str(err.value)
    lib = ps._lib.load()
    out = C.c_void_p()
    assert lib.pstat_hist_open(None, None, 1, 0, C.byref(out)) == -1 and lib.pstat_last_error()
    assert lib.pstat_hist_record(None, None) == -1 and lib.pstat_advance_hist(None, None, 1, 1) == -1
    assert lib.pstat_hist_read(None, None, None, None, None) == -1 and lib.pstat_hist_clear(None, None) == -1
    lib.pstat_hist_close(None, None)


# ---------------------------------------------------------------------------------------------- the twin
def test_twin_agrees_with_numpy_away_from_edges():
    rng = np.random.default_rng(20261019)
    for lo, hi, nbins in ((-8.0, 8.0, 32), (0.1, 0.7, 7), (-3.0, 11.5, 64), (2.0, 3.0, 1)):
        edges = lo + (hi - lo) * np.arange(nbins + 1) / nbins
        x = rng.uniform(lo - 0.2 * (hi - lo), hi + 0.2 * (hi - lo), 20000)
        x = x[np.min(np.abs(x[:, None] - edges[None, :]), axis=1) >= 1e-9]
        counts, tails = hr.bin_counts(x, lo, hi, nbins)
        want, _ = np.histogram(x, bins=edges)
        assert np.array_equal(counts, want)
        assert tails.tolist() == [int(np.sum(x < lo)), int(np.sum(x > hi)), 0]
        assert counts.sum() + tails.sum() == len(x) and counts.dtype == np.int64


def test_twin_at_the_ends_and_on_non_finite_values():
    lo, hi, nbins = -1.5, 2.5, 8
    assert hr.slots([lo], lo, hi, nbins)[0] == 0                    # lo is in bin 0
    assert hr.slots([hi], lo, hi, nbins)[0] == nbins + 1            # hi is in the upper tail
    assert hr.slots([np.nextafter(lo, -np.inf)], lo, hi, nbins)[0] == nbins
    assert hr.slots([np.nan, np.inf, -np.inf], lo, hi, nbins).tolist() == [nbins + 2] * 3
    assert hr.slots([0.0, -0.0], 0.0, 1.0, 4).tolist() == [0, 0]    # -0.0 * inv = -0.0, which is not < 0
    assert hr.slots([-1.7e308], 1e307, 1e308, 4)[0] == 4 and hr.slots([1.7e308], -1e308, -1e307, 4)[0] == 5   # x - lo overflows: t = -+inf
    counts, tails = hr.bin_counts([lo, hi, np.nan, 0.4, 0.6], lo, hi, nbins)
    assert counts.tolist() == [1, 0, 0, 1, 1, 0, 0, 0] and tails.tolist() == [0, 1, 1]
    assert hr.channel_values(np.array([[3.0, 0.0, 4.0, 0, 0, 0, 7.0]]), 7)[0] == 5.0 and hr.channel_values(np.ones((2, 7)), 6).tolist() == [1, 1]


# ---------------------------------------------------------------------------------------------- the fixture
def test_generator_against_irwin_hall(gen):
    assert gen.validate(8) < 1e-6
    s, p = gen.density_of_sum(8, 0.0, 0.0)
    assert abs(np.sum((p[:-1] + p[1:]) * 0.5 * gen.H) - 1.0) < 1e-9
    np.testing.assert_allclose(p, p[::-1], rtol=0, atol=1e-15)       # symmetric at zero force


def test_fixture_is_what_the_generator_gives(gen, golden):
    want = [(8, 0.0, 0.0), (8, 0.0, 1.0), (8, 0.0, 2.5), (8, 1.5, 0.5)]
    assert [(c["n"], c["E0"], c["Fz"]) for c in golden["cases"]] == want and golden["kT"] == 1.0 and golden["b"] == 1.0
    for c in golden["cases"]:
        p = np.array(c["prob"])
        assert p.shape == (32,) and (c["lo"], c["hi"]) == (-8.0, 8.0) and np.all(p > 0)
        assert abs(p.sum() - 1.0) < 1e-9
        kappa, f = gen.kappa_f(c)
        np.testing.assert_allclose(p, gen.bin_probabilities(c["n"], kappa, f, 32), rtol=1e-12, atol=0)
    # a force tilts the zero-force density: P_F(s) ~ P_0(s) exp(f s).  Between bins that holds at the bin centres up to the
    # curvature of exp inside a bin, which cancels in the ratio of two forces' probabilities to O(width^2)
    p0, p1 = (np.array(golden["cases"][i]["prob"]) for i in (0, 1))
    x = -8.0 + 0.5 * (np.arange(32) + 0.5)
    mid = slice(8, 24)
    slope = np.polyfit(x[mid], np.log(p1[mid] / p0[mid]), 1)[0]
    assert abs(slope - 1.0) < 0.02
    assert abs(gen.kappa_f(golden["cases"][3])[0] - 1.125) < 1e-15


# ---------------------------------------------------------------------------------------------- free energies
FORCES = np.arange(7) * 0.5
NSAMPLES = 16384


@pytest.fixture(scope="module")
def synthetic(gen):
    """Seeded multinomials of 16 384 samples from the tilted densities at Fz = 0, 0.5, ..., 3 (n = 8, 64 bins on [-8, 8]), and
    -ln of the exact F = 0 density at the bin centres' bins (bin probability / width)."""
    rng = np.random.default_rng(20261019)
    edges = np.linspace(-8.0, 8.0, 65)
    probs = np.array([gen.bin_probabilities(8, 0.0, f, 64) for f in FORCES])
    counts = np.array([rng.multinomial(NSAMPLES, p / p.sum()) for p in probs])
    exact = -np.log(probs[0] / np.diff(edges))
    return edges, probs, counts, exact


def test_wham_force_recovers_the_zero_force_free_energy(ps, synthetic):
    edges, probs, counts, exact = synthetic
    A, sigma, f, iterations, converged = ps.wham_force(counts, edges, 1.0, FORCES)
    assert converged and iterations < 100000 and f[0] == 0.0 and np.all(np.diff(f) < 0)
    col = counts.sum(axis=0)
    tested = col >= 50
    x = 0.5 * (edges[:-1] + edges[1:])
    # both curves are defined up to a constant: compare them where they are best known, weighted by the counts
    shift = np.average((A - exact)[tested], weights=col[tested])
    dev = np.abs(A - exact - shift)[tested]
    print("tested bins span [%.2f, %.2f]; largest deviation %.3f kT, %.2f sigma; %d iterations"
          % (edges[:-1][tested].min(), edges[1:][tested].max(), dev.max(), (dev / sigma[tested]).max(), iterations))
    assert np.all(dev < 5.0 * sigma[tested])
    assert edges[:-1][tested].min() <= -3.5 and edges[1:][tested].max() >= 7.0
    np.testing.assert_allclose(sigma[col > 0], 1.0 / np.sqrt(col[col > 0]), rtol=1e-15)
    assert np.all(np.isnan(A[col == 0])) and np.all(np.isnan(sigma[col == 0])) and np.nanmin(A) == 0.0
    # a single case is its own answer: WHAM of one histogram is extension_free_energy of it
    k = 3
    A1, s1, f1, it1, ok1 = ps.wham_force(counts[k:k + 1], edges, 1.0, FORCES[k:k + 1])
    E1, es1 = ps.extension_free_energy(counts[k], edges, 1.0, FORCES[k])
    assert ok1 and np.allclose(A1[counts[k] > 0], E1[counts[k] > 0], rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        ps.wham_force(counts, edges, 1.0, FORCES[:3])


@pytest.mark.parametrize("k", [0, 2, 6])
def test_extension_free_energy_on_one_window(ps, synthetic, k):
    edges, probs, counts, exact = synthetic
    A, sigma = ps.extension_free_energy(counts[k], edges, 1.0, FORCES[k])
    n = counts[k]
    tested = n >= 50
    shift = np.average((A - exact)[tested], weights=n[tested])
    # the tilt is taken at the bin centre; inside a bin exp(F x) curves: F^2 width^2 / 24 of ln, far below sigma
    assert np.all(np.abs(A - exact - shift)[tested] < 5.0 * sigma[tested] + FORCES[k] ** 2 * 0.25 ** 2 / 24)
    assert np.all(np.isnan(A[n == 0])) and np.nanmin(A) == 0.0 and tested.sum() >= 8
    np.testing.assert_allclose(sigma[n > 0], 1.0 / np.sqrt(n[n > 0]), rtol=1e-15)


# ---------------------------------------------------------------------------------------------- the tool's refusals
def test_sweep_refuses_hist_where_it_refuses_error_bars(tmp_path):
    """No GPU work is started: every refusal comes before the ensemble is made."""
    base = [sys.executable, os.path.join(ROOT, "tools", "run_sweep.py"), str(tmp_path / "x"), "--axis", "n=8", "--axis", "Fz=0,1"]
    tail = ["--", "--num-steps", "3000", "--stepout", "100"]
    for extra, more, needle in ((["--hist", "r3:-8:8:32", "--csv"], [], "--csv"), (["--hist", "r3:-8:8:32", "--gpus", "2"], [], "one device"),
                                (["--hist", "r3:-8:8:32", "--error-bars", "32"], [], "--error-bars"),
                                (["--hist", "r3:-8:8:32"], ["--umbrella-sampling"], "umbrella"), (["--hist", "r3:-8:8:32"], ["--num-inits", "2"], "num-inits"),
                                (["--hist", "r4:-8:8:32"], [], "not understood"), (["--hist", "r3:8:-8:32"], [], "LO < HI"),
                                (["--hist", "r3:-8:8:32"], ["--stepout", "5000"], "--stepout")):
        r = subprocess.run(base + extra + tail + more, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and needle in r.stderr, (extra, more, r.stderr[-500:])
    assert not (tmp_path / "x").exists() or not os.listdir(tmp_path / "x")
