"""Blocked standard errors without a GPU: the numpy twin of the estimator (tests/blocking_ref.py) against closed forms and
against the exact standard error of seeded AR(1) series; the two ABI entry points' declarations, exports and argument
errors; the tools' refusals of --error-bars."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import blocking_ref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20260518


# ---------------------------------------------------------------------------------------------- the twin, closed forms
def test_twin_four_values():
    out = br.blocking(np.array([[0.0], [2.0], [0.0], [2.0]]), min_blocks=2)
    # level 0: mean 1, sum of squares 4 -> sqrt(4 / 3 / 4); level 1: [1, 1] -> 0; no further level
    assert out["mean"][0] == 1.0
    np.testing.assert_allclose(out["levels"][0, :3], [np.sqrt(1.0 / 3.0), 0.0, 0.0], rtol=1e-15)
    assert out["level"][0] == 0 and out["converged"][0] == 1          # the maximum is not the last eligible level
    np.testing.assert_allclose(out["stderr"][0], np.sqrt(1.0 / 3.0), rtol=1e-15)
    np.testing.assert_allclose(out["stderr_err"][0], np.sqrt(1.0 / 3.0) / np.sqrt(6.0), rtol=1e-15)
    assert out["inefficiency"][0] == 1.0
    # min_blocks = 4: level 0 alone is eligible: nothing to judge a plateau by
    out = br.blocking(np.array([[0.0], [2.0], [0.0], [2.0]]), min_blocks=4)
    assert out["level"][0] == 0 and out["converged"][0] == 0


def test_twin_constant_and_nan_columns():
    rng = np.random.default_rng(SEED)
    x = rng.standard_normal((64, 3))
    x[:, 0] = 2.5
    x[17, 2] = np.nan
    out = br.blocking(x, min_blocks=8)
    assert [out[k][0] for k in br.FIELDS] == [2.5, 0.0, 0.0, 1.0, 0.0, 1.0]
    assert np.isnan(out["stderr"][2]) and out["level"][2] == -1 and out["converged"][2] == 0
    assert np.isfinite(out["stderr"][1]) and out["stderr"][1] > 0 and 0 <= out["level"][1] <= 3
    # a trailing odd element is dropped: 5 values -> levels of 5 and 2
    out = br.blocking(np.array([[1.0], [3.0], [5.0], [7.0], [100.0]]), min_blocks=2)
    np.testing.assert_allclose(out["levels"][0, 1], np.sqrt(((2.0 - 4.0) ** 2 + (6.0 - 4.0) ** 2) / 1 / 2), rtol=1e-15)
    assert np.all(out["levels"][0, 2:] == 0)


def test_twin_batches_from_rows():
    """Both baseline rules, on a hand-made series of 2 cases: cumulative means of known batch values."""
    rng = np.random.default_rng(SEED + 1)
    d, chains, nrows = 20, 5.0, 6
    b = rng.standard_normal((nrows, 2, br.NQ))                      # per-chain, per-step batch means
    for s0 in (0, 130):                                             # from empty averages; on a handle already advanced
        steps = s0 + d * np.arange(1, nrows + 1)
        S = np.cumsum(b * d * chains, axis=0) + (7.0 * chains * s0 if s0 else 0.0)
        red = np.zeros((nrows, 2, 1 + 2 * br.NQ + 2))
        red[:, :, 0] = chains
        red[:, :, 1:1 + br.NQ] = S / steps[:, None, None]
        x = br.batches(steps, red)
        want = b.reshape(nrows, -1) if s0 == 0 else b.reshape(nrows, -1)[1:]
        assert x.shape == want.shape
        np.testing.assert_allclose(x, want, rtol=0, atol=1e-11)
        np.testing.assert_allclose(br.batches(steps, red, 2, 3), b.reshape(nrows, -1)[3:5], rtol=0, atol=1e-11)
    with pytest.raises(ValueError):
        br.batches(np.array([20, 40, 70]), red[:3])
    with pytest.raises(ValueError):
        br.batches(np.array([20, 40, 20]), red[:3])


# ---------------------------------------------------------------------------------------------- the twin on AR(1)
def ar1(rng, N, phi, ncols=64):
    x = np.empty((N, ncols))
    x[0] = rng.standard_normal(ncols) / np.sqrt(1.0 - phi * phi)    # stationary start
    e = rng.standard_normal((N, ncols))
    for t in range(1, N):
        x[t] = phi * x[t - 1] + e[t]
    k = np.arange(1, N)
    var = 1.0 / (1.0 - phi * phi)
    exact = np.sqrt(var / N * (1.0 + 2.0 * np.sum((1.0 - k / N) * phi ** k)))
    return x, exact


def test_twin_on_correlated_series():
    rng = np.random.default_rng(SEED)
    x, exact = ar1(rng, 16384, 0.9)
    out = br.blocking(x)
    ratio = np.median(out["stderr"] / exact)
    print("N = 16384, phi = 0.9: median stderr / exact = %.4f, converged %d of 64" % (ratio, out["converged"].sum()))
    assert 0.90 <= ratio <= 1.15
    np.testing.assert_allclose(out["inefficiency"], (out["stderr"] / out["levels"][:, 0]) ** 2, rtol=1e-14)


def test_twin_converged_flag_on_correlated_series():
    """At least 56 of the 64 columns of the N = 16 384, phi = 0.9 series (800 correlation times long) are flagged converged.
    Measured on this seed: 62 (59 to 63 on six others).  With "not converged whenever the level picked is the last eligible
    one" it was 40 (31 to 45): on the plateau se_l scatters by 1 / sqrt(2 (N_l - 1)) -- 6 % at 128 blocks, 13 % at 32 -- so the
    largest se falls on the noisiest, last level for a third of the columns; hence the rule also asks that se rose into that
    level by more than its own uncertainty."""
    rng = np.random.default_rng(SEED)
    x, _ = ar1(rng, 16384, 0.9)
    out = br.blocking(x)
    last = out["level"] == 9                     # 32 blocks: the last eligible level
    print("N = 16384, phi = 0.9: converged %d of 64; levels picked %s; %d columns picked the last level, %d of them still rising"
          % (out["converged"].sum(), np.bincount(out["level"].astype(int)), last.sum(), (out["converged"][last] == 0).sum()))
    assert out["converged"].sum() >= 56
    assert np.all(out["converged"][~last] == 1)


def test_twin_on_white_noise():
    rng = np.random.default_rng(SEED)
    x, exact = ar1(rng, 4096, 0.0)
    out = br.blocking(x)
    ratio = np.median(out["stderr"] / exact)
    print("white noise, N = 4096: median stderr / exact = %.4f" % ratio)
    assert 0.95 <= ratio <= 1.15


def test_twin_flags_a_run_that_is_too_short():
    rng = np.random.default_rng(SEED)
    x, exact = ar1(rng, 1000, 0.98)
    out = br.blocking(x)
    print("N = 1000, phi = 0.98: median stderr / exact = %.4f, not converged %d of 64"
          % (np.median(out["stderr"] / exact), (out["converged"] == 0).sum()))
    assert (out["converged"] == 0).sum() >= 56


# ---------------------------------------------------------------------------------------------- the ABI, no device
@pytest.fixture(scope="module")
def ps():
    import polymer_stats_amd as ps
    ps._lib.load()
    return ps


def test_entry_points_are_declared_exported_and_bound(ps):
    lib = ps._lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pstat.h")).read(), flags=re.S)
    for name in ("pstat_series_error_bars", "pstat_blocking_device"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(lib, name) and name in ps._lib.SYMBOLS
    assert lib.pstat_abi_version() == 6 and "#define PSTAT_ABI_VERSION 6" in text
    assert int(re.search(r"#define PSTAT_BLOCK_LEVELS (\d+)", text).group(1)) == ps._lib.BLOCK_LEVELS == br.BLOCK_LEVELS == 24
    assert int(re.search(r"#define PSTAT_BLOCK_MAX_BATCHES (\d+)", text).group(1)) == ps._lib.BLOCK_MAX_BATCHES >= 32768
    fields = re.search(r"enum \{ (PSTAT_EB_MEAN.*?) \};", text, re.S).group(1).replace("\n", " ")
    assert [f.strip()[len("PSTAT_EB_"):].lower() for f in fields.split(",")][:-1] == ps._lib.EB_FIELDS == list(br.FIELDS)
    assert ps.EB_NAMES == ps.OBS_NAMES + ["AR", "cos2", "psi"] and len(ps.EB_NAMES) == ps.NQ == br.NQ


def test_blocking_device_argument_errors_need_no_gpu(ps):
    lib = ps._lib.load()
    out = np.zeros((4, 6))
    dp = C.POINTER(C.c_double)
    o = out.ctypes.data_as(dp)
    x = C.c_void_p(4096)        # never dereferenced: every one of these is refused before the device is touched

    def call(xp, nb, ncols, stride, mb, outp=o):
        return lib.pstat_blocking_device(xp, nb, ncols, stride, mb, 0, None, outp, None)
    assert call(None, 64, 4, 4, 32) == -1
    assert call(x, 64, 4, 4, 32, None) == -1
    assert call(x, 64, 4, 4, 1) == -1 and b"min_blocks" in lib.pstat_last_error()
    assert call(x, 64, 4, 4, -3) == -1
    assert call(x, 64, 4, 3, 32) == -1 and b"stride" in lib.pstat_last_error()
    assert call(x, 64, 0, 4, 32) == -1
    assert call(x, 31, 4, 4, 32) == -7
    assert call(x, 31, 4, 4, 0) == -7          # 0: the default, 32
    assert call(x, 7, 4, 4, 8) == -7
    assert call(x, ps._lib.BLOCK_MAX_BATCHES + 1, 4, 4, 32) == -4
    assert str(ps._lib.BLOCK_MAX_BATCHES).encode() in lib.pstat_last_error()
    with pytest.raises(ps.PstatError) as err:
        ps.blocking_device(4096, 10, 4)
    assert err.value.code == -7
    assert lib.pstat_series_error_bars(None, None, 0, -1, 0, None, o, None) == -1


def test_product_never_imports_the_twin():
    """tests/blocking_ref.py is a checker, like the oracle (tests/test_abi.py): the package, tools/, julia/ and bench.py do
    not name it in anything that runs."""
    paths = [os.path.join(ROOT, "bench.py")]
    for top in ("polymer_stats_amd", "tools", "julia"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, top)):
            paths += [os.path.join(dirpath, f) for f in files if f.endswith((".py", ".jl", ".sh", "Makefile"))]
    for p in paths:
        assert "blocking_ref" not in open(p, errors="ignore").read(), p


# ---------------------------------------------------------------------------------------------- the tools' refusals
def _tool(name, *argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", name), *argv], capture_output=True, text=True)
    return r.returncode, r.stdout + r.stderr


@pytest.mark.parametrize("extra,names", [
    (["--csv"], "cannot be combined with --csv"),       # (the refusals' own wording: an argparse usage text does not have it)
    (["--gpus", "2"], "needs one device, not --gpus 2"),
    (["--", "--devices", "0,1"], "needs one device, not 2"),
    (["--", "--num-inits", "2"], "cannot be combined with --num-inits 2"),
    (["--", "--umbrella-sampling"], "cannot be combined with --umbrella-sampling"),
    (["--", "--numeric-type", "float128"], "cannot be combined with --numeric-type float128"),
    (["--main", "mcmc_clustering_eap_chain", "--", "--umbrella-sampling"], "cannot be combined with --umbrella-sampling"),
    (["--main", "mcmc_clustering_eap_chain_2d", "--", "--numeric-type", "big"], "cannot be combined with --numeric-type big"),
], ids=lambda v: "_".join(v).replace("--", "") if isinstance(v, list) else None)
def test_run_sweep_refuses_what_error_bars_cannot_be_combined_with(tmp_path, extra, names):
    k = extra.index("--") if "--" in extra else len(extra)
    argv = [str(tmp_path / "w"), "--dry-run", "--axis", "E0=1,2", "--error-bars", "64", *extra[:k], *extra[k:]]
    rc, text = _tool("run_sweep.py", *argv)
    assert rc != 0 and "--error-bars " + names in text, text
    assert not (tmp_path / "w").exists()
    # the same plan without the flag, and the flag alone, are fine
    rc, text = _tool("run_sweep.py", *[a for a in argv if a not in ("--error-bars", "64")])
    assert rc == 0, text


def test_run_sweep_dry_run_accepts_error_bars_alone(tmp_path):
    rc, text = _tool("run_sweep.py", str(tmp_path / "w"), "--dry-run", "--axis", "E0=1,2", "--error-bars", "64",
                     "--num-chains", "1", "--", "--num-steps", "6400")
    assert rc == 0 and "2 cases" in text, text
    # a --num-steps that is no multiple of N: 64 batches of 15 steps, the other 40 steps in none
    rc, text = _tool("run_sweep.py", str(tmp_path / "w"), "--dry-run", "--axis", "E0=1,2", "--error-bars", "64", "--", "--num-steps", "1000")
    assert rc == 0 and "2 cases" in text, text
    rc, text = _tool("run_sweep.py", str(tmp_path / "w"), "--dry-run", "--axis", "E0=1,2", "--error-bars", "16")
    assert rc != 0 and "--error-bars 16: the blocking transform needs at least 32 batches" in text, text
    rc, text = _tool("run_sweep.py", str(tmp_path / "w"), "--dry-run", "--axis", "E0=1,2", "--error-bars", "64", "--", "--num-steps", "63")
    assert rc != 0 and "--error-bars 64 needs --num-steps >= 64" in text, text


def test_phase_scan_refuses_error_bars_on_several_ranks():
    rc, text = _tool("phase_scan.py", "--gpus", "2", "--error-bars", "64", "--points", "4")
    assert rc != 0 and "--error-bars needs one rank, not --gpus 2" in text, text
    rc, text = _tool("phase_scan.py", "--error-bars", "8")
    assert rc != 0 and "--error-bars 8: at least 32 batches" in text, text
