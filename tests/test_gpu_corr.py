"""GPU tests of the lag correlations (pstat_corr_*, pstat_corr.hip) against the numpy twin of the contract
(tests/corr_ref.py): totals and rows equal to the twin's on the angles of an identical second ensemble, to a bound derived from
the number of additions; every edge of the kernel's mapping; nine homes; three closed forms; error bars, tempering, refusals;
tools/run_sweep.py --corr end to end.  The protocol of the comparison, the case tables and the tool call are those of
tests/recorder_cases.py, given corr_kind below; the lifecycle rules are asserted in tests/test_gpu_recorder_lifecycle.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import corr_ref as cr
import recorder_cases as rc
from recorder_cases import angles_of_all, bits, ps, sweep_cases  # noqa: F401 (ps is the fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
ALL = ("nn", "zz", "mm")


def physics(p):
    return dict(E0=p.E0, K1=p.K1, K2=p.K2, mu=p.mu, polar=p.chain_type == 1)


def bound(n, max_lag, channels, M, case, power=1):
    """[ncols]: (8 N + 16) 2^-53 scale^power with N = (n - k) + M, M = chains * records: the longest run of additions any order
    of summation can have; power = 2 for sumsq."""
    out = []
    for ch in channels:
        s = cr.scale(ch, **physics(case)) ** power
        out += [(8.0 * ((n - k) + M) + 16.0) * U * s for k in range(max_lag + 1)]
    return np.array(out)


def corr_kind(cases, channels=ALL, max_lag=None, planar=False):
    """The descriptor of rc.run_totals_twin.  A row is held to the bound of the totals."""
    n, per, ncases = int(cases[0].n), int(cases[0].num_chains), len(cases)
    L = n - 1 if max_lag is None else max_lag

    def exact(got, rows, values, per):
        if "nn" in channels:
            dev = np.abs(got.mean["nn"][:, 0] - 1.0).max()
            print(f"largest |NN(0) - 1| = {dev:.3e}")
            assert dev <= 4 * 2.0 ** -52

    return rc.Totals(
        name="corr", ncols=len(channels) * (L + 1), open=lambda e, capacity: e.open_corr(channels, max_lag, capacity_rows=capacity),
        twin=lambda ang, k: (cr.per_chain(ang, L, channels, planar=planar, **physics(cases[k])),),
        bounds=lambda k, M, twins: (bound(n, L, channels, M, cases[k]), bound(n, L, channels, M, cases[k], power=2)),
        row_bound=lambda k, per, M, twins: bound(n, L, channels, M, cases[k]), exact=exact,
        line=f"n = {n}, max_lag = {L}, {ncases} x {per} chains: largest |device - twin| / bound = {{worst_totals:.3f}}")


def run_exact(ps, cases, planar=False, **options):
    return rc.run_totals_twin(ps, cases, corr_kind(cases, planar=planar, **options), planar=planar, records=6)


# ------------------------------------------------------------------------------------------------ every edge of the mapping
@pytest.mark.parametrize("ncases,per", rc.TILE_SHAPES)
def test_totals_and_rows_equal_the_twin(ps, ncases, per):
    run_exact(ps, sweep_cases(ps, ncases, per, 12, seed=800))


# one monomer; a lag count of one at n = 2 with max_lag 0 below; more monomers than lanes; n = 130: lags that take three passes
# of a wave, and a group of 256 threads that is not full
@pytest.mark.parametrize("n", [1, 2, 3, 65, 130])
def test_chain_lengths(ps, n):
    run_exact(ps, sweep_cases(ps, 3, 5, n, seed=820))


# max_lag + 1 = 1 (every thread a group of its own), 64 and 65 (groups of 64 and of 128 threads), 66
@pytest.mark.parametrize("max_lag", [0, 63, 64, 65])
def test_lag_counts_at_n_130(ps, max_lag):
    run_exact(ps, sweep_cases(ps, 3, 5, 130, seed=840), max_lag=max_lag)


def test_single_channels_and_their_columns(ps):
    cases = sweep_cases(ps, 2, 20, 9, seed=860)
    full = run_exact(ps, cases)
    for chans in (("zz",), ("mm",), ("nn", "mm")):
        got = run_exact(ps, cases, channels=chans)
        for ch in chans:
            assert bits(got.mean[ch]) == bits(full.mean[ch]), ch


# ------------------------------------------------------------------------------------------------ the homes
@pytest.mark.parametrize("home", list(rc.HOMES))
def test_every_home(ps, home):
    cases, planar = rc.home_cases(ps, home, seed=900)
    got = run_exact(ps, cases, planar=planar)
    assert np.all(got.mean["mm"][:, 0] > 0) and not np.allclose(got.mean["mm"][0], got.mean["mm"][2])   # the cases' own scalars


# ------------------------------------------------------------------------------------------------ closed forms
@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "corr_closed_form.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", ["bending", "fixed_force", "planar"])
def test_closed_forms(ps, golden, name):
    """16 384 chains, 1 000 n steps of burn-in, ONE record: every column within 5 of its own across-chain standard errors of the
    closed form, and every such error <= 0.01 scale (per-chain values lie in [-scale, scale], so it is at most scale /
    sqrt(16383) = 0.0078 scale).  NN(0) has no sampling variance (every chain's value is 1 up to rounding) and is held to
    4 * 2^-52 instead.  Device figures (MI355X): see DESIGN.md 3.15."""
    c = golden[name]
    planar = name == "planar"
    N = 16384
    make = ps.default_planar_params if planar else ps.default_params
    p = make(num_chains=N, precision=ps.F64, seed=20261019, **c["params"])
    channels = tuple(ch for ch in ALL if ch in c["expect"])
    with ps.Ensemble(p, planar=planar) as e:
        print(e.launch_info().kernel.decode())
        g = e.open_corr(channels)
        e.advance(1000 * c["params"]["n"])
        g.record()
        got = g.read()
    assert got.records == 1
    for ch in channels:
        want, mean, se = np.array(c["expect"][ch]), got.mean[ch][0], got.chain_stderr[ch][0]
        scale = cr.scale(ch, **physics(p))
        z = (mean - want) / np.where(se > 0, se, 1.0)
        first = 1 if ch == "nn" else 0
        print(f"{name} {ch}: max |z| = {np.abs(z[first:]).max():.2f}, max stderr / scale = {(se / scale).max():.4f}")
        print("  mean  ", np.round(mean, 5), "\n  closed", np.round(want, 5))
        if ch == "nn":
            assert abs(mean[0] - 1.0) <= 4 * 2.0 ** -52
        assert np.all(se <= 0.01 * scale)
        assert np.all(se[first:] > 0) and np.all(np.abs(mean - want)[first:] <= 5.0 * se[first:]), np.round(z, 2)


# ------------------------------------------------------------------------------------------------ composition
def test_error_bars_are_the_blocking_transform_of_the_rows(ps):
    cases = sweep_cases(ps, 3, 20, 10, seed=940)
    with ps.Ensemble(cases) as e:
        g = e.open_corr(("nn", "zz"), 4, capacity_rows=64)
        e.advance_corr(g, 64 * 25, 25)
        eb = g.error_bars()
        ptr, nrows, stride = g.rows()
        assert (nrows, stride) == (64, 3 * 2 * 5)
        by_hand = ps.blocking_device(ptr, nrows, stride)
        for f in ("mean", "stderr", "stderr_err", "inefficiency", "level", "converged"):
            assert getattr(eb, f).shape == (3, 10) and bits(getattr(eb, f)) == bits(getattr(by_hand, f).reshape(3, 10)), f
        res = g.read()
        np.testing.assert_allclose(eb.mean[:, :5], res.mean["nn"], rtol=1e-13)
        assert np.all(np.isnan(res.chain_stderr["nn"])) and eb.nbatches == 64 and np.all(eb.stderr[:, 1:5] > 0)
        with pytest.raises(ps.PstatError) as err:                    # fewer rows than min_blocks: the transform's own refusal
            g.error_bars(min_blocks=65)
        assert err.value.code == -7
        g.clear()
        assert g.read().records == 0 and g.rows()[1] == 0 and np.all(g.read().sum == 0)


def test_records_between_exchange_rounds(ps):
    cases = rc.ladder_cases(ps)
    rc.totals_between_exchange_rounds(ps, cases, corr_kind(cases, ("nn", "zz")))


def test_refusals_leave_the_handle_usable(ps):
    lib = ps._lib.load()
    with ps.Ensemble([ps.default_params(n=6, num_chains=4, kT=kT, umbrella=1) for kT in (1.0, 2.0)]) as e:
        with pytest.raises(ps.PstatError) as err:
            e.open_corr()
        assert err.value.code == -4 and "umbrella" in str(err.value)
        e.advance(20)
        assert e.chain_state(0)["steps_recorded"] == 20
    cases = [ps.default_params(n=6, num_chains=4, kT=kT, Fz=0.3) for kT in (1.0, 2.0, 3.0)]
    with ps.Ensemble(cases) as e:
        out = C.c_void_p()
        for args, needle in (((0, -1, 0), "channels"), ((8, -1, 0), "channels"), ((1, -2, 0), "max_lag"), ((1, 6, 0), "max_lag"),
                             ((1, -1, -1), "capacity_rows")):
            assert lib.pstat_corr_open(e._h, *args, C.byref(out)) == -1 and needle.encode() in lib.pstat_last_error(), args
        e.advance(5)                                                 # the handle still advances
        assert e.chain_state(0)["steps_recorded"] == 5
    with ps.Ensemble(ps.default_params(n=2561, num_chains=1)) as e:  # beyond a workgroup's LDS
        with pytest.raises(ps.PstatError) as err:
            e.open_corr()
        assert err.value.code == -4 and "2560" in str(err.value)
        e.advance(2)
        assert e.chain_state(0)["steps_recorded"] == 2
    p = ps.default_planar_params(n=2560, num_chains=2, Fz=0.5)
    with ps.Ensemble(p, planar=True) as e:                           # planar n = 2560 fits
        g = e.open_corr(("nn", "zz"), 40)
        e.advance(50)
        g.record()
        ang = angles_of_all(e)
        want = cr.per_chain(ang, 40, ("nn", "zz"), planar=True).sum(axis=0)
        assert np.all(np.abs(g.read().sum[0] - want) <= bound(2560, 40, ("nn", "zz"), 2, p))


# ------------------------------------------------------------------------------------------------ the tool
def test_sweep_writes_corr_files(tmp_path):
    axes = [("n", "8"), ("Fz", "0,0.5,1,1.5,2,2.5")]
    with_corr = rc.sweep_tool(tmp_path, "c", "--corr", "5:nn,zz", axes=axes)
    plain = rc.sweep_tool(tmp_path, "p", axes=axes)
    outs, corrs = rc.assert_out_files_unchanged(with_corr, plain, ".corr")
    assert len(outs) == 6
    zz1 = []
    for f in corrs:
        lines = (with_corr / f).read_text().strip().split("\n")
        assert lines[0] == "k,nn,nn_stderr,zz,zz_stderr" and len(lines) == 7
        t = np.array([[float(v) for v in line.split(",")] for line in lines[1:]])
        assert np.array_equal(t[:, 0], np.arange(6)) and np.all(np.isfinite(t))
        assert abs(t[0, 1] - 1.0) <= 4 * 2.0 ** -52 and np.all(t[1:, 2] > 0) and np.all(t[:, 4] > 0) and np.all(t[:, 2] < 0.05)
        zz1.append(t[1, 3])
    assert zz1[-1] > zz1[0] + 0.2                                    # a force along z aligns the monomers: <n_z>^2 grows with Fz
