"""GPU tests of the lag correlations (pstat_corr_*, pstat_corr.hip) against the numpy twin of the contract
(tests/corr_ref.py): totals and rows equal to the twin's on the angles of an identical second ensemble, to a bound derived from
the number of additions; every edge of the kernel's mapping; eight homes; three closed forms; error bars, tempering, refusals;
tools/run_sweep.py --corr end to end."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import corr_ref as cr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
ALL = ("nn", "zz", "mm")


@pytest.fixture(scope="module")
def ps():
    import polymer_stats_amd as ps
    assert ps._lib.load().pstat_device_count() >= 1, "no HIP device visible"
    return ps


def bits(x):
    return np.ascontiguousarray(x).tobytes()


def angles_of_all(e):
    return np.array([np.concatenate([s["theta"], s["phi"]]) for s in (e.chain_state(c) for c in range(e.ncases * e.num_chains))])


def hip_runtime():
    """The HIP runtime libpstat has loaded into this process (the rows of pstat_corr_rows are device memory)."""
    with open("/proc/self/maps") as f:
        path = next(line.split()[-1] for line in f if "libamdhip64" in line)
    hip = C.CDLL(path)
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip


def assert_same_chains(a, b, chains):
    for c in chains:
        ga, gb = a.chain_state(c), b.chain_state(c)
        for k in ga:
            assert bits(ga[k]) == bits(gb[k]) if isinstance(ga[k], np.ndarray) else ga[k] == gb[k], (c, k)
        assert bits(a.microstate(c)) == bits(b.microstate(c)), c


def physics(p):
    return dict(E0=p.E0, K1=p.K1, K2=p.K2, mu=p.mu, polar=p.chain_type == 1)


def bound(n, max_lag, channels, per, records, case, power=1):
    """[ncols]: (8 N + 16) 2^-53 scale^power with N = (n - k) + chains * records, the longest run of additions any order of
    summation can have; power = 2 for sumsq."""
    out = []
    for ch in channels:
        s = cr.scale(ch, **physics(case)) ** power
        out += [(8.0 * ((n - k) + per * records) + 16.0) * U * s for k in range(max_lag + 1)]
    return np.array(out)


def run_exact(ps, cases, channels=ALL, max_lag=None, planar=False, stepout=40, records=6):
    """A records with advance_corr (rows kept), B advances `stepout` at a time and reads every chain's angles: the twin on B's
    angles gives A's sum, sumsq and rows within the derived bound; a second A gives the same bits; A's chains end as B's."""
    n, per, ncases = int(cases[0].n), int(cases[0].num_chains), len(cases)
    L = n - 1 if max_lag is None else max_lag
    w = L + 1
    with ps.Ensemble(cases, planar=planar) as A, ps.Ensemble(cases, planar=planar) as B, ps.Ensemble(cases, planar=planar) as A2:
        g = A.open_corr(channels, max_lag, capacity_rows=records)
        A.advance_corr(g, records * stepout + 7, stepout)           # the remainder is advanced and not recorded
        g2 = A2.open_corr(channels, max_lag, capacity_rows=records)
        A2.advance_corr(g2, records * stepout + 7, stepout)
        values = []                                                  # [record][case] -> [per, ncols]
        for _ in range(records):
            B.advance(stepout)
            ang = angles_of_all(B).reshape(ncases, per, 2 * n)
            values.append([cr.per_chain(ang[k], L, channels, planar=planar, **physics(cases[k])) for k in range(ncases)])
        B.advance(7)
        got, again = g.read(), g2.read()
        assert got.records == records and got.sum.shape == (ncases, len(channels) * w)
        assert bits(got.sum) == bits(again.sum) and bits(got.sumsq) == bits(again.sumsq), "two identical runs differ"
        ptr, nrows, stride = g.rows()
        assert nrows == records and stride == ncases * len(channels) * w and ptr
        rows = np.zeros((nrows, stride))
        assert hip_runtime().hipMemcpy(rows.ctypes.data, ptr, rows.nbytes, 2) == 0      # 2: device to host
        rows = rows.reshape(nrows, ncases, -1)
        worst = 0.0
        for k in range(ncases):
            want_s = sum(v[k].sum(axis=0) for v in values)
            want_q = sum((v[k] * v[k]).sum(axis=0) for v in values)
            b1, b2 = bound(n, L, channels, per, records, cases[k]), bound(n, L, channels, per, records, cases[k], power=2)
            e1, e2 = np.abs(got.sum[k] - want_s), np.abs(got.sumsq[k] - want_q)
            worst = max(worst, float((e1 / b1).max()), float((e2 / b2).max()))
            assert np.all(e1 <= b1), (k, (e1 / b1).max())
            assert np.all(e2 <= b2), (k, (e2 / b2).max())
            for r in range(records):
                er = np.abs(rows[r, k] - values[r][k].sum(axis=0) / per)
                assert np.all(er <= b1), (k, r, (er / b1).max())
        print(f"n = {n}, max_lag = {L}, {ncases} x {per} chains: largest |device - twin| / bound = {worst:.3f}")
        if "nn" in channels:
            dev = np.abs(got.mean["nn"][:, 0] - 1.0).max()
            print(f"largest |NN(0) - 1| = {dev:.3e}")
            assert dev <= 4 * 2.0 ** -52
        C_ = ncases * per
        edges = {c for k in range(ncases) for j in (0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, per - 1) if j < per for c in [k * per + j]}
        assert_same_chains(A, B, range(C_) if C_ <= 700 else sorted(edges))
        g.close()
        return got


BASE = dict(E0=1.0, K1=0.5, K2=0.2, Fz=0.5, steps_per_adjust=150)
CLUSTER = dict(move_set=1, cluster_prob=0.5, bend_mod=0.3, bend_angle=0.2)


def sweep_cases(ps, ncases, per, n, seed=800, **kw):
    return [ps.default_params(n=n, num_chains=per, precision=ps.F64, kT=0.7 + 0.2 * k, seed=seed + k, **{**BASE, **kw}) for k in range(ncases)]


# ------------------------------------------------------------------------------------------------ every edge of the mapping
# chains per case: 1, 5 (one tile, not full), 64 (four full tiles of 16), 65 (a last tile of one chain), 1100 (69 tiles: more
# than the 64 lanes of the fold); 9 cases: the fold's last workgroup is not full
@pytest.mark.parametrize("ncases,per", [(1, 1), (3, 5), (9, 64), (9, 65), (2, 1100)])
def test_totals_and_rows_equal_the_twin(ps, ncases, per):
    run_exact(ps, sweep_cases(ps, ncases, per, 12))


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
# name: (parameters, precision, planar, chains per case, the kernel's name has)
HOMES = {
    "f64 sweep": (dict(n=12), 1, False, 70, "sweep_kernel<double>"),
    "fixed-force all-pairs": (dict(n=16, energy_type=1), 1, False, 70, "interacting_kernel"),
    "clustering main": (dict(n=12, **CLUSTER), 1, False, 70, "cluster"),
    "planar": (dict(n=14, cluster_prob=0.5), 1, True, 70, "planar_kernel"),
    "f32 sweep": (dict(n=12), 0, False, 70, "sweep_kernel<float>"),
    "q16 sweep": (dict(n=12), 2, False, 70, "q16 state"),
    "f64 sweep in memory": (dict(n=65), 1, False, 70, "state in L2"),
    "clustering main, chain per wavefront": (dict(n=12, **CLUSTER), 1, False, 16, "cluster_chain_wave_kernel"),
    "polar": (dict(n=12, chain_type=1, mu=1.5), 1, False, 20, "sweep_kernel<double>"),
}


@pytest.mark.parametrize("home", list(HOMES))
def test_every_home(ps, home):
    kw, precision, planar, per, has = HOMES[home]
    make = ps.default_planar_params if planar else ps.default_params
    E0 = [0.5, 1.0, 1.5]
    cases = [make(num_chains=per, precision=precision, kT=0.8 + 0.3 * k, seed=900 + k, **{**BASE, **kw, "E0": E0[k]}) for k in range(3)]
    with ps.Ensemble(cases, planar=planar) as e:
        assert has in e.launch_info().kernel.decode(), e.launch_info().kernel.decode()
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
    kTs = [0.25, 0.35, 0.5, 0.75, 1.2, 2.0, 4.0]                     # the ladder of the README's example
    cases = [ps.default_params(n=8, E0=3.0, Fz=0.2, kT=kT, num_chains=64, seed=i) for i, kT in enumerate(kTs)]
    with ps.Ensemble(cases) as A, ps.Ensemble(cases) as B:
        ta, tb = (e.open_tempering(ps.ladders_by(cases), seed=9) for e in (A, B))
        g = A.open_corr(("nn", "zz"))
        values = []
        for _ in range(5):
            A.advance_tempered(ta, 200, 50)
            g.record()
            B.advance_tempered(tb, 200, 50)
            ang = angles_of_all(B).reshape(7, 64, 16)
            values.append([cr.per_chain(ang[k], 7, ("nn", "zz")) for k in range(7)])
        got = g.read()
        sa, sb = ta.stats(), tb.stats()
        assert sa[2] == sb[2] == 20 and sa[1].sum() > 0, "no exchange was accepted: the records would not show a swapped configuration"
        assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1])
        assert_same_chains(A, B, range(7 * 64))
    for k in range(7):
        want = sum(v[k].sum(axis=0) for v in values)
        assert np.all(np.abs(got.sum[k] - want) <= bound(8, 7, ("nn", "zz"), 64, 5, cases[k]))
    assert got.records == 5


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
        g = e.open_corr(("nn",), capacity_rows=2)
        with ps.Ensemble(cases[:2]) as other:                        # an object of another handle
            assert lib.pstat_corr_record(other._h, g._g) == -1 and b"not an open one" in lib.pstat_last_error()
            assert lib.pstat_advance_corr(other._h, g._g, 10, 5) == -1
            assert lib.pstat_corr_read(other._h, g._g, None, None, None) == -1
            assert lib.pstat_corr_clear(other._h, g._g) == -1
            lib.pstat_corr_close(other._h, g._g)                     # ignored: it is not the other handle's to close
        assert lib.pstat_advance_corr(e._h, g._g, 10, 0) == -1 and lib.pstat_advance_corr(e._h, g._g, -1, 5) == -1
        e.advance_corr(g, 25, 10)
        assert g.read().records == 2 and e.chain_state(0)["steps_recorded"] == 25
        # the row buffer is full: refused with nothing enqueued
        assert lib.pstat_advance_corr(e._h, g._g, 10, 10) == -7 and lib.pstat_corr_record(e._h, g._g) == -7
        assert e.chain_state(0)["steps_recorded"] == 25 and g.read().records == 2
        e.advance_corr(g, 9, 10)                                     # no record in this call: it fits
        assert e.chain_state(0)["steps_recorded"] == 34
        g.clear()
        g.record()
        records = C.c_int64(-1)                                      # every output may be NULL
        assert lib.pstat_corr_read(e._h, g._g, None, None, C.byref(records)) == 0 and records.value == 1
        totals = e.open_corr(("zz",), 3)                             # no rows kept: no limit, and no rows to hand out
        e.advance_corr(totals, 50, 1)
        assert totals.read().records == 50 and totals.rows() == (0, 0, 3 * 4)
        with pytest.raises(ps.PstatError):
            totals.error_bars()
        raw = g._g
        g.close()
        assert lib.pstat_corr_read(e._h, raw, None, None, None) == -1    # read after close
        assert lib.pstat_corr_record(e._h, raw) == -1
        e.advance(5)
        assert e.chain_state(0)["steps_recorded"] == 89
        e.open_corr().record()                                       # destroyed with an object open
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
        assert np.all(np.abs(g.read().sum[0] - want) <= bound(2560, 40, ("nn", "zz"), 2, 1, p))


# ------------------------------------------------------------------------------------------------ the tool
def _sweep(tmp_path, name, *extra):
    out = tmp_path / name
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_sweep.py"), str(out), "--axis", "n=8", "--axis", "Fz=0,0.5,1,1.5,2,2.5",
                        "--num-chains", "64", "--seed", "11", *extra, "--", "--num-steps", "3200", "--stepout", "100", "-v", "0"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def test_sweep_writes_corr_files(tmp_path):
    with_corr = _sweep(tmp_path, "c", "--corr", "5:nn,zz")
    plain = _sweep(tmp_path, "p")
    outs = sorted(f for f in os.listdir(plain) if f.endswith(".out"))
    assert len(outs) == 6 and sorted(f for f in os.listdir(with_corr) if f.endswith(".out")) == outs
    for f in outs:                                                   # the .out files are a plain run's, byte for byte
        assert (with_corr / f).read_bytes() == (plain / f).read_bytes(), f
    assert not [f for f in os.listdir(plain) if f.endswith(".corr")]
    corrs = sorted(f for f in os.listdir(with_corr) if f.endswith(".corr"))
    assert corrs == [f[:-len(".out")] + ".corr" for f in outs]
    zz1 = []
    for f in corrs:
        lines = (with_corr / f).read_text().strip().split("\n")
        assert lines[0] == "k,nn,nn_stderr,zz,zz_stderr" and len(lines) == 7
        t = np.array([[float(v) for v in line.split(",")] for line in lines[1:]])
        assert np.array_equal(t[:, 0], np.arange(6)) and np.all(np.isfinite(t))
        assert abs(t[0, 1] - 1.0) <= 4 * 2.0 ** -52 and np.all(t[1:, 2] > 0) and np.all(t[:, 4] > 0) and np.all(t[:, 2] < 0.05)
        zz1.append(t[1, 3])
    assert zz1[-1] > zz1[0] + 0.2                                    # a force along z aligns the monomers: <n_z>^2 grows with Fz
