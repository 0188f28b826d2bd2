"""The device-side recorder of the stepout time series (pstat_series_*, pstat_advance_series) against the per-row API it
replaces.  The yardstick is never the series itself: a twin ensemble from identical parameters is driven with
advance(stepout) and then reduce_host / microstate / chain_state case by case, row after row; the series of one
advance_series call must hold the same doubles (`==`, NaN matching NaN), and the handle must end up where the twin's did."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ps():
    import polymer_stats_amd as ps
    ps._lib.load()
    return ps


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def twin_rows(e, stepout, nrows):
    """What the hosts' per-row loop fetches: after each advance(stepout), for every case k the reduction vector, the
    microstate and the angles (theta then phi) of chain k * num_chains."""
    steps, red, micro, ang = [], [], [], []
    for _ in range(nrows):
        e.advance(stepout)
        first = [e.chain_state(k * e.num_chains) for k in range(e.ncases)]
        steps.append(first[0]["steps_recorded"])
        red.append([e.reduce_host(k) for k in range(e.ncases)])
        micro.append([e.microstate(k * e.num_chains) for k in range(e.ncases)])
        ang.append([np.concatenate([c["theta"], c["phi"]]) for c in first])
    return (np.array(steps, dtype=np.int64), np.array(red).reshape(nrows, e.ncases, -1),
            np.array(micro).reshape(nrows, e.ncases, 7), np.array(ang).reshape(nrows, e.ncases, 2 * e.n))


def assert_rows(got, want, what=""):
    for name, g, w in zip(("steps_recorded", "red", "micro", "angles"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape)
        assert same(g, w), (what, name, np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w))))[:5])


def assert_same_chains(a, b, chains, what=""):
    """Angles, running sums, counters, step sizes and generator words of the chains named."""
    for c in chains:
        x, y = a.chain_state(c), b.chain_state(c)
        for key in x:
            assert same(x[key], y[key]), (what, c, key, x[key], y[key])
        if a.cases[0].move_set:
            ex, ey = a.chain_extras(c), b.chain_extras(c)
            assert same(ex["sums"], ey["sums"]) and same(ex["now"], ey["now"]), (what, c)


def probes(e):
    total = e.ncases * e.num_chains
    return sorted({0, 1 % total, total // 2, total - 1, (e.ncases - 1) * e.num_chains})


def check(ps, cases, kernel, stepout=200, nrows=3, packed=None):
    with ps.Ensemble(cases) as a, ps.Ensemble(cases) as b:
        info = b.launch_info()
        assert kernel in info.kernel.decode(), info.kernel.decode()
        if packed is not None:
            assert info.packed_cases == packed, info.kernel.decode()
        want = twin_rows(a, stepout, nrows)
        s = b.open_series(nrows, angles=True)
        b.advance_series(s, nrows * stepout, stepout)
        assert s.rows == nrows
        assert_rows(s.read(), want, kernel)
        assert_same_chains(a, b, probes(a), kernel)
        s.close()


CLUSTER = dict(n=16, E0=1.0, K1=0.3, K2=0.02, Fz=0.5, kT=1.0, seed=9, bend_mod=0.4, bend_angle=0.2, cluster_prob=0.5,
               steps_per_adjust=150)


def P(ps, **kw):
    kw.setdefault("steps_per_adjust", 150)        # the adaptation runs inside these short rows
    return ps.default_params(**kw)


# ---------------------------------------------------------------------------------------------- 1. row equality, every home
@pytest.mark.parametrize("precision,kernel", [(1, "sweep_kernel<double>"), (0, "sweep_kernel<float>"),
                                              (2, "sweep_kernel<float, q16 state>")], ids=["f64", "f32", "q16"])
def test_rows_sweep_lds(ps, precision, kernel):
    check(ps, P(ps, n=20, E0=1.0, Fz=0.5, Fx=0.2, num_chains=64, seed=3, precision=precision, energy_type=ps.ISING), kernel)


def test_rows_sweep_mem(ps):
    check(ps, P(ps, n=50, E0=1.0, Fz=0.5, num_chains=100, seed=4, precision=ps.F64), "sweep_kernel<double, state in L2>")


def test_rows_interacting(ps):
    check(ps, P(ps, n=16, E0=1.0, K1=0.5, Fz=0.5, num_chains=9, seed=5, energy_type=ps.INTERACTING, do_flips=1),
          "interacting_kernel<double>")


def test_rows_cluster_lds_f32(ps):
    check(ps, P(ps, num_chains=40, precision=ps.F32, move_set=ps.MOVES_CLUSTER, energy_type=ps.ISING, **CLUSTER),
          "cluster_kernel<float>")


def test_rows_cluster_mem(ps, monkeypatch):
    monkeypatch.setenv("PSTAT_F64_STATE", "global")
    check(ps, P(ps, num_chains=70, precision=ps.F64, move_set=ps.MOVES_CLUSTER, energy_type=ps.ISING, **CLUSTER),
          "cluster_kernel<double, state in memory>")


def test_rows_cluster_chain_wave(ps):
    check(ps, P(ps, num_chains=12, precision=ps.F64, move_set=ps.MOVES_CLUSTER, energy_type=ps.ISING, **CLUSTER),
          "cluster_chain_wave_kernel<double>")


@pytest.mark.parametrize("energy", ["interacting", "cutoff"])
def test_rows_cluster_all_pairs(ps, energy):
    kw = dict(CLUSTER, K1=0.5)
    et = ps.INTERACTING if energy == "interacting" else ps.CUTOFF
    check(ps, P(ps, num_chains=8, precision=ps.F64, move_set=ps.MOVES_CLUSTER, energy_type=et, cutoff_radius=3.0, **kw),
          "cluster_wave_kernel<double>")


def test_rows_umbrella(ps):
    check(ps, P(ps, n=14, E0=1.5, K1=1.0, Fz=0.2, num_chains=48, seed=27, umbrella=1, precision=ps.F64), "sweep_kernel<double>")


def test_rows_xoshiro(ps):
    check(ps, P(ps, n=20, E0=1.0, Fz=0.5, num_chains=64, seed=3, rng=ps.RNG_XOSHIRO128PP, precision=ps.F64), "sweep_kernel<double>")


def test_rows_packed_cases(ps, monkeypatch):
    monkeypatch.setenv("PSTAT_PACK", "1")
    cases = [P(ps, n=20, E0=0.5 + 0.1 * i, Fz=0.1 * i, kT=1.0 + 0.05 * i, num_chains=16, seed=40 + i, chain_id0=100 * i,
               precision=ps.F64) for i in range(9)]
    check(ps, cases, "[packed cases]", packed=1)


def test_rows_one_chain_per_case(ps):
    cases = [P(ps, n=12, E0=0.2 * i, Fz=0.05 * i, kT=0.5 + 0.1 * i, num_chains=1, seed=60 + i, precision=ps.F64)
             for i in range(37)]
    check(ps, cases, "sweep_kernel<double>")
    cl = [P(ps, num_chains=1, precision=ps.F64, move_set=ps.MOVES_CLUSTER, energy_type=ps.ISING, **dict(CLUSTER, E0=0.1 * i, seed=80 + i))
          for i in range(11)]
    check(ps, cl, "cluster_chain_wave_kernel<double>")


def test_rows_300_chains_two_blocks(ps):
    check(ps, P(ps, n=10, E0=1.0, Fz=0.5, num_chains=300, seed=6, precision=ps.F64), "sweep_kernel<double>")
    cases = [P(ps, n=10, E0=1.0, Fz=0.2 * i, num_chains=65, seed=7 + i, precision=ps.F64) for i in range(3)]
    check(ps, cases, "sweep_kernel<double>")       # the first size past one wavefront per case, several cases


def test_rows_more_than_65536_chains(ps):
    """A single case whose chains wrap the reduction's 256 x 256 grid: thread t of block b folds chains
    256 b + t + 65536 j in order of j."""
    check(ps, P(ps, n=6, E0=1.0, Fz=0.5, num_chains=70001, seed=8, precision=ps.F32), "sweep_kernel<float>", stepout=120, nrows=2)


# ---------------------------------------------------------------------------------------------- 2. row bookkeeping
def test_remainder_is_advanced_and_not_recorded(ps):
    p = P(ps, n=20, E0=1.0, Fz=0.5, num_chains=64, seed=11, precision=ps.F64)
    with ps.Ensemble(p) as a, ps.Ensemble(p) as b, ps.Ensemble(p) as whole:
        want = twin_rows(a, 250, 4)
        a.advance(50)
        s = b.open_series(8, angles=True)
        b.advance_series(s, 1050, 250)
        assert s.rows == 4
        assert_rows(s.read(), want)
        whole.advance(1050)
        assert_same_chains(a, b, probes(a))
        for c in probes(whole):                      # launch splitting leaves the trajectory and the counters alone
            x, y = whole.chain_state(c), b.chain_state(c)
            assert same(x["theta"], y["theta"]) and same(x["rng"], y["rng"]) and x["nacc_total"] == y["nacc_total"]
            assert x["steps_recorded"] == y["steps_recorded"] == 1050
        # stepout > nsteps: no row, the steps are taken
        b.advance_series(s, 100, 250)
        a.advance(100)
        assert s.rows == 4 and same(s.read()[1], want[1])
        assert_same_chains(a, b, probes(a))
        b.advance_series(s, 0, 5)
        assert s.rows == 4 and b.chain_state(0)["steps_recorded"] == 1150
        # a second recorded call appends
        more = twin_rows(a, 100, 3)
        b.advance_series(s, 300, 100)
        assert s.rows == 7
        got = s.read()
        assert_rows([g[:4] for g in got], want)
        assert_rows([g[4:] for g in got], more)
        assert_rows(s.read(2), [w[:2] for w in want])    # the first rows only
        # clear, then reuse: the memory is kept, the rows start over
        s.clear()
        assert s.rows == 0 and s.read()[0].shape == (0,)
        again = twin_rows(a, 60, 8)
        b.advance_series(s, 480, 60)
        assert_rows(s.read(), again)
        assert_same_chains(a, b, probes(a))


def test_rows_across_the_clustering_mains_ladder(ps):
    """reset_sampler / reset_averages / scale_kT between recorded calls behave as between two advance calls; rows
    already recorded stay."""
    cases = [P(ps, num_chains=6, precision=ps.F64, move_set=ps.MOVES_CLUSTER, energy_type=ps.ISING, **dict(CLUSTER, kT=kt))
             for kt in (0.8, 1.5)]
    with ps.Ensemble(cases) as a, ps.Ensemble(cases) as b:
        s = b.open_series(6, angles=True)
        want = []
        for mult in (10.0, 1.0):
            for e in (a, b):
                e.scale_kT(mult)
                e.reset_sampler()
                e.reset_averages()
            want.append(twin_rows(a, 150, 3))
            b.advance_series(s, 450, 150)
        got = s.read()
        assert list(got[0]) == [150, 300, 450, 150, 300, 450]
        assert_rows([g[:3] for g in got], want[0], "rung 10")
        assert_rows([g[3:] for g in got], want[1], "rung 1")
        assert_same_chains(a, b, probes(a))


def test_rows_across_reinit(ps):
    p = P(ps, n=15, E0=1.0, Fz=0.4, num_chains=40, seed=13, precision=ps.F64, energy_type=ps.ISING)
    for force in (True, False):
        with ps.Ensemble(p) as a, ps.Ensemble(p) as b:
            s = b.open_series(4)
            w0 = twin_rows(a, 200, 2)
            b.advance_series(s, 400, 200)
            a.reinit(force)
            b.reinit(force)
            w1 = twin_rows(a, 200, 2)
            b.advance_series(s, 400, 200)
            steps, red, micro, ang = s.read()
            assert ang is None and list(steps) == [200, 400, 600, 800]
            assert same(red[:2], w0[1]) and same(red[2:], w1[1]) and same(micro[:2], w0[2]) and same(micro[2:], w1[2])
            assert_same_chains(a, b, probes(a), f"force={force}")


# ---------------------------------------------------------------------------------------------- 3. refusals
def test_refusals_leave_the_handle_alone(ps):
    lib = ps._lib.load()
    p = P(ps, n=10, E0=1.0, Fz=0.5, num_chains=32, seed=14, precision=ps.F64)
    with ps.Ensemble(p) as e, ps.Ensemble(p) as other:
        s = e.open_series(2)
        e.advance_series(s, 100, 100)
        before = e.chain_state(5)
        with pytest.raises(ps.PstatError) as ei:
            e.advance_series(s, 250, 100)             # two more rows, one free
        assert ei.value.code == -7
        after = e.chain_state(5)
        assert after["steps_recorded"] == before["steps_recorded"] == 100 and same(after["rng"], before["rng"])
        assert same(after["theta"], before["theta"]) and s.rows == 1
        e.advance_series(s, 199, 100)                 # one row fits
        assert s.rows == 2 and e.chain_state(5)["steps_recorded"] == 299
        for nsteps, stepout in ((10, 0), (10, -3), (-1, 5)):
            with pytest.raises(ps.PstatError) as ei:
                e.advance_series(s, nsteps, stepout)
            assert ei.value.code == -1
        with pytest.raises(ps.PstatError) as ei:
            s.read(3)                                 # more rows than were recorded
        assert ei.value.code == -1
        with pytest.raises(ps.PstatError) as ei:
            e.open_series(0)
        assert ei.value.code == -1
        out = C.c_void_p()
        assert lib.pstat_series_open(e._h, 4, 2, C.byref(out)) == -1 and b"flags" in lib.pstat_last_error()
        buf = np.zeros(2 * e.n)
        assert lib.pstat_series_read(e._h, s._s, 1, None, None, None, buf.ctypes.data_as(C.POINTER(C.c_double))) == -1
        with pytest.raises(ps.PstatError) as ei:      # a series belongs to the handle it was opened on
            other.advance_series(s, 100, 100)
        assert ei.value.code == -1
        assert e.chain_state(5)["steps_recorded"] == 299 and other.chain_state(5)["steps_recorded"] == 0
        steps, red, micro, _ = s.read()
        assert list(steps) == [100, 200] and red.shape == (2, 1, ps.NRED) and micro.shape == (2, 1, 7)
        assert lib.pstat_series_read(e._h, s._s, 2, None, None, None, None) == 0     # any output may be NULL


# ---------------------------------------------------------------------------------------------- 4. shards
def test_shard_rows_merge_like_shard_reductions(ps):
    """Two handles holding chains 0-39 and 40-63 of one ensemble: the sum of their series rows through
    summary_from_reduction is the sum of their reduce_host vectors through the same function, row by row."""
    kw = dict(n=18, E0=1.0, Fz=0.5, seed=15, precision=ps.F64, energy_type=ps.ISING)
    shards = [P(ps, num_chains=40, chain_id0=0, **kw), P(ps, num_chains=24, chain_id0=40, **kw)]
    fields = ("avg", "stderr", "extra_avg", "extra_stderr")
    with ps.Ensemble(shards[0]) as a0, ps.Ensemble(shards[1]) as a1, ps.Ensemble(shards[0]) as b0, ps.Ensemble(shards[1]) as b1:
        want = []
        for r in range(3):
            red = np.zeros(ps.NRED)
            for e in (a0, a1):
                e.advance(200)
                red += e.reduce_host(0)
            want.append(ps.summary_from_reduction(red, 200 * (r + 1)))
        series = [e.open_series(3) for e in (b0, b1)]
        for e, s in zip((b0, b1), series):
            e.advance_series(s, 600, 200)
        reads = [s.read() for s in series]
        for r in range(3):
            red = np.zeros(ps.NRED)
            for rd in reads:
                red += rd[1][r, 0]
            got = ps.summary_from_reduction(red, int(reads[0][0][r]))
            for f in fields:
                assert same(np.array(getattr(got, f)), np.array(getattr(want[r], f))), (r, f)
            assert got.acceptance_ratio == want[r].acceptance_ratio and got.ar_stderr == want[r].ar_stderr
            assert got.num_chains == want[r].num_chains == 64 and got.steps_per_chain == want[r].steps_per_chain
            assert got.nan_rejects == want[r].nan_rejects and got.chains_collapsed == want[r].chains_collapsed
