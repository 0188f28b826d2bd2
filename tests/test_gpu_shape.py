"""GPU tests of the chain-shape recorder (pstat_shape_*, pstat_shape.hip) against the numpy twin of the contract
(tests/shape_ref.py): totals and rows equal to the twin's on the angles of an identical second ensemble, to the bound derived in the
twin's docstring; every edge of the kernel's mapping; nine homes; three closed forms; error bars, tempering, refusals;
tools/run_sweep.py --shape end to end."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import shape_ref as sr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NG = 8


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
    """The HIP runtime libpstat has loaded into this process (the rows of pstat_shape_rows are device memory)."""
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


def random_q(nq, qmax1, seed=1, zero=True):
    """[nq, 3] with |q|_1 <= qmax1; the last one is 0 when there are at least two (S(0) = n is asserted bit for bit)."""
    rng = np.random.default_rng(seed)
    q = rng.uniform(-1.0, 1.0, (nq, 3))
    q *= (qmax1 * rng.uniform(0.05, 1.0, (nq, 1))) / np.abs(q).sum(axis=1, keepdims=True)
    if zero and nq >= 2:
        q[-1] = 0.0
    return q


def run_exact(ps, cases, q, planar=False, stepout=40, records=6):
    """A records with advance_shape (rows kept), B advances `stepout` at a time and reads every chain's angles: the twin on B's
    angles gives A's sum, sumsq and rows within the derived bound (shape_ref's docstring); S(q = 0) is n M bit for bit; a second A
    gives the same bits; A's chains end as B's.  Returns (ShapeResult, largest |device - twin| / bound)."""
    n, per, ncases = int(cases[0].n), int(cases[0].num_chains), len(cases)
    q = sr.wave_vectors(q, planar=False)                             # (the library, not the test, drops a planar handle's q_y)
    nq = len(q)
    with ps.Ensemble(cases, planar=planar) as A, ps.Ensemble(cases, planar=planar) as B, ps.Ensemble(cases, planar=planar) as A2:
        g = A.open_shape(q, capacity_rows=records)
        A.advance_shape(g, records * stepout + 7, stepout)           # the remainder is advanced and not recorded
        g2 = A2.open_shape(q, capacity_rows=records)
        A2.advance_shape(g2, records * stepout + 7, stepout)
        values = []                                                  # [record][case] -> [per, ncols]
        for _ in range(records):
            B.advance(stepout)
            ang = angles_of_all(B).reshape(ncases, per, 2 * n)
            values.append([sr.per_chain(ang[k], cases[k].b, q, planar=planar) for k in range(ncases)])
        B.advance(7)
        got, again = g.read(), g2.read()
        assert got.records == records and got.sum.shape == (ncases, NG + nq)
        assert bits(got.sum) == bits(again.sum) and bits(got.sumsq) == bits(again.sumsq), "two identical runs differ"
        ptr, nrows, stride = g.rows()
        assert nrows == records and stride == ncases * (NG + nq) and ptr
        rows = np.zeros((nrows, stride))
        assert hip_runtime().hipMemcpy(rows.ctypes.data, ptr, rows.nbytes, 2) == 0      # 2: device to host
        rows = rows.reshape(nrows, ncases, -1)
        ptr2, _, _ = g2.rows()
        rows2 = np.zeros((nrows, stride))
        assert hip_runtime().hipMemcpy(rows2.ctypes.data, ptr2, rows2.nbytes, 2) == 0
        assert bits(rows) == bits(rows2), "two identical runs differ in their rows"
        worst = 0.0
        M = per * records
        for k in range(ncases):
            want_s = sum(v[k].sum(axis=0) for v in values)
            want_q = sum((v[k] * v[k]).sum(axis=0) for v in values)
            b1, b2 = sr.bounds(n, cases[k].b, M, q, planar)
            r1 = sr.bounds(n, cases[k].b, per, q, planar)[0] / per
            e1, e2 = np.abs(got.sum[k] - want_s), np.abs(got.sumsq[k] - want_q)
            worst = max(worst, float((e1 / b1).max()), float((e2 / b2).max()))
            assert np.all(e1 <= b1), (k, (e1 / b1).max(), int((e1 / b1).argmax()))
            assert np.all(e2 <= b2), (k, (e2 / b2).max(), int((e2 / b2).argmax()))
            for r in range(records):
                er = np.abs(rows[r, k] - values[r][k].sum(axis=0) / per)
                worst = max(worst, float((er / r1).max()))
                assert np.all(er <= r1), (k, r, (er / r1).max())
            for j in np.flatnonzero(~q.any(axis=1)):                 # S(0) = n for every chain: n M and n^2 M, exactly
                assert got.sum[k, NG + j] == float(n * M) and got.sumsq[k, NG + j] == float(n * n * M), (k, j)
            if planar:
                for name in ("gyy", "gxy", "gyz"):
                    i = sr.NAMES.index(name)
                    assert got.sum[k, i] == 0.0 and got.sumsq[k, i] == 0.0 and np.all(rows[:, k, i] == 0.0), name
        print(f"n = {n}, nq = {nq}, {ncases} x {per} chains: largest |device - twin| / bound = {worst:.4f}")
        C_ = ncases * per
        edges = {c for k in range(ncases) for j in (0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, per - 1) if j < per for c in [k * per + j]}
        assert_same_chains(A, B, range(C_) if C_ <= 700 else sorted(edges))
        g.close()
        return got, worst


BASE = dict(E0=1.0, K1=0.5, K2=0.2, Fz=0.5, steps_per_adjust=150)
CLUSTER = dict(move_set=1, cluster_prob=0.5, bend_mod=0.3, bend_angle=0.2)


def sweep_cases(ps, ncases, per, n, seed=800, **kw):
    return [ps.default_params(n=n, num_chains=per, precision=ps.F64, kT=0.7 + 0.2 * k, seed=seed + k, **{**BASE, **kw}) for k in range(ncases)]


# ------------------------------------------------------------------------------------------------ every edge of the mapping
# chains per case: 1, 5 (one tile, not full), 64 (four full tiles of 16), 65 (a last tile of one chain), 1100 (69 tiles: more
# than the 64 lanes of the fold); 9 cases: the fold's last workgroup is not full.  nq = 5: groups of 8 threads, three of them idle
@pytest.mark.parametrize("ncases,per", [(1, 1), (3, 5), (9, 64), (9, 65), (2, 1100)])
def test_totals_and_rows_equal_the_twin(ps, ncases, per):
    run_exact(ps, sweep_cases(ps, ncases, per, 12), random_q(5, 6.0))


# one monomer (G = 0, S = 1); two; three; more monomers than lanes (scan segments of 2, a last lane's segment short); n = 130:
# segments of 3, lanes beyond the chain's end
@pytest.mark.parametrize("n", [1, 2, 3, 65, 130])
def test_chain_lengths(ps, n):
    got, _ = run_exact(ps, sweep_cases(ps, 3, 5, n, seed=820), random_q(5, 6.0, seed=n))
    if n == 1:
        assert np.all(got.sum[:, :NG] == 0.0)
        np.testing.assert_allclose(got.mean[:, NG:], 1.0, atol=4e-16)


# nq = 0 (the hot loop is skipped), 1 (every thread a group of its own), 63 and 64 (groups of one wave), 65 (groups of 128
# threads, 63 idle), 257 (two slots per thread)
@pytest.mark.parametrize("nq", [0, 1, 63, 64, 65, 257])
def test_wave_vector_counts_at_n_130(ps, nq):
    run_exact(ps, sweep_cases(ps, 3, 5, 130, seed=840), random_q(nq, 6.0, seed=nq) if nq else None, records=3)


def test_cases_that_differ_in_b(ps):
    cases = [ps.default_params(n=12, num_chains=20, precision=ps.F64, kT=1.0, seed=870 + k, b=b, **BASE) for k, b in enumerate((0.5, 1.0, 2.5))]
    got, _ = run_exact(ps, cases, random_q(5, 6.0 / 2.5))
    rg = got.rg2
    assert rg[0] < rg[1] < rg[2] and rg[2] > 5 * rg[0]              # lengths scale with b: rg2 with b^2 (25 x between the ends)


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
    got, _ = run_exact(ps, cases, random_q(5, 6.0, seed=3), planar=planar)   # (a planar handle is given q_y != 0 and ignores it)
    assert np.all(got.rg2 > 0) and np.all(got.sq[:, :4] > 0)


# ------------------------------------------------------------------------------------------------ closed forms
@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "shape_closed_form.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", ["fjc", "fixed_force", "planar"])
def test_closed_forms(ps, golden, name):
    """16 384 chains, 1 000 n steps of burn-in, ONE record: every column the fixture has within 5 of its own across-chain standard
    errors of the closed form and each such error <= 2 % of the fixture value (shape_ref.judge_closed_form, the conditions
    tests/test_shape_cpu.py puts to directly sampled chains); the q = 0 column exactly n.  The fixture has no closed form for trg2 (its
    generator says why): that column is not judged.  Device figures (MI355X): largest |z| 1.38 / 1.93 / 1.53, largest standard
    error 0.75 / 0.84 / 0.83 % of the fixture value."""
    c = golden[name]
    planar = name == "planar"
    N = 16384
    make = ps.default_planar_params if planar else ps.default_params
    p = make(num_chains=N, precision=ps.F64, seed=20261019, **c["params"])
    with ps.Ensemble(p, planar=planar) as e:
        print(e.launch_info().kernel.decode())
        g = e.open_shape(c["q"])
        e.advance(1000 * c["params"]["n"])
        g.record()
        got = g.read()
    assert got.records == 1
    mean, se = got.mean[0], got.chain_stderr[0]
    print(f"{name}\n  mean  ", np.round(mean, 5), "\n  stderr", np.round(se, 5))
    z, r = sr.judge_closed_form(name, c, mean, se)
    print(f"{name}: largest |z| = {z:.2f}, largest stderr / value = {100 * r:.2f} %")
    if name == "fixed_force":                                        # pulled taut along z: less scattering along the pull
        along = lambda axis: {v[axis] for v in c["q"] if v[axis] != 0.0 and sum(x != 0.0 for x in v) == 1}
        common = sorted(along(2) & along(0))
        assert len(common) >= 4
        for m in common:
            par = got.sq[0, c["q"].index([0.0, 0.0, m])]
            perp = got.sq[0, c["q"].index([m, 0.0, 0.0])]
            assert par < perp, (m, par, perp)
    a = ps.shape_anisotropy(got)[0]
    assert 0.0 < a < 1.0
    if name == "planar":
        assert np.all(got.gyration[0, 1, :] == 0.0) and np.all(got.gyration[0, :, 1] == 0.0)


# ------------------------------------------------------------------------------------------------ composition
def test_error_bars_are_the_blocking_transform_of_the_rows(ps):
    cases = sweep_cases(ps, 3, 20, 10, seed=940)
    q = [[0.0, 0.0, 1.0], [1.0, 0.0, 0.0]]
    with ps.Ensemble(cases) as e:
        g = e.open_shape(q, capacity_rows=64)
        e.advance_shape(g, 64 * 25, 25)
        eb = g.error_bars()
        ptr, nrows, stride = g.rows()
        assert (nrows, stride) == (64, 3 * 10)
        by_hand = ps.blocking_device(ptr, nrows, stride)
        for f in ("mean", "stderr", "stderr_err", "inefficiency", "level", "converged"):
            assert getattr(eb, f).shape == (3, 10) and bits(getattr(eb, f)) == bits(getattr(by_hand, f).reshape(3, 10)), f
        res = g.read()
        np.testing.assert_allclose(eb.mean, res.mean, rtol=1e-13)
        assert np.all(np.isnan(res.chain_stderr)) and eb.nbatches == 64 and np.all(eb.stderr[:, [0, 1, 2, 6, 7, 8, 9]] > 0)
        assert res.gyration.shape == (3, 3, 3) and res.sq.shape == (3, 2) and res.q.shape == (2, 3)
        np.testing.assert_array_equal(res.gyration[:, 0, 2], res.mean[:, 4])
        np.testing.assert_array_equal(res.gyration, np.transpose(res.gyration, (0, 2, 1)))
        # ratio of averages: (3 <trg2> - <rg2^2>) / (2 <rg2^2>) with <rg2^2> from sumsq
        rg4 = res.sumsq[:, 6] / (64 * 20)
        np.testing.assert_allclose(ps.shape_anisotropy(res), (3 * res.mean[:, 7] - rg4) / (2 * rg4), rtol=1e-15)
        with pytest.raises(ps.PstatError) as err:                    # fewer rows than min_blocks: the transform's own refusal
            g.error_bars(min_blocks=65)
        assert err.value.code == -7
        g.clear()
        assert g.read().records == 0 and g.rows()[1] == 0 and np.all(g.read().sum == 0)


def test_records_between_exchange_rounds(ps):
    kTs = [0.25, 0.35, 0.5, 0.75, 1.2, 2.0, 4.0]                     # the ladder of the README's example
    cases = [ps.default_params(n=8, E0=3.0, Fz=0.2, kT=kT, num_chains=64, seed=i) for i, kT in enumerate(kTs)]
    q = random_q(3, 4.0, seed=9)
    with ps.Ensemble(cases) as A, ps.Ensemble(cases) as B:
        ta, tb = (e.open_tempering(ps.ladders_by(cases), seed=9) for e in (A, B))
        g = A.open_shape(q)
        values = []
        for _ in range(5):
            A.advance_tempered(ta, 200, 50)
            g.record()
            B.advance_tempered(tb, 200, 50)
            ang = angles_of_all(B).reshape(7, 64, 16)
            values.append([sr.per_chain(ang[k], cases[k].b, q) for k in range(7)])
        got = g.read()
        sa, sb = ta.stats(), tb.stats()
        assert sa[2] == sb[2] == 20 and sa[1].sum() > 0, "no exchange was accepted: the records would not show a swapped configuration"
        assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1])
        assert_same_chains(A, B, range(7 * 64))
    for k in range(7):
        want = sum(v[k].sum(axis=0) for v in values)
        assert np.all(np.abs(got.sum[k] - want) <= sr.bounds(8, cases[k].b, 64 * 5, q)[0])
    assert got.records == 5


def test_refusals_leave_the_handle_usable(ps):
    lib = ps._lib.load()
    dp = C.POINTER(C.c_double)
    with ps.Ensemble([ps.default_params(n=6, num_chains=4, kT=kT, umbrella=1) for kT in (1.0, 2.0)]) as e:
        with pytest.raises(ps.PstatError) as err:
            e.open_shape([[0.0, 0.0, 1.0]])
        assert err.value.code == -4 and "umbrella" in str(err.value)
        e.advance(20)
        assert e.chain_state(0)["steps_recorded"] == 20
    cases = [ps.default_params(n=6, num_chains=4, kT=kT, Fz=0.3) for kT in (1.0, 2.0, 3.0)]
    with ps.Ensemble(cases) as e:
        out = C.c_void_p()
        one = np.array([[0.0, 0.0, 1.0]])
        big = np.array([[0.0, 2.0e4, 0.0]])
        nan = np.array([[np.inf, 0.0, 0.0]])
        many = np.zeros((513, 3))
        for args, code, needle in (((None, -1, 0), -1, "nq"), ((many.ctypes.data_as(dp), 513, 0), -4, "PSTAT_SHAPE_MAX_Q"),
                                   ((None, 1, 0), -1, "q is null"), ((nan.ctypes.data_as(dp), 1, 0), -1, "q[0][0]"),
                                   ((one.ctypes.data_as(dp), 1, -1), -1, "capacity_rows"), ((big.ctypes.data_as(dp), 1, 0), -1, "q[0]")):
            assert lib.pstat_shape_open(e._h, *args, C.byref(out)) == code and needle.encode() in lib.pstat_last_error(), needle
        g = e.open_shape(one, capacity_rows=2)
        with ps.Ensemble(cases[:2]) as other:                        # an object of another handle
            assert lib.pstat_shape_record(other._h, g._g) == -1 and b"not an open one" in lib.pstat_last_error()
            assert lib.pstat_advance_shape(other._h, g._g, 10, 5) == -1
            assert lib.pstat_shape_read(other._h, g._g, None, None, None) == -1
            assert lib.pstat_shape_clear(other._h, g._g) == -1
            lib.pstat_shape_close(other._h, g._g)                    # ignored: it is not the other handle's to close
        assert lib.pstat_advance_shape(e._h, g._g, 10, 0) == -1 and lib.pstat_advance_shape(e._h, g._g, -1, 5) == -1
        e.advance_shape(g, 25, 10)
        assert g.read().records == 2 and e.chain_state(0)["steps_recorded"] == 25
        # the row buffer is full: refused with nothing enqueued
        assert lib.pstat_advance_shape(e._h, g._g, 10, 10) == -7 and lib.pstat_shape_record(e._h, g._g) == -7
        assert e.chain_state(0)["steps_recorded"] == 25 and g.read().records == 2
        e.advance_shape(g, 9, 10)                                    # no record in this call: it fits
        assert e.chain_state(0)["steps_recorded"] == 34
        g.clear()
        g.record()
        records = C.c_int64(-1)                                      # every output may be NULL
        assert lib.pstat_shape_read(e._h, g._g, None, None, C.byref(records)) == 0 and records.value == 1
        totals = e.open_shape()                                      # no wave-vectors, no rows kept: no limit, and no rows to hand out
        e.advance_shape(totals, 50, 1)
        assert totals.read().records == 50 and totals.rows() == (0, 0, 3 * 8) and totals.read().sq.shape == (3, 0)
        with pytest.raises(ps.PstatError):
            totals.error_bars()
        raw = g._g
        g.close()
        assert lib.pstat_shape_read(e._h, raw, None, None, None) == -1    # read after close
        assert lib.pstat_shape_record(e._h, raw) == -1
        e.advance(5)
        assert e.chain_state(0)["steps_recorded"] == 89
        e.open_shape(one).record()                                   # destroyed with an object open
    with ps.Ensemble(ps.default_params(n=2561, num_chains=1)) as e:  # beyond a workgroup's LDS
        with pytest.raises(ps.PstatError) as err:
            e.open_shape()
        assert err.value.code == -4 and "2560" in str(err.value)
        e.advance(2)
        assert e.chain_state(0)["steps_recorded"] == 2
    p = ps.default_planar_params(n=2560, num_chains=2, Fz=0.5)
    with ps.Ensemble(p, planar=True) as e:                           # planar n = 2560 fits: a tile of one chain, scan segments of 40
        q = np.array([[1.0e-3, 0.0], [0.0, 2.0e-3]])                 # [nq, 2] = (q_x, q_z)
        g = e.open_shape(q)
        e.advance(50)
        g.record()
        want = sr.per_chain(angles_of_all(e), p.b, q, planar=True).sum(axis=0)
        assert np.all(np.abs(g.read().sum[0] - want) <= sr.bounds(2560, p.b, 2, q, planar=True)[0])


# ------------------------------------------------------------------------------------------------ the tool
AXES = [("n", "8"), ("Fz", "0,1,2,3")]
FIXED = ["--num-steps", "3200", "--stepout", "100", "-v", "0"]


def _sweep(tmp_path, name, *extra):
    out = tmp_path / name
    axes = [a for k, v in AXES for a in ("--axis", f"{k}={v}")]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_sweep.py"), str(out), *axes,
                        "--num-chains", "64", "--seed", "11", *extra, "--", *FIXED], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def test_sweep_writes_shape_files(tmp_path):
    with_shape = _sweep(tmp_path, "s", "--shape", "z:6:8,x:6:8")
    plain = _sweep(tmp_path, "p")
    outs = sorted(f for f in os.listdir(plain) if f.endswith(".out"))
    assert len(outs) == 4 and sorted(f for f in os.listdir(with_shape) if f.endswith(".out")) == outs
    for f in outs:                                                   # the .out files are a plain run's, byte for byte
        assert (with_shape / f).read_bytes() == (plain / f).read_bytes(), f
    assert not [f for f in os.listdir(plain) if f.endswith(".shape")]
    shapes = sorted(f for f in os.listdir(with_shape) if f.endswith(".shape"))
    assert shapes == [f[:-len(".out")] + ".shape" for f in outs]
    # the same sweep through the Python API: the hosts' run_cases with shape=, every case of the ensemble at once
    from polymer_stats_amd import sweep as sw
    cases = sw.product_cases([(k, sw.axis_values(v)) for k, v in AXES])
    plist = sw.plan("mcmc_eap_chain", FIXED, cases, str(tmp_path / "api"), num_chains=64, seed=11)
    info = {}
    spec = sw.parse_shape("z:6:8,x:6:8")
    sw.MAINS["mcmc_eap_chain"].run_cases(plist, write_csv=False, info=info, record=sw.Recording("shape", spec))
    res, eb = info["shape"]
    assert res.records == 32 and res.q.shape == (16, 3)
    np.testing.assert_array_equal(res.q[:8, 2], 6.0 * np.arange(1, 9) / 8)
    np.testing.assert_array_equal(res.q[8:, 0], 6.0 * np.arange(1, 9) / 8)
    sz, sx = [], []
    for k, p in enumerate(plist):
        lines = (with_shape / (p["_name"] + ".shape")).read_text().strip().split("\n")
        assert lines[0] == "name,qx,qy,qz,value,stderr" and len(lines) == 1 + 8 + 16
        rows = [line.split(",") for line in lines[1:]]
        assert [r[0] for r in rows] == list(ps_names()) + ["sq"] * 16
        assert all(r[1:4] == ["", "", ""] for r in rows[:8])
        np.testing.assert_array_equal(np.array([[float(v) for v in r[1:4]] for r in rows[8:]]), res.q)
        value, stderr = np.array([float(r[4]) for r in rows]), np.array([float(r[5]) for r in rows])
        assert bits(value) == bits(res.mean[k]) and bits(stderr) == bits(eb.stderr[k]), p["_name"]
        assert np.all(np.isfinite(value)) and np.all(stderr[[0, 1, 2, 6, 7]] > 0) and np.all(stderr[8:] > 0)
        sz.append(value[8:16])
        sx.append(value[16:])
    # pulled taut along z the chain scatters less along the pull than across it, at every magnitude
    assert np.all(sz[-1] < sx[-1]) and np.all(sz[-1][:4] < sz[0][:4])


def ps_names():
    import polymer_stats_amd as ps
    return ps.SHAPE_NAMES
