"""GPU tests of the chain-shape recorder (pstat_shape_*, pstat_shape.hip) against the numpy twin of the contract
(tests/shape_ref.py): totals and rows equal to the twin's on the angles of an identical second ensemble, to the bound derived in the
twin's docstring; every edge of the kernel's mapping; nine homes; three closed forms; error bars, tempering, refusals;
tools/run_sweep.py --shape end to end.  The protocol of the comparison, the case tables and the tool call are those of
tests/recorder_cases.py, given shape_kind below; the lifecycle rules are asserted in tests/test_gpu_recorder_lifecycle.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import recorder_cases as rc
import shape_ref as sr
from recorder_cases import AXES, BASE, FIXED, angles_of_all, bits, ps, sweep_cases  # noqa: F401 (ps is the fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NG = 8


def random_q(nq, qmax1, seed=1, zero=True):
    """[nq, 3] with |q|_1 <= qmax1; the last one is 0 when there are at least two (S(0) = n is asserted bit for bit)."""
    rng = np.random.default_rng(seed)
    q = rng.uniform(-1.0, 1.0, (nq, 3))
    q *= (qmax1 * rng.uniform(0.05, 1.0, (nq, 1))) / np.abs(q).sum(axis=1, keepdims=True)
    if zero and nq >= 2:
        q[-1] = 0.0
    return q


def shape_kind(cases, q, planar=False):
    """The descriptor of rc.run_totals_twin.  A row is a mean of `per` values: the bound of a total of `per`, over `per`."""
    n, per, ncases = int(cases[0].n), int(cases[0].num_chains), len(cases)
    q = sr.wave_vectors(q, planar=False)                             # (the library, not the test, drops a planar handle's q_y)
    nq = len(q)

    def exact(got, rows, values, per):
        M = per * len(values)
        for k in range(ncases):
            for j in np.flatnonzero(~q.any(axis=1)):                 # S(0) = n for every chain: n M and n^2 M, exactly
                assert got.sum[k, NG + j] == float(n * M) and got.sumsq[k, NG + j] == float(n * n * M), (k, j)
            if planar:
                for name in ("gyy", "gxy", "gyz"):
                    i = sr.NAMES.index(name)
                    assert got.sum[k, i] == 0.0 and got.sumsq[k, i] == 0.0 and (rows is None or np.all(rows[:, k, i] == 0.0)), name

    return rc.Totals(
        name="shape", ncols=NG + nq, open=lambda e, capacity: e.open_shape(q, capacity_rows=capacity),
        twin=lambda ang, k: (sr.per_chain(ang, cases[k].b, q, planar=planar),),
        bounds=lambda k, M, twins: sr.bounds(n, cases[k].b, M, q, planar),
        row_bound=lambda k, per, M, twins: sr.bounds(n, cases[k].b, per, q, planar)[0] / per, exact=exact,
        line=f"n = {n}, nq = {nq}, {ncases} x {per} chains: largest |device - twin| / bound = {{worst:.4f}}")


def run_exact(ps, cases, q, planar=False, records=6):
    return rc.run_totals_twin(ps, cases, shape_kind(cases, q, planar), planar=planar, records=records)


# ------------------------------------------------------------------------------------------------ every edge of the mapping
# nq = 5: groups of 8 threads, three of them idle
@pytest.mark.parametrize("ncases,per", rc.TILE_SHAPES)
def test_totals_and_rows_equal_the_twin(ps, ncases, per):
    run_exact(ps, sweep_cases(ps, ncases, per, 12, seed=800), random_q(5, 6.0))


# one monomer (G = 0, S = 1); two; three; more monomers than lanes (scan segments of 2, a last lane's segment short); n = 130:
# segments of 3, lanes beyond the chain's end
@pytest.mark.parametrize("n", [1, 2, 3, 65, 130])
def test_chain_lengths(ps, n):
    got = run_exact(ps, sweep_cases(ps, 3, 5, n, seed=820), random_q(5, 6.0, seed=n))
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
    got = run_exact(ps, cases, random_q(5, 6.0 / 2.5))
    rg = got.rg2
    assert rg[0] < rg[1] < rg[2] and rg[2] > 5 * rg[0]              # lengths scale with b: rg2 with b^2 (25 x between the ends)


# ------------------------------------------------------------------------------------------------ the homes
@pytest.mark.parametrize("home", list(rc.HOMES))
def test_every_home(ps, home):
    cases, planar = rc.home_cases(ps, home, seed=900)
    got = run_exact(ps, cases, random_q(5, 6.0, seed=3), planar=planar)      # (a planar handle is given q_y != 0 and ignores it)
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
    cases = rc.ladder_cases(ps)
    rc.totals_between_exchange_rounds(ps, cases, shape_kind(cases, random_q(3, 4.0, seed=9)))


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
        e.advance(5)                                                 # the handle still advances
        assert e.chain_state(0)["steps_recorded"] == 5
        assert e.open_shape().read().sq.shape == (3, 0)              # no wave-vectors
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
def test_sweep_writes_shape_files(tmp_path):
    with_shape = rc.sweep_tool(tmp_path, "s", "--shape", "z:6:8,x:6:8")
    plain = rc.sweep_tool(tmp_path, "p")
    outs, _ = rc.assert_out_files_unchanged(with_shape, plain, ".shape")
    assert len(outs) == 4
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
