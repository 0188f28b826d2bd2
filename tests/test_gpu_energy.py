"""GPU tests of the energy recorder (pstat_energy_*, pstat_energy.hip) against the numpy twin of the contract
(tests/energy_ref.py): totals and rows equal to the twin's on the angles of an identical second ensemble, to the bound derived in
the twin's docstring; every edge of the kernel's mapping; the homes; THE PARTS ADD UP TO THE U THE STEP KERNEL CARRIES; exact
configurations; closed forms; error bars, tempering, refusals; the lifecycle rules of DESIGN.md 3.17 for this kind;
tools/run_sweep.py --energy end to end.  The protocol of the comparison, the case tables and the tool call are those of
tests/recorder_cases.py, given energy_kind below."""
import ctypes as C
import json
import os
import struct

import numpy as np
import pytest

import energy_ref as er
import recorder_cases as rc
import test_gpu_recorder_lifecycle as lc
from recorder_cases import AXES, BASE, FIXED, angles_of_all, assert_same_chains, bits, ps, sweep_cases  # noqa: F401 (ps is the fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOURPI = 4.0 * 3.14159265358979323846


def energy_kind(cases, max_sep=-1, cutoff=None, planar=False):
    """The descriptor of rc.run_totals_twin.  `cutoff`: None (no `within` column), a number, or one per case."""
    n, per, ncases = int(cases[0].n), int(cases[0].num_chains), len(cases)
    sep = n - 1 if max_sep < 0 else max_sep
    cuts = np.zeros(ncases) if cutoff is None else np.broadcast_to(np.asarray(cutoff, dtype=np.float64), (ncases,))
    ncols = er.ncols(sep, bool(cuts.any()))

    def bounds(k, M, twins):
        both = [er.bounds(t, cases[k], n, M, sep, cuts[k]) for t in twins]
        return sum(b[0] for b in both), sum(b[1] for b in both)

    def row_bound(k, per, M, twins):
        return np.max([er.row_bound(t, cases[k], n, sep, cuts[k]) for t in twins], axis=0)

    def exact(got, rows, values, per):
        for k in range(ncases):
            assert sum(int(v[k].undecided.sum()) for v in values) == 0, "a pair sits on the radius: the condition of energy_ref fails"
            if cases[k].bend_mod == 0.0:                             # no bending: 0.0, bit for bit
                assert got.sum[k, 2] == 0.0 and got.sumsq[k, 2] == 0.0 and (rows is None or np.all(rows[:, k, 2] == 0.0)), k
            if sep == n - 1:                                         # every separation has its column: nothing is left for `rest`
                assert got.sum[k, 3 + sep] == 0.0 and got.sumsq[k, 3 + sep] == 0.0 and (rows is None or np.all(rows[:, k, 3 + sep] == 0.0)), k
        assert got.has_within == bool(cuts.any()) and got.pair.shape == (ncases, sep)

    return rc.Totals(
        name="energy", ncols=ncols,
        open=lambda e, capacity: e.open_energy(max_sep, cutoff, capacity_rows=capacity),
        twin=lambda ang, k: er.per_chain(ang, cases[k], max_sep, cuts[k], planar),
        bounds=bounds, row_bound=row_bound, exact=exact,
        line=f"n = {n}, {ncases} x {per} chains, max_sep {max_sep}, cutoff {cutoff}: largest |device - twin| / bound = {{worst:.3g}}")


def run_exact(ps, cases, planar=False, records=3, **options):
    return rc.run_totals_twin(ps, cases, energy_kind(cases, planar=planar, **options), planar=planar, records=records)


# ------------------------------------------------------------------------------------------------ every edge of the mapping
@pytest.mark.parametrize("ncases,per", rc.TILE_SHAPES)
def test_totals_and_rows_equal_the_twin(ps, ncases, per):
    run_exact(ps, sweep_cases(ps, ncases, per, 12, seed=2100), max_sep=5, cutoff=1.5, records=2 if per == 1100 else 3)


# one monomer (no pair); two (one pair, u = 1 alone); three (u = 1 paired with s' = 2); 63, 64, 65: the n pairs of a pass end one
# short of the 64 lanes, fill them, spill one into a second stride; 130: three strides, scan segments of 3
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 130])
def test_chain_lengths(ps, n):
    got = run_exact(ps, sweep_cases(ps, 3, 5, n, seed=2120), cutoff=1.5 if n > 1 else None, records=2)
    assert got.pair.shape == (3, n - 1)
    if n == 1:
        assert got.sum.shape == (3, 4) and np.all(got.sum[:, 3] == 0.0)


@pytest.mark.parametrize("cutoff", [None, 1.5, [1.0, 1.5, 2.5]], ids=["no cutoff", "shared", "per case"])
@pytest.mark.parametrize("max_sep", [0, 1, 5, 11])
def test_separations_at_n_12(ps, max_sep, cutoff):
    got = run_exact(ps, sweep_cases(ps, 3, 5, 12, seed=2130), max_sep=max_sep, cutoff=cutoff, records=2)
    assert got.pair.shape == (3, max_sep) and got.sum.shape[1] == 3 + max_sep + 1 + (cutoff is not None)
    assert (got.within is None) == (cutoff is None) and np.all(np.isfinite(got.sum))


@pytest.mark.parametrize("n", [12, 65])
def test_one_separation_per_pass_gives_the_same_within_the_bound(ps, monkeypatch, n):
    """PSTAT_ENERGY_MAP=s: the mapping that was measured against the one kept meets the same contract."""
    monkeypatch.setenv("PSTAT_ENERGY_MAP", "s")
    run_exact(ps, sweep_cases(ps, 3, 5, n, seed=2140), max_sep=4, cutoff=1.5, records=2)


# ------------------------------------------------------------------------------------------------ the homes
ALL_PAIRS_CLUSTER = dict(n=16, energy_type=1, move_set=1, cluster_prob=0.5, bend_mod=0.3, bend_angle=0.2)
CUTOFF_HOME = dict(n=16, energy_type=3, move_set=1, cluster_prob=0.5, bend_mod=0.3, bend_angle=0.2, cutoff_radius=1.5)
EXTRA_HOMES = {"clustering all-pairs": (ALL_PAIRS_CLUSTER, "cluster_wave_kernel"), "cutoff": (CUTOFF_HOME, "cluster_wave_kernel")}
F64_HOMES = [h for h, row in rc.HOMES.items() if row[1] == 1] + list(EXTRA_HOMES)


def cases_of_home(ps, home, seed):
    """(cases, planar) of a row of rc.HOMES or of EXTRA_HOMES."""
    if home in rc.HOMES:
        return rc.home_cases(ps, home, seed)
    kw, has = EXTRA_HOMES[home]
    cases = [ps.default_params(num_chains=70, precision=ps.F64, kT=0.8 + 0.3 * k, seed=seed + k, **{**BASE, **kw, "E0": E0})
             for k, E0 in enumerate((0.5, 1.0, 1.5))]
    with ps.Ensemble(cases) as e:
        assert has in e.launch_info().kernel.decode(), e.launch_info().kernel.decode()
    return cases, False


def own_cutoff(ps, cases):
    return [float(c.cutoff_radius) for c in cases] if int(cases[0].energy_type) == ps.CUTOFF else None


@pytest.mark.parametrize("home", list(rc.HOMES) + list(EXTRA_HOMES))
def test_every_home(ps, home):
    cases, planar = cases_of_home(ps, home, seed=2200)
    got = run_exact(ps, cases, max_sep=4, cutoff=1.5, planar=planar, records=2)
    assert np.all(np.isfinite(got.sum)) and got.records == 2


def test_packed_cases(ps, monkeypatch):
    monkeypatch.setenv("PSTAT_PACK", "1")
    cases = [ps.default_params(n=20, E0=0.5 + 0.1 * i, Fz=0.1 * i, kT=1.0 + 0.05 * i, num_chains=16, seed=2240 + i, chain_id0=100 * i,
                               precision=ps.F64) for i in range(9)]
    with ps.Ensemble(cases) as e:
        assert e.launch_info().packed_cases == 1, e.launch_info().kernel.decode()
    run_exact(ps, cases, max_sep=6, cutoff=1.5, records=2)


# ------------------------------------------------------------------------------------------------ the parts add up to the kernel's U
ALL_PAIRS_E0 = (0.1, 0.2, 0.3)


def model_against_microstate(ps, home, seed):
    """After 47 steps and again after 127 more: per case, (|model_sum - sum_c U_c|, the derived bound, the scale).  The all-pairs
    homes run at ALL_PAIRS_E0 in place of the homes' 0.5, 1, 1.5: at those the dipole attraction draws pairs together within the
    174 steps (a case's scale grew from 1e3 to 2e4, one pair at r ~ 0.005 b), where the bound on that pair's cancelling
    separation, 11.5 eps_d / r of its term, passes the 1e-9 that keeps the test meaningful.  At the lower fields the chains stay
    open; every term is still far above 1e-9 of the scale."""
    cases, planar = cases_of_home(ps, home, seed)
    if int(cases[0].energy_type) in (ps.INTERACTING, ps.CUTOFF):
        for c, E0 in zip(cases, ALL_PAIRS_E0):
            c.E0 = E0
    n, per, ncases = int(cases[0].n), int(cases[0].num_chains), len(cases)
    cutoff = own_cutoff(ps, cases)
    cuts = cutoff or [0.0] * ncases
    out = []
    with ps.Ensemble(cases, planar=planar) as e:
        g = e.open_energy(-1, None)                                  # (a CUTOFF handle: its cases' own radii)
        snaps = [[er.per_chain(a, cases[k], -1, cuts[k], planar) for k, a in enumerate(angles_of_all(e).reshape(ncases, per, 2 * n))]]
        T = 0
        for steps in (47, 127):
            e.advance(steps)
            T += steps
            g.clear()
            g.record()
            got = g.read()
            snaps.append([er.per_chain(a, cases[k], -1, cuts[k], planar) for k, a in enumerate(angles_of_all(e).reshape(ncases, per, 2 * n))])
            U = rc.micro_of_all(e)[:, :, 6].sum(axis=1)
            for k in range(ncases):
                bound, scale = er.model_bound([s[k] for s in snaps], cases[k], n, T, int(cases[k].energy_type), -1, cuts[k])
                assert snaps[-1][k].undecided.sum() == 0
                out.append((T, k, abs(got.model_sum[k] - U[k]), bound, scale))
    return out


@pytest.mark.parametrize("home", F64_HOMES)
def test_the_parts_add_up_to_the_step_kernels_energy(ps, home):
    """The test this recorder exists for: on every f64 home the model total of the columns (field + work + bend, + pair[1] for
    Ising, + every pair column and rest for interacting, `within` alone for cutoff) equals the sum of the chains' U as the step
    kernel carries it (pstat_microstate), within energy_ref.model_bound -- and that bound stays below 1e-9 of the ensemble's sum of
    |terms|, where a wrong or missing term is of order 1."""
    for T, k, diff, bound, scale in model_against_microstate(ps, home, seed=2300):
        print(f"{home}, T = {T}, case {k}: |model - sum U| = {diff:.3g}, bound {bound:.3g}, scale {scale:.3g}, diff / scale = {diff / scale:.3g}")
        assert bound <= 1e-9 * scale, (home, T, k, bound, scale)
        assert diff <= bound, (home, T, k, diff, bound)


@pytest.mark.parametrize("home", ["f32 sweep", "q16 sweep"])
def test_the_f32_and_q16_energies_beside_the_recorder(ps, home):
    """Their U is f32 arithmetic along a path this recorder does not restate: the difference is printed with its scale, not
    asserted beyond being finite."""
    for T, k, diff, bound, scale in model_against_microstate(ps, home, seed=2300):
        print(f"{home}, T = {T}, case {k}: |model - sum U| = {diff:.3g}, scale {scale:.3g}, diff / scale = {diff / scale:.3g}")
        assert np.isfinite(diff)


# ------------------------------------------------------------------------------------------------ exact configurations
def set_angles(e, theta, phi):
    """Overwrites the angle planes of the handle's checkpoint image ([2][n][C] behind the header and the per-case kT list, plane
    0 theta; element type by the header's precision) and restores the image, as tests/test_gpu_pdist.py does."""
    blob = bytearray(e.checkpoint())
    header_bytes, = struct.unpack_from("<i", blob, 12)
    n, C_, ncases = struct.unpack_from("<qqq", blob, 16)
    precision, = struct.unpack_from("<i", blob, 56)
    dt = {0: np.dtype(np.float32), 1: np.dtype(np.float64)}[precision]
    off = header_bytes + 8 * ncases
    plane = n * C_ * dt.itemsize
    blob[off:off + plane] = np.ascontiguousarray(np.asarray(theta, dtype=dt).T).tobytes()
    blob[off + plane:off + 2 * plane] = np.ascontiguousarray(np.asarray(phi, dtype=dt).T).tobytes()
    e.restore(bytes(blob))


@pytest.mark.parametrize("precision", [1, 0], ids=["f64", "f32"])
@pytest.mark.parametrize("n", [9, 70])
def test_straight_chain_has_closed_forms(ps, precision, n):
    """theta = 0 is exact in the f64 and in the f32 storage: with K1 E0 = 1 and b = 1, mu = z and d = s z, so
    pair[s] = -2 (n - s) / (4 pi s^3), field = -n E0 / 2, work = -Fz n, bend = (n - 1)(kappa / 2) psi0^2."""
    per = 5
    cases = [ps.default_params(n=n, num_chains=per, precision=precision, kT=1.0 + k, seed=2400 + k, b=1.0, E0=2.0, K1=0.5, K2=0.0,
                               Fz=0.3, Fx=0.7, move_set=1, cluster_prob=0.5, bend_mod=1.2, bend_angle=0.25) for k in range(2)]
    with ps.Ensemble(cases) as e:
        set_angles(e, np.zeros((2 * per, n)), np.zeros((2 * per, n)))
        s = e.chain_state(2 * per - 1)
        assert np.all(s["theta"] == 0.0) and np.all(s["phi"] == 0.0)
        g = e.open_energy(-1, 2.5)
        g.record()
        got = g.read()
    sep = np.arange(1, n)
    want = -2.0 * (n - sep) / (FOURPI * sep ** 3.0)
    for k in range(2):
        assert got.field[k] == -n * 2.0 / 2 and got.rest[k] == 0.0
        np.testing.assert_allclose(got.work[k], -0.3 * n, rtol=1e-14)
        np.testing.assert_allclose(got.bend[k], (n - 1) * 0.6 * 0.25 ** 2, rtol=1e-14)
        np.testing.assert_allclose(got.pair[k], want, rtol=1e-14)
        np.testing.assert_allclose(got.within[k], want[:2].sum(), rtol=1e-14)                  # crad2 = 6.25: s = 1, 2
        np.testing.assert_allclose(got.sumsq[k, 3:n + 2], per * want ** 2, rtol=1e-14)


@pytest.mark.parametrize("n", [9, 70])
def test_planar_chain_along_x_has_dipoles_across_the_axis(ps, n):
    """phi = 0: n = (1, 0), mu = (0, K2 E0), mu . d = 0: pair[s] = +(n - s)(K2 E0)^2 / (4 pi s^3 b^3)."""
    per, b, K2E0 = 5, 1.2, 0.4 * 1.5
    p = ps.default_planar_params(n=n, num_chains=per, E0=1.5, K1=0.9, K2=0.4, Fz=0.3, Fx=0.7, b=b, seed=2420)
    with ps.Ensemble(p, planar=True) as e:
        set_angles(e, np.zeros((per, n)), np.zeros((per, n)))
        assert np.all(e.chain_state(per - 1)["phi"] == 0.0)
        g = e.open_energy()
        g.record()
        got = g.read()
    sep = np.arange(1, n)
    np.testing.assert_allclose(got.pair[0], (n - sep) * K2E0 ** 2 / (FOURPI * (sep * b) ** 3.0), rtol=1e-14)
    np.testing.assert_allclose(got.field[0], -n * 1.5 * K2E0 / 2, rtol=1e-14)
    np.testing.assert_allclose(got.work[0], -0.7 * n * b, rtol=1e-14)
    assert got.bend[0] == 0.0 and got.rest[0] == 0.0 and got.within is None


# ------------------------------------------------------------------------------------------------ closed forms
@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "energy_closed_form.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", ["fixed_force", "polar", "planar", "bend"])
def test_closed_forms(ps, golden, name):
    """16 384 chains, 1 000 n steps of burn-in, ONE record: field, work and bend within 5 of their own across-chain standard errors
    of the closed form, each such error at most 2 % of the value (energy_ref.judge, the judge tests/test_energy_cpu.py puts to
    directly sampled chains).  Beside them, on the same ensemble: field + work + bend of the snapshot against the time average
    <U> of the 100 n steps that follow it (reset_averages, then summary().avg[14]) within 5 combined standard errors -- the two
    differ statistically only; the snapshot's error is taken as the sum of its parts' errors, which bounds it.  No pair column
    is judged: their variance is infinite (tests/golden/make_energy_closed_form.py)."""
    c = golden[name]
    planar, N = c["planar"], 16384
    make = ps.default_planar_params if planar else ps.default_params
    with ps.Ensemble(make(num_chains=N, precision=ps.F64, seed=20261021, **c["params"]), planar=planar) as e:
        print(e.launch_info().kernel.decode())
        e.advance(1000 * c["params"]["n"])
        g = e.open_energy(0)
        g.record()
        got = g.read()
        e.reset_averages()                                           # the time average of the equilibrated chain, not of its start
        e.advance(100 * c["params"]["n"])
        summary = e.summary()
    assert got.records == 1
    mean, se = got.mean[0], got.chain_stderr[0]
    for i, col in enumerate(("field", "work", "bend")):
        if col in c["expect"]:
            z, rel = er.judge(f"{name} {col}", mean[i], se[i], c["expect"][col])
            print(f"{name} {col}: mean {mean[i]:.5f}, closed form {c['expect'][col]:.5f}, |z| = {z:.2f}, stderr / value = {100 * rel:.3f} %")
    s, q = got.sum[0, :3].sum(), got.sumsq[0, :3]
    snapshot = s / N                                                 # the parts are correlated: bound their sum's error by the parts'
    snap_se = se[:3].sum()
    avg, avg_se = summary.avg[14], summary.stderr[14]
    z = abs(snapshot - avg) / np.hypot(snap_se, avg_se)
    print(f"{name}: field + work + bend = {snapshot:.5f} +- {snap_se:.5f}, <U> = {avg:.5f} +- {avg_se:.5f}, |z| = {z:.2f}")
    assert z <= 5.0 and np.all(q >= 0)


# ------------------------------------------------------------------------------------------------ composition
def test_error_bars_are_the_blocking_transform_of_the_rows(ps):
    cases = sweep_cases(ps, 3, 20, 10, seed=2500, energy_type=2)     # Ising: the model is field + work + bend + pair[1]
    with ps.Ensemble(cases) as e, ps.Ensemble(cases) as plain:
        g = e.open_energy(3, 1.5, capacity_rows=64)
        e.advance_energy(g, 64 * 25, 25)
        for _ in range(64):
            plain.advance(25)
        assert_same_chains(e, plain, range(60))                      # advance_energy leaves chains, generators and sums as advance
        eb = g.error_bars()
        ptr, nrows, stride = g.rows()
        cols = 3 + 3 + 1 + 1
        assert (nrows, stride) == (64, 3 * cols) and g.ncols == cols
        by_hand = ps.blocking_device(ptr, nrows, stride)
        for f in ("mean", "stderr", "stderr_err", "inefficiency", "level", "converged"):
            assert getattr(eb, f).shape == (3, cols) and bits(getattr(eb, f)) == bits(getattr(by_hand, f).reshape(3, cols)), f
        res = g.read()
        np.testing.assert_allclose(eb.mean, res.mean, rtol=1e-12)
        assert np.all(np.isnan(res.chain_stderr)) and eb.nbatches == 64 and np.all(eb.stderr[:, [0, 1, 3, 4, 5, 6, 7]] > 0)
        assert np.all(eb.stderr[:, 2] == 0.0)                        # no bending: 0.0 in every row
        rows = rc.device_rows(g).reshape(64, 3, cols)
        meb = g.model_error_bars()                                   # the blocking transform of the rows' combined column
        np.testing.assert_allclose(meb.mean, rows[:, :, [0, 1, 2, 3]].sum(axis=2).mean(axis=0), rtol=1e-13)
        np.testing.assert_allclose(meb.mean, res.model, rtol=1e-12)
        assert meb.stderr.shape == (3,) and np.all(meb.stderr > 0) and np.all(meb.stderr < eb.stderr[:, :4].sum(axis=1))
        with pytest.raises(ps.PstatError) as err:                    # fewer rows than min_blocks: the transform's own refusal
            g.error_bars(min_blocks=65)
        assert err.value.code == -7
        g.clear()
        assert g.read().records == 0 and g.rows()[1] == 0 and np.all(g.read().sum == 0)


def test_records_between_exchange_rounds(ps):
    cases = rc.ladder_cases(ps)
    rc.totals_between_exchange_rounds(ps, cases, energy_kind(cases, max_sep=3, cutoff=1.5))


def test_refusals_leave_the_handle_usable(ps):
    with ps.Ensemble([ps.default_params(n=6, num_chains=4, kT=kT, umbrella=1) for kT in (1.0, 2.0)]) as e:
        with pytest.raises(ps.PstatError) as err:
            e.open_energy()
        assert err.value.code == -4 and "umbrella" in str(err.value) and "whose gauge the sums do not hold" in str(err.value)
        e.advance(20)
        assert e.chain_state(0)["steps_recorded"] == 20
    cases = [ps.default_params(n=6, num_chains=4, kT=kT, Fz=0.3) for kT in (1.0, 2.0, 3.0)]
    with ps.Ensemble(cases) as e:
        for kw, code, needle in ((dict(max_sep=6), -1, "max_sep"), (dict(max_sep=-2), -1, "max_sep"), (dict(cutoff=-1.0), -1, "cutoff"),
                                 (dict(cutoff=[1.0, np.inf, 1.0]), -1, "case 1"), (dict(capacity_rows=-1), -1, "capacity_rows")):
            with pytest.raises(ps.PstatError) as err:
                e.open_energy(**kw)
            assert err.value.code == code and needle in str(err.value), (kw, str(err.value))
        e.advance(5)                                                 # the handle still advances
        assert e.chain_state(0)["steps_recorded"] == 5
        assert e.open_energy(max_sep=0).read().pair.shape == (3, 0)
    cut = [ps.default_params(n=6, num_chains=4, kT=1.0, energy_type=ps.CUTOFF, move_set=1, cutoff_radius=r) for r in (1.5, 2.5)]
    with ps.Ensemble(cut) as e:                                      # a CUTOFF handle: its own radii by default; none: no model total
        assert e.open_energy().cutoff.tolist() == [1.5, 2.5]
        g = e.open_energy(cutoff=0.0)
        g.record()
        with pytest.raises(ValueError):
            g.read().model_sum
    for planar, n in ((False, 1280), (True, 1920)):                  # beyond a workgroup's LDS; fits at the limit, a tile of one chain
        make = ps.default_planar_params if planar else ps.default_params
        with ps.Ensemble(make(n=n + 1, num_chains=1), planar=planar) as e:
            with pytest.raises(ps.PstatError) as err:
                e.open_energy()
            assert err.value.code == -4 and str(n) in str(err.value)
            e.advance(2)
            assert e.chain_state(0)["steps_recorded"] == 2
        p = make(n=n, num_chains=2, Fz=0.5, E0=1.0)
        with ps.Ensemble(p, planar=planar) as e:
            g = e.open_energy(max_sep=3, cutoff=2.0)
            e.advance(3)
            g.record()
            tw = er.per_chain(angles_of_all(e), p, 3, 2.0, planar)
            got = g.read()
            assert tw.undecided.sum() == 0
            assert np.all(np.abs(got.sum[0] - tw.values.sum(axis=0)) <= er.bounds(tw, p, n, 2, 3, 2.0)[0])


# ------------------------------------------------------------------------------------------------ the lifecycle
KIND, NSTEPS, STEPOUT = "energy", lc.NSTEPS, lc.STEPOUT
NOT_OPEN, NOUN = b"the energy object is not an open one", b"the energy object has"


def open_energy(e, capacity=8):
    return e.open_energy(cutoff=1.5, capacity_rows=capacity)


@pytest.mark.parametrize("planar", [False, True], ids=["3d", "planar"])
def test_an_object_belongs_to_its_handle(ps, planar):
    lib = ps._lib.load()
    with lc.ensemble(ps, planar) as e, lc.ensemble(ps, planar) as other:
        obj = open_energy(e)
        for name, f in lc.entry_points(lib, KIND).items():
            assert f(other._h, obj._g) == -1 and NOT_OPEN in lib.pstat_last_error(), name
        assert lc.advance_raw(lib, KIND, other._h, obj._g, NSTEPS, 0) == -1 and NOT_OPEN in lib.pstat_last_error()
        lib.pstat_energy_close(other._h, obj._g)                     # ignored: it is not the other handle's to close
        assert lc.steps_recorded(other) == [0, 0]
        e.advance_energy(obj, NSTEPS, STEPOUT)                       # the object still works
        assert obj.read().records == 3 and lc.steps_recorded(e) == [NSTEPS, NSTEPS]
        for name, f in lc.entry_points(lib, KIND).items():
            assert f(e._h, obj._g) == 0, (name, lib.pstat_last_error())


@pytest.mark.parametrize("planar", [False, True], ids=["3d", "planar"])
def test_advance_refuses_before_it_enqueues(ps, planar):
    lib = ps._lib.load()
    with lc.ensemble(ps, planar) as e:
        obj = open_energy(e, capacity=3)
        raw = lambda nsteps, stepout: lc.advance_raw(lib, KIND, e._h, obj._g, nsteps, stepout)
        assert raw(NSTEPS, 0) == -1 and b"stepout" in lib.pstat_last_error()
        assert raw(-1, STEPOUT) == -1 and b"nsteps" in lib.pstat_last_error()
        assert raw(-1, 0) == -1 and b"nsteps" in lib.pstat_last_error()
        assert lc.steps_recorded(e) == [0, 0] and obj.read().records == 0
        assert raw(NSTEPS, STEPOUT) == 0, lib.pstat_last_error()
        assert lc.steps_recorded(e) == [NSTEPS, NSTEPS] and obj.read().records == 3
        assert raw(STEPOUT, STEPOUT) == -7                           # the row buffer is full: refused with nothing enqueued
        assert NOUN + b" 0 of 3 rows free, this call would record 1" in lib.pstat_last_error()
        assert raw(-1, STEPOUT) == -1                                # an argument error comes before the full buffer
        assert lib.pstat_energy_record(e._h, obj._g) == -7
        assert lc.steps_recorded(e) == [NSTEPS, NSTEPS] and obj.read().records == 3
        assert raw(STEPOUT - 1, STEPOUT) == 0                        # a call that records nothing always fits
        assert lc.steps_recorded(e) == [NSTEPS + STEPOUT - 1] * 2 and obj.read().records == 3
        obj.clear()                                                  # no records, and every row free again
        assert obj.read().records == 0 and obj.rows()[1] == 0
        assert raw(NSTEPS, STEPOUT) == 0, lib.pstat_last_error()
        records = C.c_int64(-1)                                      # every output may be NULL
        assert lib.pstat_energy_read(e._h, obj._g, None, None, C.byref(records)) == 0 and records.value == 3


@pytest.mark.parametrize("planar", [False, True], ids=["3d", "planar"])
def test_totals_without_rows_have_no_limit(ps, planar):
    with lc.ensemble(ps, planar) as e:
        obj = open_energy(e, capacity=0)                             # no rows kept: no limit, and no rows to hand out
        e.advance_energy(obj, 50, 1)
        assert obj.read().records == 50 and obj.rows() == (0, 0, e.ncases * obj.ncols)
        with pytest.raises(ps.PstatError):
            obj.error_bars()


@pytest.mark.parametrize("planar", [False, True], ids=["3d", "planar"])
def test_a_closed_object_is_refused(ps, planar):
    lib = ps._lib.load()
    with lc.ensemble(ps, planar) as e:
        keep, obj = open_energy(e), open_energy(e)
        e.advance_energy(obj, NSTEPS, STEPOUT)
        raw = obj._g
        obj.close()                                                  # with its last record still in flight
        assert obj._g is None
        for name, f in lc.entry_points(lib, KIND).items():
            assert f(e._h, raw) == -1 and NOT_OPEN in lib.pstat_last_error(), name
        lib.pstat_energy_close(e._h, raw)                            # a second close is harmless
        obj.close()
        e.advance_energy(keep, NSTEPS, STEPOUT)                      # the handle and its other objects go on
        assert keep.read().records == 3 and lc.steps_recorded(e) == [2 * NSTEPS, 2 * NSTEPS]
        e.restore(e.checkpoint())                                    # no object is part of a checkpoint
        assert keep.read().records == 3 and lc.steps_recorded(e) == [2 * NSTEPS, 2 * NSTEPS]


@pytest.mark.parametrize("planar", [False, True], ids=["3d", "planar"])
def test_destroy_with_an_energy_object_open(ps, planar):
    e = lc.ensemble(ps, planar)
    objs = [open_energy(e), lc.open_kind(ps, e, "pdist")]
    e.advance_energy(objs[0], NSTEPS, STEPOUT)                       # no synchronise: the last record is in flight
    e.close()
    for obj in objs:
        obj.close()                                                  # the ensemble has closed them: nothing left to do
    with lc.ensemble(ps, planar) as e:                               # the next handle of the process works
        obj = open_energy(e)
        e.advance_energy(obj, NSTEPS, STEPOUT)
        assert lc.steps_recorded(e) == [NSTEPS] * 2 and obj.read().records == 3


# ------------------------------------------------------------------------------------------------ the tool
SPEC = "5,cut=1.5"


def test_sweep_writes_energy_files(tmp_path):
    with_energy = rc.sweep_tool(tmp_path, "s", "--energy", SPEC)
    plain = rc.sweep_tool(tmp_path, "p")
    outs, _ = rc.assert_out_files_unchanged(with_energy, plain, ".energy")
    assert len(outs) == 4
    # the same sweep through the Python API: the hosts' run_cases with a Recording, every case of the ensemble at once
    from polymer_stats_amd import sweep as sw
    cases = sw.product_cases([(k, sw.axis_values(v)) for k, v in AXES])
    plist = sw.plan("mcmc_eap_chain", FIXED, cases, str(tmp_path / "api"), num_chains=64, seed=11)
    info = {}
    sw.MAINS["mcmc_eap_chain"].run_cases(plist, write_csv=False, info=info, record=sw.Recording("energy", sw.parse_energy(SPEC)))
    res, eb, meb = info["energy"]
    assert res.records == 32 and res.max_sep == 5 and res.has_within and res.cutoff.tolist() == [1.5] * 4
    work = []
    for k, p in enumerate(plist):
        lines = (with_energy / (p["_name"] + ".energy")).read_text().strip().split("\n")
        assert lines[0] == "name,x,value,stderr" and len(lines) == 1 + 3 + 5 + 1 + 1 + 1
        rows = [line.split(",") for line in lines[1:]]
        assert [r[0] for r in rows] == ["field", "work", "bend"] + ["pair"] * 5 + ["rest", "within", "model"]
        assert [r[1] for r in rows] == ["", "", "", "1", "2", "3", "4", "5", "", "1.5", ""]
        value, stderr = np.array([float(r[2]) for r in rows]), np.array([float(r[3]) for r in rows])
        assert bits(value[:10]) == bits(res.mean[k]) and bits(stderr[:10]) == bits(eb.stderr[k]), p["_name"]
        assert value[10] == res.model[k] and stderr[10] == meb.stderr[k]
        np.testing.assert_allclose(value[10], value[:3].sum(), rtol=1e-14)   # non-interacting: field + work + bend
        assert np.all(np.isfinite(value)) and value[2] == 0.0 and stderr[2] == 0.0
        work.append(value[1])
    assert work[0] == 0.0 and 0 > work[1] > work[2] > work[3]        # -Fz <R_z>: pulled harder, the work term falls
