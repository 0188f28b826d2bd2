"""GPU tests of the pair-distance recorder (pstat_pdist_*, pstat_pdist.hip) against the numpy twin of the
contract (tests/pdist_ref.py): totals and rows equal to the twin's on the angles of an identical second ensemble, to the bound
derived in the twin's docstring, the histogram's counts as integers; every edge of the kernel's mapping; the homes; a straight
chain that sits on the bin edges; closed forms; the shape recorder's S(q) beside the Debye one; error bars, tempering, refusals;
tools/run_sweep.py --pdist end to end.  The protocol of the comparison, the case tables and the tool call are those of
tests/recorder_cases.py, given pdist_kind below; the lifecycle rules are asserted in tests/test_gpu_recorder_lifecycle.py."""
import json
import os
import struct

import numpy as np
import pytest

import pdist_ref as pr
import recorder_cases as rc
from recorder_cases import AXES, BASE, FIXED, angles_of_all, assert_same_chains, bits, ps, sweep_cases  # noqa: F401 (ps is the fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def magnitudes(nq, qmax, seed=1):
    """[nq] in (0, qmax]; the last one is 0 when there are at least two (S(0) = n is asserted bit for bit)."""
    q = np.random.default_rng(seed).uniform(0.05, 1.0, nq) * qmax
    if nq >= 2:
        q[-1] = 0.0
    return q


def pdist_kind(cases, max_sep=-1, min_sep=1, nbins=24, rmax=None, q=None, planar=False):
    """The descriptor of rc.run_totals_twin.  `rmax`: None (1.5 sqrt(n) b of case 0), a number, or one per case.  The twin also
    tells how many pairs it could not decide the bin of, and the smallest distance in the data, which the bounds depend on.  A row
    is a mean of `per` values: the bound of a total of `per`, over `per`."""
    n, per, ncases = int(cases[0].n), int(cases[0].num_chains), len(cases)
    q = np.zeros(0) if q is None else np.asarray(q, dtype=np.float64)
    if rmax is None:
        rmax = 1.5 * np.sqrt(n) * cases[0].b
    rmaxes = np.broadcast_to(np.asarray(rmax, dtype=np.float64), (ncases,))
    sep = n - 1 if max_sep < 0 else max_sep
    _, _, hist, sq = pr.columns(sep, nbins, len(q))
    pairs = pr.pairs_counted(n, min_sep)

    def bounds(k, M, twins):
        return pr.bounds(n, cases[k].b, M, sep, nbins, q, min(t[2] for t in twins))

    def exact(got, rows, values, per):
        M = per * len(values)
        for k in range(ncases):
            assert sum(v[k][1].sum() for v in values) == 0, "the input has a pair on a bin edge: the condition of pdist_ref fails"
            if nbins:                                                # integers: equal, and every counted pair is in one column
                want_s = sum(v[k][0].sum(axis=0) for v in values)
                want_q = sum((v[k][0] * v[k][0]).sum(axis=0) for v in values)
                assert bits(got.sum[k, hist]) == bits(want_s[hist]) and bits(got.sumsq[k, hist]) == bits(want_q[hist]), k
                assert got.sum[k, hist].sum() == M * pairs and got.counts[k].sum() + got.above[k] == M * pairs
            for j in np.flatnonzero(q == 0.0):                       # S(0) = n for every chain: n M and n^2 M, exactly
                assert got.sum[k, sq.start + j] == float(n * M) and got.sumsq[k, sq.start + j] == float(n * n * M), (k, j)

    return rc.Totals(
        name="pdist", ncols=pr.ncols(sep, nbins, len(q)),
        open=lambda e, capacity: e.open_pdist(max_sep, min_sep, (nbins, rmax) if nbins else None, q, capacity_rows=capacity),
        twin=lambda ang, k: pr.per_chain(ang, cases[k].b, max_sep, min_sep, nbins, rmaxes[k], q, planar),
        bounds=bounds, row_bound=lambda k, per, M, twins: bounds(k, per, twins)[0] / per, exact=exact,
        line=f"n = {n}, {ncases} x {per} chains, max_sep {max_sep}, min_sep {min_sep}, nbins {nbins}, nq {len(q)}: largest "
             f"|device - twin| / bound = {{worst:.4f}}")


def run_exact(ps, cases, planar=False, records=3, **options):
    return rc.run_totals_twin(ps, cases, pdist_kind(cases, planar=planar, **options), planar=planar, records=records)


# ------------------------------------------------------------------------------------------------ every edge of the mapping
@pytest.mark.parametrize("ncases,per", rc.TILE_SHAPES)
def test_totals_and_rows_equal_the_twin(ps, ncases, per):
    big = per == 1100                                                # (fewer bins and q: 2200 chains through the twin)
    run_exact(ps, sweep_cases(ps, ncases, per, 12, seed=1800), nbins=8 if big else 24, q=magnitudes(2 if big else 5, 6.0), records=2 if big else 3)


# two monomers (one pair, rows for one wavefront only); three; 63, 64, 65: the first row's pairs end one short of the 64 lanes,
# fill all but one, fill them exactly; 130: rows of three lane strides, scan segments of 3
@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 130])
def test_chain_lengths(ps, n):
    got = run_exact(ps, sweep_cases(ps, 3, 5, n, seed=1820), q=magnitudes(5, 6.0, seed=n), records=2)
    if n == 2:
        np.testing.assert_allclose(got.msd[:, 0], got.sumsq[:, 1] / (2 * 5), rtol=1e-14)    # one pair: R2(1) = rmin^2


@pytest.mark.parametrize("min_sep", [1, 2, 11])
@pytest.mark.parametrize("max_sep", [0, 1, 11])
def test_separations_at_n_12(ps, max_sep, min_sep):
    got = run_exact(ps, sweep_cases(ps, 3, 5, 12, seed=1830), max_sep=max_sep, min_sep=min_sep, q=magnitudes(3, 6.0), records=2)
    assert got.msd.shape == (3, max_sep) and got.pairs == (12 - min_sep) * (13 - min_sep) // 2


# nbins = 0 and nq = 0 skip their work; one bin; 64 and 512 bins (one, two and three counters per thread of the fold); nq = 1, 63,
# 64: one block of q with seven idle slots, eight blocks with one idle slot, eight full blocks
@pytest.mark.parametrize("nbins,nq", [(0, 0), (1, 1), (64, 63), (512, 64), (0, 64), (512, 0)])
def test_bin_and_magnitude_counts_at_n_65(ps, nbins, nq):
    run_exact(ps, sweep_cases(ps, 3, 5, 65, seed=1840), nbins=nbins, q=magnitudes(nq, 1.0, seed=nq) if nq else None, records=2)


def test_cases_that_differ_in_b_with_their_own_rmax(ps):
    bs = (0.5, 1.0, 2.5)
    cases = [ps.default_params(n=12, num_chains=20, precision=ps.F64, kT=1.0, seed=1870 + k, b=b, **BASE) for k, b in enumerate(bs)]
    got = run_exact(ps, cases, rmax=[4.0 * b for b in bs], q=magnitudes(5, 6.0 / 2.5))
    assert got.rmin[0] < got.rmin[1] < got.rmin[2] and got.msd[2, 4] > 20 * got.msd[0, 4]     # lengths scale with b
    assert np.all(got.rmax == [2.0, 4.0, 10.0])
    share = got.counts / (got.counts.sum(axis=1, keepdims=True) + got.above[:, None])
    assert np.all(np.abs(share[0] - share[2]) < 0.05)               # the same distribution in units of b
    np.testing.assert_allclose(got.edges(2), 10.0 * np.arange(25) / 24, rtol=1e-15)


# ------------------------------------------------------------------------------------------------ the homes
@pytest.mark.parametrize("home", list(rc.HOMES))
def test_every_home(ps, home):
    cases, planar = rc.home_cases(ps, home, seed=1900)
    got = run_exact(ps, cases, q=magnitudes(5, 6.0, seed=3), planar=planar, records=2)
    assert np.all(got.rmin > 0) and np.all(got.sq[:, :4] > 0) and np.all(got.msd[:, 0] > 0)


def test_packed_cases(ps, monkeypatch):
    monkeypatch.setenv("PSTAT_PACK", "1")
    cases = [ps.default_params(n=20, E0=0.5 + 0.1 * i, Fz=0.1 * i, kT=1.0 + 0.05 * i, num_chains=16, seed=1940 + i, chain_id0=100 * i,
                               precision=ps.F64) for i in range(9)]
    with ps.Ensemble(cases) as e:
        assert e.launch_info().packed_cases == 1, e.launch_info().kernel.decode()
    run_exact(ps, cases, q=magnitudes(3, 6.0), records=2)


# ------------------------------------------------------------------------------------------------ the straight chain, on the edges
def set_angles(e, theta, phi):
    """Overwrites the angle planes of the handle's checkpoint image ([2][n][C] behind the header and the per-case kT list, plane
    0 theta; element type by the header's precision) and restores the image, as tests/pair_ref.py does for the pair census."""
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
@pytest.mark.parametrize("n,min_sep", [(9, 2), (70, 1)])
def test_straight_chain_sits_on_the_bin_edges(ps, precision, n, min_sep):
    """theta = 0 is exact in the f64 and in the f32 storage (radians and turns; the q16 lattice has no 0): x_i = i + 1/2 with b = 1,
    r2 and r are integers, and with rmax = 4 and 16 bins the pair at separation s lands in bin 4 s exactly, s >= 4 in "above"."""
    nbins, rmax, per = 16, 4.0, 5
    cases = [ps.default_params(n=n, num_chains=per, precision=precision, kT=1.0 + k, seed=1950 + k, b=1.0) for k in range(2)]
    with ps.Ensemble(cases) as e:
        set_angles(e, np.zeros((2 * per, n)), np.zeros((2 * per, n)))
        for c in (0, 2 * per - 1):
            s = e.chain_state(c)
            assert np.all(s["theta"] == 0.0) and np.all(s["phi"] == 0.0)                 # load_angle returns 0 exactly
        g = e.open_pdist(-1, min_sep, (nbins, rmax), [0.0, 0.25])
        g.record()
        got = g.read()
    want = np.zeros(nbins + 1)
    for s in range(min_sep, n):
        want[4 * s if s < 4 else nbins] += n - s
    for k in range(2):
        np.testing.assert_array_equal(got.sum[k, n:n + nbins + 1], per * want)
        np.testing.assert_array_equal(got.sumsq[k, n:n + nbins + 1], per * want * want)
        np.testing.assert_array_equal(got.msd[k], np.arange(1, n) ** 2.0)                # R2(s) = s^2
        assert got.rmin[k] == float(min_sep) and got.sumsq[k, n - 1] == per * float(min_sep) ** 2
        assert got.sq[k, 0] == float(n)
        debye = 1.0 + 2.0 * sum((n - s) * np.sin(0.25 * s) / (0.25 * s) for s in range(1, n)) / n
        np.testing.assert_allclose(got.sq[k, 1], debye, rtol=1e-13)
    assert want[nbins] == sum(n - s for s in range(max(4, min_sep), n)) and got.above[0] == per * want[nbins]


# ------------------------------------------------------------------------------------------------ closed forms
@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "pdist_closed_form.json")) as f:
        return json.load(f)


def equilibrated(ps, c, planar, N=16384):
    make = ps.default_planar_params if planar else ps.default_params
    e = ps.Ensemble(make(num_chains=N, precision=ps.F64, seed=20261020, **c["params"]), planar=planar)
    e.advance(1000 * c["params"]["n"])
    return e


@pytest.mark.parametrize("name", ["fjc", "fixed_force", "planar", "dimer", "planar_dimer"])
def test_closed_forms(ps, golden, name):
    """16 384 chains, 1 000 n steps of burn-in, ONE record: every column the fixture has within 5 of its own across-chain standard
    errors of the closed form; on msd, rmin and sq each such error <= 2 % of the value; histogram columns on |z| <= 5 alone
    (pdist_ref.judge_closed_form, the conditions tests/test_pdist_cpu.py puts to directly sampled chains); the q = 0 column
    exactly n.  Device figures (MI355X; fjc / fixed_force / planar / dimer / planar_dimer): largest |z| 0.79 / 0.74 / 0.63 / 2.27 /
    1.45, largest standard error 0.61 / 0.37 / 0.74 / 0.45 / 0.55 % of the value."""
    c = golden[name]
    o = c["options"]
    planar = name.startswith("planar")
    with equilibrated(ps, c, planar) as e:
        print(e.launch_info().kernel.decode())
        g = e.open_pdist(o["max_sep"], o["min_sep"], (o["nbins"], o["rmax"]) if o["nbins"] else None, o["q"])
        g.record()
        got = g.read()
    assert got.records == 1
    mean, se = got.mean[0], got.chain_stderr[0]
    print(f"{name}\n  mean  ", np.round(mean, 5), "\n  stderr", np.round(se, 5))
    z, r = pr.judge_closed_form(name, c, mean, se)
    print(f"{name}: largest |z| = {z:.2f}, largest stderr / value = {100 * r:.2f} %")
    if o["nbins"]:
        assert abs((got.density(0) * (o["rmax"] / o["nbins"])).sum() - (1.0 - got.above[0] / (16384 * got.pairs))) < 1e-12


def test_debye_beside_the_directional_form_factor(ps, golden):
    """The same ensembles through both recorders.  Free chain: isotropic, so the shape recorder's S(q z) and the Debye S(|q|) agree
    within 5 combined standard errors.  Under a force along z the chain is drawn out along z and scatters less along the pull
    than on the orientational average."""
    mags = [0.5, 1.5, 3.0, 6.0]
    qz = [[0.0, 0.0, m] for m in mags]
    for name in ("fjc", "fixed_force"):
        with equilibrated(ps, golden[name], False) as e:
            gp, gs = e.open_pdist(0, 1, None, mags), e.open_shape(qz)
            gp.record()
            gs.record()
            p, s = gp.read(), gs.read()
        deb, dse = p.sq[0], p.chain_stderr[0, 1:]
        along, ase = s.sq[0], s.chain_stderr[0, 8:]
        z = (deb - along) / np.sqrt(dse ** 2 + ase ** 2)
        print(name, "Debye", np.round(deb, 4), "along z", np.round(along, 4), "z", np.round(z, 2))
        if name == "fjc":
            assert np.all(np.abs(z) <= 5.0), z
        else:
            assert np.all(along < deb) and np.all(z[:3] > 5.0), (along, deb, z)


# ------------------------------------------------------------------------------------------------ composition
def test_error_bars_are_the_blocking_transform_of_the_rows(ps):
    cases = sweep_cases(ps, 3, 20, 10, seed=1960)
    with ps.Ensemble(cases) as e, ps.Ensemble(cases) as plain:
        g = e.open_pdist(3, 2, (6, 4.0), [0.0, 1.0], capacity_rows=64)
        e.advance_pdist(g, 64 * 25, 25)
        for _ in range(64):
            plain.advance(25)
        assert_same_chains(e, plain, range(60))                      # advance_pdist leaves chains, generators and sums as advance
        eb = g.error_bars()
        ptr, nrows, stride = g.rows()
        cols = 3 + 1 + 7 + 2
        assert (nrows, stride) == (64, 3 * cols) and g.ncols == cols
        by_hand = ps.blocking_device(ptr, nrows, stride)
        for f in ("mean", "stderr", "stderr_err", "inefficiency", "level", "converged"):
            assert getattr(eb, f).shape == (3, cols) and bits(getattr(eb, f)) == bits(getattr(by_hand, f).reshape(3, cols)), f
        res = g.read()
        np.testing.assert_allclose(eb.mean, res.mean, rtol=1e-13)
        assert np.all(np.isnan(res.chain_stderr)) and eb.nbatches == 64 and np.all(eb.stderr[:, :4] > 0) and np.all(eb.stderr[:, 12] > 0)
        assert np.all(eb.stderr[:, 11] == 0.0)                        # S(0) = n in every row
        assert res.msd.shape == (3, 3) and res.counts.shape == (3, 6) and res.sq.shape == (3, 2) and res.rmin.shape == (3,)
        np.testing.assert_array_equal(res.counts.sum(axis=1) + res.above, 64 * 20 * res.pairs)
        assert abs((res.density(1) * (4.0 / 6)).sum() - (1 - res.above[1] / (64 * 20 * res.pairs))) < 1e-12
        with pytest.raises(ps.PstatError) as err:                    # fewer rows than min_blocks: the transform's own refusal
            g.error_bars(min_blocks=65)
        assert err.value.code == -7
        g.clear()
        assert g.read().records == 0 and g.rows()[1] == 0 and np.all(g.read().sum == 0)


def test_records_between_exchange_rounds(ps):
    cases = rc.ladder_cases(ps)
    rc.totals_between_exchange_rounds(ps, cases, pdist_kind(cases, nbins=12, rmax=5.0, q=magnitudes(3, 4.0, seed=9)))


def test_refusals_leave_the_handle_usable(ps):
    with ps.Ensemble([ps.default_params(n=6, num_chains=4, kT=kT, umbrella=1) for kT in (1.0, 2.0)]) as e:
        with pytest.raises(ps.PstatError) as err:
            e.open_pdist()
        assert err.value.code == -4 and "umbrella" in str(err.value) and "whose gauge the sums do not hold" in str(err.value)
        e.advance(20)
        assert e.chain_state(0)["steps_recorded"] == 20
    cases = [ps.default_params(n=6, num_chains=4, kT=kT, Fz=0.3) for kT in (1.0, 2.0, 3.0)]
    with ps.Ensemble(cases) as e:
        for kw, code, needle in ((dict(max_sep=6), -1, "max_sep"), (dict(min_sep=0), -1, "min_sep"), (dict(min_sep=6), -1, "min_sep"),
                                 (dict(bins=(-1, 1.0)), -1, "nbins"), (dict(bins=(4, 0.0)), -1, "rmax"),
                                 (dict(bins=(4, [1.0, np.inf, 1.0])), -1, "rmax_per_case"), (dict(q=[-1.0]), -1, "q[0]"),
                                 (dict(q=[2.0e4]), -1, "q[0]"), (dict(capacity_rows=-1), -1, "capacity_rows"),
                                 (dict(q=[0.1] * 65), -4, "PSTAT_PDIST_MAX_Q"), (dict(bins=(513, 1.0)), -4, "PSTAT_PDIST_MAX_BINS")):
            with pytest.raises(ps.PstatError) as err:
                e.open_pdist(**kw)
            assert err.value.code == code and needle in str(err.value), (kw, str(err.value))
        e.advance(5)                                                 # the handle still advances
        assert e.chain_state(0)["steps_recorded"] == 5
        assert e.open_pdist(max_sep=0).read().sq.shape == (3, 0)     # rmin alone
    with ps.Ensemble(ps.default_params(n=2475, num_chains=1)) as e:  # beyond a workgroup's LDS with 512 bins; fits with none
        with pytest.raises(ps.PstatError) as err:
            e.open_pdist(bins=(512, 50.0))
        assert err.value.code == -4 and "2474" in str(err.value)
        e.advance(2)
        assert e.chain_state(0)["steps_recorded"] == 2
    p = ps.default_planar_params(n=2560, num_chains=2, Fz=0.5)
    with ps.Ensemble(p, planar=True) as e:                           # planar n = 2560 fits: tiles of one chain, scan segments of 40
        g = e.open_pdist(max_sep=3, bins=(16, 400.0), q=[1.0e-3])
        e.advance(50)
        g.record()
        v, und, rfloor = pr.per_chain(angles_of_all(e), p.b, 3, 1, 16, 400.0, [1.0e-3], planar=True)
        got = g.read()
        smooth = [0, 1, 2, 3, 21]
        assert np.all(np.abs(got.sum[0] - v.sum(axis=0))[smooth] <= pr.bounds(2560, p.b, 2, 3, 16, [1.0e-3], rfloor)[0][smooth])
        lo = v.sum(axis=0)[4:21]                                     # 6.5e6 pairs: one may sit within the twin's window of an edge
        assert np.all(lo <= got.sum[0, 4:21]) and np.all(got.sum[0, 4:21] <= lo + und.sum(axis=0))
        assert got.sum[0, 4:21].sum() == 2 * 2560 * 2559 // 2


# ------------------------------------------------------------------------------------------------ the tool
SPEC = "6:12,sep=5,min=2,q=6:4"


def test_sweep_writes_pdist_files(tmp_path):
    with_pdist = rc.sweep_tool(tmp_path, "s", "--pdist", SPEC)
    plain = rc.sweep_tool(tmp_path, "p")
    outs, _ = rc.assert_out_files_unchanged(with_pdist, plain, ".pdist")
    assert len(outs) == 4
    # the same sweep through the Python API: the hosts' run_cases with a Recording, every case of the ensemble at once
    from polymer_stats_amd import sweep as sw
    cases = sw.product_cases([(k, sw.axis_values(v)) for k, v in AXES])
    plist = sw.plan("mcmc_eap_chain", FIXED, cases, str(tmp_path / "api"), num_chains=64, seed=11)
    info = {}
    sw.MAINS["mcmc_eap_chain"].run_cases(plist, write_csv=False, info=info, record=sw.Recording("pdist", sw.parse_pdist(SPEC)))
    res, eb = info["pdist"]
    assert res.records == 32 and res.q.tolist() == [1.5, 3.0, 4.5, 6.0] and (res.max_sep, res.min_sep, res.nbins) == (5, 2, 12)
    msd5 = []
    for k, p in enumerate(plist):
        lines = (with_pdist / (p["_name"] + ".pdist")).read_text().strip().split("\n")
        assert lines[0] == "name,x,value,stderr" and len(lines) == 1 + 5 + 1 + 12 + 1 + 4
        rows = [line.split(",") for line in lines[1:]]
        assert [r[0] for r in rows] == ["msd"] * 5 + ["rmin"] + ["hist"] * 12 + ["above"] + ["sq"] * 4
        assert [r[1] for r in rows[:6]] == ["1", "2", "3", "4", "5", ""]
        np.testing.assert_array_equal([float(r[1]) for r in rows[6:18]], res.centers(k))
        np.testing.assert_array_equal([float(r[1]) for r in rows[19:]], res.q)
        value, stderr = np.array([float(r[2]) for r in rows]), np.array([float(r[3]) for r in rows])
        smooth = [0, 1, 2, 3, 4, 5, 19, 20, 21, 22]
        assert bits(value[smooth]) == bits(res.mean[k][smooth]) and bits(stderr[smooth]) == bits(eb.stderr[k][smooth]), p["_name"]
        assert bits(value[6:18]) == bits(res.density(k))
        assert abs((value[6:18] * 0.5).sum() + value[18] - 1.0) < 1e-12      # density and "above" make up every counted pair
        assert np.all(np.isfinite(value)) and np.all(stderr[smooth] > 0)
        msd5.append(value[4])
    assert msd5[0] < msd5[1] < msd5[2] < msd5[3]                     # pulled taut, the chain's internal distances grow
