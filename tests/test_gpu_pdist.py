"""GPU tests of the pair-distance recorder (pstat_pdist_*, pstat_pdist.hip) against the numpy twin of the
contract (tests/pdist_ref.py): totals and rows equal to the twin's on the angles of an identical second ensemble, to the bound
derived in the twin's docstring, the histogram's counts as integers; every edge of the kernel's mapping; the homes; a straight
chain that sits on the bin edges; closed forms; the shape recorder's S(q) beside the Debye one; error bars, tempering, refusals,
the lifecycle rules of DESIGN.md 3.17; tools/run_sweep.py --pdist end to end."""
import ctypes as C
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import pdist_ref as pr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    """The HIP runtime libpstat has loaded into this process (the rows of pstat_pdist_rows are device memory)."""
    with open("/proc/self/maps") as f:
        path = next(line.split()[-1] for line in f if "libamdhip64" in line)
    hip = C.CDLL(path)
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip


def rows_of(g):
    ptr, nrows, stride = g.rows()
    rows = np.zeros((nrows, stride))
    if nrows:
        assert ptr and hip_runtime().hipMemcpy(rows.ctypes.data, ptr, rows.nbytes, 2) == 0      # 2: device to host
    return rows


def assert_same_chains(a, b, chains):
    for c in chains:
        ga, gb = a.chain_state(c), b.chain_state(c)
        for k in ga:
            assert bits(ga[k]) == bits(gb[k]) if isinstance(ga[k], np.ndarray) else ga[k] == gb[k], (c, k)
        assert bits(a.microstate(c)) == bits(b.microstate(c)), c


def magnitudes(nq, qmax, seed=1):
    """[nq] in (0, qmax]; the last one is 0 when there are at least two (S(0) = n is asserted bit for bit)."""
    q = np.random.default_rng(seed).uniform(0.05, 1.0, nq) * qmax
    if nq >= 2:
        q[-1] = 0.0
    return q


def compare(n, per, cases, o, rmax, q, planar, values, got, rows):
    """`values`: [record][case] -> (per-chain columns, undecided, rfloor) of the twin; `got`: the PdistResult; `rows`: [records,
    ncases, ncols] or None.  Returns the largest |device - twin| / bound."""
    records, ncases = len(values), len(cases)
    max_sep = n - 1 if o["max_sep"] < 0 else o["max_sep"]
    nbins, nq = o["nbins"], len(q)
    msd, rmin, hist, sq = pr.columns(max_sep, nbins, nq)
    smooth = np.r_[np.arange(msd.start, rmin.stop), np.arange(sq.start, sq.stop)].astype(int)
    worst, M = 0.0, per * records
    pairs = pr.pairs_counted(n, o["min_sep"])
    for k in range(ncases):
        assert sum(v[k][1].sum() for v in values) == 0, "the input has a pair on a bin edge: the condition of pdist_ref fails"
        rfloor = min(v[k][2] for v in values)
        want_s = sum(v[k][0].sum(axis=0) for v in values)
        want_q = sum((v[k][0] * v[k][0]).sum(axis=0) for v in values)
        b1, b2 = pr.bounds(n, cases[k].b, M, max_sep, nbins, q, rfloor)
        r1 = pr.bounds(n, cases[k].b, per, max_sep, nbins, q, rfloor)[0] / per
        e1, e2 = np.abs(got.sum[k] - want_s), np.abs(got.sumsq[k] - want_q)
        worst = max(worst, float((e1[smooth] / b1[smooth]).max()), float((e2[smooth] / b2[smooth]).max()))
        assert np.all(e1 <= b1), (k, e1, b1, int((e1 - b1).argmax()))
        assert np.all(e2 <= b2), (k, e2, b2, int((e2 - b2).argmax()))
        if nbins:                                                    # integers: equal, and every counted pair is in one column
            assert bits(got.sum[k, hist]) == bits(want_s[hist]) and bits(got.sumsq[k, hist]) == bits(want_q[hist]), k
            assert got.sum[k, hist].sum() == M * pairs and got.counts[k].sum() + got.above[k] == M * pairs
        for j in np.flatnonzero(np.asarray(q) == 0.0):               # S(0) = n for every chain: n M and n^2 M, exactly
            assert got.sum[k, sq.start + j] == float(n * M) and got.sumsq[k, sq.start + j] == float(n * n * M), (k, j)
        for r in range(records if rows is not None else 0):
            want_r = values[r][k][0].sum(axis=0) / per
            er = np.abs(rows[r, k] - want_r)
            worst = max(worst, float((er[smooth] / r1[smooth]).max()))
            assert np.all(er <= r1), (k, r, er, r1)
    return worst


def run_exact(ps, cases, max_sep=-1, min_sep=1, nbins=24, rmax=None, q=None, planar=False, stepout=40, records=3):
    """A records with advance_pdist (rows kept), B advances `stepout` at a time and reads every chain's angles: the twin on B's
    angles gives A's sum, sumsq and rows within the derived bound (pdist_ref's docstring) and the histogram's integers exactly; a
    second A gives the same bits; A's chains end as B's.  `rmax`: None (1.5 sqrt(n) b of case 0), a number, or one per case."""
    n, per, ncases = int(cases[0].n), int(cases[0].num_chains), len(cases)
    q = np.zeros(0) if q is None else np.asarray(q, dtype=np.float64)
    if rmax is None:
        rmax = 1.5 * np.sqrt(n) * cases[0].b
    rmaxes = np.broadcast_to(np.asarray(rmax, dtype=np.float64), (ncases,))
    bins = (nbins, rmax) if nbins else None
    o = dict(max_sep=max_sep, min_sep=min_sep, nbins=nbins)
    with ps.Ensemble(cases, planar=planar) as A, ps.Ensemble(cases, planar=planar) as B, ps.Ensemble(cases, planar=planar) as A2:
        g = A.open_pdist(max_sep, min_sep, bins, q, capacity_rows=records)
        A.advance_pdist(g, records * stepout + 7, stepout)           # the remainder is advanced and not recorded
        g2 = A2.open_pdist(max_sep, min_sep, bins, q, capacity_rows=records)
        A2.advance_pdist(g2, records * stepout + 7, stepout)
        values = []
        for _ in range(records):
            B.advance(stepout)
            ang = angles_of_all(B).reshape(ncases, per, 2 * n)
            values.append([pr.per_chain(ang[k], cases[k].b, max_sep, min_sep, nbins, rmaxes[k], q, planar) for k in range(ncases)])
        B.advance(7)
        got, again = g.read(), g2.read()
        cols = pr.ncols(n - 1 if max_sep < 0 else max_sep, nbins, len(q))
        assert got.records == records and got.sum.shape == (ncases, cols) == (ncases, g.ncols)
        assert bits(got.sum) == bits(again.sum) and bits(got.sumsq) == bits(again.sumsq), "two identical runs differ"
        rows, rows2 = rows_of(g), rows_of(g2)
        assert rows.shape == (records, ncases * cols) and bits(rows) == bits(rows2), "two identical runs differ in their rows"
        worst = compare(n, per, cases, o, rmaxes, q, planar, values, got, rows.reshape(records, ncases, cols))
        print(f"n = {n}, {ncases} x {per} chains, max_sep {max_sep}, min_sep {min_sep}, nbins {nbins}, nq {len(q)}: largest "
              f"|device - twin| / bound = {worst:.4f}")
        C_ = ncases * per
        edges = {c for k in range(ncases) for j in (0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, per - 1) if j < per for c in [k * per + j]}
        assert_same_chains(A, B, range(C_) if C_ <= 700 else sorted(edges))
        g.close()
        return got, worst


BASE = dict(E0=1.0, K1=0.5, K2=0.2, Fz=0.5, steps_per_adjust=150)
CLUSTER = dict(move_set=1, cluster_prob=0.5, bend_mod=0.3, bend_angle=0.2)


def sweep_cases(ps, ncases, per, n, seed=1800, **kw):
    return [ps.default_params(n=n, num_chains=per, precision=ps.F64, kT=0.7 + 0.2 * k, seed=seed + k, **{**BASE, **kw}) for k in range(ncases)]


# ------------------------------------------------------------------------------------------------ every edge of the mapping
# chains per case: 1, 5 (one tile, not full), 64 (four full tiles of 16), 65 (a last tile of one chain), 1100 (69 tiles: more
# than the 64 lanes of the fold); 9 cases: the fold's last workgroup is not full
@pytest.mark.parametrize("ncases,per", [(1, 1), (3, 5), (9, 64), (9, 65), (2, 1100)])
def test_totals_and_rows_equal_the_twin(ps, ncases, per):
    big = per == 1100                                                # (fewer bins and q: 2200 chains through the twin)
    run_exact(ps, sweep_cases(ps, ncases, per, 12), nbins=8 if big else 24, q=magnitudes(2 if big else 5, 6.0), records=2 if big else 3)


# two monomers (one pair, rows for one wavefront only); three; 63, 64, 65: the first row's pairs end one short of the 64 lanes,
# fill all but one, fill them exactly; 130: rows of three lane strides, scan segments of 3
@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 130])
def test_chain_lengths(ps, n):
    got, _ = run_exact(ps, sweep_cases(ps, 3, 5, n, seed=1820), q=magnitudes(5, 6.0, seed=n), records=2)
    if n == 2:
        np.testing.assert_allclose(got.msd[:, 0], got.sumsq[:, 1] / (2 * 5), rtol=1e-14)    # one pair: R2(1) = rmin^2


@pytest.mark.parametrize("min_sep", [1, 2, 11])
@pytest.mark.parametrize("max_sep", [0, 1, 11])
def test_separations_at_n_12(ps, max_sep, min_sep):
    got, _ = run_exact(ps, sweep_cases(ps, 3, 5, 12, seed=1830), max_sep=max_sep, min_sep=min_sep, q=magnitudes(3, 6.0), records=2)
    assert got.msd.shape == (3, max_sep) and got.pairs == (12 - min_sep) * (13 - min_sep) // 2


# nbins = 0 and nq = 0 skip their work; one bin; 64 and 512 bins (one, two and three counters per thread of the fold); nq = 1, 63,
# 64: one block of q with seven idle slots, eight blocks with one idle slot, eight full blocks
@pytest.mark.parametrize("nbins,nq", [(0, 0), (1, 1), (64, 63), (512, 64), (0, 64), (512, 0)])
def test_bin_and_magnitude_counts_at_n_65(ps, nbins, nq):
    run_exact(ps, sweep_cases(ps, 3, 5, 65, seed=1840), nbins=nbins, q=magnitudes(nq, 1.0, seed=nq) if nq else None, records=2)


def test_cases_that_differ_in_b_with_their_own_rmax(ps):
    bs = (0.5, 1.0, 2.5)
    cases = [ps.default_params(n=12, num_chains=20, precision=ps.F64, kT=1.0, seed=1870 + k, b=b, **BASE) for k, b in enumerate(bs)]
    got, _ = run_exact(ps, cases, rmax=[4.0 * b for b in bs], q=magnitudes(5, 6.0 / 2.5))
    assert got.rmin[0] < got.rmin[1] < got.rmin[2] and got.msd[2, 4] > 20 * got.msd[0, 4]     # lengths scale with b
    assert np.all(got.rmax == [2.0, 4.0, 10.0])
    share = got.counts / (got.counts.sum(axis=1, keepdims=True) + got.above[:, None])
    assert np.all(np.abs(share[0] - share[2]) < 0.05)               # the same distribution in units of b
    np.testing.assert_allclose(got.edges(2), 10.0 * np.arange(25) / 24, rtol=1e-15)


# ------------------------------------------------------------------------------------------------ the homes
# name: (parameters, precision, planar, chains per case, the kernel's name has), as tests/test_gpu_shape.py lists them
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
    cases = [make(num_chains=per, precision=precision, kT=0.8 + 0.3 * k, seed=1900 + k, **{**BASE, **kw, "E0": E0[k]}) for k in range(3)]
    with ps.Ensemble(cases, planar=planar) as e:
        assert has in e.launch_info().kernel.decode(), e.launch_info().kernel.decode()
    got, _ = run_exact(ps, cases, q=magnitudes(5, 6.0, seed=3), planar=planar, records=2)
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
    kTs = [0.25, 0.35, 0.5, 0.75, 1.2, 2.0, 4.0]
    cases = [ps.default_params(n=8, E0=3.0, Fz=0.2, kT=kT, num_chains=64, seed=i) for i, kT in enumerate(kTs)]
    q = magnitudes(3, 4.0, seed=9)
    o = dict(max_sep=-1, min_sep=1, nbins=12)
    with ps.Ensemble(cases) as A, ps.Ensemble(cases) as B:
        ta, tb = (e.open_tempering(ps.ladders_by(cases), seed=9) for e in (A, B))
        g = A.open_pdist(-1, 1, (12, 5.0), q)
        values = []
        for _ in range(5):
            A.advance_tempered(ta, 200, 50)
            g.record()
            B.advance_tempered(tb, 200, 50)
            ang = angles_of_all(B).reshape(7, 64, 16)
            values.append([pr.per_chain(ang[k], cases[k].b, -1, 1, 12, 5.0, q) for k in range(7)])
        got = g.read()
        sa, sb = ta.stats(), tb.stats()
        assert sa[2] == sb[2] == 20 and sa[1].sum() > 0, "no exchange was accepted: the records would not show a swapped configuration"
        assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1])
        assert_same_chains(A, B, range(7 * 64))
    assert got.records == 5
    compare(8, 64, cases, o, np.full(7, 5.0), q, False, values, got, None)


def test_refusals_leave_the_handle_usable(ps):
    lib = ps._lib.load()
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
        g = e.open_pdist(q=[1.0], capacity_rows=2)
        with ps.Ensemble(cases[:2]) as other:                        # an object of another handle
            assert lib.pstat_pdist_record(other._h, g._g) == -1 and b"the pdist object is not an open one" in lib.pstat_last_error()
            assert lib.pstat_advance_pdist(other._h, g._g, 10, 5) == -1
            assert lib.pstat_advance_pdist(other._h, g._g, 10, 0) == -1 and b"not an open one" in lib.pstat_last_error()
            assert lib.pstat_pdist_read(other._h, g._g, None, None, None) == -1
            assert lib.pstat_pdist_clear(other._h, g._g) == -1
            ptr, a, b = C.c_void_p(), C.c_int64(), C.c_int64()
            assert lib.pstat_pdist_rows(other._h, g._g, C.byref(ptr), C.byref(a), C.byref(b)) == -1
            lib.pstat_pdist_close(other._h, g._g)                    # ignored: it is not the other handle's to close
            assert other.chain_state(0)["steps_recorded"] == 0
        assert lib.pstat_advance_pdist(e._h, g._g, 10, 0) == -1 and b"stepout" in lib.pstat_last_error()
        assert lib.pstat_advance_pdist(e._h, g._g, -1, 5) == -1 and b"nsteps" in lib.pstat_last_error()
        assert e.chain_state(0)["steps_recorded"] == 0 and g.read().records == 0
        e.advance_pdist(g, 25, 10)
        assert g.read().records == 2 and e.chain_state(0)["steps_recorded"] == 25
        # the row buffer is full: refused with nothing enqueued
        assert lib.pstat_advance_pdist(e._h, g._g, 10, 10) == -7
        assert b"the pdist object has 0 of 2 rows free, this call would record 1" in lib.pstat_last_error()
        assert lib.pstat_advance_pdist(e._h, g._g, -1, 10) == -1     # an argument error comes before the full buffer
        assert lib.pstat_pdist_record(e._h, g._g) == -7
        assert e.chain_state(0)["steps_recorded"] == 25 and g.read().records == 2
        e.advance_pdist(g, 9, 10)                                    # no record in this call: it fits
        assert e.chain_state(0)["steps_recorded"] == 34
        g.clear()
        g.record()
        records = C.c_int64(-1)                                      # every output may be NULL
        assert lib.pstat_pdist_read(e._h, g._g, None, None, C.byref(records)) == 0 and records.value == 1
        totals = e.open_pdist(max_sep=0)                             # rmin alone, no rows kept: no limit, and no rows to hand out
        e.advance_pdist(totals, 50, 1)
        assert totals.read().records == 50 and totals.rows() == (0, 0, 3 * 1) and totals.read().sq.shape == (3, 0)
        with pytest.raises(ps.PstatError):
            totals.error_bars()
        keep = e.open_pdist()
        raw = g._g
        g.close()                                                    # with its last record still in flight
        assert g._g is None
        assert lib.pstat_pdist_read(e._h, raw, None, None, None) == -1 and b"not an open one" in lib.pstat_last_error()
        assert lib.pstat_pdist_record(e._h, raw) == -1 and lib.pstat_advance_pdist(e._h, raw, 0, 1) == -1
        assert lib.pstat_pdist_clear(e._h, raw) == -1
        lib.pstat_pdist_close(e._h, raw)                             # a second close is harmless
        e.advance_pdist(keep, 5, 5)                                  # the handle and its other objects go on
        assert keep.read().records == 1 and e.chain_state(0)["steps_recorded"] == 89
        blob = e.checkpoint()                                        # the object is not part of a checkpoint
        e.restore(blob)
        assert keep.read().records == 1
        e.open_pdist(bins=(8, 3.0), q=[1.0]).record()                # destroyed with objects open, a record in flight
    with ps.Ensemble(cases) as e:                                    # the next handle of the process works
        g = e.open_pdist()
        e.advance_pdist(g, 10, 3)
        assert g.read().records == 3
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
AXES = [("n", "8"), ("Fz", "0,1,2,3")]
FIXED = ["--num-steps", "3200", "--stepout", "100", "-v", "0"]
SPEC = "6:12,sep=5,min=2,q=6:4"


def _sweep(tmp_path, name, *extra):
    out = tmp_path / name
    axes = [a for k, v in AXES for a in ("--axis", f"{k}={v}")]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_sweep.py"), str(out), *axes,
                        "--num-chains", "64", "--seed", "11", *extra, "--", *FIXED], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def test_sweep_writes_pdist_files(tmp_path):
    with_pdist = _sweep(tmp_path, "s", "--pdist", SPEC)
    plain = _sweep(tmp_path, "p")
    outs = sorted(f for f in os.listdir(plain) if f.endswith(".out"))
    assert len(outs) == 4 and sorted(f for f in os.listdir(with_pdist) if f.endswith(".out")) == outs
    for f in outs:                                                   # the .out files are a plain run's, byte for byte
        assert (with_pdist / f).read_bytes() == (plain / f).read_bytes(), f
    assert not [f for f in os.listdir(plain) if f.endswith(".pdist")]
    files = sorted(f for f in os.listdir(with_pdist) if f.endswith(".pdist"))
    assert files == [f[:-len(".out")] + ".pdist" for f in outs]
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
