"""GPU tests of the per-case histograms (pstat_hist_*, pstat_histogram_device, pstat_hist.hip) against the numpy
twin of the binning formula (tests/hist_ref.py): counts equal AS INTEGERS to the twin on the microstates of an identical second
ensemble, on every mapping of the kernel and on four homes; crafted edge values through a torch tensor; a closed-form density;
recording between exchange rounds; refusals and lifetime; tools/run_sweep.py --hist and tools/free_energy.py end to end."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import hist_ref as hr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ps():
    import polymer_stats_amd as ps
    assert ps._lib.load().pstat_device_count() >= 1, "no HIP device visible"
    return ps


def bits(x):
    return np.ascontiguousarray(x).tobytes()


def micro_of_all(e):
    return np.array([e.microstate(c) for c in range(e.ncases * e.num_chains)]).reshape(e.ncases, e.num_chains, 7)


def twin_counts(micro_records, rows, ncases):
    """What the twin makes of micro_records[record][case, chain, 7] under rows[case or 0][spec]: (counts per spec
    [ncases, nbins], tails [ncases, nspecs, 3])."""
    nspecs = len(rows[0])
    counts = [np.zeros((ncases, rows[0][i].nbins), dtype=np.int64) for i in range(nspecs)]
    tails = np.zeros((ncases, nspecs, 3), dtype=np.int64)
    for k in range(ncases):
        for i in range(nspecs):
            sp = rows[k if len(rows) > 1 else 0][i]
            x = np.concatenate([hr.channel_values(m[k], sp.channel) for m in micro_records])
            counts[i][k], tails[k, i] = hr.bin_counts(x, sp.lo, sp.hi, sp.nbins)
    return counts, tails


def assert_same_chains(a, b, chains):
    for c in chains:
        ga, gb = a.chain_state(c), b.chain_state(c)
        for k in ga:
            assert bits(ga[k]) == bits(gb[k]) if isinstance(ga[k], np.ndarray) else ga[k] == gb[k], (c, k)
        assert bits(a.microstate(c)) == bits(b.microstate(c)), c


def run_exact(ps, cases, rows, per_case=False, planar=False, stepout=40, records=6):
    """A records with advance_hist, B advances `stepout` at a time and reads every chain's microstate: the twin's counts on B's
    values equal A's as integers on the component channels; on the magnitude channels they may differ only where a value is
    within 2 ulp of an edge.  Returns A's result."""
    with ps.Ensemble(cases, planar=planar) as A, ps.Ensemble(cases, planar=planar) as B:
        h = A.open_hist(rows if per_case else rows[0], per_case=per_case)
        A.advance_hist(h, records * stepout + 7, stepout)           # the remainder is advanced and not recorded
        micro = []
        for _ in range(records):
            B.advance(stepout)
            micro.append(micro_of_all(B))
        B.advance(7)
        got = h.read()
        ncases, per = A.ncases, A.num_chains
        assert got.records == records and got.samples == records * per
        want, want_tails = twin_counts(micro, rows, ncases)
        for i, sp in enumerate(rows[0]):
            total = got.counts[i].sum(axis=1) + got.tails[:, i].sum(axis=1)
            assert np.array_equal(total, np.full(ncases, records * per)), (i, total)
            if sp.channel < 7:
                assert got.counts[i].dtype == np.int64 and np.array_equal(got.counts[i], want[i]), f"spec {i}: counts differ"
                assert np.array_equal(got.tails[:, i], want_tails[:, i]), f"spec {i}: tails differ"
            else:       # the one place where the device's sqrt may differ from numpy's
                near = 0
                for k in range(ncases):
                    s = rows[k if per_case else 0][i]
                    x = np.concatenate([hr.channel_values(m[k], s.channel) for m in micro])
                    near += int(hr.near_edge(x, s.lo, s.hi, s.nbins).sum())
                diff = int(np.abs(got.counts[i] - want[i]).sum() + np.abs(got.tails[:, i] - want_tails[:, i]).sum())
                print(f"magnitude channel {sp.channel}: |E| = {near} of {records * per * ncases} samples, sum |device - twin| = {diff}")
                assert diff <= 2 * near and near <= 0.01 * records * per * ncases
        C_ = ncases * per
        # recording disturbed nothing: every chain where that is quick, else the lanes and chains at which the mapping changes
        # (a wave's last lane and the next one, either side of a workgroup's 1 024 samples, a case's first and last chain)
        edges = {c for k in range(ncases) for j in (0, 1, 63, 64, 65, 255, 256, 1023, 1024, 1025, per - 1) if j < per for c in [k * per + j]}
        assert_same_chains(A, B, range(C_) if C_ <= 1000 else sorted(edges))
        h.close()
        return got


BASE = dict(E0=1.0, K1=0.5, Fz=0.5, steps_per_adjust=150)
CLUSTER = dict(move_set=1, cluster_prob=0.5, bend_mod=0.3, bend_angle=0.2)


def component_specs(ps, n, with_magnitudes=True):
    """nbins 1, 2 and 64; ranges that leave samples in both tails of some and in none of others."""
    s = [ps.hist_spec("r1", 64, -0.3 * n, 0.3 * n), ps.hist_spec("r2", 2, -1.0, 1.5), ps.hist_spec("r3", 1, 0.0, 0.5 * n),
         ps.hist_spec("p1", 64, -1.0, 1.0), ps.hist_spec("p2", 2, -50.0, 50.0), ps.hist_spec("p3", 64, 0.0, 0.4 * n),
         ps.hist_spec("U", 64, -1.0 * n, 0.25 * n)]
    if with_magnitudes:
        s += [ps.hist_spec("rmag", 64, 0.0, 1.0 * n), ps.hist_spec("pmag", 64, 0.0, 0.6 * n)]
    return s


# ------------------------------------------------------------------------------------------------ every mapping of the kernel
# chains per case: 1, 5, 64 (one wavefront per case, its last lane), 65 (the LDS kernel), 300, and 1100 > GROUP_SAMPLES = 1024 of
# pstat_hist.hip (two workgroups per case); 1, 3 and 9 cases (9: the last workgroup of the wave kernel is not full)
SHAPES = [(1, 1), (3, 5), (9, 64), (9, 65), (3, 300), (2, 1100)]


@pytest.mark.parametrize("ncases,per", SHAPES)
def test_counts_equal_the_twin_as_integers(ps, ncases, per):
    cases = [ps.default_params(n=12, num_chains=per, precision=ps.F64, kT=0.7 + 0.2 * k, seed=500 + k, **BASE) for k in range(ncases)]
    got = run_exact(ps, cases, [component_specs(ps, 12)])
    assert sum(int(c.sum()) for c in got.counts) > 0
    if ncases * per >= 64:
        assert got.tails[:, 0].sum() > 0 and got.counts[0].sum() > 0, "r1's range shows nothing: no sample in a tail, or none inside"


@pytest.mark.parametrize("ncases,per", [(2, 5), (3, 300)])
def test_a_handle_with_exactly_the_most_bins(ps, ncases, per):
    n = 12
    nb = [4096, 2048, 1024, 512, 256, 128, 128]
    assert sum(nb) == ps._lib.HIST_MAX_BINS
    rng = [(-0.3 * n, 0.3 * n), (-0.3 * n, 0.3 * n), (-0.2 * n, 0.6 * n), (-1.0, 1.0), (-1.0, 1.0), (0.0, 0.4 * n), (-1.0 * n, 0.25 * n)]
    specs = [ps.hist_spec(ch, nb[ch], *rng[ch]) for ch in range(7)]
    cases = [ps.default_params(n=n, num_chains=per, precision=ps.F64, kT=0.7 + 0.2 * k, seed=600 + k, **BASE) for k in range(ncases)]
    got = run_exact(ps, cases, [specs])
    assert got.counts[0].shape == (ncases, 4096) and got.counts[6][:, -1].shape == (ncases,)
    with ps.Ensemble(cases) as e:                                    # one bin more is refused, the handle stays usable
        with pytest.raises(ps.PstatError) as err:
            e.open_hist(specs + [ps.hist_spec("U", 1, 0.0, 1.0)])
        assert err.value.code == -4 and "8193" in str(err.value)
        e.advance(10)
        assert e.chain_state(0)["steps_recorded"] == 10


# ------------------------------------------------------------------------------------------------ the homes
# name: (parameters, precision, planar, the kernel's name has)
HOMES = {
    "f64 sweep": (dict(n=12), 1, False, "sweep_kernel<double>"),
    "fixed-force all-pairs": (dict(n=16, energy_type=1), 1, False, "interacting_kernel"),
    "clustering main": (dict(n=12, **CLUSTER), 1, False, "cluster"),
    "planar": (dict(n=14, cluster_prob=0.5), 1, True, "planar_kernel"),
    "f32 sweep": (dict(n=12), 0, False, "sweep_kernel<float>"),
}


@pytest.mark.parametrize("home", list(HOMES))
def test_every_home_and_a_per_case_range(ps, home):
    kw, precision, planar, has = HOMES[home]
    make = ps.default_planar_params if planar else ps.default_params
    E0 = [0.5, 1.0, 1.5]
    cases = [make(num_chains=70, precision=precision, kT=0.8 + 0.3 * k, seed=700 + k, **{**BASE, **kw, "E0": E0[k]}) for k in range(3)]
    n = kw["n"]
    with ps.Ensemble(cases, planar=planar) as e:
        assert has in e.launch_info().kernel.decode(), e.launch_info().kernel.decode()
    # U's range follows E0: only lo and hi differ between the cases
    rows = [component_specs(ps, n)[:6] + [ps.hist_spec("U", 64, -(0.4 + x * x) * n, 0.3 * n)] + component_specs(ps, n)[7:] for x in E0]
    got = run_exact(ps, cases, rows, per_case=True, planar=planar)
    assert not np.array_equal(got.edges(6, 0), got.edges(6, 2)) and np.array_equal(got.edges(0, 0), got.edges(0, 2))
    if planar:      # the y channels (r2, p2): every sample in whichever bin holds 0
        for i in (1, 4):
            sp = rows[0][i]
            zero = np.bincount(hr.slots([0.0], sp.lo, sp.hi, sp.nbins), minlength=sp.nbins)[:sp.nbins] * got.samples
            assert zero.sum() == got.samples and np.array_equal(got.counts[i], np.tile(zero, (3, 1))) and got.tails[:, i].sum() == 0


# ------------------------------------------------------------------------------------------------ crafted values
def test_crafted_values_through_a_torch_tensor():
    """tests/hist_device_cases.py in a process of its own: torch brings its own HIP runtime, which has to be the first one loaded,
    and this process has loaded libpstat's already.  Edge values, +-0, denormals, NaN, +-inf in matrices of 1, 63, 64, 65 and
    100 000 rows with a stride above the column count: all equal to the twin exactly."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "hist_device_cases.py")], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "all matrices agree" in r.stdout


# ------------------------------------------------------------------------------------------------ a closed-form density
def test_closed_form_density_of_the_extension(ps):
    """Device figures (MI355X): see DESIGN.md 3.14."""
    with open(os.path.join(ROOT, "tests", "golden", "hist_closed_form.json")) as f:
        golden = json.load(f)
    N = 16384
    cases = [ps.default_params(n=c["n"], E0=c["E0"], K1=c["K1"], K2=c["K2"], Fz=c["Fz"], kT=golden["kT"], b=golden["b"], num_chains=N,
                               precision=ps.F64, seed=20261019 + i) for i, c in enumerate(golden["cases"])]
    with ps.Ensemble(cases) as e:
        assert "sweep_kernel" in e.launch_info().kernel.decode()
        h = e.open_hist([ps.hist_spec("r3", golden["nbins"], golden["cases"][0]["lo"], golden["cases"][0]["hi"])])
        e.advance(400 * golden["cases"][0]["n"])
        h.record()
        got = h.read()
    assert got.records == 1 and got.samples == N and got.tails.sum() == 0
    for k, c in enumerate(golden["cases"]):
        p = np.array(c["prob"])
        tested = N * p >= 50
        z = (got.counts[0][k] - N * p) / np.sqrt(N * p * (1 - p))
        print(f"case {k} (E0 = {c['E0']}, Fz = {c['Fz']}): {tested.sum()} bins tested holding {p[tested].sum():.4f}, max |z| = {np.abs(z[tested]).max():.2f}")
        assert p[tested].sum() >= 0.99
        assert np.all(np.abs(z[tested]) < 5.0), np.round(z, 2)
        np.testing.assert_allclose(got.density(0, k).sum() * 0.5, 1.0, rtol=1e-12)
        assert np.array_equal(got.centers(0, k), -8.0 + 0.5 * (np.arange(32) + 0.5))


# ------------------------------------------------------------------------------------------------ with tempering
def test_records_between_exchange_rounds(ps):
    kTs = [0.25, 0.35, 0.5, 0.75, 1.2, 2.0, 4.0]                     # the ladder of the README's example
    cases = [ps.default_params(n=8, E0=3.0, Fz=0.2, kT=kT, num_chains=64, seed=i) for i, kT in enumerate(kTs)]
    rows = [[ps.hist_spec("r3", 32, -8.0, 8.0), ps.hist_spec("U", 64, -40.0, 0.0)]]
    micro = []
    with ps.Ensemble(cases) as A, ps.Ensemble(cases) as B:
        ta, tb = (e.open_tempering(ps.ladders_by(cases), seed=9) for e in (A, B))
        h = A.open_hist(rows[0])
        for _ in range(5):
            A.advance_tempered(ta, 200, 50)
            h.record()
            B.advance_tempered(tb, 200, 50)
            micro.append(micro_of_all(B))
        got = h.read()
        att, acc, rounds = ta.stats()
        assert rounds == 20 and acc.sum() > 0, "no exchange was accepted: the records would not show a swapped configuration"
    want, want_tails = twin_counts(micro, rows, 7)
    for i in range(2):
        assert np.array_equal(got.counts[i], want[i]) and np.array_equal(got.tails[:, i], want_tails[:, i])
        assert np.array_equal(got.counts[i].sum(axis=1) + got.tails[:, i].sum(axis=1), np.full(7, 5 * 64))
    assert got.records == 5 and got.samples == 5 * 64


# ------------------------------------------------------------------------------------------------ refusals and lifetime
def test_refusals_leave_the_handle_usable(ps):
    lib = ps._lib.load()
    spec = [ps.hist_spec("r3", 8, -6.0, 6.0)]
    with ps.Ensemble([ps.default_params(n=6, num_chains=4, kT=kT, umbrella=1) for kT in (1.0, 2.0)]) as e:
        with pytest.raises(ps.PstatError) as err:
            e.open_hist(spec)
        assert err.value.code == -4 and "umbrella" in str(err.value)
        e.advance(20)
        assert e.chain_state(0)["steps_recorded"] == 20
    cases = [ps.default_params(n=6, num_chains=4, kT=kT, Fz=0.3) for kT in (1.0, 2.0, 3.0)]
    with ps.Ensemble(cases) as e:
        for bad, code, needle in (([ps.hist_spec(9, 8, 0.0, 1.0)], -1, "channel 9"), ([ps.hist_spec("U", 0, 0.0, 1.0)], -1, "nbins"),
                                  ([ps.hist_spec("U", 4, 1.0, 1.0)], -1, "above lo"), ([ps.hist_spec("U", 4, 0.0, float("nan"))], -1, "finite"),
                                  (spec * 17, -1, "nspecs")):
            with pytest.raises(ps.PstatError) as err:
                e.open_hist(bad)
            assert err.value.code == code and needle in str(err.value), str(err.value)
        with pytest.raises(ps.PstatError) as err:                   # per case: channel and nbins must agree
            e.open_hist([spec, [ps.hist_spec("r3", 9, -6.0, 6.0)], spec], per_case=True)
        assert err.value.code == -1 and "case 1" in str(err.value)
        with pytest.raises(ValueError):
            e.open_hist([spec, spec], per_case=True)
        h = e.open_hist(spec)
        with ps.Ensemble(cases[:2]) as other:                        # a histogram of another handle
            assert lib.pstat_hist_record(other._h, h._g) == -1 and b"not an open histogram" in lib.pstat_last_error()
            assert lib.pstat_advance_hist(other._h, h._g, 10, 5) == -1
            assert lib.pstat_hist_read(other._h, h._g, None, None, None) == -1
            assert lib.pstat_hist_clear(other._h, h._g) == -1
            lib.pstat_hist_close(other._h, h._g)                     # ignored: it is not the other handle's to close
        assert lib.pstat_advance_hist(e._h, h._g, 10, 0) == -1 and lib.pstat_advance_hist(e._h, h._g, -1, 5) == -1
        e.advance_hist(h, 25, 10)
        got = h.read()
        assert got.records == 2 and e.chain_state(0)["steps_recorded"] == 25
        assert np.array_equal(got.counts[0].sum(axis=1) + got.tails[:, 0].sum(axis=1), [8, 8, 8])
        h.clear()                                                    # clear, then read: zeros
        got = h.read()
        assert got.records == 0 and got.counts[0].sum() == 0 and got.tails.sum() == 0
        h.record()
        assert h.read().counts[0].sum() + h.read().tails.sum() == 12
        records = C.c_int64(-1)                                      # every output may be NULL
        assert lib.pstat_hist_read(e._h, h._g, None, None, C.byref(records)) == 0 and records.value == 1
        g = h._g
        h.close()
        assert lib.pstat_hist_read(e._h, g, None, None, None) == -1  # read after close
        assert lib.pstat_hist_record(e._h, g) == -1
        e.advance(5)
        assert e.chain_state(0)["steps_recorded"] == 30
        e.open_hist(spec).record()                                   # destroyed with a histogram open
    with ps.Ensemble(cases) as e:
        e.advance(3)
        assert e.chain_state(0)["steps_recorded"] == 3


# ------------------------------------------------------------------------------------------------ the tools
def _sweep(tmp_path, name, *extra):
    out = tmp_path / name
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_sweep.py"), str(out), "--axis", "n=8", "--axis", "Fz=0,0.5,1,1.5,2,2.5",
                        "--num-chains", "64", "--seed", "11", *extra, "--", "--num-steps", "3000", "--stepout", "100", "-v", "0"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def test_sweep_writes_hist_files_and_free_energy_reads_them(tmp_path):
    with_hist = _sweep(tmp_path, "h", "--hist", "r3:-8:8:32", "--hist", "U:-10:2:16")
    plain = _sweep(tmp_path, "p")
    outs = sorted(f for f in os.listdir(plain) if f.endswith(".out"))
    assert len(outs) == 6 and sorted(f for f in os.listdir(with_hist) if f.endswith(".out")) == outs
    for f in outs:                                                   # the .out files are a plain run's, byte for byte
        assert (with_hist / f).read_bytes() == (plain / f).read_bytes(), f
    assert not [f for f in os.listdir(plain) if f.endswith(".hist")]
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import free_energy as fe
    hists = sorted(f for f in os.listdir(with_hist) if f.endswith(".hist"))
    assert hists == [f[:-len(".out")] + ".hist" for f in outs]
    for f in hists:
        r3, U = fe.read_hist(str(with_hist / f))
        assert (r3["channel"], r3["nbins"], r3["records"], r3["chains"], r3["lo"], r3["hi"]) == ("r3", 32, 30, 64, -8.0, 8.0)
        assert r3["counts"].sum() + sum(r3["tails"].values()) == 30 * 64 and U["counts"].sum() + sum(U["tails"].values()) == 30 * 64
        assert U["channel"] == "U" and len(U["counts"]) == 16 and np.array_equal(r3["edges"], np.linspace(-8, 8, 33))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "free_energy.py"), str(with_hist), "--component", "r3"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    csvs = [f for f in os.listdir(with_hist) if f.endswith(".csv")]
    assert csvs == ["n-0008000_A_r3.csv"], csvs
    lines = (with_hist / csvs[0]).read_text().strip().split("\n")
    assert lines[0] == "x,A,sigma,samples" and len(lines) > 8
    table = np.array([[float(v) for v in line.split(",")] for line in lines[1:]])
    assert np.all(np.isfinite(table)) and table[:, 1].min() == 0.0 and table[:, 3].sum() == 6 * 30 * 64 and np.all(table[:, 3] > 0)
    # the zero-force free energy of a chain of 8 free monomers has its minimum near r_z = 0
    assert abs(table[np.argmin(table[:, 1]), 0]) <= 1.5
