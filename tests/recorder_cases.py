"""What the GPU tests of the recorders share (tests/test_gpu_{hist,corr,shape,pdist,recorder_lifecycle}.py): the
`ps` fixture and the small helpers, which chains to compare, the case tables and homes, the twin protocol of the kinds that keep
column totals (run_totals_twin, driven by a Totals descriptor) and of the histograms (run_hist_twin), recording between
exchange rounds, and the tools/run_sweep.py call.  A plain module: it holds no test of its own."""
import collections
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import hist_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ helpers
@pytest.fixture(scope="module")
def ps():
    import polymer_stats_amd as ps
    assert ps._lib.load().pstat_device_count() >= 1, "no HIP device visible"
    return ps


def bits(x):
    return np.ascontiguousarray(x).tobytes()


def angles_of_all(e):
    return np.array([np.concatenate([s["theta"], s["phi"]]) for s in (e.chain_state(c) for c in range(e.ncases * e.num_chains))])


def micro_of_all(e):
    return np.array([e.microstate(c) for c in range(e.ncases * e.num_chains)]).reshape(e.ncases, e.num_chains, 7)


@functools.lru_cache(maxsize=None)
def hip_runtime():
    """The HIP runtime libpstat has loaded into this process (the rows of pstat_X_rows are device memory)."""
    with open("/proc/self/maps") as f:
        path = next(line.split()[-1] for line in f if "libamdhip64" in line)
    hip = C.CDLL(path)
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip


def device_rows(g):
    """[nrows, stride]: the rows that g.rows() hands out, copied to the host."""
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


# ------------------------------------------------------------------------------------------------ which chains to compare
# recording disturbed nothing: every chain where that is quick, else the chains at which the mapping changes.  The tile kinds
# (corr, shape, pdist): either side of a tile of 16 chains, of the 64 lanes of the fold, of 1 024.  The histograms: a wave's last
# lane and the next one, either side of a workgroup's 1 024 samples.  Both: a case's first and last chain.
TILE_EDGES, TILE_EVERY_BELOW = (0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024), 700
HIST_EDGES, HIST_EVERY_BELOW = (0, 1, 63, 64, 65, 255, 256, 1023, 1024, 1025), 1000


def edge_chains(ncases, per, offsets, every_below):
    if ncases * per <= every_below:
        return range(ncases * per)
    return sorted({k * per + j for k in range(ncases) for j in (*offsets, per - 1) if j < per})


# ------------------------------------------------------------------------------------------------ case tables
BASE = dict(E0=1.0, K1=0.5, K2=0.2, Fz=0.5, steps_per_adjust=150)
CLUSTER = dict(move_set=1, cluster_prob=0.5, bend_mod=0.3, bend_angle=0.2)

# chains per case: 1, 5 (one tile, not full), 64 (four full tiles of 16), 65 (a last tile of one chain), 1100 (69 tiles: more
# than the 64 lanes of the fold); 9 cases: the fold's last workgroup is not full
TILE_SHAPES = [(1, 1), (3, 5), (9, 64), (9, 65), (2, 1100)]


def sweep_cases(ps, ncases, per, n, seed, **kw):
    return [ps.default_params(n=n, num_chains=per, precision=ps.F64, kT=0.7 + 0.2 * k, seed=seed + k, **{**BASE, **kw}) for k in range(ncases)]


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


def home_cases(ps, home, seed, base=BASE):
    """(three cases that differ in kT and E0, planar) of a row of HOMES, once the home's kernel has been seen to be the one named."""
    kw, precision, planar, per, has = HOMES[home]
    make = ps.default_planar_params if planar else ps.default_params
    E0 = [0.5, 1.0, 1.5]
    cases = [make(num_chains=per, precision=precision, kT=0.8 + 0.3 * k, seed=seed + k, **{**base, **kw, "E0": E0[k]}) for k in range(3)]
    with ps.Ensemble(cases, planar=planar) as e:
        assert has in e.launch_info().kernel.decode(), e.launch_info().kernel.decode()
    return cases, planar


# ------------------------------------------------------------------------------------------------ the twin protocol, column totals
STEPOUT, REMAINDER = 40, 7

# What a kind that keeps column totals (a _Totals of ensemble.py) states about itself, for ONE choice of its options on ONE list
# of cases; k is a case's index.
#   name                        "corr": Ensemble.advance_corr, and the word in messages
#   ncols                       columns per case
#   open(e, capacity_rows)      the object, on the ensemble e
#   twin(ang, k)                a tuple: ([chains, ncols] per-chain values of the numpy twin on angles [chains, 2 n], and whatever
#                               else the kind's bounds and exact statements need of it)
#   bounds(k, M, twins)         (bound on |sum - twin's|, on |sumsq - twin's|), each [ncols], for M values per column; `twins`: the
#                               case's tuples, one per record.  A column with bound 0 is an integer and has to be equal.
#   row_bound(k, per, M, twins) [ncols]: the bound on a kept row, the mean over the case's `per` chains of one record
#   exact(got, rows, values, per)   the kind's own bit-for-bit statements; rows: [records, ncases, ncols] or None, values[record][k]
#   line                        the line to print, a format of `worst_totals` (the largest |device - twin| / bound of the totals) and
#                               `worst` (of totals and rows)
Totals = collections.namedtuple("Totals", "name ncols open twin bounds row_bound exact line")


def compare_totals(kind, ncases, per, values, got, rows):
    """The totals `got` and the kept rows ([records, ncases, ncols] or None) against values[record][k], the twin's tuples: within
    the kind's bounds, then the kind's exact statements.  Prints the kind's line."""
    def ratio(err, bound):
        return float((err[bound > 0] / bound[bound > 0]).max())

    M = per * len(values)
    worst_totals = worst_rows = 0.0
    for k in range(ncases):
        twins = [v[k] for v in values]
        want_s = sum(t[0].sum(axis=0) for t in twins)
        want_q = sum((t[0] * t[0]).sum(axis=0) for t in twins)
        b1, b2 = kind.bounds(k, M, twins)
        e1, e2 = np.abs(got.sum[k] - want_s), np.abs(got.sumsq[k] - want_q)
        worst_totals = max(worst_totals, ratio(e1, b1), ratio(e2, b2))
        assert np.all(e1 <= b1), (k, e1, b1, int((e1 - b1).argmax()))
        assert np.all(e2 <= b2), (k, e2, b2, int((e2 - b2).argmax()))
        if rows is not None:
            r1 = kind.row_bound(k, per, M, twins)
            for r, t in enumerate(twins):
                er = np.abs(rows[r, k] - t[0].sum(axis=0) / per)
                worst_rows = max(worst_rows, ratio(er, r1))
                assert np.all(er <= r1), (k, r, er, r1)
    print(kind.line.format(worst_totals=worst_totals, worst=max(worst_totals, worst_rows)))
    kind.exact(got, rows, values, per)


def run_totals_twin(ps, cases, kind, *, planar=False, records):
    """A records with advance_X (rows kept), B advances STEPOUT at a time and reads every chain's angles: the twin on B's angles
    gives A's sum, sumsq and rows within the kind's bounds; a second A gives the same bits, rows included; A's chains end as B's;
    the remainder of the steps is advanced and not recorded.  Returns A's result."""
    n, per, ncases = int(cases[0].n), int(cases[0].num_chains), len(cases)
    nsteps = records * STEPOUT + REMAINDER
    with ps.Ensemble(cases, planar=planar) as A, ps.Ensemble(cases, planar=planar) as B, ps.Ensemble(cases, planar=planar) as A2:
        g = kind.open(A, records)
        getattr(A, f"advance_{kind.name}")(g, nsteps, STEPOUT)
        g2 = kind.open(A2, records)
        getattr(A2, f"advance_{kind.name}")(g2, nsteps, STEPOUT)
        values = []                                                  # [record][case] -> the twin's tuple
        for _ in range(records):
            B.advance(STEPOUT)
            ang = angles_of_all(B).reshape(ncases, per, 2 * n)
            values.append([kind.twin(ang[k], k) for k in range(ncases)])
        B.advance(REMAINDER)
        got, again = g.read(), g2.read()
        assert got.records == records and got.sum.shape == (ncases, kind.ncols) == (ncases, g.ncols)
        assert bits(got.sum) == bits(again.sum) and bits(got.sumsq) == bits(again.sumsq), "two identical runs differ"
        rows, rows2 = device_rows(g), device_rows(g2)
        assert rows.shape == (records, ncases * kind.ncols) and bits(rows) == bits(rows2), "two identical runs differ in their rows"
        compare_totals(kind, ncases, per, values, got, rows.reshape(records, ncases, kind.ncols))
        assert_same_chains(A, B, edge_chains(ncases, per, TILE_EDGES, TILE_EVERY_BELOW))
        g.close()
        return got


# ------------------------------------------------------------------------------------------------ the twin protocol, histograms
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


def run_hist_twin(ps, cases, rows, per_case=False, planar=False, records=6):
    """A records with advance_hist, B advances STEPOUT at a time and reads every chain's microstate: the twin's counts on B's
    values equal A's as integers on the component channels; on the magnitude channels they may differ only where a value is
    within 2 ulp of an edge.  Returns A's result."""
    with ps.Ensemble(cases, planar=planar) as A, ps.Ensemble(cases, planar=planar) as B:
        h = A.open_hist(rows if per_case else rows[0], per_case=per_case)
        A.advance_hist(h, records * STEPOUT + REMAINDER, STEPOUT)    # the remainder is advanced and not recorded
        micro = []
        for _ in range(records):
            B.advance(STEPOUT)
            micro.append(micro_of_all(B))
        B.advance(REMAINDER)
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
        assert_same_chains(A, B, edge_chains(ncases, per, HIST_EDGES, HIST_EVERY_BELOW))
        h.close()
        return got


# ------------------------------------------------------------------------------------------------ with tempering
def ladder_cases(ps):
    kTs = [0.25, 0.35, 0.5, 0.75, 1.2, 2.0, 4.0]                     # the ladder of the README's example
    return [ps.default_params(n=8, E0=3.0, Fz=0.2, kT=kT, num_chains=64, seed=i) for i, kT in enumerate(kTs)]


def records_between_exchange_rounds(ps, cases, open_on, observe):
    """Five times {200 tempered steps with an exchange round every 50, one record} on A with the object open_on(A), the same steps
    on B with observe(B) after each: 20 rounds, some exchange accepted, the same statistics and chains in A and B.  Returns
    (what the object reads, the five observations)."""
    with ps.Ensemble(cases) as A, ps.Ensemble(cases) as B:
        ta, tb = (e.open_tempering(ps.ladders_by(cases), seed=9) for e in (A, B))
        g = open_on(A)
        seen = []
        for _ in range(5):
            A.advance_tempered(ta, 200, 50)
            g.record()
            B.advance_tempered(tb, 200, 50)
            seen.append(observe(B))
        got = g.read()
        sa, sb = ta.stats(), tb.stats()
        assert sa[2] == sb[2] == 20 and sa[1].sum() > 0, "no exchange was accepted: the records would not show a swapped configuration"
        assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1])
        assert_same_chains(A, B, range(len(cases) * int(cases[0].num_chains)))
    assert got.records == 5
    return got, seen


def totals_between_exchange_rounds(ps, cases, kind):
    """records_between_exchange_rounds for a kind that keeps column totals (no rows kept): the totals against the twin."""
    n, per, ncases = int(cases[0].n), int(cases[0].num_chains), len(cases)
    got, seen = records_between_exchange_rounds(ps, cases, lambda e: kind.open(e, 0), angles_of_all)
    values = [[kind.twin(ang.reshape(ncases, per, 2 * n)[k], k) for k in range(ncases)] for ang in seen]
    compare_totals(kind, ncases, per, values, got, None)


# ------------------------------------------------------------------------------------------------ the tool
AXES = [("n", "8"), ("Fz", "0,1,2,3")]
FIXED = ["--num-steps", "3200", "--stepout", "100", "-v", "0"]


def sweep_tool(tmp_path, name, *extra, axes=AXES, fixed=FIXED):
    """tools/run_sweep.py over `axes`, 64 chains per case, seed 11, into tmp_path / name, which it returns."""
    out = tmp_path / name
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_sweep.py"), str(out), *(a for k, v in axes for a in ("--axis", f"{k}={v}")),
                        "--num-chains", "64", "--seed", "11", *extra, "--", *fixed], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def assert_out_files_unchanged(with_kind, plain, suffix):
    """The .out files of a recorded sweep are a plain run's, byte for byte; the plain run writes no file of the kind, the recorded
    one writes one per .out file.  Returns (the .out names, the kind's names), sorted alike."""
    outs = sorted(f for f in os.listdir(plain) if f.endswith(".out"))
    assert outs and sorted(f for f in os.listdir(with_kind) if f.endswith(".out")) == outs
    for f in outs:
        assert (with_kind / f).read_bytes() == (plain / f).read_bytes(), f
    assert not [f for f in os.listdir(plain) if f.endswith(suffix)]
    files = sorted(f for f in os.listdir(with_kind) if f.endswith(suffix))
    assert files == [f[:-len(".out")] + suffix for f in outs]
    return outs, files
