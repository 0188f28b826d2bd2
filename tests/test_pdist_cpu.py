"""Pair distances without a GPU: the seven entry points' declarations, exports and argument errors; the numpy
twin of the contract (tests/pdist_ref.py) against brute-force loops; the closed-form fixture, its generator and directly sampled
chains; the condition the GPU tests put on their random inputs; the sweep tool's --pdist strings and refusals."""
import ctypes as C
import importlib.util
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pdist_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["pstat_pdist_open", "pstat_pdist_record", "pstat_advance_pdist", "pstat_pdist_read", "pstat_pdist_rows",
                "pstat_pdist_clear", "pstat_pdist_close"]
PI = np.pi


@pytest.fixture(scope="module")
def ps():
    import polymer_stats_amd as ps
    ps._lib.load()
    return ps


# ---------------------------------------------------------------------------------------------- declarations
def test_declared_exported_and_listed(ps):
    with open(os.path.join(ROOT, "include", "pstat.h")) as f:
        header = f.read()
    lib = ps._lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\b(int|void)\s+%s\(" % name, header), name
        assert name in ps._lib.SYMBOLS and getattr(lib, name) is not None
        assert getattr(lib, name).argtypes is not None, name
    assert "#define PSTAT_ABI_VERSION 6" in header and lib.pstat_abi_version() == 6 and ps._lib.ABI_VERSION == 6
    assert "#define PSTAT_PDIST_MAX_Q 64" in header and "#define PSTAT_PDIST_MAX_BINS 512" in header
    assert (ps._lib.PDIST_MAX_Q, ps._lib.PDIST_MAX_BINS) == (64, 512)
    assert re.search(r"typedef struct pstat_pdist_spec \{\s*int32_t max_sep, min_sep, nbins, nq;\s*double rmax;\s*\} pstat_pdist_spec;", header)
    assert C.sizeof(ps._lib.PdistSpec) == 24 and ps._lib.PdistSpec.rmax.offset == 16
    for name in ("PDIST_NAMES", "Pdist", "PdistResult"):
        assert name in ps.__all__ and hasattr(ps, name), name
    assert hasattr(ps.Ensemble, "open_pdist") and hasattr(ps.Ensemble, "advance_pdist")
    listed = header[header.index("Like every accessor that"):header.index("int pstat_summary_get")]
    assert "pstat_pdist_read" in listed
    assert "J0" in header[header.index("Pair distances on the device"):header.index("#define PSTAT_PDIST_MAX_Q")]


def test_null_arguments_are_refused_before_a_device_is_touched(ps):
    lib = ps._lib.load()
    out, ptr, n64 = C.c_void_p(), C.c_void_p(), C.c_int64(0)
    spec = ps._lib.PdistSpec(-1, 1, 0, 0, 1.0)
    assert lib.pstat_pdist_open(None, C.byref(spec), None, None, 0, C.byref(out)) == -1 and b"null" in lib.pstat_last_error()
    assert lib.pstat_pdist_record(None, None) == -1 and lib.pstat_advance_pdist(None, None, 1, 1) == -1
    assert lib.pstat_pdist_read(None, None, None, None, None) == -1 and lib.pstat_pdist_clear(None, None) == -1
    assert lib.pstat_pdist_rows(None, None, C.byref(ptr), C.byref(n64), C.byref(n64)) == -1
    lib.pstat_pdist_close(None, None)


# what: (handle parameters, arguments, return code, what the message names); the handle has n = 6, b = 1 unless said otherwise
BAD = {
    "null spec": ({}, dict(spec=None), -1, "null"),
    "null out": ({}, dict(out=None), -1, "null"),
    "n 1": (dict(n=1), {}, -1, "n = 1"),
    "max_sep -2": ({}, dict(max_sep=-2), -1, "max_sep"),
    "max_sep n": ({}, dict(max_sep=6), -1, "max_sep"),
    "min_sep 0": ({}, dict(min_sep=0), -1, "min_sep"),
    "min_sep n": ({}, dict(min_sep=6), -1, "min_sep"),
    "nbins -1": ({}, dict(nbins=-1), -1, "nbins"),
    "nq -1": ({}, dict(nq=-1), -1, "nq"),
    "rmax 0": ({}, dict(nbins=4, rmax=0.0), -1, "rmax"),
    "rmax inf": ({}, dict(nbins=4, rmax=float("inf")), -1, "rmax"),
    "rmax NaN": ({}, dict(nbins=4, rmax=float("nan")), -1, "rmax"),
    "rmax tiny": ({}, dict(nbins=512, rmax=5e-324), -1, "nbins / rmax"),
    "rmax per case -1": ({}, dict(nbins=4, rmax=1.0, rmax_per_case=[-1.0]), -1, "rmax_per_case"),
    "null q": ({}, dict(nq=1, q=None), -1, "q is null"),
    "negative q": ({}, dict(q=[1.0, -0.5]), -1, "q[1]"),
    "NaN q": ({}, dict(q=[float("nan")]), -1, "q[0]"),
    "q b n beyond 1e5": ({}, dict(q=[1.0, 2.0e4]), -1, "q[1]"),                  # 2e4 * 1 * 6 = 1.2e5
    "negative capacity": ({}, dict(capacity_rows=-1), -1, "capacity_rows"),
    "nq 65": ({}, dict(q=[0.1] * 65), -4, "PSTAT_PDIST_MAX_Q"),
    "nbins 513": ({}, dict(nbins=513, rmax=1.0), -4, "PSTAT_PDIST_MAX_BINS"),
    "umbrella": (dict(umbrella=1), {}, -4, "umbrella"),
    "n beyond LDS": (dict(n=2561), {}, -4, "2560"),
    "n beyond LDS with 512 bins": (dict(n=2475), dict(nbins=512, rmax=100.0), -4, "2474"),
}


@pytest.mark.parametrize("what", list(BAD))
def test_bad_arguments_are_refused_before_a_device_is_touched(ps, what):
    """The return code is the contract's and the message names the argument.  Where there is no device the handle cannot be made
    (rc -2 from pstat_create with valid arguments): the refusals are then shown on the null handle, which is refused first."""
    lib = ps._lib.load()
    pkw, kw, code, needle = BAD[what]
    p = ps.default_params(**{"n": 6, "num_chains": 4, **pkw})
    h = C.c_void_p()
    rc = lib.pstat_create(C.byref(p), 1, None, C.byref(h))
    assert rc in (0, -2), rc
    out = C.c_void_p()
    a = dict(max_sep=-1, min_sep=1, nbins=0, rmax=1.0, q=[], rmax_per_case=None, capacity_rows=0, out=C.byref(out))
    a.update(kw)
    dp = C.POINTER(C.c_double)
    qa = np.ascontiguousarray(a["q"], dtype=np.float64) if a["q"] is not None else None
    qp = qa.ctypes.data_as(dp) if qa is not None and len(qa) else None
    ra = np.ascontiguousarray(a["rmax_per_case"], dtype=np.float64) if a["rmax_per_case"] is not None else None
    rp = ra.ctypes.data_as(dp) if ra is not None else None
    nq = a["nq"] if "nq" in a else (len(qa) if qa is not None else 0)
    spec = ps._lib.PdistSpec(a["max_sep"], a["min_sep"], a["nbins"], nq, a["rmax"])
    sp = C.byref(spec) if "spec" not in a else a["spec"]
    if rc == -2:
        assert lib.pstat_device_count() == 0
        assert lib.pstat_pdist_open(None, sp, qp, rp, a["capacity_rows"], a["out"]) == -1
        return
    try:
        assert lib.pstat_pdist_open(h, sp, qp, rp, a["capacity_rows"], a["out"]) == code, lib.pstat_last_error()
        assert needle.encode() in lib.pstat_last_error(), lib.pstat_last_error()
        if what == "q b n beyond 1e5":
            assert b"case 0" in lib.pstat_last_error()
    finally:
        lib.pstat_destroy(h)


def test_python_refuses_misshapen_options():
    import polymer_stats_amd.ensemble as en
    e = object.__new__(en.Ensemble)
    e.planar, e.ncases, e.n = False, 3, 8
    with pytest.raises(ValueError):
        en.Ensemble.open_pdist(e, q=[[1.0, 2.0]])
    with pytest.raises(ValueError):
        en.Ensemble.open_pdist(e, bins=(4, [1.0, 2.0]))              # two rmax for three cases
    with pytest.raises(ValueError):
        en.Ensemble.open_pdist(e, bins=4)
    assert en._pdist_bins(None, 3)[0] == 0 and en._pdist_bins((8, 2.0), 3)[1].tolist() == [2.0]
    assert en._pdist_bins((8, [1.0, 2.0, 3.0]), 3)[1].tolist() == [1.0, 2.0, 3.0] and en._pdist_q(None).shape == (0,)


def test_result_views_and_density(ps):
    """PdistResult on hand-made totals: the views, edges, centres, and a density that integrates to the share below rmax."""
    n, max_sep, min_sep, nbins, nq, N = 5, 2, 2, 4, 2, 10
    pairs = pr.pairs_counted(n, min_sep)
    assert pairs == 6
    cols = pr.ncols(max_sep, nbins, nq)
    s = np.zeros((2, cols))
    s[:, :2] = [[10.0, 20.0], [30.0, 40.0]]
    s[:, 2] = [5.0, 7.0]
    s[0, 3:8] = [6, 12, 18, 12, 12]                                  # N * pairs = 60 pairs of case 0: 48 below rmax
    s[1, 3:8] = [0, 0, 0, 0, 60]
    s[:, 8:] = [[50.0, 20.0], [50.0, 30.0]]
    res = ps.PdistResult(n, max_sep, min_sep, nbins, np.array([2.0, 4.0]), np.array([0.0, 1.0]), N, s, s * s, 1)
    assert res.pairs == pairs and res.msd.shape == (2, 2) and res.sq.shape == (2, 2) and res.counts.shape == (2, 4)
    np.testing.assert_array_equal(res.msd[1], [3.0, 4.0])
    np.testing.assert_array_equal(res.rmin, [0.5, 0.7])
    np.testing.assert_array_equal(res.above, [12.0, 60.0])
    np.testing.assert_array_equal(res.sq[0], [5.0, 2.0])
    np.testing.assert_array_equal(res.edges(1), [0.0, 1.0, 2.0, 3.0, 4.0])
    np.testing.assert_array_equal(res.centers(0), [0.25, 0.75, 1.25, 1.75])
    assert abs((res.density(0) * 0.5).sum() - 48.0 / 60.0) < 1e-15 and np.all(res.density(1) == 0.0)
    np.testing.assert_allclose(res.density(0), pr.density(s[0, 3:7], N * pairs, 2.0), rtol=1e-15)


# ---------------------------------------------------------------------------------------------- the twin against brute force
def brute(angles, b, max_sep, min_sep, nbins, rmax, q, planar):
    """One chain in Python floats, loop by loop, from the contract."""
    n = len(angles) // 2
    theta, phi = angles[:n], angles[n:]
    nh = [(math.cos(p), 0.0, math.sin(p)) if planar else (math.cos(p) * math.sin(t), math.sin(p) * math.sin(t), math.cos(t))
          for t, p in zip(theta, phi)]
    x, run = [], [0.0, 0.0, 0.0]
    for v in nh:
        run = [run[a] + v[a] for a in range(3)]
        x.append([b * (run[a] - v[a] / 2) for a in range(3)])
    r2 = {(i, j): sum((x[j][a] - x[i][a]) ** 2 for a in range(3)) for i in range(n) for j in range(i + 1, n)}
    out = [sum(r2[i, i + s] for i in range(n - s)) / (n - s) for s in range(1, max_sep + 1)]
    out.append(min(math.sqrt(v) for (i, j), v in r2.items() if j - i >= min_sep))
    if nbins:
        counts = [0.0] * (nbins + 1)
        for (i, j), v in r2.items():
            if j - i >= min_sep:
                t = math.sqrt(v) * (nbins / rmax)
                counts[int(t) if t < nbins else nbins] += 1
        out += counts
    for qk in q:
        tot = 0.0
        for v in r2.values():
            xx = qk * math.sqrt(v)
            tot += 1.0 if xx == 0.0 else math.sin(xx) / xx
        out.append(1.0 + 2.0 * tot / n)
    return out


@pytest.mark.parametrize("n", [2, 3, 7])
@pytest.mark.parametrize("planar", [False, True])
def test_twin_equals_brute_force_loops(n, planar):
    rng = np.random.default_rng(10 + n)
    a = np.concatenate([rng.uniform(0, PI, (6, n)), rng.uniform(-7, 7, (6, n))], axis=1)
    b, q = 1.3, [0.0, 0.7, 4.0]
    for max_sep, min_sep, nbins in ((n - 1, 1, 5), (0, n - 1, 0), (1, max(1, n - 2), 16)):
        rmax = 0.6 * n * b
        v, und, rfloor = pr.per_chain(a, b, max_sep, min_sep, nbins, rmax, q, planar)
        assert v.shape == (6, pr.ncols(max_sep, nbins, 3)) and not und.any() and rfloor > 0
        for c in range(6):
            want = brute(list(a[c]), b, max_sep, min_sep, nbins, rmax, q, planar)
            np.testing.assert_allclose(v[c], want, rtol=1e-13, atol=1e-14)
        msd, rmin, hist, sq = pr.columns(max_sep, nbins, 3)
        assert np.all(v[:, sq][:, 0] == n)                           # q = 0 gives n exactly
        if nbins:
            assert np.all(v[:, hist].sum(axis=1) == pr.pairs_counted(n, min_sep))
            hb = np.array([brute(list(a[c]), b, max_sep, min_sep, nbins, rmax, q, planar)[hist] for c in range(6)])
            np.testing.assert_array_equal(v[:, hist], hb)
    assert np.array_equal(pr.per_chain(a, b, -1, 1, 0, 1.0, None, planar)[0], pr.per_chain(a, b, n - 1, 1, 0, 1.0, [], planar)[0])


def test_twin_on_the_straight_chain_sits_on_the_edges():
    """theta = 0, b = 1: x_i = i + 1/2, r2 and r exact integers; with rmax and nbins powers of two every t is an exact integer, so
    under the twin every pair at s <= rmax is undecided -- this input is compared with the formula, not with the intervals."""
    n, nbins, rmax = 9, 16, 4.0
    a = np.zeros((1, 2 * n))
    a[0, n:] = 0.4
    x = pr.positions(a, 1.0)
    assert np.all(x[0, :, 2] == np.arange(n) + 0.5) and np.all(x[0, :, :2] == 0.0)
    I, J = pr.pair_index(n)
    r2, r = pr.pair_distances(x)
    assert np.all(r[0] == J - I) and np.all(r2[0] == (J - I) ** 2)
    v, und, rfloor = pr.per_chain(a, 1.0, -1, 2, nbins, rmax, [0.0])
    assert rfloor == 1.0 and v[0, n - 1] == 2.0                      # rmin = min_sep
    np.testing.assert_array_equal(v[0, :n - 1], np.arange(1, n) ** 2.0)
    assert und.sum() == 2 * sum(n - s for s in (2, 3, 4))            # s = 2, 3, 4 sit on integers <= nbins


def test_twin_flags_a_pair_on_an_edge_and_only_that():
    n, b = 3, 1.0
    a = np.array([[0.0, 0.0, PI / 2, 0.3, 0.3, 0.0]])                # r01 = 1, r02 = |(1/2, 0, 3/2)|, r12 = |(1/2, 0, 1/2)|
    v, und, _ = pr.per_chain(a, b, 0, 1, 4, 2.0, None)               # t01 = 2 exactly: undecided between bins 1 and 2
    np.testing.assert_array_equal(und[0], [0, 1, 1, 0, 0])
    np.testing.assert_array_equal(v[0, 1:], [0, 1, 0, 1, 0])         # t12 = 1.41, t02 = 3.16 are decided
    b1, b2 = pr.bounds(n, b, 10, 0, 4, None, 0.7)
    assert np.all(b1[1:] == 0.0) and np.all(b2[1:] == 0.0) and 0 < b1[0] < 1e-11


def test_bounds_are_the_docstrings():
    n, b, u = 10, 0.8, 2.0 ** -53
    L, P = 8.0, 45
    e2 = L * L * u * (12 * n + 108)
    assert pr.eps_r2(n, b) == e2
    assert pr.eps_r(0.5, n, b) == e2 / 0.5 + 2 * u * L and pr.eps_r(0.0, n, b) == 2.5 * math.sqrt(e2) + 2 * u * L
    E, V = pr.value_bounds(n, b, 3, 2, [0.0, 2.0], 0.5)
    er = e2 / 0.5 + 2 * u * L
    assert list(E[:3]) == [L * L * u * (13 * n + 108)] * 3 and E[3] == er and list(E[4:7]) == [0.0] * 3
    assert E[7] == 9 * (3 * u + P * u) + 20 * u
    assert E[8] == 9 * (0.44 * 2.0 * (er + u * L) + 3 * u + P * u) + 20 * u
    assert list(V) == [64.0] * 3 + [8.0] + [45.0] * 3 + [10.0] * 2
    b1, b2 = pr.bounds(n, b, 7, 3, 2, [0.0, 2.0], 0.5)
    assert b1[0] == 2 * 7 * E[0] + 49 * u * 64.0 and b2[3] == 2 * 7 * (2 * 8.0 * er + u * 64.0) + 49 * u * 64.0


# shapes of tests/test_gpu_pdist.py: (n, chains, nbins, rmax / (n b), planar)
@pytest.mark.parametrize("n,C,nbins,planar", [(12, 640, 24, False), (2, 64, 64, False), (3, 64, 64, True), (63, 15, 64, False),
                                              (64, 15, 1, False), (65, 15, 512, False), (130, 15, 512, True)])
def test_random_inputs_have_no_undecided_pair(n, C, nbins, planar):
    """The condition the GPU tests put on their random-angle inputs, shown here on random angles of the same shapes: no pair within
    the twin's window of a bin edge, so the histogram comparison is an equality of integers."""
    rng = np.random.default_rng(n)
    a = np.concatenate([rng.uniform(0, PI, (C, n)), rng.uniform(-PI, PI, (C, n))], axis=1)
    v, und, rfloor = pr.per_chain(a, 1.0, 0, 1, nbins, 0.5 * n, None, planar)
    assert und.sum() == 0 and rfloor > 0
    assert np.all(v[:, 1:].sum(axis=1) == n * (n - 1) // 2)


# ---------------------------------------------------------------------------------------------- the fixture
@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_pdist_closed_form", os.path.join(ROOT, "tests", "golden", "make_pdist_closed_form.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "pdist_closed_form.json")) as f:
        return json.load(f)


CASES = ["fjc", "fixed_force", "planar", "dimer", "planar_dimer"]


def test_fixture_is_what_the_generator_gives(gen, golden):
    fresh = gen.closed_forms()
    assert {k for k in golden if not k.startswith("_")} == set(fresh) == set(CASES)
    for name in fresh:
        assert golden[name]["params"] == fresh[name]["params"] and golden[name]["options"] == fresh[name]["options"]
        assert set(golden[name]["expect"]) == set(fresh[name]["expect"])
        for col, want in fresh[name]["expect"].items():
            np.testing.assert_allclose(golden[name]["expect"][col], want, rtol=1e-13, atol=1e-16)
    f, ff = golden["fjc"], golden["fixed_force"]
    assert f["options"]["q"] == [0.0, 0.5, 1.5, 3.0, 6.0] and f["expect"]["sq"][0] == 12.0
    for got, want in zip(f["expect"]["sq"][1:], (10.423, 4.714, 1.847, 1.004)):
        assert abs(got - want) < 6e-4
    assert f["expect"]["msd"] == [s - 0.5 for s in range(1, 12)] == golden["planar"]["expect"]["msd"]
    for s, want in zip((1, 2, 5, 11), (0.5960, 1.9799, 8.4350, 31.711)):
        assert abs(ff["expect"]["msd"][s - 1] - want) < 6e-4
    d, pd = golden["dimer"]["expect"], golden["planar_dimer"]["expect"]
    assert abs(sum(d["hist"]) - 1.0) < 1e-15 and abs(sum(pd["hist"]) - 1.0) < 1e-15 and d["hist"][-1] == pd["hist"][-1] == 0.0
    assert d["rmin"] == 2.0 / 3.0 and abs(pd["rmin"] - 2.0 / PI) < 1e-16 and d["hist"][3] == 7.0 / 64.0


def sample_angles(name, params, N, rng):
    """[N, 2n] angles of N chains of iid monomers: uniform on the sphere, cos theta by inverse CDF under force; uniform phi for a
    planar chain."""
    n, f = params["n"], params["Fz"] * params.get("b", 1.0) / params["kT"]
    if name.startswith("planar"):
        assert f == 0.0
        return np.concatenate([np.zeros((N, n)), rng.uniform(0.0, 2 * PI, (N, n))], axis=1)
    u = rng.random((N, n))
    c = 2.0 * u - 1.0 if f == 0 else np.log(np.exp(-f) + u * (np.exp(f) - np.exp(-f))) / f      # ~ exp(f c) on [-1, 1]
    return np.concatenate([np.arccos(np.clip(c, -1.0, 1.0)), rng.uniform(0.0, 2 * PI, (N, n))], axis=1)


@pytest.mark.parametrize("name", CASES)
def test_directly_sampled_chains_meet_the_fixture(golden, name):
    """200 000 iid chains per case, drawn in numpy with a fixed seed, through the twin, judged by pdist_ref.judge_closed_form: 5
    sigma on every column, 2 % on msd, rmin and sq.  Measured here: largest |z| 1.7 (fjc 1.7, fixed_force 1.1, planar 1.0, dimer
    1.3, planar_dimer 1.1), largest standard error 0.21 % of the value."""
    case = golden[name]
    o = case["options"]
    N = 200000
    a = sample_angles(name, case["params"], N, np.random.default_rng(20261020))
    v, und, _ = pr.per_chain(a, case["params"].get("b", 1.0), o["max_sep"], o["min_sep"], o["nbins"], o["rmax"], o["q"],
                             planar=name.startswith("planar"))
    assert und.sum() == 0
    mean, se = v.mean(axis=0), v.std(axis=0, ddof=1) / np.sqrt(N)
    z, r = pr.judge_closed_form(name, case, mean, se)
    print(f"{name}: largest |z| = {z:.2f}, largest stderr / value = {100 * r:.2f} %")
    if o["nbins"]:                                                   # the density integrates to the share below rmax
        _, _, hist, _ = pr.columns(case["params"]["n"] - 1, o["nbins"], len(o["q"]))
        counts = v[:, hist].sum(axis=0)
        pairs = N * pr.pairs_counted(case["params"]["n"], o["min_sep"])
        dens = pr.density(counts[:-1], pairs, o["rmax"])
        assert abs((dens * (o["rmax"] / o["nbins"])).sum() - (1.0 - counts[-1] / pairs)) < 1e-12


def test_twin_density_integrates_to_the_share_below_rmax():
    rng = np.random.default_rng(4)
    n, C, nbins, rmax = 9, 50, 10, 3.0
    a = np.concatenate([rng.uniform(0, PI, (C, n)), rng.uniform(-PI, PI, (C, n))], axis=1)
    v, und, _ = pr.per_chain(a, 1.0, 0, 2, nbins, rmax, None)
    assert not und.any()
    counts = v[:, 1:].sum(axis=0)
    pairs = C * pr.pairs_counted(n, 2)
    assert counts.sum() == pairs and 0 < counts[-1] < pairs
    dens = pr.density(counts[:-1], pairs, rmax)
    assert abs((dens * (rmax / nbins)).sum() - (pairs - counts[-1]) / pairs) < 1e-14


# ---------------------------------------------------------------------------------------------- the tool's strings and refusals
def test_parse_of_pdist_strings():
    from polymer_stats_amd import sweep as sw
    kind, o = sw.parse_pdist("4.5:32")
    assert kind == "pdist" and o == dict(rmax=4.5, nbins=32, max_sep=-1, min_sep=1, q=[])
    _, o = sw.parse_pdist("8:64,sep=5,min=2,q=6:4")
    assert o == dict(rmax=8.0, nbins=64, max_sep=5, min_sep=2, q=[1.5, 3.0, 4.5, 6.0])
    assert sw.parse_pdist("1:0,sep=0")[1]["nbins"] == 0 and sw.parse_pdist("1:0,sep=0")[1]["max_sep"] == 0
    for bad in ("", "4", "4:x", "0:8", "-1:8", "inf:8", "4:-1", "4:8,sep=-2", "4:8,min=0", "4:8,q=6", "4:8,q=0:4", "4:8,q=6:0",
                "4:8,lag=3", "4:8:2", "4:8,sep"):
        with pytest.raises(sw.ReferenceError_, match="not understood"):
            sw.parse_pdist(bad)
    with pytest.raises(sw.ReferenceError_, match="at most 512"):
        sw.parse_pdist("4:513")
    with pytest.raises(sw.ReferenceError_, match="at most 64"):
        sw.parse_pdist("4:8,q=6:65")
    from polymer_stats_amd import _host
    row = _host.RECORDINGS["pdist"]
    assert (row.flag, row.ext) == ("--pdist", ".pdist") and list(_host.RECORDINGS)[-1] == "pdist" and len(_host.RECORDINGS) == 5


def test_sweep_refuses_pdist_where_it_refuses_shape(tmp_path):
    """No GPU work is started: every refusal comes before the ensemble is made."""
    base = [sys.executable, os.path.join(ROOT, "tools", "run_sweep.py"), str(tmp_path / "x"), "--axis", "n=8", "--axis", "Fz=0,1"]
    tail = ["--", "--num-steps", "6400", "--stepout", "100"]
    P = ["--pdist", "4:16,q=6:4"]
    for extra, more, needle in ((P + ["--csv"], [], "--csv"), (P + ["--gpus", "2"], [], "one device"),
                                (P + ["--error-bars", "32"], [], "--error-bars"), (P + ["--hist", "r3:-8:8:32"], [], "--hist"),
                                (P + ["--corr", "5"], [], "--corr"), (P + ["--shape", "z:6:8"], [], "--shape"),
                                (P, ["--umbrella-sampling"], "umbrella"), (P, ["--num-inits", "2"], "num-inits"),
                                (["--pdist", "4"], [], "not understood"), (["--pdist", "4:16,sep=8"], [], "n - 1"),
                                (["--pdist", "4:16,min=8"], [], "n - 1"), (["--pdist", "4:600"], [], "at most 512"),
                                (["--pdist", "4:16,q=20000:4"], [], "1e5"), (P, ["--stepout", "5000"], "--stepout")):
        r = subprocess.run(base + extra + tail + more, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and needle in r.stderr, (extra, more, r.stderr[-500:])
        assert "Traceback" not in r.stderr, r.stderr[-800:]
    assert not (tmp_path / "x").exists() or not os.listdir(tmp_path / "x")


def test_pdist_lines_on_hand_made_results(ps):
    from polymer_stats_amd import _host
    n, N = 4, 2
    s = np.array([[2.0, 6.0, 1.5, 8.0, 2.0, 2.0, 8.0, 4.0]])        # msd x 2, rmin, 2 bins + above (6 pairs x 2 chains), sq x 2
    res = ps.PdistResult(n, 2, 1, 2, np.array([3.0]), np.array([0.0, 1.5]), N, s, s * s, 1)

    class EB:
        stderr = np.arange(8.0)[None, :] / 10
    lines = _host.pdist_lines(res, EB, 0)
    assert lines[0] == "name,x,value,stderr" and len(lines) == 1 + 2 + 1 + 2 + 1 + 2
    assert lines[1] == "msd,1,1.0,0.0" and lines[2] == "msd,2,3.0,0.1" and lines[3] == "rmin,,0.75,0.2"
    name, x, value, err = lines[4].split(",")
    assert (name, float(x)) == ("hist", 0.75) and float(value) == 8.0 / (12 * 1.5) and abs(float(err) - 0.3 / (6 * 1.5)) < 1e-16
    assert lines[6].split(",")[:2] == ["above", ""] and float(lines[6].split(",")[2]) == 2.0 / 12
    assert lines[7].split(",")[:3] == ["sq", "0.0", "4.0"] and lines[8].split(",")[:3] == ["sq", "1.5", "2.0"]
