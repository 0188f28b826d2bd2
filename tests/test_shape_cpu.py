"""Chain shape without a GPU: the seven entry points' declarations, exports and argument errors; the numpy twin
of the contract (tests/shape_ref.py) against hand values; the closed-form fixture, its generator and directly sampled chains; the
sweep tool's refusals."""
import ctypes as C
import importlib.util
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import shape_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["pstat_shape_open", "pstat_shape_record", "pstat_advance_shape", "pstat_shape_read", "pstat_shape_rows",
                "pstat_shape_clear", "pstat_shape_close"]
PI = np.pi


@pytest.fixture(scope="module")
def ps():
    import polymer_stats_amd as ps
    ps._lib.load()
    return ps


@pytest.fixture(scope="module", autouse=True)
def twin_and_library_name_the_same_columns(ps):
    """Every test here is about the feature: the twin's column order is the library's."""
    assert hasattr(ps._lib.load(), "pstat_shape_open") and tuple(ps.SHAPE_NAMES) == sr.NAMES


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
    assert "#define PSTAT_SHAPE_GYR 8" in header and "#define PSTAT_SHAPE_MAX_Q 512" in header
    assert ps.SHAPE_NAMES == ("gxx", "gyy", "gzz", "gxy", "gxz", "gyz", "rg2", "trg2") == sr.NAMES
    for name in ("SHAPE_NAMES", "Shape", "ShapeResult", "shape_anisotropy"):
        assert name in ps.__all__ and hasattr(ps, name), name
    # the list of synchronising accessors in the pstat_summary_get comment
    listed = header[header.index("Like every accessor that"):header.index("int pstat_summary_get")]
    assert "pstat_shape_read" in listed and "pstat_shape_rows" in listed


def test_null_arguments_are_refused_before_a_device_is_touched(ps):
    lib = ps._lib.load()
    out, ptr, n64 = C.c_void_p(), C.c_void_p(), C.c_int64(0)
    assert lib.pstat_shape_open(None, None, 0, 0, C.byref(out)) == -1 and b"null" in lib.pstat_last_error()
    assert lib.pstat_shape_record(None, None) == -1 and lib.pstat_advance_shape(None, None, 1, 1) == -1
    assert lib.pstat_shape_read(None, None, None, None, None) == -1 and lib.pstat_shape_clear(None, None) == -1
    assert lib.pstat_shape_rows(None, None, C.byref(ptr), C.byref(n64), C.byref(n64)) == -1
    lib.pstat_shape_close(None, None)


Q1 = [[0.0, 0.0, 1.0]]
# what: (arguments, return code, what the message names)
BAD = {
    "nq -1": (dict(nq=-1), -1, "nq"),
    "nq 513": (dict(q=[[0.0, 0.0, 0.1]] * 513, nq=513), -4, "PSTAT_SHAPE_MAX_Q"),
    "a NaN q": (dict(q=[[0.0, float("nan"), 1.0]], nq=1), -1, "q[0][1]"),
    "null q": (dict(q=None, nq=1), -1, "q is null"),
    "negative capacity": (dict(q=Q1, nq=1, capacity_rows=-1), -1, "capacity_rows"),
    "phase beyond 1e5": (dict(q=[[0.0, 0.0, 1.0], [1.0e4, 1.0e4, 0.0]], nq=2), -1, "q[1]"),      # 2e4 * b * n = 1.2e5 at n = 6
    "null out": (dict(out=None), -1, "null"),
}


@pytest.mark.parametrize("what", list(BAD))
def test_bad_arguments_are_refused_before_a_device_is_touched(ps, what):
    """The return code is the contract's and the message names the argument.  Where there is no device the handle cannot be made
    (rc -2 from pstat_create with valid arguments): the refusals are then shown on the null handle, which is refused first."""
    lib = ps._lib.load()
    kw, code, needle = BAD[what]
    p = ps.default_params(n=6, num_chains=4)
    h = C.c_void_p()
    rc = lib.pstat_create(C.byref(p), 1, None, C.byref(h))
    assert rc in (0, -2), rc
    out = C.c_void_p()
    a = dict(q=None, nq=0, capacity_rows=0, out=C.byref(out))
    a.update(kw)
    qa = np.ascontiguousarray(a["q"], dtype=np.float64) if a["q"] is not None else None
    qp = qa.ctypes.data_as(C.POINTER(C.c_double)) if qa is not None else None
    if rc == -2:
        assert lib.pstat_device_count() == 0
        assert lib.pstat_shape_open(None, qp, a["nq"], a["capacity_rows"], a["out"]) == -1
        return
    try:
        assert lib.pstat_shape_open(h, qp, a["nq"], a["capacity_rows"], a["out"]) == code
        assert needle.encode() in lib.pstat_last_error(), lib.pstat_last_error()
        if what == "phase beyond 1e5":
            assert b"case 0" in lib.pstat_last_error()
    finally:
        lib.pstat_destroy(h)


def test_python_refuses_a_misshapen_q():
    import polymer_stats_amd.ensemble as en
    e = object.__new__(en.Ensemble)
    e.planar = False
    with pytest.raises(ValueError):
        en.Ensemble.open_shape(e, q=[[1.0, 2.0]])                    # [nq, 2] is a planar handle's
    with pytest.raises(ValueError):
        en.Ensemble.open_shape(e, q=[1.0, 2.0, 3.0])
    np.testing.assert_array_equal(en._shape_q([[1.0, 2.0]], True), [[1.0, 0.0, 2.0]])
    assert en._shape_q(None, False).shape == (0, 3)


# ---------------------------------------------------------------------------------------------- the twin, by hand
def angles(theta, phi):
    return np.concatenate([np.asarray(theta, dtype=float), np.asarray(phi, dtype=float)])[None, :]


def test_twin_on_one_monomer():
    q = [[0.3, -2.0, 5.0], [0.0, 0.0, 0.0], [100.0, 0.0, 0.0]]
    v = sr.per_chain(angles([0.7], [1.9]), b=2.5, q=q)
    assert v.shape == (1, 8 + 3)
    np.testing.assert_array_equal(v[0, :8], np.zeros(8))             # one point: G = 0
    np.testing.assert_allclose(v[0, 8:], 1.0, atol=4e-16)            # cos^2 + sin^2


def test_twin_on_a_straight_chain_along_z():
    n, b = 8, 2.0
    x = sr.positions(angles([0.0] * n, [0.4] * n), b)
    np.testing.assert_allclose(x[0, :, 2], 2.0 * np.arange(n) + 1.0, atol=1e-14)     # x_i = 2 i + 1
    np.testing.assert_allclose(x[0, :, :2], 0.0, atol=1e-14)
    q = [[0.0, 0.0, 0.0], [1.7, 0.0, 0.0], [0.0, 0.0, 2 * PI / (n * b)], [0.0, 0.0, 0.3]]
    v = sr.per_chain(angles([0.0] * n, [0.4] * n), b, q)[0]
    want = np.zeros(8)
    want[2] = want[6] = b * b * (n * n - 1) / 12.0                   # G_zz of n equally spaced points
    want[7] = want[2] ** 2
    np.testing.assert_allclose(v[:8], want, rtol=1e-14, atol=1e-14)
    assert v[8] == n                                                  # q = 0, exactly
    np.testing.assert_allclose(v[9], n, rtol=1e-14)                  # q along x: every phase is 0
    assert abs(v[10]) <= 1e-12                                        # q_z b = 2 pi / n: the n phases close a polygon
    geo = np.sin(n * 0.3 * b / 2) ** 2 / np.sin(0.3 * b / 2) ** 2 / n
    np.testing.assert_allclose(v[11], geo, rtol=1e-13)


def test_twin_on_two_monomers_at_right_angles():
    # monomer 0 along x, monomer 1 along z, b = 1: centres (1/2, 0, 0) and (1, 0, 1/2); centre of mass (3/4, 0, 1/4)
    v = sr.per_chain(angles([PI / 2, 0.0], [0.0, 0.0]), 1.0, [[PI, 0.0, 0.0], [0.0, 0.0, 2 * PI], [1.0, 5.0, 1.0]])[0]
    gxx = gzz = 1.0 / 16.0
    gxz = ((-0.25) * (-0.25) + 0.25 * 0.25) / 2.0                    # the two deviations are (-1/4, -1/4) and (1/4, 1/4)
    want = [gxx, 0.0, gzz, 0.0, gxz, 0.0, gxx + gzz, gxx ** 2 + gzz ** 2 + 2 * gxz ** 2]
    np.testing.assert_allclose(v[:8], want, atol=1e-15)
    # S = (1/2) |e^{i q.x0} + e^{i q.x1}|^2 = 1 + cos(q . (x1 - x0)), x1 - x0 = (1/2, 0, 1/2)
    np.testing.assert_allclose(v[8:], [1 + np.cos(PI / 2), 1 + np.cos(PI), 1 + np.cos(1.0)], atol=1e-15)


def test_twin_planar_keeps_y_at_zero_and_ignores_qy():
    rng = np.random.default_rng(5)
    a = np.concatenate([np.zeros((4, 7)), rng.uniform(-7, 7, (4, 7))], axis=1)
    q = [[0.5, 3.0, -1.0], [2.0, 0.0, 0.25]]
    v = sr.per_chain(a, 1.3, q, planar=True)
    for name in ("gyy", "gxy", "gyz"):
        assert np.all(v[:, sr.NAMES.index(name)] == 0.0), name
    assert np.all(sr.positions(a, 1.3, planar=True)[:, :, 1] == 0.0)
    other = sr.per_chain(a, 1.3, [[0.5, -40.0, -1.0], [2.0, 7.0, 0.25]], planar=True)
    np.testing.assert_array_equal(v, other)
    np.testing.assert_array_equal(v, sr.per_chain(a, 1.3, [[0.5, -1.0], [2.0, 0.25]], planar=True))     # [nq, 2] = (q_x, q_z)
    # planar (cos phi, sin phi) in the x and z slots = the 3D chain with theta = pi / 2 - phi... checked on the first monomer
    np.testing.assert_allclose(sr.unit_vectors(a, planar=True)[:, :, 0], np.cos(a[:, 7:]))
    np.testing.assert_allclose(sr.unit_vectors(a, planar=True)[:, :, 2], np.sin(a[:, 7:]))


def test_twin_columns_totals_and_bounds():
    rng = np.random.default_rng(3)
    a = np.concatenate([rng.uniform(0, PI, (5, 4)), rng.uniform(-7, 7, (5, 4))], axis=1)
    v = sr.per_chain(a, 0.8, [[0.0, 0.0, 0.0], [1.0, 2.0, 3.0]])
    assert v.shape == (5, 10)
    i = {name: k for k, name in enumerate(sr.NAMES)}
    np.testing.assert_allclose(v[:, i["rg2"]], v[:, i["gxx"]] + v[:, i["gyy"]] + v[:, i["gzz"]], rtol=1e-15)
    tr = sum(v[:, i[k]] ** 2 for k in ("gxx", "gyy", "gzz")) + 2 * sum(v[:, i[k]] ** 2 for k in ("gxy", "gxz", "gyz"))
    np.testing.assert_allclose(v[:, i["trg2"]], tr, rtol=1e-15)
    # the tensor against numpy's own covariance of the positions
    x = sr.positions(a, 0.8)
    for c in range(5):
        cov = np.cov(x[c].T, bias=True)
        np.testing.assert_allclose([v[c, i["gxx"]], v[c, i["gyy"]], v[c, i["gzz"]], v[c, i["gxy"]], v[c, i["gxz"]], v[c, i["gyz"]]],
                                   [cov[0, 0], cov[1, 1], cov[2, 2], cov[0, 1], cov[0, 2], cov[1, 2]], rtol=1e-12, atol=1e-15)
    assert np.all(v[:, 8] == 4.0)
    s, q = sr.totals(v)
    np.testing.assert_allclose(s, v.sum(axis=0))
    np.testing.assert_allclose(q, (v ** 2).sum(axis=0))
    assert np.all(sr.per_chain(a, 0.8)[:, :8] == v[:, :8]) and sr.per_chain(a, 0.8).shape == (5, 8)
    E, V = sr.value_bounds(4, 0.8, [[0.0, 0.0, 0.0], [1.0, 2.0, 3.0]])
    L, u = 3.2, 2.0 ** -53
    assert E[0] == L * L * u * (7 * 4 + 51) and E[6] == 3 * E[0] and V[7] == 3 * L ** 4 and V[8] == 4.0
    assert E[8] == 4 * 4 * u * (4 + 3) and E[9] == 4 * 4 * u * (6.0 * L * 15 + 4 + 3)
    b1, b2 = sr.bounds(4, 0.8, 10, [[1.0, 2.0, 3.0]])
    assert b1[8] == 2 * 10 * E[9] + 100 * u * 4.0 and b2[8] == 2 * 10 * (2 * 4.0 * E[9] + u * 16.0) + 100 * u * 16.0
    assert np.all(np.abs(v) <= V * (1 + 1e-12))


# ---------------------------------------------------------------------------------------------- the fixture
@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_shape_closed_form", os.path.join(ROOT, "tests", "golden", "make_shape_closed_form.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "shape_closed_form.json")) as f:
        return json.load(f)


@pytest.mark.filterwarnings("ignore::scipy.integrate.IntegrationWarning")
def test_fixture_is_what_the_generator_gives(gen, golden):
    fresh = gen.closed_forms()
    assert {k for k in golden if not k.startswith("_")} == set(fresh) == {"fjc", "fixed_force", "planar"}
    for name in fresh:
        assert golden[name]["params"] == fresh[name]["params"] and golden[name]["q"] == fresh[name]["q"]
        assert set(golden[name]["expect"]) == set(fresh[name]["expect"]) == set(sr.NAMES[:7]) | {"sq"}
        for col, want in fresh[name]["expect"].items():
            np.testing.assert_allclose(golden[name]["expect"][col], want, rtol=1e-12, atol=1e-15)
        q = np.array(golden[name]["q"])
        assert not q[0].any() and golden[name]["expect"]["sq"][0] == 12.0             # q = 0 gives n
        for axis in (0, 2):                                                            # at least four magnitudes along x and along z
            along = q[(q[:, axis] != 0) & (np.count_nonzero(q, axis=1) == 1)]
            assert len(along) >= 4
    at = lambda name, qv: golden[name]["expect"]["sq"][golden[name]["q"].index(list(qv))]
    f, ff = golden["fjc"]["expect"], golden["fixed_force"]["expect"]
    assert abs(f["rg2"] - 1.7569444) < 5e-8 and abs(f["rg2"] - 253.0 / 144.0) < 1e-12
    for m, want in zip((0.5, 1.5, 3.0, 6.0), (10.42333, 4.71384, 1.84694, 1.00389)):
        assert abs(at("fjc", (0.0, 0.0, m)) - want) < 6e-6 and abs(at("fjc", (m, 0.0, 0.0)) - want) < 6e-6
    for m, par, perp in zip((0.5, 1.5, 3.0, 6.0), (6.25297, 1.27372, 0.80781, 0.67321), (10.60124, 5.13690, 2.04252, 1.03432)):
        assert abs(at("fixed_force", (0.0, 0.0, m)) - par) < 6e-6 and abs(at("fixed_force", (m, 0.0, 0.0)) - perp) < 6e-6
    assert abs(at("fixed_force", (1.0, 1.0, 1.0)) - 2.45860) < 6e-6
    assert abs(ff["gzz"] - 2.680789) < 6e-7 and abs(ff["gxx"] - 0.513174) < 6e-7
    # the free chain: chi(q) = sin(q b) / (q b)
    chi = gen.monomer_3d(0.0)[0]
    for m in (0.5, 1.5, 3.0, 6.0):
        assert abs(chi(np.array([0.0, 0.0, m])) - np.sin(m) / m) < 1e-12
    p = golden["planar"]["expect"]
    assert p["gyy"] == p["gxy"] == p["gyz"] == 0.0


def sample_angles(name, params, N, rng):
    """[N, 2n] angles of N chains of iid monomers drawn from the single-monomer density of fixture case `name`."""
    n, f = params["n"], params["Fz"] * params.get("b", 1.0) / params["kT"]
    if name == "planar":                                             # ~ exp(f sin phi): von Mises about pi / 2
        return np.concatenate([np.zeros((N, n)), rng.vonmises(PI / 2, f, (N, n))], axis=1)
    u = rng.random((N, n))
    c = 2.0 * u - 1.0 if f == 0 else np.log(np.exp(-f) + u * (np.exp(f) - np.exp(-f))) / f      # ~ exp(f c) on [-1, 1]
    return np.concatenate([np.arccos(np.clip(c, -1.0, 1.0)), rng.uniform(0.0, 2 * PI, (N, n))], axis=1)


@pytest.mark.parametrize("name", ["fjc", "fixed_force", "planar"])
def test_directly_sampled_chains_meet_the_fixture(golden, name):
    """16 384 iid chains per case, drawn in numpy with a fixed seed, through the twin.  Measured here: largest |z| 3.0, largest
    standard error 0.84 % of the fixture value (S at the largest q, whose per-chain values are nearly exponentially distributed)."""
    case = golden[name]
    N = 16384
    a = sample_angles(name, case["params"], N, np.random.default_rng(20261019))
    v = sr.per_chain(a, case["params"].get("b", 1.0), case["q"], planar=name == "planar")
    mean, se = v.mean(axis=0), v.std(axis=0, ddof=1) / np.sqrt(N)
    z, r = sr.judge_closed_form(name, case, mean, se)
    print(f"{name}: largest |z| = {z:.2f}, largest stderr / value = {100 * r:.2f} %")


# ---------------------------------------------------------------------------------------------- the tool's refusals
def test_sweep_refuses_shape_where_it_refuses_corr(tmp_path):
    """No GPU work is started: every refusal comes before the ensemble is made."""
    base = [sys.executable, os.path.join(ROOT, "tools", "run_sweep.py"), str(tmp_path / "x"), "--axis", "n=8", "--axis", "Fz=0,1"]
    tail = ["--", "--num-steps", "6400", "--stepout", "100"]
    for extra, more, needle in ((["--shape", "z:6:8", "--csv"], [], "--csv"), (["--shape", "z:6:8", "--gpus", "2"], [], "one device"),
                                (["--shape", "z:6:8", "--error-bars", "32"], [], "--error-bars"),
                                (["--shape", "z:6:8", "--hist", "r3:-8:8:32"], [], "--hist"),
                                (["--shape", "z:6:8", "--corr", "5"], [], "--corr"), (["--shape"], ["--umbrella-sampling"], "umbrella"),
                                (["--shape", "z:6:8"], ["--num-inits", "2"], "num-inits"),
                                (["--shape", "w:6:8"], [], "not understood"), (["--shape", "z:6"], [], "not understood"),
                                (["--shape", "z:6:0"], [], "not understood"), (["--shape", "z:6:300,x:6:300"], [], "at most 512"),
                                (["--shape", "z:20000:4"], [], "1e5"), (["--shape", "z:6:8"], ["--stepout", "5000"], "--stepout")):
        r = subprocess.run(base + extra + tail + more, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and needle in r.stderr, (extra, more, r.stderr[-500:])
        assert "Traceback" not in r.stderr, r.stderr[-800:]
    r = subprocess.run(base[:2] + [str(tmp_path / "x"), "--main", "mcmc_clustering_eap_chain_2d", "--axis", "n=8", "--shape", "y:6:8"] + tail,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "along y" in r.stderr, r.stderr[-500:]
    assert not (tmp_path / "x").exists() or not os.listdir(tmp_path / "x")
