"""Correlations without a GPU: the seven entry points' declarations, exports and argument errors; the numpy twin
of the contract (tests/corr_ref.py) against hand values; the closed-form fixture and its generator; the sweep tool's refusals."""
import ctypes as C
import importlib.util
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import corr_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["pstat_corr_open", "pstat_corr_record", "pstat_advance_corr", "pstat_corr_read", "pstat_corr_rows",
                "pstat_corr_clear", "pstat_corr_close"]
PI = np.pi


@pytest.fixture(scope="module")
def ps():
    import polymer_stats_amd as ps
    ps._lib.load()
    return ps


@pytest.fixture(scope="module", autouse=True)
def twin_and_library_name_the_same_channels(ps):
    """Every test here is about the feature: the twin's column order is the library's."""
    assert hasattr(ps._lib.load(), "pstat_corr_open") and tuple(ps.CORR_NAMES) == cr.CHANNELS


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
    assert "enum { PSTAT_CORR_NN = 1, PSTAT_CORR_ZZ = 2, PSTAT_CORR_MM = 4 };" in header
    assert ps.CORR_NAMES == ("nn", "zz", "mm") == cr.CHANNELS
    # the list of synchronising accessors in the pstat_summary_get comment
    listed = header[header.index("Like every accessor that"):header.index("int pstat_summary_get")]
    assert "pstat_corr_read" in listed and "pstat_corr_rows" in listed


def test_null_arguments_are_refused_before_a_device_is_touched(ps):
    lib = ps._lib.load()
    out, ptr, n64 = C.c_void_p(), C.c_void_p(), C.c_int64(0)
    assert lib.pstat_corr_open(None, 1, -1, 0, C.byref(out)) == -1 and b"null" in lib.pstat_last_error()
    assert lib.pstat_corr_record(None, None) == -1 and lib.pstat_advance_corr(None, None, 1, 1) == -1
    assert lib.pstat_corr_read(None, None, None, None, None) == -1 and lib.pstat_corr_clear(None, None) == -1
    assert lib.pstat_corr_rows(None, None, C.byref(ptr), C.byref(n64), C.byref(n64)) == -1
    lib.pstat_corr_close(None, None)


BAD = {
    "no channel": (dict(channels=0), "channels"),
    "channel 8": (dict(channels=8), "channels"),
    "negative mask": (dict(channels=-1), "channels"),
    "max_lag -2": (dict(max_lag=-2), "max_lag"),
    "max_lag n": (dict(max_lag=6), "max_lag"),
    "negative capacity": (dict(capacity_rows=-1), "capacity_rows"),
    "null out": (dict(out=None), "null"),
}


@pytest.mark.parametrize("what", list(BAD))
def test_bad_arguments_are_refused_before_a_device_is_touched(ps, what):
    """rc -1 names the argument.  Where there is no device the handle cannot be made (rc -2 from pstat_create with valid
    arguments): the refusals are then shown on the null handle, which is refused first."""
    lib = ps._lib.load()
    kw, needle = BAD[what]
    p = ps.default_params(n=6, num_chains=4)
    h = C.c_void_p()
    rc = lib.pstat_create(C.byref(p), 1, None, C.byref(h))
    assert rc in (0, -2), rc
    out = C.c_void_p()
    a = dict(channels=1, max_lag=-1, capacity_rows=0, out=C.byref(out))
    a.update(kw)
    if rc == -2:
        assert lib.pstat_device_count() == 0
        assert lib.pstat_corr_open(None, a["channels"], a["max_lag"], a["capacity_rows"], a["out"]) == -1
        return
    try:
        assert lib.pstat_corr_open(h, a["channels"], a["max_lag"], a["capacity_rows"], a["out"]) == -1
        assert needle.encode() in lib.pstat_last_error(), lib.pstat_last_error()
    finally:
        lib.pstat_destroy(h)


def test_python_refuses_an_unknown_channel_name():
    import polymer_stats_amd.ensemble as en
    with pytest.raises(ValueError):
        en.Ensemble.open_corr(object.__new__(en.Ensemble), channels=("nn", "xx"))


# ---------------------------------------------------------------------------------------------- the twin, by hand
def angles(theta, phi):
    return np.concatenate([np.asarray(theta, dtype=float), np.asarray(phi, dtype=float)])[None, :]


def test_twin_on_chains_along_the_axes():
    # n = 2: x then z.  nn(0) = 1, nn(1) = x.z = 0; zz(0) = (0 + 1) / 2, zz(1) = 0 * 1
    v = cr.per_chain(angles([PI / 2, 0.0], [0.0, 0.0]), 1, ("nn", "zz"))
    np.testing.assert_allclose(v, [[1.0, 0.0, 0.5, 0.0]], atol=1e-15)
    # n = 3: x, y, z.  All mutually orthogonal; zz(0) = 1/3; zz(k > 0) = 0
    v = cr.per_chain(angles([PI / 2, PI / 2, 0.0], [0.0, PI / 2, 0.0]), 2, ("nn", "zz"))
    np.testing.assert_allclose(v, [[1.0, 0.0, 0.0, 1.0 / 3.0, 0.0, 0.0]], atol=1e-15)
    # n = 3: z, -z, z.  nn = zz = 1, -1, 1
    v = cr.per_chain(angles([0.0, PI, 0.0], [0.3, 1.0, 2.0]), 2, ("nn", "zz"))
    np.testing.assert_allclose(v, [[1.0, -1.0, 1.0, 1.0, -1.0, 1.0]], atol=1e-15)
    # planar: (1, 0), (0, 1): the field axis is component 2
    v = cr.per_chain(angles([0.0, 0.0], [0.0, PI / 2]), 1, ("nn", "zz"), planar=True)
    np.testing.assert_allclose(v, [[1.0, 0.0, 0.5, 0.0]], atol=1e-15)


def test_twin_on_a_straight_and_on_an_alternating_chain():
    n = 9
    v = cr.per_chain(angles([0.7] * n, [1.1] * n), n - 1, ("nn",))
    np.testing.assert_allclose(v, np.ones((1, n)), atol=4e-16)
    # alternating n, -n: (theta, phi) -> (pi - theta, phi + pi)
    th = [0.7 if i % 2 == 0 else PI - 0.7 for i in range(n)]
    ph = [1.1 if i % 2 == 0 else 1.1 + PI for i in range(n)]
    v = cr.per_chain(angles(th, ph), n - 1, ("nn",))
    np.testing.assert_allclose(v, [[(-1.0) ** k for k in range(n)]], atol=1e-15)
    # planar alternating
    v = cr.per_chain(angles([0.0] * n, [0.4 if i % 2 == 0 else 0.4 + PI for i in range(n)]), n - 1, ("nn",), planar=True)
    np.testing.assert_allclose(v, [[(-1.0) ** k for k in range(n)]], atol=1e-15)


def test_twin_dipole_channel_by_hand():
    E0, K1, K2, mu = 2.0, 0.75, 0.25, 1.5
    a, b = (K1 - K2) * E0, K2 * E0          # 1.0, 0.5
    # n = 2: monomer 0 along z: mu_0 = (0, 0, a + b); monomer 1 along x: cos theta = 0, mu_1 = (0, 0, b)
    v = cr.per_chain(angles([0.0, PI / 2], [0.0, 0.0]), 1, ("mm",), E0=E0, K1=K1, K2=K2)
    np.testing.assert_allclose(v, [[((a + b) ** 2 + b * b) / 2, (a + b) * b]], atol=1e-15)
    # a monomer at 60 degrees from z in the xz plane: mu = a cos (sin, 0, cos) + (0, 0, b)
    c, s = np.cos(PI / 3), np.sin(PI / 3)
    v = cr.per_chain(angles([PI / 3], [0.0]), 0, ("mm",), E0=E0, K1=K1, K2=K2)
    np.testing.assert_allclose(v, [[(a * c * s) ** 2 + (a * c * c + b) ** 2]], atol=1e-15)
    # planar dielectric: n = (cos phi, sin phi), mu = a sin phi n + (0, b)
    phi = 0.9
    v = cr.per_chain(angles([0.0, 0.0], [phi, PI / 2]), 1, ("mm",), planar=True, E0=E0, K1=K1, K2=K2)
    m0 = np.array([a * np.sin(phi) * np.cos(phi), a * np.sin(phi) ** 2 + b])
    m1 = np.array([0.0, a + b])
    np.testing.assert_allclose(v, [[(m0 @ m0 + m1 @ m1) / 2, m0 @ m1]], atol=1e-15)
    # polar: mm = mu^2 nn
    th, ph = [0.3, 1.2, 2.0, 0.9], [0.1, 2.2, 4.0, 5.5]
    vm = cr.per_chain(angles(th, ph), 3, ("mm",), polar=True, mu=mu, E0=E0, K1=K1, K2=K2)
    vn = cr.per_chain(angles(th, ph), 3, ("nn",))
    np.testing.assert_allclose(vm, mu * mu * vn, rtol=1e-15, atol=1e-15)
    assert cr.scale("mm", E0=E0, K1=K1, K2=K2) == (abs(a) + abs(b)) ** 2 and cr.scale("mm", mu=mu, polar=True) == mu * mu
    assert cr.scale("nn") == 1.0 and cr.scale("zz", E0=5.0) == 1.0


def test_twin_columns_and_totals():
    rng = np.random.default_rng(3)
    a = np.concatenate([rng.uniform(0, PI, (5, 4)), rng.uniform(-7, 7, (5, 4))], axis=1)
    v = cr.per_chain(a, 2, ("mm", "nn"), E0=1.0, K1=0.5, K2=0.2)          # the order is nn, zz, mm whatever is asked
    assert v.shape == (5, 6)
    np.testing.assert_array_equal(v[:, :3], cr.per_chain(a, 2, ("nn",)))
    np.testing.assert_array_equal(v[:, 3:], cr.per_chain(a, 2, ("mm",), E0=1.0, K1=0.5, K2=0.2))
    s, q = cr.totals(v)
    np.testing.assert_allclose(s, v.sum(axis=0)) and np.testing.assert_allclose(q, (v ** 2).sum(axis=0))
    np.testing.assert_allclose(v[:, 0], 1.0, atol=4e-16)


# ---------------------------------------------------------------------------------------------- the fixture
@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_corr_closed_form", os.path.join(ROOT, "tests", "golden", "make_corr_closed_form.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_fixture_is_what_the_generator_gives(gen):
    with open(os.path.join(ROOT, "tests", "golden", "corr_closed_form.json")) as f:
        golden = json.load(f)
    fresh = gen.closed_forms()
    assert {k for k in golden if not k.startswith("_")} == set(fresh) == {"bending", "fixed_force", "planar"}
    for name in fresh:
        assert golden[name]["params"] == fresh[name]["params"]
        for ch, want in fresh[name]["expect"].items():
            np.testing.assert_allclose(golden[name]["expect"][ch], want, rtol=1e-12, atol=0)
    assert abs(golden["bending"]["cos_psi"] - 0.63387114) < 5e-9
    np.testing.assert_allclose(golden["bending"]["expect"]["nn"][:3], [1.0, 0.63387114, 0.63387114 ** 2], rtol=1e-7)
    # planar, E0 = 0, F = 1 along the field axis: <n> = (0, I1(1) / I0(1))
    np.testing.assert_allclose(golden["planar"]["expect"]["nn"][1], 0.44638999 ** 2, rtol=1e-6)


# ---------------------------------------------------------------------------------------------- the tool's refusals
def test_sweep_refuses_corr_where_it_refuses_hist(tmp_path):
    """No GPU work is started: every refusal comes before the ensemble is made."""
    base = [sys.executable, os.path.join(ROOT, "tools", "run_sweep.py"), str(tmp_path / "x"), "--axis", "n=8", "--axis", "Fz=0,1"]
    tail = ["--", "--num-steps", "6400", "--stepout", "100"]
    for extra, more, needle in ((["--corr", "5", "--csv"], [], "--csv"), (["--corr", "5", "--gpus", "2"], [], "one device"),
                                (["--corr", "5", "--error-bars", "32"], [], "--error-bars"),
                                (["--corr", "5", "--hist", "r3:-8:8:32"], [], "--hist"),
                                (["--corr", "5"], ["--umbrella-sampling"], "umbrella"), (["--corr", "5"], ["--num-inits", "2"], "num-inits"),
                                (["--corr", "5:nn,xx"], [], "not understood"), (["--corr", "8"], [], "n - 1"),
                                (["--corr", "5"], ["--stepout", "5000"], "--stepout")):
        r = subprocess.run(base + extra + tail + more, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and needle in r.stderr, (extra, more, r.stderr[-500:])
    assert not (tmp_path / "x").exists() or not os.listdir(tmp_path / "x")
