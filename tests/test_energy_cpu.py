"""The energy recorder without a GPU: the seven entry points' declarations, exports and argument errors; the numpy
twin of the contract (tests/energy_ref.py) against independent statements of the same energy -- the oracle's chain and pair
energies, the planar restatement, closed forms by hand; the closed-form fixture, its generator and directly sampled chains;
the sweep tool's --energy strings and refusals."""
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

import energy_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["pstat_energy_open", "pstat_energy_record", "pstat_advance_energy", "pstat_energy_read", "pstat_energy_rows",
                "pstat_energy_clear", "pstat_energy_close"]
PI = np.pi
FOURPI = 4.0 * 3.14159265358979323846


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
    assert re.search(r"typedef struct pstat_energy_spec \{\s*int32_t max_sep, reserved;\s*double cutoff;\s*\} pstat_energy_spec;", header)
    assert C.sizeof(ps._lib.EnergySpec) == 16 and ps._lib.EnergySpec.cutoff.offset == 8
    for name in ("ENERGY_NAMES", "Energy", "EnergyResult"):
        assert name in ps.__all__ and hasattr(ps, name), name
    assert ps.ENERGY_NAMES == ("field", "work", "bend")
    assert hasattr(ps.Ensemble, "open_energy") and hasattr(ps.Ensemble, "advance_energy")
    listed = header[header.index("Like every accessor that"):header.index("int pstat_summary_get")]
    assert "pstat_energy_read" in listed and "pstat_energy_rows" in listed
    contract = header[header.index("The energy by term and separation on the device"):header.index("typedef struct pstat_energy_spec")]
    for word in ("FOURPI", "model total", "PSTAT_CUTOFF          within alone", "r2 > crad2", "1280", "1920"):
        assert word in contract, word


def test_null_arguments_are_refused_before_a_device_is_touched(ps):
    lib = ps._lib.load()
    out, ptr, n64 = C.c_void_p(), C.c_void_p(), C.c_int64(0)
    spec = ps._lib.EnergySpec(-1, 0, 0.0)
    assert lib.pstat_energy_open(None, C.byref(spec), None, 0, C.byref(out)) == -1 and b"null" in lib.pstat_last_error()
    assert lib.pstat_energy_record(None, None) == -1 and lib.pstat_advance_energy(None, None, 1, 1) == -1
    assert lib.pstat_energy_read(None, None, None, None, None) == -1 and lib.pstat_energy_clear(None, None) == -1
    assert lib.pstat_energy_rows(None, None, C.byref(ptr), C.byref(n64), C.byref(n64)) == -1
    lib.pstat_energy_close(None, None)


# what: (handle parameters, arguments, return code, what the message names); the handle has n = 6 unless said otherwise
BAD = {
    "null spec": ({}, dict(spec=None), -1, "null"),
    "null out": ({}, dict(out=None), -1, "null"),
    "max_sep -2": ({}, dict(max_sep=-2), -1, "max_sep"),
    "max_sep n": ({}, dict(max_sep=6), -1, "max_sep"),
    "max_sep 1 at n 1": (dict(n=1), dict(max_sep=1), -1, "max_sep"),
    "reserved 1": ({}, dict(reserved=1), -1, "reserved"),
    "cutoff -1": ({}, dict(cutoff=-1.0), -1, "cutoff"),
    "cutoff inf": ({}, dict(cutoff=float("inf")), -1, "cutoff"),
    "cutoff NaN": ({}, dict(cutoff=float("nan")), -1, "cutoff"),
    "cutoff per case NaN": ({}, dict(cutoff=1.0, cutoff_per_case=[float("nan")]), -1, "cutoff_per_case"),
    "cutoff per case -1": ({}, dict(cutoff_per_case=[-1.0]), -1, "case 0"),
    "negative capacity": ({}, dict(capacity_rows=-1), -1, "capacity_rows"),
    "umbrella": (dict(umbrella=1), {}, -4, "whose gauge the sums do not hold"),
    "n beyond LDS": (dict(n=1281), {}, -4, "1280"),
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
    a = dict(max_sep=-1, reserved=0, cutoff=0.0, cutoff_per_case=None, capacity_rows=0, out=C.byref(out))
    a.update(kw)
    ca = np.ascontiguousarray(a["cutoff_per_case"], dtype=np.float64) if a["cutoff_per_case"] is not None else None
    cp = ca.ctypes.data_as(C.POINTER(C.c_double)) if ca is not None else None
    spec = ps._lib.EnergySpec(a["max_sep"], a["reserved"], a["cutoff"])
    sp = C.byref(spec) if "spec" not in a else a["spec"]
    if rc == -2:
        assert lib.pstat_device_count() == 0
        assert lib.pstat_energy_open(None, sp, cp, a["capacity_rows"], a["out"]) == -1
        return
    try:
        assert lib.pstat_energy_open(h, sp, cp, a["capacity_rows"], a["out"]) == code, lib.pstat_last_error()
        assert needle.encode() in lib.pstat_last_error(), lib.pstat_last_error()
    finally:
        lib.pstat_destroy(h)


def test_python_refuses_misshapen_options_and_states_the_model(ps):
    import polymer_stats_amd.ensemble as en
    e = object.__new__(en.Ensemble)
    e.planar, e.ncases, e.n = False, 3, 8
    e.cases = [ps.default_params(n=8) for _ in range(3)]
    with pytest.raises(ValueError):
        en.Ensemble.open_energy(e, cutoff=[1.0, 2.0])                # two radii for three cases
    with pytest.raises(ValueError):
        en.Ensemble.open_energy(e, cutoff=[[1.0, 2.0, 3.0]])
    assert en.energy_model_columns(ps.NONINTERACTING, 5, True) == [0, 1, 2]
    assert en.energy_model_columns(ps.ISING, 5, False) == [0, 1, 2, 3]
    assert en.energy_model_columns(ps.INTERACTING, 5, True) == list(range(9))            # every pair column and rest, not within
    assert en.energy_model_columns(ps.CUTOFF, 5, True) == [9]
    with pytest.raises(ValueError, match="within"):
        en.energy_model_columns(ps.CUTOFF, 5, False)
    for t in range(4):
        assert en.energy_model_columns(t, 5, True) == er.model_columns(t, 5, 1.5)


def test_result_views_and_model(ps):
    s = np.array([[-4.0, -2.0, 1.0, 0.5, 0.25, 0.125, 3.0], [-8.0, -4.0, 2.0, 1.0, 0.5, 0.25, 6.0]])      # max_sep 2, rest, within
    types = [ps.INTERACTING, ps.INTERACTING]
    res = ps.EnergyResult(2, np.array([1.5, 1.5]), types, 2, s, s * s, 1)
    assert res.has_within and res.pair.shape == (2, 2)
    np.testing.assert_array_equal(res.field, [-2.0, -4.0])
    np.testing.assert_array_equal(res.pair[1], [0.5, 0.25])
    np.testing.assert_array_equal(res.rest, [0.0625, 0.125])
    np.testing.assert_array_equal(res.within, [1.5, 3.0])
    np.testing.assert_array_equal(res.model_sum, [-4.0 - 2.0 + 1.0 + 0.5 + 0.25 + 0.125, -8.0 - 4.0 + 2.0 + 1.0 + 0.5 + 0.25])
    np.testing.assert_array_equal(res.model, res.model_sum / 2)
    cut = ps.EnergyResult(2, np.array([1.5, 1.5]), [ps.CUTOFF] * 2, 2, s, s * s, 1)
    np.testing.assert_array_equal(cut.model_sum, [3.0, 6.0])
    bare = ps.EnergyResult(2, np.zeros(2), [ps.CUTOFF] * 2, 2, s[:, :6], s[:, :6] ** 2, 1)
    assert not bare.has_within and bare.within is None
    with pytest.raises(ValueError):
        bare.model_sum
    with pytest.raises(ValueError):
        bare.model
    ising = ps.EnergyResult(2, np.zeros(2), [ps.ISING, ps.NONINTERACTING], 2, s[:, :6], s[:, :6] ** 2, 1)
    np.testing.assert_array_equal(ising.model_sum, [-4.5, -10.0])


# ---------------------------------------------------------------------------------------------- the twin against independent statements
def random_angles(rng, C_, n):
    return np.concatenate([np.arccos(rng.uniform(-1, 1, (C_, n))), rng.uniform(-PI, PI, (C_, n))], axis=1)


@pytest.mark.parametrize("chain_type", [0, 1], ids=["dielectric", "polar"])
@pytest.mark.parametrize("energy_type", [0, 1, 2, 3], ids=["non-interacting", "interacting", "Ising", "cutoff"])
@pytest.mark.parametrize("n", [2, 3, 12])
def test_twin_model_total_is_the_oracles_chain_energy(n, energy_type, chain_type):
    """Random angles: the twin's model total against oracle.binding.chain_energy, which adds the terms chain by chain in its own
    order (and knows the bending term and UCutoff), within the derived bound of the columns involved."""
    from oracle import binding as ob
    rng = np.random.default_rng(100 * n + 10 * energy_type + chain_type)
    a = random_angles(rng, 8, n)
    phys = dict(E0=1.3, K1=0.8, K2=0.3, mu=0.9, Fz=0.4, Fx=-0.3, b=1.2, bend_mod=0.6, bend_angle=0.3)
    case = er.Case(chain_type=chain_type, **phys)
    rcut = 1.7
    p = ob.make_params(n=n, chain_type=chain_type, energy_type=energy_type, cutoff_radius=rcut, **phys)
    cutoff = rcut if energy_type == er.CUTOFF else 0.0
    tw = er.per_chain(a, case, -1, cutoff)
    assert tw.undecided.sum() == 0
    E = er.value_bounds(tw, case, n, -1, cutoff)
    cols = er.model_columns(energy_type, n - 1, cutoff)
    model = er.model_values(tw, energy_type, n - 1, cutoff)
    worst = 0.0
    for c in range(len(a)):
        U, _, _ = ob.chain_energy(p, a[c, n:], a[c, :n])
        bound = E[c, cols].sum() + (len(cols) + 2) * er.U * tw.absum[c]
        worst = max(worst, abs(U - model[c]) / bound)
        assert abs(U - model[c]) <= bound, (c, U, model[c], bound)
    print(f"n = {n}, energy {energy_type}, chain {chain_type}: largest |oracle - twin| / bound = {worst:.3g}")


@pytest.mark.parametrize("n", [2, 3, 12])
def test_twin_bend_column_is_the_three_line_loop(n):
    rng = np.random.default_rng(7 + n)
    a = random_angles(rng, 5, n)
    case = er.Case(E0=0.7, bend_mod=1.1, bend_angle=0.4)
    tw = er.per_chain(a, case)
    for c in range(5):
        nh = er.unit_vectors(a[c:c + 1])[0]
        want = 0.0
        for i in range(n - 1):
            want += 1.1 / 2 * (math.acos(min(1.0, max(-1.0, float(np.dot(nh[i], nh[i + 1]))))) - 0.4) ** 2
        assert abs(tw.values[c, 2] - want) <= er.value_bounds(tw, case, n)[c, 2]
    flat = er.per_chain(a, case._replace(bend_mod=0.0))
    assert np.all(flat.values[:, 2] == 0.0) and np.all(er.value_bounds(flat, case._replace(bend_mod=0.0), n)[:, 2] == 0.0)


@pytest.mark.parametrize("chain_type", [0, 1], ids=["dielectric", "polar"])
@pytest.mark.parametrize("n", [2, 3, 12])
def test_twin_pair_sums_are_the_oracles_pair_energy(n, chain_type):
    from oracle import binding as ob
    rng = np.random.default_rng(40 + n)
    a = random_angles(rng, 6, n)
    case = er.Case(E0=1.1, K1=0.9, K2=0.2, mu=0.7, b=0.8, chain_type=chain_type)
    tw = er.per_chain(a, case, 1)
    E = er.value_bounds(tw, case, n, 1)
    nh = er.unit_vectors(a)
    xs, mus = er.positions(nh, case.b), er.dipoles(nh, case)
    for c in range(6):
        full, ising = ob.pair_energy(xs[c], mus[c], ising=False), ob.pair_energy(xs[c], mus[c], ising=True)
        assert abs(tw.values[c, 3] - ising) <= E[c, 3]
        assert abs(tw.values[c, 3] + tw.values[c, 4] - full) <= E[c, 3] + E[c, 4] + 2 * er.U * tw.absum[c]
    every = er.per_chain(a, case)                                    # max_sep = n - 1: the same pairs, one column each, rest 0
    assert np.all(every.values[:, n + 2] == 0.0)
    np.testing.assert_allclose(every.values[:, 3:n + 2].sum(axis=1), tw.values[:, 3] + tw.values[:, 4], rtol=0, atol=float(E[:, 3:5].sum()))


@pytest.mark.parametrize("chain_type", [0, 1], ids=["dielectric", "polar"])
@pytest.mark.parametrize("energy_type", [0, 1, 2], ids=["non-interacting", "interacting", "Ising"])
@pytest.mark.parametrize("n", [2, 3, 12])
def test_planar_twin_model_total_is_the_planar_restatement(n, energy_type, chain_type):
    from planar import binding as pb
    rng = np.random.default_rng(900 + 100 * n + 10 * energy_type + chain_type)
    phi = rng.uniform(-PI, PI, (8, n))
    a = np.concatenate([np.zeros((8, n)), phi], axis=1)
    phys = dict(E0=1.3, K1=0.8, K2=0.3, mu=0.9, Fz=0.4, Fx=-0.3, b=1.2)
    case = er.Case(chain_type=chain_type, **phys)
    p = pb.make_params(n=n, chain_type=chain_type, energy_type=energy_type, **phys)
    tw = er.per_chain(a, case, planar=True)
    E = er.value_bounds(tw, case, n)
    cols = er.model_columns(energy_type, n - 1, 0.0)
    model = er.model_values(tw, energy_type, n - 1)
    for c in range(8):
        U = pb.energy(p, phi[c])[0]
        bound = E[c, cols].sum() + (len(cols) + 2) * er.U * tw.absum[c]
        assert abs(U - model[c]) <= bound, (c, U, model[c], bound)
    assert np.all(tw.values[:, 2] == 0.0)                            # the planar main has no bending term


# ---------------------------------------------------------------------------------------------- by hand
def test_dimer_has_a_one_line_closed_form():
    """Two polar monomers, c = n_0 . n_1: d = b (n_0 + n_1) / 2, r^2 = b^2 (1 + c) / 2, mu_i . d = mu b (1 + c) / 2, so
    t = mu^2 (c - 3 (1 + c) / 2) / (4 pi r^3) = -mu^2 (3 + c) / (8 pi r^3)."""
    rng = np.random.default_rng(5)
    a = random_angles(rng, 40, 2)
    case = er.Case(mu=0.8, b=1.3, chain_type=1)
    tw = er.per_chain(a, case)
    nh = er.unit_vectors(a)
    c = (nh[:, 0] * nh[:, 1]).sum(axis=1)
    r = 1.3 * np.sqrt((1 + c) / 2)
    want = -0.64 * (3 + c) / (2 * FOURPI * r ** 3)
    assert tw.values.shape == (40, 5) and np.all(tw.values[:, 4] == 0.0)
    assert np.all(np.abs(tw.values[:, 3] - want) <= er.value_bounds(tw, case, 2)[:, 3] + 8 * er.U * np.abs(want))


@pytest.mark.parametrize("n", [1, 2, 9, 70])
def test_straight_chain(n):
    """theta = 0, K1 E0 = 1, b = 1: mu = z, d = s z, t = (1 - 3) / (4 pi s^3)."""
    a = np.zeros((1, 2 * n))
    a[0, n:] = 0.4
    case = er.Case(E0=2.0, K1=0.5, K2=0.0, Fz=0.3, Fx=0.7, b=1.0, bend_mod=1.2, bend_angle=0.25)
    tw = er.per_chain(a, case, -1, 2.5)
    v = tw.values[0]
    assert v[0] == -n * 2.0 / 2 and v[1] == -0.3 * n
    np.testing.assert_allclose(v[2], (n - 1) * 0.6 * 0.25 ** 2, rtol=1e-15)
    s = np.arange(1, n)
    np.testing.assert_allclose(v[3:n + 2], -2.0 * (n - s) / (FOURPI * s ** 3.0), rtol=1e-14)
    assert v[n + 2] == 0.0
    np.testing.assert_allclose(v[n + 3], sum(-2.0 * (n - k) / (FOURPI * k ** 3.0) for k in (1, 2) if k < n), rtol=1e-14, atol=0)
    assert tw.undecided.sum() == 0                                   # crad2 = 6.25 lies between r2 = 4 and 9
    short = er.per_chain(a, case, min(2, n - 1), 0.0).values[0]
    np.testing.assert_allclose(short[-1], v[3 + min(2, n - 1):n + 2].sum(), rtol=1e-13, atol=0)      # rest is what lies beyond max_sep


def test_two_monomers_on_one_point_poison_their_own_columns_only():
    """n_1 = -n_0 puts x_1 on x_0: pair[1] is not finite, and so are `within` and, when max_sep = 0, `rest`; the other
    separations and field, work, bend stay finite."""
    nh = np.array([[[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]])
    case = er.Case(E0=1.0, K1=0.5, K2=0.2, Fz=0.3, bend_mod=0.5)
    with np.errstate(all="ignore"):
        v = er.per_chain(np.zeros((1, 8)), case, -1, 1.5, nhat=nh).values[0]
        w = er.per_chain(np.zeros((1, 8)), case, 0, 0.0, nhat=nh).values[0]
        u = er.per_chain(np.zeros((1, 8)), case, 1, 0.0, nhat=nh).values[0]
    assert not np.isfinite(v[3]) and not np.isfinite(v[7]) and np.all(np.isfinite(v[[0, 1, 2, 4, 5]])) and v[6] == 0.0
    assert not np.isfinite(w[3]) and np.all(np.isfinite(w[:3])) and w.shape == (4,)
    assert not np.isfinite(u[3]) and np.isfinite(u[4])


def test_bounds_are_the_docstrings():
    rng = np.random.default_rng(3)
    n, u = 6, 2.0 ** -53
    a = random_angles(rng, 4, n)
    case = er.Case(E0=1.5, K1=0.7, K2=0.3, Fz=0.4, Fx=0.3, b=1.3)
    tw = er.per_chain(a, case, 2, 1.5)
    E = er.value_bounds(tw, case, n, 2, 1.5)
    L, mm = n * 1.3, abs((0.7 - 0.3) * 1.5) + abs(0.3 * 1.5)
    assert er.mumax(case) == mm and er.eps_d(n, 1.3, 2) == L * u * 22 + 12 * u * 1.3 * 3 and er.eps_d(130, 1.0, 1) == 130 * u * 30 + 24 * u
    assert np.all(E[:, 0] == 1.5 * mm * n * u * (17 + n)) and np.all(E[:, 1] == 2 * 0.7 * L * u * (n + 14)) and np.all(E[:, 2] == 0.0)
    I, J = np.triu_indices(n, 1)
    x = er.positions(er.unit_vectors(a), 1.3)
    r = np.sqrt(((x[:, J] - x[:, I]) ** 2).sum(axis=2))
    mod = np.sqrt((er.dipoles(er.unit_vectors(a), case) ** 2).sum(axis=2))
    m2, msum = 1.01 * mod[:, I] * mod[:, J], 1.01 * (mod[:, I] + mod[:, J])
    w = (m2 * (46 * er.eps_d(n, 1.3, J - I) / r + 160 * u) + 224 * u * mm * msum) / (FOURPI * r ** 3)
    np.testing.assert_allclose(tw.weight, w, rtol=1e-9)
    np.testing.assert_allclose(E[:, 3], w[:, J - I == 1].sum(axis=1) + 2 * 15 * u * tw.abscols[:, 3], rtol=1e-9)
    np.testing.assert_allclose(E[:, 5], w[:, J - I > 2].sum(axis=1) + 2 * 15 * u * tw.abscols[:, 5], rtol=1e-9)
    b1, b2 = er.bounds(tw, case, n, 4, 2, 1.5)
    np.testing.assert_allclose(b1, E.sum(axis=0) + 8 * u * np.abs(tw.values).sum(axis=0), rtol=1e-15)
    assert np.all(np.delete(b2, 2) > 0) and b2[2] == 0.0 and tw.absum.shape == (4,)      # (no bending: the column is 0.0 on both sides)
    np.testing.assert_allclose(tw.absum, tw.abscols[:, :6].sum(axis=1), rtol=1e-14)


# ---------------------------------------------------------------------------------------------- the fixture
@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_energy_closed_form", os.path.join(ROOT, "tests", "golden", "make_energy_closed_form.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "energy_closed_form.json")) as f:
        return json.load(f)


CASES = ["fixed_force", "polar", "planar", "bend"]


def test_fixture_is_what_the_generator_gives(gen, golden):
    fresh = gen.generate()
    assert set(golden) == set(fresh) == set(CASES)
    for name in fresh:
        assert golden[name]["params"] == fresh[name]["params"] and golden[name]["planar"] == fresh[name]["planar"]
        assert set(golden[name]["expect"]) == set(fresh[name]["expect"])
        for col, want in fresh[name]["expect"].items():
            np.testing.assert_allclose(golden[name]["expect"][col], want, rtol=1e-12, atol=1e-16)
    assert "infinite" in gen.__doc__ and "r dr" in gen.__doc__      # why no pair column is judged statistically
    # the free rotor at kappa = 2: <kappa psi^2 / 2> per bond is below kT (the sin psi measure's share is bounded by pi)
    assert 0.5 < golden["bend"]["expect"]["bend"] / 11 < 1.0
    # a polar chain in a field along the force: <field> = -n E0 mu <n_z> / 2 and <work> = -n b Fz <n_z>, the same Langevin <n_z>
    pol = golden["polar"]["expect"]
    f = 1.0 * 1.0 / 2 + 1.0                                          # E0 mu / (2 kT) + Fz b / kT
    langevin = 1 / math.tanh(f) - 1 / f
    np.testing.assert_allclose([pol["field"], pol["work"]], [-20 * 0.5 * langevin, -20 * langevin], rtol=1e-10)


def case_of(c):
    return er.Case(**{k: v for k, v in c["params"].items() if k in er.Case._fields})


def sample_monomers(c, planar, N, rng):
    """[N, 2n] angles of N chains of iid monomers from rho ~ (sin theta) exp(-(u - b F . n) / kT), by rejection from the uniform
    distribution on the sphere (the circle)."""
    case, n, kT = case_of(c), c["params"]["n"], c["params"].get("kT", 1.0)
    need, th, ph = N * n, [], []
    bound = (abs(case.E0) / 2 * er.mumax(case) + abs(case.b) * (abs(case.Fx) + abs(case.Fz))) / kT      # -w / kT <= bound
    while need > 0:
        m = 4 * need + 1000
        t = np.zeros(m) if planar else np.arccos(rng.uniform(-1, 1, m))
        p = rng.uniform(0, 2 * PI, m)
        nh = er.unit_vectors(np.stack([t, p], axis=1), planar)[:, 0, :]
        mu = er.dipoles(nh[:, None, :], case)[:, 0, :]
        w = -0.5 * case.E0 * mu[:, 2] - case.b * (case.Fx * nh[:, 0] + case.Fz * nh[:, 2])
        keep = rng.random(m) < np.exp(-w / kT - bound)
        th.append(t[keep][:need])
        ph.append(p[keep][:need])
        need -= len(th[-1])
    return np.concatenate([np.concatenate(th).reshape(N, n), np.concatenate(ph).reshape(N, n)], axis=1)


def sample_free_rotor(c, N, rng):
    """[N, 2n] angles of N freely rotating chains: bond angles iid ~ exp(-kappa psi^2 / (2 kT)) sin psi by rejection, each new
    monomer at that angle from the last one and a uniform azimuth around it."""
    n, k, kT = c["params"]["n"], c["params"]["bend_mod"], c["params"]["kT"]
    need, psis = N * (n - 1), []
    while need > 0:
        x = rng.uniform(0, PI, 4 * need + 1000)
        keep = rng.random(len(x)) < np.exp(-k * x * x / (2 * kT)) * np.sin(x)
        psis.append(x[keep][:need])
        need -= len(psis[-1])
    psi = np.concatenate(psis).reshape(N, n - 1)
    v = rng.normal(size=(N, 3))
    nh = [v / np.linalg.norm(v, axis=1, keepdims=True)]
    for i in range(n - 1):
        cur = nh[-1]
        t = rng.normal(size=(N, 3))
        t -= (t * cur).sum(axis=1, keepdims=True) * cur
        t /= np.linalg.norm(t, axis=1, keepdims=True)
        nh.append(np.cos(psi[:, i:i + 1]) * cur + np.sin(psi[:, i:i + 1]) * t)
    nh = np.stack(nh, axis=1)
    return np.concatenate([np.arccos(np.clip(nh[:, :, 2], -1, 1)), np.arctan2(nh[:, :, 1], nh[:, :, 0])], axis=1)


@pytest.mark.parametrize("name", CASES)
def test_directly_sampled_chains_meet_the_fixture(golden, name):
    """50 000 chains per case, drawn in numpy with a fixed seed, through the twin, judged by energy_ref.judge, the judge of
    tests/test_gpu_energy.py: field, work and bend within 5 of their across-chain standard errors of the closed form, that error at
    most 2 % of the value.  So the reference statement alone stays inside the judge."""
    c = golden[name]
    N, rng = 50000, np.random.default_rng(20261021)
    a = sample_free_rotor(c, N, rng) if name == "bend" else sample_monomers(c, c["planar"], N, rng)
    tw = er.per_chain(a, case_of(c), 0, 0.0, c["planar"])
    mean, se = tw.values.mean(axis=0), tw.values.std(axis=0, ddof=1) / np.sqrt(N)
    for i, col in enumerate(("field", "work", "bend")):
        if col in c["expect"]:
            z, rel = er.judge(f"{name} {col}", mean[i], se[i], c["expect"][col])
            print(f"{name} {col}: mean {mean[i]:.5f}, closed form {c['expect'][col]:.5f}, |z| = {z:.2f}, stderr / value = {100 * rel:.3f} %")


# ---------------------------------------------------------------------------------------------- the tool's strings and refusals
def test_parse_of_energy_strings():
    from polymer_stats_amd import sweep as sw
    assert sw.parse_energy("5") == ("energy", dict(max_sep=5, cutoff=None))
    assert sw.parse_energy("-1,cut=1.5") == ("energy", dict(max_sep=-1, cutoff=1.5))
    assert sw.parse_energy(" 0 , cut=7.5 ")[1] == dict(max_sep=0, cutoff=7.5)
    for bad in ("", "x", "-2", "5,cut", "5,cut=0", "5,cut=-1", "5,cut=inf", "5,cut=nan", "5,sep=2", "5,cut=1,cut=2", "5:2", "1.5"):
        with pytest.raises(sw.ReferenceError_, match="not understood"):
            sw.parse_energy(bad)
    from polymer_stats_amd import _host
    row = _host.RECORDING_KINDS["energy"]
    assert (row.flag, row.ext) == ("--energy", ".energy") and list(_host.RECORDING_KINDS)[-1] == "energy"
    assert list(_host.RECORDING_KINDS)[:-1] == list(_host.RECORDINGS) and row.words[3] == _host.RECORDINGS["pdist"].words[3]


def test_sweep_refuses_energy_where_it_refuses_pdist(tmp_path):
    """No GPU work is started: every refusal comes before the ensemble is made, under --dry-run too."""
    base = [sys.executable, os.path.join(ROOT, "tools", "run_sweep.py"), str(tmp_path / "x"), "--dry-run", "--axis", "n=8", "--axis", "Fz=0,1"]
    tail = ["--", "--num-steps", "6400", "--stepout", "100"]
    P = ["--energy", "5,cut=1.5"]
    for extra, more, needle in ((P + ["--csv"], [], "--energy cannot be combined with --csv"), (P + ["--gpus", "2"], [], "one device"),
                                (P + ["--error-bars", "32"], [], "--error-bars"), (P + ["--hist", "r3:-8:8:32"], [], "--hist"),
                                (P + ["--corr", "5"], [], "--corr"), (P + ["--shape", "z:6:8"], [], "--shape"),
                                (P + ["--pdist", "4:16"], [], "--energy cannot be combined with --pdist"),
                                (P, ["--umbrella-sampling"], "whose gauge the sums do not hold"), (P, ["--num-inits", "2"], "num-inits"),
                                (["--energy", "x"], [], "not understood"), (["--energy", "8"], [], "n - 1"),
                                (P, ["--stepout", "5000"], "--stepout"), (P, ["--numeric-type", "float32"], "float64")):
        r = subprocess.run(base + extra + tail + more, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and needle in r.stderr, (extra, more, r.stderr[-500:])
        assert "Traceback" not in r.stderr, r.stderr[-800:]
    ok = subprocess.run(base + P + tail, capture_output=True, text=True, timeout=120)
    assert ok.returncode == 0, ok.stderr[-500:]
    assert not (tmp_path / "x").exists() or not os.listdir(tmp_path / "x")


def test_energy_lines_on_hand_made_results(ps):
    from polymer_stats_amd import _host
    s = np.array([[-4.0, -2.0, 1.0, 0.5, 0.25, 0.125, 3.0]])
    res = ps.EnergyResult(2, np.array([1.5]), [ps.ISING], 2, s, s * s, 1)

    class EB:
        stderr = np.arange(7.0)[None, :] / 10

    class MEB:
        stderr = np.array([0.77])
    lines = _host.energy_lines(res, EB, MEB, 0)
    assert lines == ["name,x,value,stderr", "field,,-2.0,0.0", "work,,-1.0,0.1", "bend,,0.5,0.2", "pair,1,0.25,0.3", "pair,2,0.125,0.4",
                     "rest,,0.0625,0.5", "within,1.5,1.5,0.6", "model,,-2.25,0.77"]
    bare = ps.EnergyResult(0, np.zeros(1), [ps.NONINTERACTING], 2, s[:, :4], s[:, :4] ** 2, 1)
    assert [ln.split(",")[0] for ln in _host.energy_lines(bare, EB, MEB, 0)] == ["name", "field", "work", "bend", "rest", "model"]
