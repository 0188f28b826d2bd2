"""CPU tests of the planar (2D) clustering main: the ABI entry point and its argument checking, the CPU restatement
(tests/planar/planar_ref.c) against hand arithmetic and against closed-form single-monomer integrals, the host's option
table, the sweep plan of the reference's 880-case grid and the (unexecuted) Julia host."""
import ctypes as C
import json
import math
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ps():
    import polymer_stats_amd as ps
    ps._lib.load()
    return ps


@pytest.fixture(scope="module")
def pb():
    from planar import binding
    binding.lib()
    return binding


# ------------------------------------------------------------------------------------------------ 1. the entry point

def test_create_planar_is_exported_declared_and_listed(ps):
    lib = ps._lib.load()
    assert hasattr(lib, "pstat_create_planar"), "libpstat.so does not export pstat_create_planar"
    header = open(os.path.join(ROOT, "include", "pstat.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+pstat_create_planar\s*\(\s*const\s+pstat_params\s*\*\s*cases\s*,\s*int32_t\s+ncases\s*,"
                     r"\s*void\s*\*\s*stream\s*,\s*pstat_handle\s*\*\*\s*out\s*\)\s*;", code)
    assert "pstat_create_planar" in ps._lib.SYMBOLS
    assert lib.pstat_abi_version() == 6 and "#define PSTAT_ABI_VERSION 6" in header
    assert ps.PLANAR_OBS_NAMES == ["r1", "r3", "r1sq", "r3sq", "rsq", "p1", "p3", "p1sq", "p3sq", "psq", "U", "Usq"]
    assert [ps.OBS_NAMES[i] for i in ps.PLANAR_OBS_INDEX] == ps.PLANAR_OBS_NAMES
    p = ps.default_planar_params(n=25)
    assert p.adj_ub == 0.40 and p.n == 25 and p.adj_lb == 0.15 and p.cluster_prob == 0.5     # 2D/mcmc_clustering_eap_chain.jl:71-82


# ------------------------------------------------------------------------------------------------ 2. argument checking

def _create(ps, **kw):
    lib = ps._lib.load()
    h = C.c_void_p()
    p = ps.default_planar_params(**kw)
    rc = lib.pstat_create_planar(C.byref(p), 1, None, C.byref(h))
    msg = lib.pstat_last_error().decode()
    if rc == 0:
        lib.pstat_destroy(h)
    return rc, msg


def test_argument_checking_comes_before_the_device(ps):
    lib = ps._lib.load()
    # options the planar main does not have: the field is named
    for field, bad in (("do_flips", 1), ("bend_mod", 0.5), ("bend_angle", 0.1), ("use_x0", 1)):
        rc, msg = _create(ps, **{field: bad})
        assert rc == -1 and field in msg, (field, rc, msg)
    for bad in (dict(n=0), dict(kT=-1.0), dict(chain_type=7), dict(energy_type=9), dict(num_chains=0), dict(precision=5),
                dict(phi_step=0.0), dict(rng=3), dict(uniform_bits=1), dict(cluster_prob=1.5), dict(energy_type=ps.CUTOFF)):
        rc, msg = _create(ps, **bad)
        assert rc == -1 and msg, (bad, rc, msg)
    # valid options of the reference that the device lacks
    for bad in (dict(precision=ps.F32), dict(precision=ps.Q16), dict(energy_type=ps.INTERACTING), dict(n=2561)):
        rc, msg = _create(ps, **bad)
        assert rc == -4 and msg, (bad, rc, msg)
    assert "2560" in _create(ps, n=2561)[1]
    # ignored fields may hold anything; valid parameters reach the device
    want = 0 if lib.pstat_device_count() > 0 else -2
    for ok in (dict(), dict(theta_step=123.0, x0_phi=1.0, dx0_theta=9.0, cutoff_radius=-1.0, move_set=0),
               dict(move_set=1, energy_type=ps.ISING, chain_type=ps.POLAR, umbrella=1, uniform_bits=23, n=2560)):
        rc, msg = _create(ps, num_chains=8, **ok)
        assert rc == want, (ok, rc, msg)
    h = C.c_void_p()
    assert lib.pstat_create_planar(None, 1, None, C.byref(h)) == -1


def test_product_never_touches_the_planar_restatement():
    """The rule of test_product_never_touches_the_oracle for tests/planar: the package, the Julia hosts, tools/ and bench.py
    neither import nor name it."""
    for top in ("polymer_stats_amd", "julia", "tools", "include"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith((".py", ".hip", ".h", ".cpp", ".jl", ".sh", "Makefile")):
                    text = open(os.path.join(dirpath, f), errors="ignore").read()
                    assert "planar_ref" not in text.replace("tests/planar/planar_ref.c", ""), (top, f)
                    assert "from planar" not in text and "import planar" not in text, (top, f)
    for f in ("bench.py", "__graft_entry__.py"):
        text = open(os.path.join(ROOT, f)).read()
        assert "planar_ref" not in text and "from planar" not in text, f
    out = subprocess.check_output(["ldd", os.path.join(ROOT, "polymer_stats_amd", "libpstat.so")]).decode()
    assert "planar" not in out


# ------------------------------------------------------------------------------------------------ 3. hand checks

def _hand(kw, phi):
    """mu, u, r, p, U of the chain phi from the formulas of the issue, in numpy."""
    phi = np.asarray(phi, dtype=float)
    nh = np.stack([np.cos(phi), np.sin(phi)], axis=1)
    E0, b = kw.get("E0", 0.0), kw.get("b", 1.0)
    if kw.get("chain_type", 0) == 0:
        K1, K2 = kw.get("K1", 1.0), kw.get("K2", 0.0)
        mu = (K1 - K2) * E0 * np.sin(phi)[:, None] * nh + np.array([0.0, K2 * E0])
    else:
        mu = kw.get("mu", 1e-2) * nh
    us = -0.5 * E0 * mu[:, 1]
    xs = b * (np.cumsum(nh, axis=0) - 0.5 * nh)
    r, p = b * nh.sum(axis=0), mu.sum(axis=0)

    def pair(i, j):
        d = xs[i] - xs[j]
        rm = np.linalg.norm(d)
        rh = d / rm
        return (mu[i] @ mu[j] - 3 * (mu[i] @ rh) * (mu[j] @ rh)) / (4 * math.pi * rm ** 3)

    n = len(phi)
    et = kw.get("energy_type", 0)
    up = 0.0
    if et == 2:
        up = sum(pair(i, i + 1) for i in range(n - 1))
    elif et == 1:
        up = sum(pair(i, j) for i in range(n) for j in range(i + 1, n))
    U = us.sum() + up - (kw.get("Fx", 0.0) * r[0] + kw.get("Fz", 0.0) * r[1])
    return mu, us, r, p, U


@pytest.mark.parametrize("chain_type", [0, 1], ids=["dielectric", "polar"])
@pytest.mark.parametrize("energy_type", [0, 1, 2], ids=["noninteracting", "interacting", "Ising"])
@pytest.mark.parametrize("phi", [[0.3, 2.1], [0.3, 2.1, -1.2], [math.pi / 2, math.pi / 2, 0.0]], ids=["n2", "n3", "n3_axes"])
def test_restatement_energy_by_hand(pb, chain_type, energy_type, phi):
    kw = dict(E0=0.8, K1=1.3, K2=0.4, mu=0.7, Fz=0.6, Fx=-0.35, b=1.25, kT=0.9, chain_type=chain_type, energy_type=energy_type)
    P = pb.make_params(n=len(phi), **kw)
    mu, us, r, p, U = _hand(kw, phi)
    for i, f in enumerate(phi):
        np.testing.assert_allclose(pb.dipole(P, f), mu[i], rtol=1e-13, atol=1e-15)
    Ur, rr, pr, usr = pb.energy(P, phi)
    np.testing.assert_allclose(rr, r, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(pr, p, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(usr, us.sum(), rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(Ur, U, rtol=1e-12, atol=1e-14)
    if phi[0] == math.pi / 2:      # monomers along the field: dielectric mu = (0, K1 E0), u = -K1 E0^2 / 2; polar (0, mu), u = -E0 mu / 2
        want = [0.0, 1.3 * 0.8] if chain_type == 0 else [0.0, 0.7]
        np.testing.assert_allclose(pb.dipole(P, phi[0]), want, atol=1e-15)


def test_restatement_cluster_flip_by_hand(pb):
    link = lambda a, b: (1 + math.cos(a - b)) / 2                      # (1 + n_i . n_j) / 2
    # a chain of equal phi: every link has p = 1, the whole chain joins whatever the draws, and flipping it gives
    # alpha = 1 (both ends of the cluster are chain ends)
    P = pb.make_params(n=6, cluster_prob=1.0)
    phi = [0.7] * 6
    alpha, after, lo, up, flipped, used = pb.cluster_flip(P, phi, 2, [0.4] + [0.999999] * 10)
    assert (lo, up, flipped, alpha) == (0, 5, True, 1.0)
    assert used == 1 + 3 + 2                                           # flip draw, links 2-3, 3-4, 4-5 above, 2-1, 1-0 below
    np.testing.assert_array_equal(after, np.array(phi) + math.pi)      # flip_n!: phi += pi
    # n = 3, cluster {2} (1-based): both links fail
    phi = [0.3, 1.1, 2.4]
    pu, pl = link(phi[1], phi[2]), link(phi[1], phi[0])
    P = pb.make_params(n=3, cluster_prob=0.5)
    alpha, after, lo, up, flipped, used = pb.cluster_flip(P, phi, 1, [0.5, pu + 1e-9, pl + 1e-9])
    assert (lo, up, flipped, used) == (1, 1, True, 3)
    npu, npl = link(phi[1] + math.pi, phi[2]), link(phi[1] + math.pi, phi[0])
    np.testing.assert_allclose(alpha, (1 - npu) * (1 - npl) / ((1 - pu) * (1 - pl)), rtol=1e-13)
    np.testing.assert_array_equal(after, [phi[0], phi[1] + math.pi, phi[2]])
    # n = 3, cluster {1, 2}: the link above fails, the link below joins and reaches the chain end (p = 0 there, before and after)
    alpha, after, lo, up, flipped, used = pb.cluster_flip(P, phi, 1, [0.5, pu + 1e-9, pl])          # rand() <= p joins
    assert (lo, up, flipped, used) == (0, 1, True, 3)
    np.testing.assert_allclose(alpha, (1 - npu) / (1 - pu), rtol=1e-13)
    np.testing.assert_array_equal(after, [phi[0] + math.pi, phi[1] + math.pi, phi[2]])
    # no flip: one draw, no growth, alpha = 1, the chain untouched -- and cluster_prob is the probability OF flipping
    alpha, after, lo, up, flipped, used = pb.cluster_flip(P, phi, 1, [0.5 + 1e-9, 0.0, 0.0])
    assert (lo, up, flipped, used, alpha) == (1, 1, False, 1, 1.0)
    np.testing.assert_array_equal(after, phi)
    # from the chain's first monomer: no draw below
    alpha, after, lo, up, flipped, used = pb.cluster_flip(P, phi, 0, [0.1, 0.999999])
    assert (lo, up, flipped, used) == (0, 0, True, 2)
    np.testing.assert_allclose(alpha, (1 - link(phi[0] + math.pi, phi[1])) / (1 - link(phi[0], phi[1])), rtol=1e-13)


@pytest.mark.parametrize("rng", [0, 1], ids=["mwc64x", "xoshiro128pp"])
def test_restatement_consumes_the_words_the_contract_says(pb, rng):
    N = 4000
    # start: n words; a step that does not flip: idx, dphi, flip, eps
    r = pb.run(pb.make_params(n=7, num_steps=N, cluster_prob=0.0, E0=0.5, Fz=0.3, rng=rng, seed=3), chain_id=5)
    assert r.flips_proposed == 0 and r.link_tests == 0 and r.words == 7 + 4 * N
    # n = 2 and every step flips: exactly one link to test (the other end is a chain end) -> five words
    r = pb.run(pb.make_params(n=2, num_steps=N, cluster_prob=1.0, E0=0.5, Fz=0.3, rng=rng, seed=3), chain_id=5)
    assert r.flips_proposed == N and r.link_tests == N and r.words == 2 + 5 * N
    # in general: four words and one per link tested, links tested only by steps that flip
    r = pb.run(pb.make_params(n=30, num_steps=N, cluster_prob=0.5, E0=0.5, Fz=0.3, rng=rng, seed=3), chain_id=5)
    assert 0.45 * N < r.flips_proposed < 0.55 * N and r.link_tests >= r.flips_proposed
    assert r.words == 30 + 4 * N + r.link_tests
    # the generator state after the run is the seeded stream advanced by exactly that many words
    s = pb.stream(pb.make_params(rng=rng, seed=3), 5, r.words + 1)
    P2 = pb.make_params(rng=rng, seed=3)
    st = (C.c_uint32 * 4)(*[int(x) for x in r.rng])
    assert pb.lib().planar_next(P2.rng, st) == s[r.words]
    # uniform_bits 23 and 53 consume the same stream; eps is built from the words the contract names
    a = pb.run(pb.make_params(n=2, num_steps=50, cluster_prob=1.0, uniform_bits=23, rng=rng), chain_id=1)
    b = pb.run(pb.make_params(n=2, num_steps=50, cluster_prob=1.0, uniform_bits=53, rng=rng), chain_id=1)
    assert a.words == b.words
    w_eps, w_idx, w_phi, w_flip = 0x80000000, 0xFFFFFFFD, 0x000001FF, 0x00000101
    assert pb.lib().planar_eps(23, w_eps, w_idx, w_phi, w_flip) == 0.5
    assert pb.lib().planar_eps(53, w_eps, w_idx, w_phi, w_flip) == 0.5 + ((0x1FF << 12) | (0x101 << 3) | 5) * 2.0 ** -53


def test_restatement_carried_chain_continues_the_stream(pb):
    """planar_run from (phi, generator state) of an earlier run = what a carried burn-in rung starts from: with the averagers,
    step size and acceptor cache fresh, and the same trajectory as an uninterrupted run while nothing adapts."""
    kw = dict(n=12, E0=0.6, K1=0.8, Fz=0.4, energy_type=2, adj_scale=1.0, seed=11)
    # (a restart drops the acceptor's cached log(alpha), so the comparison is made without cluster flips)
    kw["cluster_prob"] = 0.0
    whole = pb.run(pb.make_params(num_steps=3000, **kw), chain_id=2)
    first = pb.run(pb.make_params(num_steps=1000, **kw), chain_id=2)
    rest = pb.run(pb.make_params(num_steps=2000, **kw), chain_id=2, phi0=first.final_phi, rng0=first.rng)
    np.testing.assert_array_equal(rest.final_phi, whole.final_phi)
    np.testing.assert_array_equal(rest.rng, whole.rng)
    assert first.nacc_total + rest.nacc_total == whole.nacc_total


# ------------------------------------------------------------------------------------------------ 4. closed form

def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "planar_closed_form.json")) as f:
        return json.load(f)["cases"]


def test_closed_form_fixture_holds_the_values_of_the_issue():
    g = _golden()
    a = g["n20_E0_0_Fz1"]["avg"]
    for k, v in (("r3", 8.9277993), ("r1sq", 8.9277993), ("r3sq", 86.792521), ("U", -8.9277993)):
        assert abs(a[k] - v) < 6e-8 * max(1.0, abs(v)), (k, a[k])
    a = g["diel_n25_E0_1_K1_1_Fz05"]["avg"]
    for k, v in (("r3", 6.7722192), ("p3", 14.414327), ("U", -10.593273), ("Usq", 116.81008)):
        assert abs(a[k] - v) < 6e-8 * max(1.0, abs(v)), (k, a[k])
    a = g["diel_n100_E0_1_K2_1_Fx1"]["avg"]
    for k, v in (("r1", 49.099051), ("p3", 61.316214), ("U", -79.757158)):
        assert abs(a[k] - v) < 6e-8 * max(1.0, abs(v)), (k, a[k])
    a = g["polar_n25_E0_1_mu09_Fz1_Fx025_kT08_b12"]["avg"]
    for k, v in (("r1", 3.8262176), ("r3", 21.044197), ("p3", 15.783148), ("U", -29.892325)):
        assert abs(a[k] - v) < 6e-8 * max(1.0, abs(v)), (k, a[k])
    # 20 I1(1) / I0(1)
    i0 = sum((0.25 ** k) / math.factorial(k) ** 2 for k in range(30))
    i1 = 0.5 * sum((0.25 ** k) / (math.factorial(k) * math.factorial(k + 1)) for k in range(30))
    assert abs(g["n20_E0_0_Fz1"]["avg"]["r3"] - 20 * i1 / i0) < 1e-10
    for c in g.values():
        assert all(c["avg"][k] == 0.0 for k in ("r2", "r2sq", "p2", "p2sq"))


def golden_kw(c):
    p = c["params"]
    return dict(n=p["n"], E0=p["E0"], K1=p["K1"], K2=p["K2"], mu=p["mu"], kT=p["kT"], Fz=p["Fz"], Fx=p["Fx"], b=p["b"],
                chain_type=0 if p["chain"] == "dielectric" else 1)


@pytest.mark.parametrize("name", ["n20_E0_0_Fz1", "diel_n25_E0_1_K1_1_Fz05", "diel_n100_E0_1_K2_1_Fx1",
                                  "polar_n25_E0_1_mu09_Fz1_Fx025_kT08_b12"])
def test_restatement_against_closed_form_single_monomer_metropolis(pb, name):
    """cluster_prob = 0 is single-monomer Metropolis, which samples the Boltzmann density: pooled means of 64 chains after a
    discarded transient within 5 of their own standard errors of the quadrature, every observable."""
    import polymer_stats_amd as ps
    c = _golden()[name]
    kw = golden_kw(c)
    n = kw["n"]
    nch, transient, nsteps = 64, 400 * n, 4000 * n         # 400 / 4 000 sweeps of the chain

    def one(cid):
        t = pb.run(pb.make_params(num_steps=transient, cluster_prob=0.0, seed=20260507, **kw), chain_id=cid)
        r = pb.run(pb.make_params(num_steps=nsteps, cluster_prob=0.0, seed=20260507, **kw), chain_id=cid,
                   phi0=t.final_phi, rng0=t.rng)
        return r.avg

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        m = np.array(list(ex.map(one, range(nch))))
    mean, se = m.mean(axis=0), m.std(axis=0, ddof=1) / math.sqrt(nch)
    eq = c["avg"]
    z = np.array([(mean[k] - eq[nm]) / (se[k] + 1e-12 * (1 + abs(eq[nm]))) for k, nm in enumerate(ps.OBS_NAMES)])
    print(name, dict(zip(ps.OBS_NAMES, np.round(z, 2))))
    assert np.all(np.abs(z) < 5.0), dict(zip(ps.OBS_NAMES, np.round(z, 2)))
    assert np.all(m[:, [1, 4, 8, 11]] == 0.0)               # the y slots


# ------------------------------------------------------------------------------------------------ 6. hosts and sweep

def test_host_option_table_is_the_references():
    from polymer_stats_amd import mcmc_clustering_eap_chain_2d as host
    with open(os.path.join(ROOT, "tests", "golden", "planar_options.json")) as f:
        table = json.load(f)
    parser = host.build_parser()
    by_flag = {s: a for a in parser._actions for s in a.option_strings}
    d = host.parse_args([])
    assert len(table["options"]) == 28
    for o in table["options"]:
        a = by_flag.get("--" + o["name"])
        assert a is not None, o["name"]
        if o["alias"]:
            assert by_flag.get("-" + o["alias"]) is a, o
        else:
            assert [s for s in a.option_strings if not s.startswith("--")] == [], o
        assert d[o["name"]] == o["default"] and type(d[o["name"]]) is type(o["default"]), (o, d[o["name"]])
    for name in table["absent"]:
        assert "--" + name not in by_flag, name
    for ours in ("num-chains", "seed", "devices", "rng", "uniform-bits", "carry-burn-in"):
        assert "--" + ours in by_flag, ours
    assert d["carry-burn-in"] is False
    # the Julia twin declares the same options with the same aliases
    jl = open(os.path.join(ROOT, "julia", "mcmc_clustering_eap_chain_2d.jl")).read()
    for o in table["options"]:
        decl = f'"--{o["name"]}", "-{o["alias"]}"' if o["alias"] else f'"--{o["name"]}";'
        assert decl in jl, decl
    for name in table["absent"]:
        assert f'"--{name}"' not in jl, name
    # headers and the ten lines
    assert host.TRAJ_HEADER == "step,r1,r3,p1,p3,U"
    assert host.ROLL_HEADER == "step,r1,r3,r1sq,r3sq,rsq,p1,p3,p1sq,p3sq,psq,U,Usq"
    A = host.Averager
    lines = host.summary_lines([A(5.0, 0), A(6.0, 0), A(-7.5, 0), A(60.0, 0)],
                               [A(np.array([1.0, 2.0]), 0), A(np.array([1.5, 4.5]), 0), A(np.array([0.0, 3.0]), 0),
                                A(np.array([0.25, 9.5]), 0)], 0.3125, host.default_pargs(**{"num-monomers": 4, "mlen": 0.5}))
    assert lines == ["<r>    =   [1.0, 2.0]", "<r/nb> =   [0.5, 1.0]", "<rj2>  =   [1.5, 4.5]", "<r2>   =   5.0",
                     "<p>    =   [0.0, 3.0]", "<pj2>  =   [0.25, 9.5]", "<p2>   =   6.0", "<U>    =   -7.5", "<U2>   =   60.0",
                     "AR     =   0.3125"]
    # pargs -> pstat_params: the planar defaults, nothing the planar main lacks
    p = host.params_from_pargs(host.default_pargs(seed=3), 5, 2, 0)
    assert (p.adj_ub, p.cluster_prob, p.num_chains, p.chain_id0, p.seed, p.precision) == (0.40, 0.5, 5, 2, 3, 1)
    assert (p.do_flips, p.bend_mod, p.bend_angle, p.use_x0) == (0, 0.0, 0.0, 0)


ISING_2024_11_06 = ["--main", "mcmc_clustering_eap_chain_2d", "--num-chains", "1", "--axis", "b=1", "--axis", "n=25", "--axis", "Fx=0",
                    "--axis", "Fz=0,0.1,0.2,0.3,0.4,0.5,1,2,3,4,5,7.5,10,12.5,15,20,25,30,35,40,45,50", "--axis", "kT=1",
                    "--axis", "E0=0.1", "--axis", "K1=0.01,0.04,0.1,0.4", "--axis", "K2=0", "--axis", "run=1:10",
                    "--name", "E0,K1,K2,kT,Fz,Fx,n,b,run:raw", "--", "--chain-type", "dielectric", "--energy-type", "Ising",
                    "--num-steps", "10000000", "--burn-in", "200000", "-v", "2"]


def test_sweep_plans_the_880_cases_of_ising_2024_11_06(tmp_path):
    """2D/run/Ising_2024-11-06.jl:18-36,47: 4 K1 x 22 Fz x 10 runs of the planar main, file names as its prefix() builds them."""
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "run_sweep.py"), str(tmp_path), "--dry-run"]
                                  + ISING_2024_11_06).decode()
    assert out.startswith("880 cases (0 already there), 1 ensemble(s)") and "main mcmc_clustering_eap_chain_2d" in out
    assert "n = 25, Ising, dielectric, 10000000 steps: 880 cases, 880 chains" in out
    assert "E0-0000100_K1-0000010_K2-0000000_kT-0001000_Fz-0000000_Fx-0000000_n-0025000_b-0001000_run-1.out" in out
    assert "E0-0000100_K1-0000400_K2-0000000_kT-0001000_Fz-0050000_Fx-0000000_n-0025000_b-0001000_run-10.out" in out
    from polymer_stats_amd import sweep as sw
    axes = [(a.split("=")[0], sw.axis_values(a.split("=")[1])) for a in ISING_2024_11_06[5:23:2]]
    cases = sw.product_cases(axes)
    pl = sw.plan("mcmc_clustering_eap_chain_2d", ISING_2024_11_06[ISING_2024_11_06.index("--") + 1:], cases, str(tmp_path),
                 name="E0,K1,K2,kT,Fz,Fx,n,b,run:raw", num_chains=1, seed=5)
    assert len(pl) == 880 and len({p["_name"] for p in pl}) == 880
    # the loop order of the run script: Fz outside K1 outside run
    assert [(p["Fz"], p["K1"], p["_case"]["run"]) for p in pl[:12]] == [(0.0, 0.01, r) for r in range(1, 11)] + [(0.0, 0.04, 1), (0.0, 0.04, 2)]
    p = pl[879]
    assert (p["E0"], p["K1"], p["Fz"], p["num-monomers"], p["num-steps"], p["burn-in"], p["energy-type"], p["seed"]) == \
        (0.1, 0.4, 50.0, 25, 10000000, 200000, "Ising", 5 + 879)
    assert len({sw._signature(p) for p in pl}) == 1             # one ensemble


def test_aggregator_reads_the_planar_lines(tmp_path):
    from polymer_stats_amd import aggregate_mcmc as ag
    from polymer_stats_amd import mcmc_clustering_eap_chain_2d as host
    A = host.Averager
    for run in (1, 2):
        lines = host.summary_lines([A(5.0, 0), A(6.0, 0), A(-7.5, 0), A(60.0, 0)],
                                   [A(np.array([1.0, 2.0 * run]), 0), A(np.array([1.5, 4.5]), 0), A(np.array([0.0, 3.0]), 0),
                                    A(np.array([0.25, 9.5]), 0)], 0.3125, host.default_pargs(**{"num-monomers": 25}))
        name = f"E0-0000100_K1-0000040_K2-0000000_kT-0001000_Fz-0001000_Fx-0000000_n-0025000_b-0001000_run-{run}.out"
        (tmp_path / name).write_text("\n".join(lines) + "\n")
    out = tmp_path / "agg.csv"
    assert ag.aggregate(str(out), str(tmp_path), "*.out", "dielectric", False, True) == 0
    rows = out.read_text().splitlines()
    assert rows[0] == "E0,K1,K2,kT,Fz,Fx,n,b,r1,r2,lambda1,lambda2,r1sq,r2sq,rsquared,p1,p2,p1sq,p2sq,psquared,U,Usquared,AR"
    assert rows[1] == "0.1,0.04,0.0,1.0,1.0,0.0,25.0,1.0,1.0,2.0,0.04,0.08,1.5,4.5,5.0,0.0,3.0,0.25,9.5,6.0,-7.5,60.0,0.3125"
    assert len(rows) == 3 and rows[2].split(",")[9] == "4.0"


def test_julia_planar_host_mirrors_the_structs(ps):
    """The (unexecuted) Julia planar host, checked the way test_julia_hosts_mirror_the_structs checks the other two."""
    jl_type = {C.c_double: "Cdouble", C.c_int64: "Int64", C.c_uint64: "UInt64", C.c_int32: "Int32"}
    src = open(os.path.join(ROOT, "julia", "mcmc_clustering_eap_chain_2d.jl")).read()
    body = re.search(r"struct PstatParams\n(.*?)\nend", src, re.S).group(1)
    assert re.findall(r"(\w+)::(\w+)", body) == [(f, jl_type[t]) for f, t in ps._lib.Params._fields_]
    body = re.search(r"struct PstatSummary\n(.*?)\nend", src, re.S).group(1)
    want = [(f, jl_type[t] if t in jl_type else "NTuple{%d,Cdouble}" % (C.sizeof(t) // 8)) for f, t in ps._lib.Summary._fields_]
    assert re.findall(r"(\w+)::([\w{},]+)", body) == want
    i = src.index("  PstatParams(pargs[") + len("  PstatParams(")
    depth, args = 1, 1
    while depth > 0:
        c = src[i]
        if c in "([":
            depth += 1
        elif c in ")]":
            depth -= 1
        elif c == "," and depth == 1:
            args += 1
        elif c == "#":
            i = src.index("\n", i)
        i += 1
    assert args == len(ps._lib.Params._fields_), args
    syms = set(re.findall(r"ccall\(\(:(\w+), LIBPSTAT\)", src))
    assert "pstat_create_planar" in syms and "pstat_create" not in syms
    for sym in syms:
        assert sym in ps._lib.SYMBOLS, sym
    assert 'println(outfile, "step,r1,r3,p1,p3,U")' in src
    assert 'println(rollfile, "step,r1,r3,r1sq,r3sq,rsq,p1,p3,p1sq,p3sq,psq,U,Usq")' in src
