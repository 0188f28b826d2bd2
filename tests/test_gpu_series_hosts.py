"""The hosts' two time-series files now come out of the device-side series.  Their bytes must be what the per-row loop
wrote: here that loop is restated on a twin ensemble with the per-row API (advance, microstate, chain_state, reduce_host,
summary_from_reduction) and jl_row, and compared with the files host.main(argv) leaves -- also when the series' device
budget is lowered until a run takes several chunks -- and a batched sweep's files with each case run alone."""
import contextlib
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _run_main(host, argv):
    with contextlib.redirect_stdout(io.StringIO()) as buf:
        assert host.main(argv) == 0
    return buf.getvalue()


def _files(prefix):
    return open(prefix + "_trajectory.csv", "rb").read(), open(prefix + "_rolling.csv", "rb").read()


def _pooled(e, steps):
    import polymer_stats_amd as ps
    red = np.zeros(ps.NRED)
    red += e.reduce_host(0)                       # the pool adds its shards' vectors to zeros
    return ps.summary_from_reduction(red, steps)


def _fixed_force_twin(host, argv):
    """The per-row loop of the fixed-force main, one case on one device."""
    import polymer_stats_amd as ps
    from polymer_stats_amd.julia_fmt import jl_row
    pargs = host.parse_args(argv)
    nsteps, stepout = pargs["num-steps"], pargs["stepout"]
    traj, roll = [host.TRAJ_HEADER], [host.ROLL_HEADER]
    with ps.Ensemble(host.params_from_pargs(pargs, pargs["num-chains"], 0, 0)) as e:
        total = 0
        for init in range(1, pargs["num-inits"] + 1):
            for r in range(1, nsteps // stepout + 1):
                e.advance(stepout)
                total += stepout
                traj.append(jl_row([r * stepout, *e.microstate(0)]))
                roll.append(jl_row([r * stepout, *_pooled(e, total).avg]))
            e.advance(nsteps % stepout)
            total += nsteps % stepout
            if init < pargs["num-inits"]:
                e.reinit(bool(pargs["force-init"]))
    return ("\n".join(traj) + "\n").encode(), ("\n".join(roll) + "\n").encode()


def _clustering_twin(host, argv):
    """The per-row loop of the clustering main under its burn-in ladder, one case on one device."""
    import polymer_stats_amd as ps
    from polymer_stats_amd.julia_fmt import jl_row
    pargs = host.parse_args(argv)
    n, nsteps, stepout = pargs["num-monomers"], pargs["num-steps"], pargs["stepout"]
    traj, roll = [host.traj_header(n)], [host.ROLL_HEADER]
    with ps.Ensemble(host.params_from_pargs(pargs, pargs["num-chains"], 0, 0)) as e:
        for mult in host.julia_vector(pargs["burn-schedule"]):
            e.scale_kT(mult)
            e.reset_sampler()
            e.reset_averages()
            e.advance(pargs["burn-in"])
        e.scale_kT(1.0)
        e.reset_sampler()
        e.reset_averages()
        for r in range(1, nsteps // stepout + 1):
            e.advance(stepout)
            st = e.chain_state(0)
            mus = host._dipoles(pargs, st["phi"], st["theta"])
            angles = np.stack([st["phi"], st["theta"]], axis=1).reshape(-1)
            s = _pooled(e, r * stepout)
            traj.append(jl_row([r * stepout, *e.microstate(0), *angles, *mus.reshape(-1)]))
            roll.append(jl_row([r * stepout, *s.avg, *s.extra_avg]))
    return ("\n".join(traj) + "\n").encode(), ("\n".join(roll) + "\n").encode()


FIXED = [
    ["-n", "20", "-e", "1.0", "-J", "1.0", "-F", "0.5", "-N", "2250", "-s", "300", "--num-chains", "96", "--seed", "3"],
    ["-n", "12", "-e", "0.8", "-F", "0.3", "-N", "1200", "-M", "2", "-I", "-s", "400", "--num-chains", "40", "--seed", "5",
     "-T", "polar", "-m", "0.7", "-u", "Ising", "-S", "300"],
    ["-n", "14", "-e", "0.9", "-F", "0.2", "-N", "900", "-M", "2", "-B", "-s", "300", "--num-chains", "33", "--seed", "6",
     "--precision", "f32", "--rng", "xoshiro128++"],
]


@pytest.mark.parametrize("argv", FIXED, ids=["remainder", "two-forced-inits", "two-inits-umbrella-f32"])
def test_fixed_force_main_writes_the_per_row_loops_bytes(tmp_path, monkeypatch, argv):
    from polymer_stats_amd import _host, mcmc_eap_chain as host
    argv = argv + ["-v", "0"]
    want = _fixed_force_twin(host, argv + ["--prefix", "unused"])
    assert want[0].count(b"\n") == 1 + host.parse_args(argv)["num-inits"] * (int(argv[argv.index("-N") + 1]) // int(argv[argv.index("-s") + 1]))
    _run_main(host, argv + ["--prefix", str(tmp_path / "a")])
    assert _files(str(tmp_path / "a")) == want
    # the same run with room for two rows, then one row, per chunk
    row_bytes = 8 * (host._lib.NRED + 7)
    for tag, budget in (("b", 2 * row_bytes + 8), ("c", 1)):
        monkeypatch.setattr(_host, "SERIES_BUDGET_BYTES", budget)
        _run_main(host, argv + ["--prefix", str(tmp_path / tag)])
        assert _files(str(tmp_path / tag)) == want, budget


def test_fixed_force_main_sharded_over_two_handles(tmp_path):
    """--devices 0,0: two shards' rows are added; the trajectory row is shard 0's.  Against the per-row API on twin shards."""
    import polymer_stats_amd as ps
    from polymer_stats_amd import mcmc_eap_chain as host
    from polymer_stats_amd.julia_fmt import jl_row
    argv = ["-n", "16", "-e", "1.0", "-F", "0.6", "-N", "900", "-s", "300", "--num-chains", "50", "--seed", "12", "-v", "0",
            "--devices", "0,0"]
    pargs = host.parse_args(argv)
    traj, roll = [host.TRAJ_HEADER], [host.ROLL_HEADER]
    with ps.Ensemble(host.params_from_pargs(pargs, 25, 0, 0)) as e0, ps.Ensemble(host.params_from_pargs(pargs, 25, 25, 0)) as e1:
        for r in (1, 2, 3):
            red = np.zeros(ps.NRED)
            for e in (e0, e1):
                e.advance(300)
            for e in (e0, e1):
                red += e.reduce_host(0)
            traj.append(jl_row([300 * r, *e0.microstate(0)]))
            roll.append(jl_row([300 * r, *ps.summary_from_reduction(red, 300 * r).avg]))
    _run_main(host, argv + ["--prefix", str(tmp_path / "s")])
    assert _files(str(tmp_path / "s")) == (("\n".join(traj) + "\n").encode(), ("\n".join(roll) + "\n").encode())


@pytest.mark.parametrize("energy,chains", [("Ising", "24"), ("interacting", "6")])
def test_clustering_main_writes_the_per_row_loops_bytes(tmp_path, monkeypatch, energy, chains):
    from polymer_stats_amd import mcmc_clustering_eap_chain as host, _host as fixed
    argv = ["-n", "12", "-e", "1.0", "-J", "0.4", "-F", "0.5", "-u", energy, "-a", "0.5", "-g", "0.2", "--cluster-prob", "0.5",
            "-N", "1300", "--burn-in", "300", "--burn-schedule", "[10; 1]", "-s", "400", "-v", "0", "--num-chains", chains,
            "--seed", "4", "-S", "250"]
    want = _clustering_twin(host, argv + ["--prefix", "unused"])
    assert want[0].count(b"\n") == 4 and want[1].count(b"\n") == 4
    _run_main(host, argv + ["--prefix", str(tmp_path / "a")])
    assert _files(str(tmp_path / "a")) == want
    monkeypatch.setattr(fixed, "SERIES_BUDGET_BYTES", 8 * (fixed._lib.NRED + 7 + 24) * 2)     # two rows per chunk
    _run_main(host, argv + ["--prefix", str(tmp_path / "b")])
    assert _files(str(tmp_path / "b")) == want


def test_wide_numeric_type_keeps_the_per_row_calls(tmp_path):
    """--numeric-type other than float64 merges per-chain means in a wide type at every row: that input stays on the
    per-row path and writes what it wrote."""
    from polymer_stats_amd import mcmc_eap_chain as host
    argv = ["-n", "10", "-e", "1.0", "-F", "0.5", "-N", "700", "-s", "300", "--num-chains", "20", "--seed", "8", "-v", "0"]
    _run_main(host, argv + ["--prefix", str(tmp_path / "d")])
    _run_main(host, argv + ["--numeric-type", "big", "--prefix", str(tmp_path / "w")])
    td, rd = _files(str(tmp_path / "d"))
    tw, rw = _files(str(tmp_path / "w"))
    assert td == tw and rd.count(b"\n") == rw.count(b"\n") == 3
    a = np.array([[float(x) for x in l.split(",")] for l in rd.decode().splitlines()[1:]])
    b = np.array([[float(x) for x in l.split(",")] for l in rw.decode().splitlines()[1:]])
    np.testing.assert_allclose(b, a, rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("main_name,fixed", [
    ("mcmc_eap_chain", ["--num-steps", "1100", "--stepout", "250", "-v", "0", "--energy-type", "Ising"]),
    ("mcmc_clustering_eap_chain", ["--energy-type", "Ising", "--num-steps", "900", "--burn-in", "200", "--burn-schedule", "[10; 1]",
                                   "--stepout", "300", "-v", "0"]),
])
def test_sweep_csv_files_are_those_of_each_case_run_alone(tmp_path, main_name, fixed):
    from polymer_stats_amd import sweep as sw
    cases = [dict(E0=e0, K1=0.5, Fz=fz, n=14) for e0 in (0.5, 1.0, 1.5) for fz in (0.0, 0.7)]
    kw = dict(num_chains=8, seed=21)
    res = sw.run_sweep(main_name, fixed, cases, str(tmp_path), write_csv=True, **kw)
    assert len(res["ran"]) == 6 and res["launches"] == 1
    main = sw.MAINS[main_name]
    for p in sw.plan(main_name, fixed, cases, str(tmp_path), **kw):
        alone = {k: v for k, v in p.items() if not k.startswith("_")}
        alone["prefix"] = p["prefix"] + "_alone"
        if main is sw.cluster_main:
            main.run(alone)
        else:
            main.mcmc(alone["num-steps"], alone)
        got, want = _files(p["prefix"]), _files(alone["prefix"])
        assert got[0].count(b"\n") == 1 + int(fixed[fixed.index("--num-steps") + 1]) // int(fixed[fixed.index("--stepout") + 1])
        assert got == want, p["_name"]
