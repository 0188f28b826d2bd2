"""Host side of the drop-in for mcmc_clustering_eap_chain.jl: its command line, its burn-in ladder, its
two CSV files and its twelve stdout lines, with the step loop (single-monomer move + cluster_flip!) on
the GPU through libpstat (move_set = PSTAT_MOVES_CLUSTER).

    python -m polymer_stats_amd.mcmc_clustering_eap_chain -n 100 -e 1 -F 1 -u noninteracting \
           --bend-mod 1 --cluster-prob 0.5 -N 1000000 --num-chains 16384 --prefix out/run1 -v 2

Option names, aliases, types and defaults are the reference's (mcmc_clustering_eap_chain.jl:14-152;
note they differ from mcmc_eap_chain.jl: energy-type defaults to Ising, step-adjust-ub to 0.40,
num-steps to 1e6, and there is a 5-rung burn-in ladder by default).  Added: --num-chains, --seed,
--devices, --precision, --rng.

All four energy types run on the device (interacting and cutoff: one chain per wavefront, n <= 512),
and both forms of --x0 ([phi; theta] for every monomer, or 2 n interleaved per-monomer angles).

What it shares with the other two mains is in polymer_stats_amd/_host.py; here are its options, its headers and rows,
its own pstat_params fields and its protocol (the ladder, with a per-monomer --x0 applied in front of it).
"""
from __future__ import annotations

import sys

import numpy as np

from . import _host, _lib
from ._host import Averager, ReferenceError_, julia_vector      # (reached through this module too)
from .julia_fmt import jl_float, jl_row

ROLL_HEADER = "step,r1,r2,r3,r1sq,r2sq,r3sq,rsq,p1,p2,p3,p1sq,p2sq,p3sq,psq,U,Usq,Ealign,psi"   # :259

# the reference's table in its order (mcmc_clustering_eap_chain.jl:14-152), then ours
build_parser, parse_args, default_pargs = _host.parser_functions(_host.CLUSTER, """
    E0 chain-type K1 K2 mu bend-mod bend-angle energy-type cutoff-radius kT Fz Fx mlen num-monomers num-steps phi-step theta-step
    cluster-prob step-adjust-lb step-adjust-ub step-adjust-scale steps-per-adjust umbrella-sampling update-freq verbose prefix
    postfix stepout numeric-type burn-in burn-schedule x0 dx0 profile
    num-chains seed devices rng precision uniform-bits""".split())


def params_from_pargs(pargs: dict, num_chains: int, chain_id0: int, device: int) -> _lib.Params:
    kw = _host.common_params(pargs, num_chains, chain_id0, device,
                             {"noninteracting": _lib.NONINTERACTING, "Ising": _lib.ISING, "interacting": _lib.INTERACTING,
                              "cutoff": _lib.CUTOFF}, {"f32": _lib.F32, "f64": _lib.F64})
    if pargs.get("x0") is not None:                                                   # inc/eap_chain.jl:61-80
        try:
            x0, dx0 = julia_vector(pargs["x0"]), julia_vector(pargs["dx0"])
        except (ValueError, SyntaxError):
            raise ReferenceError_(f"Invalid input for 'x0' and/or 'dx0', {pargs['x0']}; {pargs['dx0']}")
        if len(x0) == 2 and len(dx0) >= 2:
            kw.update(use_x0=1, x0_phi=x0[0], x0_theta=x0[1], dx0_phi=dx0[0], dx0_theta=dx0[1])
        elif len(x0) == 2 * pargs["num-monomers"] and len(dx0) >= 2:
            pass        # per-monomer start: applied after creation (run_cases(): Ensemble.restart_from_x0)
        else:
            raise ReferenceError_(f"Invalid input for 'x0' and/or 'dx0', {pargs['x0']}; {pargs['dx0']}")
    return _lib.default_params(move_set=_lib.MOVES_CLUSTER, bend_mod=pargs["bend-mod"], bend_angle=pargs["bend-angle"],
                               cluster_prob=pargs["cluster-prob"], cutoff_radius=pargs["cutoff-radius"], **kw)


def traj_header(n: int) -> str:
    """mcmc_clustering_eap_chain.jl:253-258: phi/theta interleaved per monomer, then mux/muy/muz."""
    cols = ["step", "r1", "r2", "r3", "p1", "p2", "p3", "U"]
    for i in range(1, n + 1):
        cols += [f"phi{i}", f"theta{i}"]
    for i in range(1, n + 1):
        cols += [f"mux{i}", f"muy{i}", f"muz{i}"]
    return ",".join(cols)


def _dipoles(pargs, phi, theta) -> np.ndarray:
    """mu_i of the printed microstate (inc/dipole_response.jl:7-29), for the trajectory file only."""
    nx, ny, nz = np.cos(phi) * np.sin(theta), np.sin(phi) * np.sin(theta), np.cos(theta)
    if pargs["chain-type"] == "dielectric":
        a = (pargs["K1"] - pargs["K2"]) * pargs["E0"] * nz
        return np.stack([a * nx, a * ny, a * nz + pargs["K2"] * pargs["E0"]], axis=1)
    return pargs["mu"] * np.stack([nx, ny, nz], axis=1)


def _rows(pargs, step, micro, ang, s):                              # :312-335
    n = pargs["num-monomers"]
    theta, phi = ang[:n], ang[n:]
    mus = _dipoles(pargs, phi, theta)
    angles = np.stack([phi, theta], axis=1).reshape(-1)
    return jl_row([step, *micro, *angles, *mus.reshape(-1)]), jl_row([step, *s.avg, *s.extra_avg])


def run(pargs: dict):
    """The top level of mcmc_clustering_eap_chain.jl:354-387 -> (scalar_averagers, vector_averagers, ar)."""
    return run_cases([pargs])[0]


def averagers(s):
    """A summary -> (scalar_averagers with the two extras, vector_averagers, ar)."""
    sas, vas, ar = _host._averagers(s)
    ex, exse = np.array(s.extra_avg), np.array(s.extra_stderr)
    return sas + [Averager(ex[0], exse[0]), Averager(ex[1], exse[1])], vas, ar


def run_cases(plist: list, write_csv: bool = True, info: dict | None = None, record=None) -> list:
    """The top level of the clustering main for every case of `plist` at once -- parsed options that differ only in their
    physics scalars, prefix and seed (one case: the command line; many: a sweep, polymer_stats_amd/sweep.py) -- as ONE
    ensemble: every rung of the ladder and the recorded run are one launch (per segment) for all of them.  `record` = a
    _host.Recording: the production run is recorded its way and info[record.kind] holds what that gives (_Pool.record)."""
    pargs = plist[0]
    if record:
        _host.check_recording(pargs, record, write_csv)
    _host.check_numeric_type(pargs)                                     # :191
    ladder = _host.burn_ladder(pargs)
    with _host._Pool(plist, params_from_pargs, info=info) as pool:
        if pargs.get("x0") is not None:
            x0 = julia_vector(pargs["x0"])
            if len(x0) == 2 * pargs["num-monomers"] and len(x0) != 2:      # inc/eap_chain.jl:73-75
                dx0 = julia_vector(pargs["dx0"])
                for e in pool.parts:
                    e.restart_from_x0(x0, dx0[0], dx0[1])
        # every stage is one call of the reference's mcmc(nsteps, pargs, chain) (:172-352) at kT x mult: the rungs (:366-383), then
        # the production run (:385-386).  Every call rewrites the two CSV files, so only the last one's survive: the rungs skip them
        for mult, nsteps, write, rec in [(m, pargs["burn-in"], False, None) for m in ladder] + [(1.0, pargs["num-steps"], write_csv, record)]:
            pool.stage(mult)
            out = _host.recorded_stage(pool, int(nsteps), write, lambda p: traj_header(p["num-monomers"]), ROLL_HEADER, _rows,
                                       angles=True, record=rec)
        for k, s in enumerate(out):
            pool.report_failures(k, s)
    return [averagers(s) for s in out]


def summary_lines(sas, vas, ar, pargs) -> list[str]:
    """The twelve println lines, mcmc_clustering_eap_chain.jl:389-400."""
    return _host.summary_lines(sas, vas, ar, pargs, extra=[f"<cos2(θ)>   =   {jl_float(_host.get_avg(sas[4]))}",
                                                           f"<ψ>    =   {jl_float(_host.get_avg(sas[5]))}"])


def main(argv=None) -> int:
    return _host.main(parse_args(argv), "Not currently implemented...", run, summary_lines)     # :358


if __name__ == "__main__":
    sys.exit(main())
