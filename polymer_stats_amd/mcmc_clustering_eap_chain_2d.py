"""Host side of the drop-in for the planar main, 2D/mcmc_clustering_eap_chain.jl: its command line, its two CSV files
and its ten stdout lines, with the step loop (single-monomer move + cluster_flip!, one angle per monomer) on the GPU
through libpstat (pstat_create_planar).

    python -m polymer_stats_amd.mcmc_clustering_eap_chain_2d -n 25 -e 0.1 -J 0.04 -u Ising -F 1 -N 10000000 \
           --num-chains 64 --prefix out/run1 -v 2

Option names, aliases, types and defaults are the reference's (2D/mcmc_clustering_eap_chain.jl:15-129; note
--step-adjust-ub 0.40 and --cluster-prob = the probability OF flipping a cluster).  Added: --num-chains, --seed,
--devices, --rng, --uniform-bits, --carry-burn-in.

THE BURN-IN LADDER.  In the reference `mcmc(nsteps, pargs, chain)` overwrites the chain it is handed with a fresh
`EAPChain(pargs)` on its first line (2D/mcmc_clustering_eap_chain.jl:151), so every rung of the ladder (:323-335) and the
production run start from a fresh uniform chain, and only the production run's averagers are printed and its CSV files
survive.  --burn-in and --burn-schedule therefore change no output of the reference, and none here: the rungs are not
run (said once on stderr at -v 2 or higher).  --carry-burn-in runs the ladder on the chains and carries them into the
production run the way the 3D clustering main does -- what the options' help texts promise.

--energy-type interacting (planar all-pairs) has no device implementation: the library refuses it.
"""
from __future__ import annotations

import math
import sys
import time

import argparse
import numpy as np

from . import _lib
from .julia_fmt import jl_float, jl_row, jl_vector
from .mcmc_clustering_eap_chain import julia_vector
from .mcmc_eap_chain import Averager, CsvFiles, ReferenceError_, _Pool, _log, get_avg, resolve_seed

TRAJ_HEADER = "step,r1,r3,p1,p3,U"                                             # :228
ROLL_HEADER = "step,r1,r3,r1sq,r3sq,rsq,p1,p3,p1sq,p3sq,psq,U,Usq"             # :230


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="mcmc_clustering_eap_chain_2d", add_help=True, allow_abbrev=False)
    a = p.add_argument
    # --- the reference's table, 2D/mcmc_clustering_eap_chain.jl:15-129
    a("--E0", "-e", dest="E0", type=float, default=0.0, help="magnitude of electric field")
    a("--chain-type", "-T", dest="chain-type", type=str, default="dielectric", help="chain type (dielectric|polar)")
    a("--K1", "-J", dest="K1", type=float, default=1.0, help="dipole susceptibility along the monomer axis (dielectric chain)")
    a("--K2", "-K", dest="K2", type=float, default=0.0, help="dipole susceptibility orthogonal to the monomer axis (dielectric chain)")
    a("--mu", "-m", dest="mu", type=float, default=1e-2, help="dipole magnitude (electret chain)")
    a("--energy-type", "-u", dest="energy-type", type=str, default="noninteracting", help="energy type (noninteracting|interacting|Ising)")
    a("--kT", "-k", dest="kT", type=float, default=1.0, help="dimensionless temperature")
    a("--Fz", "-F", dest="Fz", type=float, default=0.0, help="force in the z-direction (direction of E-field; force ensemble)")
    a("--Fx", "-G", dest="Fx", type=float, default=0.0, help="force in the x-direction (force ensemble)")
    a("--mlen", "-b", dest="mlen", type=float, default=1.0, help="monomer length")
    a("--num-monomers", "-n", dest="num-monomers", type=int, default=100, help="number of monomers")
    a("--num-steps", "-N", dest="num-steps", type=int, default=int(1e6), help="number of steps")
    a("--phi-step", "-p", dest="phi-step", type=float, default=3 * math.pi / 8, help="maximum phi step length")
    a("--cluster-prob", dest="cluster-prob", type=float, default=0.5, help="probability of flipping a cluster")
    a("--step-adjust-lb", "-L", dest="step-adjust-lb", type=float, default=0.15, help="adjust step sizes if acc. ratio below this threshold")
    a("--step-adjust-ub", "-U", dest="step-adjust-ub", type=float, default=0.40, help="adjust step sizes if acc. ratio above this threshold")
    a("--step-adjust-scale", "-A", dest="step-adjust-scale", type=float, default=1.1, help="scale factor for adjusting step sizes (> 1.0)")
    a("--steps-per-adjust", "-S", dest="steps-per-adjust", type=int, default=2500, help="steps between step size adjustments")
    a("--umbrella-sampling", "-B", dest="umbrella-sampling", action="store_true", help="use umbrella sampling (w/ electrostatic weight function)")
    a("--update-freq", dest="update-freq", type=float, default=15.0, help="update frequency (seconds)")
    a("--verbose", "-v", dest="verbose", type=int, default=3, help="verbosity level: 0-nothing, 1-errors, 2-warnings, 3-info")
    a("--prefix", "-P", dest="prefix", type=str, default="eap-mcmc", help="prefix for output files")
    a("--postfix", "-Q", dest="postfix", type=str, default="", help="postfix for output files")
    a("--stepout", "-s", dest="stepout", type=int, default=500, help="steps between storing microstates")
    a("--numeric-type", dest="numeric-type", type=str, default="float64", help="numerical data type for averaging (float64|float128|dec128|big)")
    a("--profile", "-Z", dest="profile", action="store_true", help="profile the program")
    a("--burn-in", dest="burn-in", type=int, default=50000, help="steps for burn-in; i.e. steps before averaging")
    a("--burn-schedule", dest="burn-schedule", type=str, default="[1000; 100; 10; 2; 1]", help="temperature schedule for burn-in")
    # --- ours
    a("--carry-burn-in", dest="carry-burn-in", action="store_true",
      help="run the burn-in ladder on the chains and carry them into the production run (the reference's ladder starts every "
           "rung and the production run from a fresh chain, so it changes no output: without this option it is not run)")
    a("--num-chains", dest="num-chains", type=int, default=4096, help="independent chains run at once on the GPU(s) and pooled")
    a("--seed", dest="seed", type=int, default=None,
      help="seed of the per-chain generators; default: fresh OS entropy per run, like the reference's unseeded RNG "
           "(the seed drawn is echoed on stderr at --verbose >= 2)")
    a("--devices", dest="devices", type=str, default="0", help="comma-separated HIP device ordinals; chains are sharded over them")
    a("--rng", dest="rng", type=str, default="mwc64x", help="per-chain generator: mwc64x | xoshiro128++")
    a("--uniform-bits", dest="uniform-bits", type=int, default=0,
      help="random bits of the Metropolis draw rand(): 0 = the default (53, like Julia's Float64 rand()) | 23 | 53")
    return p


def parse_args(argv=None) -> dict:
    return vars(build_parser().parse_args(argv))


def default_pargs(**overrides) -> dict:
    d = parse_args([])
    for k, v in overrides.items():
        if k not in d:
            raise KeyError(k)
        d[k] = v
    return d


def params_from_pargs(pargs: dict, num_chains: int, chain_id0: int, device: int) -> _lib.Params:
    resolve_seed(pargs)
    ct = {"dielectric": _lib.DIELECTRIC, "polar": _lib.POLAR}.get(pargs["chain-type"])
    if ct is None:
        raise ReferenceError_("chain-type is not understood.")                       # 2D/inc/eap_chain.jl:74
    et = {"noninteracting": _lib.NONINTERACTING, "Ising": _lib.ISING, "interacting": _lib.INTERACTING}.get(pargs["energy-type"])
    if et is None:
        raise ReferenceError_("energy-type is not understood.")                      # 2D/inc/eap_chain.jl:88
    rng = {"mwc64x": _lib.RNG_MWC64X, "xoshiro128++": _lib.RNG_XOSHIRO128PP}.get(pargs["rng"])
    if rng is None:
        raise ReferenceError_(f"rng '{pargs['rng']}' not understood")
    return _lib.default_planar_params(
        E0=pargs["E0"], K1=pargs["K1"], K2=pargs["K2"], mu=pargs["mu"], kT=pargs["kT"],
        Fz=pargs["Fz"], Fx=pargs["Fx"], b=pargs["mlen"], phi_step=pargs["phi-step"],
        adj_lb=pargs["step-adjust-lb"], adj_ub=pargs["step-adjust-ub"], adj_scale=pargs["step-adjust-scale"],
        steps_per_adjust=pargs["steps-per-adjust"], n=pargs["num-monomers"], num_chains=num_chains,
        seed=pargs["seed"], chain_id0=chain_id0, chain_type=ct, energy_type=et,
        umbrella=1 if pargs["umbrella-sampling"] else 0, precision=_lib.F64, device=device, rng=rng,
        uniform_bits=int(pargs.get("uniform-bits", 0)), cluster_prob=pargs["cluster-prob"])


def _planar(v) -> np.ndarray:
    """A 3-vector of the 16-vector's layout -> the planar 2-vector (component 1 in the x slot, component 2 in the z slot)."""
    v = np.asarray(v)
    return v[[0, 2]]


def _stage(pool, nsteps, mult, write: bool):
    """One call of the reference's mcmc(nsteps, pargs, chain) (:148-310) at kT x mult on the pool's chains, for every case."""
    pool.stage(mult)
    plist = pool.plist
    pargs = plist[0]
    stepout = int(pargs["stepout"]) if write else 0
    files = None
    try:
        if write:                                                        # :227-230
            files = CsvFiles([p["prefix"] for p in plist], [TRAJ_HEADER] * len(plist), ROLL_HEADER)
        start = time.time()
        last_update = [start]

        def tick(step):                                                  # :251-255 (per chunk of rows)
            if time.time() - last_update[0] > pargs["update-freq"]:
                _log(pargs, 3, "Info", f"elapsed: {time.time() - start}")
                _log(pargs, 3, "Info", f"step:    {step} / {nsteps}")
                last_update[0] = time.time()
        for step, micro, _, sums in pool.recorded(nsteps, stepout, tick=tick):       # rows :279-298
            for k in range(len(files)):
                m, avg = micro[k], np.array(sums[k].avg)
                files.rows(k, jl_row([step, m[0], m[2], m[3], m[5], m[6]]), jl_row([step, *avg[_lib.PLANAR_OBS_INDEX]]))
        out = [pool.summary(k) for k in range(len(plist))]
        _log(pargs, 3, "Info", f"total time elapsed: {time.time() - start}")
        for k, s in enumerate(out):
            _log(plist[k], 3, "Info", f"acceptance rate: {s.acceptance_ratio}")
        return out
    finally:
        if files:
            files.close()


def run(pargs: dict):
    """The top level of 2D/mcmc_clustering_eap_chain.jl:312-337 -> (scalar_averagers, vector_averagers, ar)."""
    return run_cases([pargs])[0]


def run_cases(plist: list, write_csv: bool = True, info: dict | None = None) -> list:
    """The top level of the planar main for every case of `plist` at once -- parsed options that differ only in their physics
    scalars, prefix and seed (one case: the command line; many: a sweep, polymer_stats_amd/sweep.py) -- as ONE ensemble."""
    pargs = plist[0]
    if pargs["numeric-type"] not in ("float64", "float128", "dec128", "big"):
        raise ReferenceError_(f"numeric-type '{pargs['numeric-type']}' not understood")    # :167
    try:
        ladder = julia_vector(pargs["burn-schedule"])                                      # :323 (evaluated whatever follows)
    except (ValueError, SyntaxError):
        raise ReferenceError_(f"burn-schedule '{pargs['burn-schedule']}' not understood")
    pool = _Pool(plist, factory=params_from_pargs, planar=True)
    try:
        if pargs["carry-burn-in"]:
            for mult in ladder:
                _stage(pool, int(pargs["burn-in"]), mult, write=False)
        elif ladder and int(pargs["burn-in"]) > 0:
            _log(pargs, 2, "Warning", "the burn-in ladder is not run: in the reference every rung and the production run start "
                                      "from a fresh chain (2D/mcmc_clustering_eap_chain.jl:151), so --burn-in / --burn-schedule "
                                      "change no output; --carry-burn-in carries the chains through the ladder")
        out = _stage(pool, int(pargs["num-steps"]), 1.0, write=write_csv)                  # :336
        for k, s in enumerate(out):
            pool.report_failures(k, s)
        if info is not None:
            info["kernel"] = pool.kernel()
    finally:
        pool.close()
    res = []
    for s in out:
        avg, se = np.array(s.avg), np.array(s.stderr)
        sas = [Averager(avg[6], se[6]), Averager(avg[13], se[13]), Averager(avg[14], se[14]), Averager(avg[15], se[15])]
        vas = [Averager(_planar(avg[0:3]), _planar(se[0:3])), Averager(_planar(avg[3:6]), _planar(se[3:6])),
               Averager(_planar(avg[7:10]), _planar(se[7:10])), Averager(_planar(avg[10:13]), _planar(se[10:13]))]
        res.append((sas, vas, s.acceptance_ratio))
    return res


def summary_lines(sas, vas, ar, pargs) -> list[str]:
    """The ten println lines, 2D/mcmc_clustering_eap_chain.jl:339-348, with 2-element vectors."""
    nb = pargs["mlen"] * pargs["num-monomers"]
    return [
        f"<r>    =   {jl_vector(get_avg(vas[0]))}",
        f"<r/nb> =   {jl_vector(np.asarray(get_avg(vas[0])) / nb)}",
        f"<rj2>  =   {jl_vector(get_avg(vas[1]))}",
        f"<r2>   =   {jl_float(get_avg(sas[0]))}",
        f"<p>    =   {jl_vector(get_avg(vas[2]))}",
        f"<pj2>  =   {jl_vector(get_avg(vas[3]))}",
        f"<p2>   =   {jl_float(get_avg(sas[1]))}",
        f"<U>    =   {jl_float(get_avg(sas[2]))}",
        f"<U2>   =   {jl_float(get_avg(sas[3]))}",
        f"AR     =   {jl_float(ar)}",
    ]


def main(argv=None) -> int:
    pargs = parse_args(argv)
    if pargs["profile"]:
        raise ReferenceError_("Not currently implemented...")           # :316
    sas, vas, ar = run(pargs)
    for line in summary_lines(sas, vas, ar, pargs):
        print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
