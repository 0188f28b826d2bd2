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

What it shares with the other two mains is in polymer_stats_amd/_host.py; here are its options, its headers and rows,
its own pstat_params fields and its protocol (the --carry-burn-in rule).
"""
from __future__ import annotations

import sys

import numpy as np

from . import _host, _lib
from ._host import Averager, summary_lines      # (reached through this module too; the ten lines, :339-348, with 2-element vectors)
from .julia_fmt import jl_row

TRAJ_HEADER = "step,r1,r3,p1,p3,U"                                             # :228
ROLL_HEADER = "step,r1,r3,r1sq,r3sq,rsq,p1,p3,p1sq,p3sq,psq,U,Usq"             # :230

# the reference's table in its order (2D/mcmc_clustering_eap_chain.jl:15-129), then ours
build_parser, parse_args, default_pargs = _host.parser_functions(_host.PLANAR, """
    E0 chain-type K1 K2 mu energy-type kT Fz Fx mlen num-monomers num-steps phi-step cluster-prob step-adjust-lb step-adjust-ub
    step-adjust-scale steps-per-adjust umbrella-sampling update-freq verbose prefix postfix stepout numeric-type profile burn-in
    burn-schedule
    carry-burn-in num-chains seed devices rng uniform-bits""".split())


def params_from_pargs(pargs: dict, num_chains: int, chain_id0: int, device: int) -> _lib.Params:
    return _lib.default_planar_params(precision=_lib.F64, cluster_prob=pargs["cluster-prob"], **_host.common_params(
        pargs, num_chains, chain_id0, device,
        {"noninteracting": _lib.NONINTERACTING, "Ising": _lib.ISING, "interacting": _lib.INTERACTING}, None))


def _planar(v) -> np.ndarray:
    """A 3-vector of the 16-vector's layout -> the planar 2-vector (component 1 in the x slot, component 2 in the z slot)."""
    v = np.asarray(v)
    return v[[0, 2]]


def _rows(pargs, step, m, ang, s):                                              # :279-298
    return jl_row([step, m[0], m[2], m[3], m[5], m[6]]), jl_row([step, *np.array(s.avg)[_lib.PLANAR_OBS_INDEX]])


def run(pargs: dict):
    """The top level of 2D/mcmc_clustering_eap_chain.jl:312-337 -> (scalar_averagers, vector_averagers, ar)."""
    return run_cases([pargs])[0]


def averagers(s):
    """A summary -> (scalar_averagers, planar vector_averagers, ar)."""
    sas, vas, ar = _host._averagers(s)
    return sas, [Averager(_planar(a.value), _planar(a.stderr)) for a in vas], ar


def run_cases(plist: list, write_csv: bool = True, info: dict | None = None, record=None) -> list:
    """The top level of the planar main for every case of `plist` at once -- parsed options that differ only in their physics
    scalars, prefix and seed (one case: the command line; many: a sweep, polymer_stats_amd/sweep.py) -- as ONE ensemble.
    `record` = a _host.Recording: the production run is recorded its way and info[record.kind] holds what that gives (_Pool.record)."""
    pargs = plist[0]
    if record:
        _host.check_recording(pargs, record, write_csv)
    _host.check_numeric_type(pargs)                                                        # :167
    ladder = _host.burn_ladder(pargs)                                                      # :323 (evaluated whatever follows)
    with _host._Pool(plist, params_from_pargs, planar=True, info=info) as pool:
        if not pargs["carry-burn-in"] and ladder and int(pargs["burn-in"]) > 0:
            _host._log(pargs, 2, "Warning", "the burn-in ladder is not run: in the reference every rung and the production run start "
                                            "from a fresh chain (2D/mcmc_clustering_eap_chain.jl:151), so --burn-in / --burn-schedule "
                                            "change no output; --carry-burn-in carries the chains through the ladder")
        # every stage is one call of the reference's mcmc(nsteps, pargs, chain) (:148-310) at kT x mult on the pool's chains
        rungs = [(m, pargs["burn-in"], False, None) for m in ladder] if pargs["carry-burn-in"] else []
        for mult, nsteps, write, rec in rungs + [(1.0, pargs["num-steps"], write_csv, record)]:         # :336
            pool.stage(mult)
            out = _host.recorded_stage(pool, int(nsteps), write, lambda p: TRAJ_HEADER, ROLL_HEADER, _rows, record=rec)
        for k, s in enumerate(out):
            pool.report_failures(k, s)
    return [averagers(s) for s in out]


def main(argv=None) -> int:
    return _host.main(parse_args(argv), "Not currently implemented...", run, summary_lines)     # :316


if __name__ == "__main__":
    sys.exit(main())
