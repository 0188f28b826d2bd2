"""Host side of the drop-in: the command line, `mcmc(nsteps, pargs)` and the three outputs of the
reference's mcmc_eap_chain.jl, with the step loop running on the GPU through libpstat (C ABI).

    python -m polymer_stats_amd.mcmc_eap_chain --chain-type dielectric -n 100 -e 1 -F 1 -N 100000 \
           --num-chains 65536 --prefix out/run1 -v 2

Same option names, short aliases, types and defaults as mcmc_eap_chain.jl:19-153; same files
(<prefix>_trajectory.csv, <prefix>_rolling.csv: :256-259,329-348) and the same ten stdout lines
(:386-395).  Options added by this implementation: --num-chains, --seed, --devices, --precision, --rng, --uniform-bits,
--burn-in, --burn-schedule.
`--num-chains C` runs C independent chains, each statistically one reference run with the given
options, and pools them; everything the reference prints is then the pooled estimate.

This is the Python twin of julia/mcmc_eap_chain.jl (no Julia toolchain exists in the build image).  What it shares with
the other two mains is in polymer_stats_amd/_host.py; here are its options, its headers and rows, and its protocol (an
optional burn-in, then --num-inits recorded runs into the same files).
"""
from __future__ import annotations

import sys

from . import _host, _lib
from ._host import Averager, CsvFiles, ReferenceError_, fresh_seed, resolve_seed, summary_lines      # (reached through this module too)
from .julia_fmt import jl_row

TRAJ_HEADER = "step,r1,r2,r3,p1,p2,p3,U"
ROLL_HEADER = "step,r1,r2,r3,r1sq,r2sq,r3sq,rsq,p1,p2,p3,p1sq,p2sq,p3sq,psq,U,Usq"

# the reference's table in its order (mcmc_eap_chain.jl:19-153), then ours
build_parser, parse_args, default_pargs = _host.parser_functions(_host.FIXED, """
    E0 chain-type K1 K2 mu energy-type kT ensemble-type Fz Fx rz rx mlen num-monomers num-steps num-inits force-init phi-step
    do-flips theta-step chain-frac-step step-adjust-lb step-adjust-ub step-adjust-scale steps-per-adjust acc umbrella-sampling
    update-freq verbose prefix postfix stepout numeric-type profile
    num-chains seed devices burn-in burn-schedule rng precision uniform-bits""".split())


def params_from_pargs(pargs: dict, num_chains: int, chain_id0: int, device: int) -> _lib.Params:
    """pargs -> pstat_params, with the reference's error() branches (inc/eap_chain.jl:81-105)."""
    return _lib.default_params(do_flips=1 if pargs["do-flips"] else 0, **_host.common_params(
        pargs, num_chains, chain_id0, device,
        {"noninteracting": _lib.NONINTERACTING, "interacting": _lib.INTERACTING, "Ising": _lib.ISING},
        {"f32": _lib.F32, "f64": _lib.F64, "q16": _lib.Q16}))


def _rows(pargs, step, micro, ang, s):                          # :329-348
    return jl_row([step, *micro]), jl_row([step, *s.avg])


def mcmc(nsteps: int, pargs: dict):
    """mcmc(nsteps, pargs) of mcmc_eap_chain.jl:171-376 -> (scalar_averagers, vector_averagers, ar)."""
    return mcmc_cases(nsteps, [pargs])[0]


averagers = _host._averagers      # a summary -> (scalar_averagers, vector_averagers, ar)


def mcmc_cases(nsteps: int, plist: list, write_csv: bool = True, info: dict | None = None, record=None) -> list:
    """mcmc(nsteps, pargs) for every case of `plist` at once -- parsed options that differ only in their physics scalars,
    prefix and seed (one case: the command line; many: a sweep, polymer_stats_amd/sweep.py) -- as ONE ensemble: one launch
    per init for all of them, or, with the two CSV files of every case (`write_csv`), one per --stepout steps followed by the
    launch that records the row of every case on the device (_Pool.recorded).  `record` = a _host.Recording: the run is
    recorded its way and info[record.kind] holds what that gives (_host.check_recording, _Pool.record)."""
    pargs = plist[0]
    if record:
        _host.check_recording(pargs, record, write_csv)
    if pargs["acc"] != "metropolis":
        raise ReferenceError_(f"'{pargs['acc']}' acceptance criteria has not yet been implemented.")  # :184
    _host.check_numeric_type(pargs)                                                                    # :195
    if pargs["ensemble-type"] != "force":
        raise ReferenceError_("'end-to-end' ensemble is an experimental option of the reference; "
                              "it has no device implementation")
    with _host._Pool(plist, params_from_pargs, info=info) as pool:
        if pargs["burn-in"] > 0:
            ladder = [float(x) for x in pargs["burn-schedule"].strip("[] ").replace(",", ";").split(";") if x.strip()]
            pool.burn_in(int(pargs["burn-in"]), ladder or [1.0])

        def inits():                                                 # :266
            for init in range(1, pargs["num-inits"] + 1):
                yield f"init:    {init} / {pargs['num-inits']}"      # (the run of nsteps happens here)
                if init < pargs["num-inits"]:                        # :352-361
                    pool.reinit(bool(pargs["force-init"]))
        out = _host.recorded_stage(pool, nsteps, write_csv, lambda p: TRAJ_HEADER, ROLL_HEADER, _rows, runs=inits(),
                                   report=pool.report_failures, record=record)
    return [averagers(s) for s in out]


def run_cases(plist: list, write_csv: bool = True, info: dict | None = None, record=None) -> list:
    """mcmc_cases for each case's own --num-steps: the call every main offers (polymer_stats_amd/sweep.py)."""
    return mcmc_cases(int(plist[0]["num-steps"]), plist, write_csv=write_csv, info=info, record=record)


def main(argv=None) -> int:
    pargs = parse_args(argv)
    if pargs["ensemble-type"] == "end-to-end":
        _host._log(pargs, 2, "Warning", "'end-to-end' ensemble is an experimental option; it has not been validated.")
    return _host.main(pargs, "not implemented for the HPC env", lambda p: mcmc(p["num-steps"], p), summary_lines)     # :379


if __name__ == "__main__":
    sys.exit(main())
