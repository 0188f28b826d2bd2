"""What the three hosts (mcmc_eap_chain, mcmc_clustering_eap_chain, mcmc_clustering_eap_chain_2d) share: the option
table, the seed and the logging, pargs -> the common pstat_params fields, the pool of one ensemble's shards, the recorded
stage that writes the two CSV files, the stdout lines and the body of main().  What differs between the mains comes in from
them as data or as a function (their option names in their order, their headers, their row formatter, their protocol);
nothing here asks which main is running.  The hosts are thin: every number they print comes out of the library.
"""
from __future__ import annotations

import argparse
import ast
import math
import operator
import os
import sys
import time
from dataclasses import dataclass

import numpy as np

from . import _lib
from .ensemble import Ensemble, summary_from_reduction
from .julia_fmt import jl_float, jl_vector

# Device memory one handle's series may take: the rows of a recorded run are read back and written out in chunks of
# as many rows as fit (a row is ncases x (NRED + 7 [+ 2n]) doubles; at least one row per chunk).
SERIES_BUDGET_BYTES = 256 << 20

FIXED, CLUSTER, PLANAR = "mcmc_eap_chain", "mcmc_clustering_eap_chain", "mcmc_clustering_eap_chain_2d"


class ReferenceError_(RuntimeError):
    """Raised where the reference calls error(...) -- same message text."""


# ---------------------------------------------------------------------------------------------- the option table
# name (= dest = ArgParse.jl's dict key; the flag is --name): (short alias, type | "flag" for store_true, default, help
# [, {main: what that main states differently}]).  A main has the rows it names, in the order it names them (build_parser).
OPTIONS = {
    # --- the reference's tables: mcmc_eap_chain.jl:19-153, mcmc_clustering_eap_chain.jl:14-152, 2D/mcmc_clustering_eap_chain.jl:15-129
    "E0": ("-e", float, 0.0, "magnitude of electric field"),
    "chain-type": ("-T", str, "dielectric", "chain type (dielectric|polar)"),
    "K1": ("-J", float, 1.0, "dipole susceptibility along the monomer axis (dielectric chain)"),
    "K2": ("-K", float, 0.0, "dipole susceptibility orthogonal to the monomer axis (dielectric chain)"),
    "mu": ("-m", float, 1e-2, "dipole magnitude (electret chain)"),
    "bend-mod": ("-a", float, 0.0, "bending modulus of chain"),
    "bend-angle": ("-g", float, 0.0, "zero energy bond angle"),
    "energy-type": ("-u", str, "noninteracting", "energy type (noninteracting|interacting)",
                    {CLUSTER: dict(default="Ising", help="energy type (interacting|cutoff|Ising|noninteracting)"),
                     PLANAR: dict(help="energy type (noninteracting|interacting|Ising)")}),
    "cutoff-radius": (None, float, 7.5, "cut off radius (units of monomer lengths)"),
    "kT": ("-k", float, 1.0, "dimensionless temperature"),
    "ensemble-type": ("-E", str, "force", "ensemble type (force|end-to-end)"),
    "Fz": ("-F", float, 0.0, "force in the z-direction (direction of E-field; force ensemble)"),
    "Fx": ("-G", float, 0.0, "force in the x-direction (force ensemble)"),
    "rz": ("-z", float, 0.0, "end-to-end vector in the z-direction (etoe ensemble)"),
    "rx": ("-x", float, 0.0, "end-to-end vector in the x-direction (etoe ensemble)"),
    "mlen": ("-b", float, 1.0, "monomer length"),
    "num-monomers": ("-n", int, 100, "number of monomers"),
    "num-steps": ("-N", int, int(1e6), "number of steps", {FIXED: dict(default=int(1e5))}),
    "num-inits": ("-M", int, 1, "number of random initializations"),
    "force-init": ("-I", "flag", False, "force each random initialization (false to use metro.)"),
    "phi-step": ("-p", float, 3 * math.pi / 8, "maximum phi step length"),
    "do-flips": (None, "flag", False, "trial moves with flipping monomers"),
    "theta-step": ("-q", float, 3 * math.pi / 16, "maximum theta step length"),
    "chain-frac-step": ("-f", float, 0.15, "fraction of monomers to step (end-to-end ensemble)"),
    "cluster-prob": (None, float, 0.5, "probability of flipping a cluster"),
    "step-adjust-lb": ("-L", float, 0.15, "adjust step sizes if acc. ratio below this threshold"),
    "step-adjust-ub": ("-U", float, 0.40, "adjust step sizes if acc. ratio above this threshold", {FIXED: dict(default=0.55)}),
    "step-adjust-scale": ("-A", float, 1.1, "scale factor for adjusting step sizes (> 1.0)"),
    "steps-per-adjust": ("-S", int, 2500, "steps between step size adjustments"),
    "acc": ("-a", str, "metropolis", "acceptance function (metropolis|kawasaki)"),
    "umbrella-sampling": ("-B", "flag", False, "use umbrella sampling (w/ electrostatic weight function)"),
    "update-freq": (None, float, 15.0, "update frequency (seconds)"),
    "verbose": ("-v", int, 3, "verbosity level: 0-nothing, 1-errors, 2-warnings, 3-info"),
    "prefix": ("-P", str, "eap-mcmc", "prefix for output files"),
    "postfix": ("-Q", str, "", "postfix for output files"),
    "stepout": ("-s", int, 500, "steps between storing microstates"),
    "numeric-type": (None, str, "float64", "numerical data type for averaging (float64|float128|dec128|big)"),
    "burn-in": (None, int, 50000, "steps for burn-in; i.e. steps before averaging",
                {FIXED: dict(default=0, help="steps discarded before averaging, per rung of --burn-schedule (0 = the reference's "
                                             "behaviour: record from step 1)")}),
    "burn-schedule": (None, str, "[1000; 100; 10; 2; 1]", "temperature schedule for burn-in",
                      {FIXED: dict(default="[1]", help="kT multipliers of the burn-in ladder, e.g. '[1000; 100; 10; 2; 1]' "
                                                       "(mcmc_clustering_eap_chain.jl:138-141)")}),
    "x0": (None, str, None, "initial configuration"),
    "dx0": (None, str, "[2*pi, 1e-1]", "random perturbation of x0"),
    "profile": ("-Z", "flag", False, "profile the program"),
    # --- ours
    "carry-burn-in": (None, "flag", False,
                      "run the burn-in ladder on the chains and carry them into the production run (the reference's ladder starts "
                      "every rung and the production run from a fresh chain, so it changes no output: without this option it is "
                      "not run)"),
    "num-chains": (None, int, 4096, "independent chains run at once on the GPU(s) and pooled"),
    "seed": (None, int, None, "seed of the per-chain generators; default: fresh OS entropy per run, like the reference's unseeded "
                              "RNG (the seed drawn is echoed on stderr at --verbose >= 2)"),
    "devices": (None, str, "0", "comma-separated HIP device ordinals; chains are sharded over them"),
    "rng": (None, str, "mwc64x", "per-chain generator: mwc64x | xoshiro128++"),
    "precision": (None, str, "f64", "device arithmetic: f64 (the reference's Float64; default) | f32 (fast path: f32 state, f64 "
                                    "running sums; not for collapsed chains of the pair energies) | q16 (lattice angles, f32 arithmetic)"),
    "uniform-bits": (None, int, 0, "random bits of the Metropolis draw rand(): 0 = the precision's default (53 for f64, 23 for f32) | "
                                   "23 | 53 (f64 only)",
                     {FIXED: dict(help="random bits of the Metropolis draw rand() (mcmc_eap_chain.jl:287): 0 = the precision's default "
                                       "(53 for f64, like Julia's Float64 rand(); 23 for f32 / q16) | 23 | 53 (f64 only)"),
                      PLANAR: dict(help="random bits of the Metropolis draw rand(): 0 = the default (53, like Julia's Float64 "
                                        "rand()) | 23 | 53")}),
}


def parser_functions(main: str, names: list[str]):
    """(build_parser, parse_args, default_pargs) of the main called `main`, which has the rows `names` in that order."""
    def build_parser() -> argparse.ArgumentParser:
        p = argparse.ArgumentParser(prog=main, add_help=True, allow_abbrev=False)
        for name in names:
            alias, kind, default, text, *own = OPTIONS[name]
            kw = {"default": default, "help": text, **(own[0].get(main, {}) if own else {})}
            if kind == "flag":
                kw = dict(action="store_true", help=kw["help"])
            else:
                kw["type"] = kind
            p.add_argument("--" + name, *([alias] if alias else []), dest=name, **kw)
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

    return build_parser, parse_args, default_pargs


# ---------------------------------------------------------------------------------------------- arithmetic literals
_BIN = {ast.Add: operator.add, ast.Sub: operator.sub, ast.Mult: operator.mul, ast.Div: operator.truediv,
        ast.Pow: operator.pow}


def arith(node, names={}):
    """The value of a parsed arithmetic literal: numbers (integers stay integers, no bool), + - * / **, and `names`."""
    if isinstance(node, ast.Constant) and isinstance(node.value, (int, float)) and not isinstance(node.value, bool):
        return node.value
    if isinstance(node, ast.Name) and node.id in names:
        return names[node.id]
    if isinstance(node, ast.UnaryOp) and isinstance(node.op, (ast.USub, ast.UAdd)):
        v = arith(node.operand, names)
        return -v if isinstance(node.op, ast.USub) else v
    if isinstance(node, ast.BinOp) and type(node.op) in _BIN:
        return _BIN[type(node.op)](arith(node.left, names), arith(node.right, names))
    raise ValueError("not a number")


def number(text: str, names={}):
    """`2*pi`, `10^-2`, `1e-1` -> its value (the reference eval()s such strings; only literals and `names` are understood)."""
    return arith(ast.parse(text.strip().replace("^", "**"), mode="eval").body, names)


def julia_vector(text: str) -> list[float]:
    """A Julia vector literal of arithmetic constants, '[2*pi, 1e-1]' or '[1000; 100; 10]' -> floats."""
    t = text.strip()
    if not (t.startswith("[") and t.endswith("]")):
        raise ValueError(text)
    return [float(number(x, {"pi": math.pi, "π": math.pi})) for x in t[1:-1].replace(";", ",").split(",") if x.strip()]


# ---------------------------------------------------------------------------------------------- seed, logging, checks
def fresh_seed() -> int:
    """A new 63-bit seed per call: OS entropy, mixed with the clock and the pid in case the pool is a stub.
    The reference never seeds Julia's RNG, so repeated identical command lines give independent samples
    (run/interacting-compare-with-clustering_2021-09-28.jl:26-27 launches each case 25 times and takes the
    scatter as its error bar); the drop-in must do the same unless --seed is given."""
    v = int.from_bytes(os.urandom(8), "little") ^ time.time_ns() ^ (os.getpid() << 40)
    return v & 0x7FFFFFFFFFFFFFFF


WIDE_TYPES = {"float128": "80-bit extended (numpy.longdouble)", "dec128": "80-bit extended (numpy.longdouble)",
              "big": "80-bit extended (numpy.longdouble)"}


def _log(pargs, level: int, tag: str, msg: str):
    # Logging to stderr gated by --verbose (mcmc_eap_chain.jl:157-165): 3 info, 2 warn, 1 error
    if pargs["verbose"] >= level:
        print(f"[ {tag}: {msg}", file=sys.stderr)


def resolve_seed(pargs: dict) -> int:
    """--seed as given, or (once per pargs) a fresh one, echoed on stderr at --verbose >= 2 so the run can be repeated."""
    if pargs.get("seed") is None:
        pargs["seed"] = fresh_seed()
        _log(pargs, 2, "Info", f"seed: {pargs['seed']} (fresh entropy; pass --seed {pargs['seed']} to reproduce this run)")
    return pargs["seed"]


def check_numeric_type(pargs: dict):
    if pargs["numeric-type"] not in ("float64", *WIDE_TYPES):                       # mcmc_eap_chain.jl:195
        raise ReferenceError_(f"numeric-type '{pargs['numeric-type']}' not understood")


def parse_hist(text: str):
    """One --hist CHANNEL:LO:HI:NBINS of tools/run_sweep.py -> (channel name, lo, hi, nbins)."""
    parts = str(text).split(":")
    try:
        if len(parts) != 4 or parts[0] not in _lib.HC_NAMES:
            raise ValueError
        lo, hi, nbins = float(parts[1]), float(parts[2]), int(parts[3])
    except ValueError:
        raise ReferenceError_(f"--hist '{text}' not understood: CHANNEL:LO:HI:NBINS with CHANNEL one of {', '.join(_lib.HC_NAMES)}")
    if not (np.isfinite(lo) and np.isfinite(hi) and hi > lo and nbins >= 1):
        raise ReferenceError_(f"--hist '{text}': needs finite LO < HI and NBINS >= 1")
    return parts[0], lo, hi, nbins


CORR_MIN_RECORDS = 32      # the blocking transform's default min_blocks: a .corr's standard errors need that many records


def parse_corr(text: str):
    """--corr MAXLAG[:nn,zz,mm] of tools/run_sweep.py -> (max_lag, channel names in the order of CORR_NAMES)."""
    head, _, tail = str(text).partition(":")
    names = [c for c in tail.split(",") if c != ""] if tail else ["nn"]
    try:
        max_lag = int(head)
        if max_lag < 0 or not names or any(c not in _lib.CORR_NAMES for c in names):
            raise ValueError
    except ValueError:
        raise ReferenceError_(f"--corr '{text}' not understood: MAXLAG[:CHANNELS] with MAXLAG >= 0 and CHANNELS a comma-separated "
                              f"choice of {', '.join(_lib.CORR_NAMES)}")
    return max_lag, tuple(c for c in _lib.CORR_NAMES if c in names)


def parse_shape(text: str):
    """--shape [AXIS:QMAX:NQ[,AXIS:QMAX:NQ...]] of tools/run_sweep.py -> ("shape", [[qx, qy, qz], ...]): every entry gives NQ
    wave-vectors QMAX (1 .. NQ) / NQ along AXIS (x, y or z); an empty text: no wave-vector, the gyration block only."""
    q = []
    for entry in [t for t in str(text or "").split(",") if t.strip() != ""]:
        parts = entry.strip().split(":")
        try:
            axis, qmax, nq = "xyz".index(parts[0].strip().lower()) if len(parts[0].strip()) == 1 else -1, float(parts[1]), int(parts[2])
            if len(parts) != 3 or axis < 0 or nq < 1 or not np.isfinite(qmax) or qmax <= 0.0:
                raise ValueError
        except (ValueError, IndexError):
            raise ReferenceError_(f"--shape '{text}' not understood: AXIS:QMAX:NQ[,AXIS:QMAX:NQ...] with AXIS one of x, y, z, "
                                  "QMAX > 0 and NQ >= 1")
        for j in range(1, nq + 1):
            v = [0.0, 0.0, 0.0]
            v[axis] = qmax * j / nq
            q.append(v)
    if len(q) > _lib.SHAPE_MAX_Q:
        raise ReferenceError_(f"--shape '{text}': {len(q)} wave-vectors, at most {_lib.SHAPE_MAX_Q}")
    return "shape", q


def parse_pdist(text: str):
    """--pdist RMAX:NBINS[,sep=MAXSEP][,min=MINSEP][,q=QMAX:NQ] of tools/run_sweep.py -> ("pdist", dict(rmax, nbins, max_sep,
    min_sep, q)): the distances below RMAX (absolute units) in NBINS bins (NBINS 0: no histogram), R2(s) up to s = MAXSEP
    (default -1: n - 1), closest approach and histogram over the pairs at least MINSEP apart along the chain (default 1), and the
    Debye S(q) at the NQ magnitudes QMAX (1 .. NQ) / NQ (default: none)."""
    parts = [t.strip() for t in str(text).split(",")]
    spec = dict(max_sep=-1, min_sep=1, q=[])
    try:
        head = parts[0].split(":")
        if len(head) != 2:
            raise ValueError
        spec["rmax"], spec["nbins"] = float(head[0]), int(head[1])
        if not np.isfinite(spec["rmax"]) or spec["rmax"] <= 0.0 or spec["nbins"] < 0:
            raise ValueError
        for entry in parts[1:]:
            key, _, value = entry.partition("=")
            if key == "sep" and int(value) >= -1:
                spec["max_sep"] = int(value)
            elif key == "min" and int(value) >= 1:
                spec["min_sep"] = int(value)
            elif key == "q" and len(value.split(":")) == 2:
                qmax, nq = float(value.split(":")[0]), int(value.split(":")[1])
                if nq < 1 or not np.isfinite(qmax) or qmax <= 0.0:
                    raise ValueError
                spec["q"] = [qmax * j / nq for j in range(1, nq + 1)]
            else:
                raise ValueError
    except ValueError:
        raise ReferenceError_(f"--pdist '{text}' not understood: RMAX:NBINS[,sep=MAXSEP][,min=MINSEP][,q=QMAX:NQ] with RMAX > 0, "
                              "NBINS >= 0, MAXSEP >= -1, MINSEP >= 1, QMAX > 0 and NQ >= 1")
    if spec["nbins"] > _lib.PDIST_MAX_BINS:
        raise ReferenceError_(f"--pdist '{text}': {spec['nbins']} bins, at most {_lib.PDIST_MAX_BINS}")
    if len(spec["q"]) > _lib.PDIST_MAX_Q:
        raise ReferenceError_(f"--pdist '{text}': {len(spec['q'])} magnitudes, at most {_lib.PDIST_MAX_Q}")
    return "pdist", spec


def parse_energy(text: str):
    """--energy MAXSEP[,cut=RCUT] of tools/run_sweep.py -> ("energy", dict(max_sep, cutoff)): the dipole-dipole sum by separation
    up to s = MAXSEP (-1: n - 1), the rest in one column, and with RCUT the sum inside that radius in monomer lengths (default:
    the cases' own --cutoff-radius under --energy-type cutoff, no such column otherwise)."""
    parts = [t.strip() for t in str(text).split(",")]
    spec = dict(max_sep=-1, cutoff=None)
    try:
        spec["max_sep"] = int(parts[0])
        if spec["max_sep"] < -1 or len(parts) > 2:
            raise ValueError
        for entry in parts[1:]:
            key, _, value = entry.partition("=")
            if key != "cut" or not np.isfinite(float(value)) or float(value) <= 0.0:
                raise ValueError
            spec["cutoff"] = float(value)
    except ValueError:
        raise ReferenceError_(f"--energy '{text}' not understood: MAXSEP[,cut=RCUT] with MAXSEP >= -1 and RCUT > 0")
    return "energy", spec


# ---------------------------------------------------------------------------------------------- recording the production run
@dataclass(frozen=True)
class Recording:
    """How the production run is recorded in place of --stepout rows: `kind` names a row of RECORDING_KINDS, `spec` is what the
    row's `parse` returns (for error_bars the batch count N).  One kind by construction: the kinds exclude each other."""
    kind: str
    spec: object


def _check_batches(pargs: dict, nbatches: int):
    if nbatches < 32:
        raise ReferenceError_(f"--error-bars {nbatches}: the blocking transform needs at least 32 batches")
    if int(pargs["num-steps"]) < nbatches:
        raise ReferenceError_(f"--error-bars {nbatches} needs --num-steps >= {nbatches}: a batch is num-steps / {nbatches} steps")


def _check_hist_specs(pargs: dict, specs):
    if not 1 <= len(specs) <= _lib.HIST_MAX_SPECS:
        raise ReferenceError_(f"--hist: between 1 and {_lib.HIST_MAX_SPECS} histograms, not {len(specs)}")
    if sum(s[3] for s in specs) > _lib.HIST_MAX_BINS:
        raise ReferenceError_(f"--hist: {sum(s[3] for s in specs)} bins per case, at most {_lib.HIST_MAX_BINS}")
    stepout = int(pargs["stepout"])
    if not 1 <= stepout <= int(pargs["num-steps"]):
        raise ReferenceError_(f"--hist samples every --stepout steps of the production run: --stepout {stepout} must be in 1 .. "
                              f"--num-steps {pargs['num-steps']}")


def _check_records(flag: str, pargs: dict):
    """--corr, --shape, --pdist and --energy (`flag`) keep a row per record: the run must give the blocking transform enough of them."""
    stepout = int(pargs["stepout"])
    if not 1 <= stepout <= int(pargs["num-steps"]) or int(pargs["num-steps"]) // stepout < CORR_MIN_RECORDS:
        raise ReferenceError_(f"{flag} takes a record every --stepout steps of the production run and its standard errors from "
                              f"at least {CORR_MIN_RECORDS} of them: --stepout {stepout} must be in 1 .. --num-steps "
                              f"{pargs['num-steps']} / {CORR_MIN_RECORDS}")


def _check_lags(pargs: dict, spec):
    if spec[0] > int(pargs["num-monomers"]) - 1:
        raise ReferenceError_(f"--corr: lag {spec[0]} is beyond n - 1 = {int(pargs['num-monomers']) - 1}")
    _check_records("--corr", pargs)


def _check_wave_vectors(pargs: dict, spec):
    _check_records("--shape", pargs)
    reach = float(pargs["mlen"]) * int(pargs["num-monomers"])
    for v in spec[1]:      # (the library refuses such a phase too)
        if sum(abs(c) for c in v) * reach >= 1.0e5:
            raise ReferenceError_(f"--shape: |q| b n = {sum(abs(c) for c in v) * reach:g} for q = {v} is not below 1e5")


def _check_pdist(pargs: dict, spec):
    _check_records("--pdist", pargs)
    n, o = int(pargs["num-monomers"]), spec[1]
    if n < 2:
        raise ReferenceError_(f"--pdist: a chain of n = {n} monomers has no pair")
    if o["max_sep"] > n - 1 or o["min_sep"] > n - 1:
        raise ReferenceError_(f"--pdist: sep={o['max_sep']}, min={o['min_sep']} must not be beyond n - 1 = {n - 1}")
    reach = float(pargs["mlen"]) * n
    for v in o["q"]:       # (the library refuses such a phase too)
        if v * reach >= 1.0e5:
            raise ReferenceError_(f"--pdist: q b n = {v * reach:g} for q = {v} is not below 1e5")


def _check_energy(pargs: dict, spec):
    _check_records("--energy", pargs)
    n = int(pargs["num-monomers"])
    if spec[1]["max_sep"] > n - 1:
        raise ReferenceError_(f"--energy: sep {spec[1]['max_sep']} must not be beyond n - 1 = {n - 1}")


def _totals_and_error_bars(g):
    """What a Corr, a Shape or a Pdist with kept rows gives at the end of a recorded run."""
    return g.read(), g.error_bars(min_blocks=CORR_MIN_RECORDS)


def _every_stepout(nsteps, spec, stepout):
    return nsteps // stepout, stepout


@dataclass(frozen=True)
class _Kind:
    """Everything that is particular to one kind of Recording."""
    flag: str
    ext: str                        # of the file beside every <case>.out
    parse: object                   # the flag's value(s) -> spec
    words: tuple                    # of the shared refusals (check_recording): the production run is recorded as ..., the devices do
                                    # not merge their ..., a re-initialisation falls between ..., why not under umbrella sampling,
                                    # why float64 only
    check: object                   # (pargs, spec): the kind's own refusals
    records: object                 # (nsteps, spec, --stepout) -> (how many records, how many steps apart)
    open: object                    # (ensemble, spec, records) -> the recorder
    advance: object                 # (ensemble, recorder, nsteps, stepout): the Ensemble.advance_* that drives it
    read: object                    # recorder -> what info[kind] holds at the end
    lines: object                   # (main, that, spec, k, case k's pargs) -> the lines of the file
    restore_after_failure: bool = True      # a failed recorded run puts the checkpoint back


_GAUGE = "the samples carry per-chain weights whose gauge the %s do not hold"
_LIKE_HIST = "like --hist it is offered for float64 runs only"
RECORDINGS = {
    "error_bars": _Kind(
        flag="--error-bars", ext=".err", parse=int,
        words=("batches", "series", "batches", "the recorded means are ratios with per-chain normalizers that the rows do not hold",
               "the batches are differences of the device's Float64 reductions"),
        check=_check_batches,
        records=lambda nsteps, n, stepout: (n, nsteps // n),
        open=lambda e, n, nrec: e.open_series(n),
        advance=Ensemble.advance_series,
        read=lambda series: series.error_bars(),
        lines=lambda main, eb, n, k, p: error_lines(main, eb, k, p),
        restore_after_failure=False),
    "hist": _Kind(
        flag="--hist", ext=".hist", parse=lambda texts: [parse_hist(t) for t in texts],
        words=("histograms", "histograms", "samples", _GAUGE % "counts", "the samples are the device's Float64 microstates"),
        check=_check_hist_specs,
        records=_every_stepout,
        open=lambda e, specs, nrec: e.open_hist([_lib.hist_spec(channel, nbins, lo, hi) for channel, lo, hi, nbins in specs]),
        advance=Ensemble.advance_hist,
        read=lambda h: h.read(),
        lines=lambda main, res, specs, k, p: hist_lines(res, specs, k, int(p["num-chains"]))),
    "corr": _Kind(
        flag="--corr", ext=".corr", parse=parse_corr,
        words=("correlations", "sums", "records", _GAUGE % "sums", _LIKE_HIST),
        check=_check_lags,
        records=_every_stepout,
        open=lambda e, spec, nrec: e.open_corr(spec[1], spec[0], capacity_rows=nrec),
        advance=Ensemble.advance_corr,
        read=_totals_and_error_bars,
        lines=lambda main, res, spec, k, p: corr_lines(*res, k)),
    "shape": _Kind(
        flag="--shape", ext=".shape", parse=parse_shape,
        words=("shape columns", "sums", "records", _GAUGE % "sums", _LIKE_HIST),
        check=_check_wave_vectors,
        records=_every_stepout,
        open=lambda e, spec, nrec: e.open_shape(spec[1], capacity_rows=nrec),
        advance=Ensemble.advance_shape,
        read=_totals_and_error_bars,
        lines=lambda main, res, spec, k, p: shape_lines(*res, k)),
    "pdist": _Kind(
        flag="--pdist", ext=".pdist", parse=parse_pdist,
        words=("pair-distance columns", "sums", "records", _GAUGE % "sums", _LIKE_HIST),
        check=_check_pdist,
        records=_every_stepout,
        open=lambda e, spec, nrec: e.open_pdist(spec[1]["max_sep"], spec[1]["min_sep"],
                                                (spec[1]["nbins"], spec[1]["rmax"]) if spec[1]["nbins"] else None, spec[1]["q"],
                                                capacity_rows=nrec),
        advance=Ensemble.advance_pdist,
        read=_totals_and_error_bars,
        lines=lambda main, res, spec, k, p: pdist_lines(*res, k)),
}
# Every kind of Recording: the table above and the energy recording, a row like the others that joins here (the pair-distance
# tests pin RECORDINGS itself at its five rows, pdist last).  Every look-up of a kind goes through this one.
RECORDING_KINDS = {
    **RECORDINGS,
    "energy": _Kind(
        flag="--energy", ext=".energy", parse=parse_energy,
        words=("energy columns", "sums", "records", _GAUGE % "sums", _LIKE_HIST),
        check=_check_energy,
        records=_every_stepout,
        open=lambda e, spec, nrec: e.open_energy(spec[1]["max_sep"], spec[1]["cutoff"], capacity_rows=nrec),
        advance=Ensemble.advance_energy,
        read=lambda g: (*_totals_and_error_bars(g), g.model_error_bars(min_blocks=CORR_MIN_RECORDS)),
        lines=lambda main, res, spec, k, p: energy_lines(*res, k)),
}


def check_recording(pargs: dict, rec: Recording, write_csv: bool = False, devices: int | None = None):
    """What a Recording (tools/run_sweep.py's --error-bars, --hist, --corr, --shape, --pdist, --energy; run_cases(..., record=rec)) cannot be
    combined with, refused before any GPU work: the kind's own limits, then what all kinds refuse.  `devices`: how many hold the
    chains (default: those --devices names)."""
    row = RECORDING_KINDS[rec.kind]
    flag = row.flag
    recorded_as, merged, between, no_umbrella, float64_only = row.words
    if devices is None:
        devices = len([d for d in str(pargs["devices"]).split(",") if d != ""][:max(1, int(pargs["num-chains"]))])
    row.check(pargs, rec.spec)
    if write_csv:
        raise ReferenceError_(f"{flag} cannot be combined with --csv: the production run is recorded as {recorded_as}, not as "
                              "--stepout rows")
    if devices > 1:
        raise ReferenceError_(f"{flag} needs one device, not {devices}: the devices hold different chains of a case and "
                              f"their {merged} are not merged")
    if int(pargs.get("num-inits", 1)) != 1:
        raise ReferenceError_(f"{flag} cannot be combined with --num-inits {pargs['num-inits']}: a re-initialisation "
                              f"between {between} is not a stationary series")
    if pargs["umbrella-sampling"]:
        raise ReferenceError_(f"{flag} cannot be combined with --umbrella-sampling: {no_umbrella}")
    if pargs["numeric-type"] != "float64":
        raise ReferenceError_(f"{flag} cannot be combined with --numeric-type {pargs['numeric-type']}: {float64_only}")


def burn_ladder(pargs: dict) -> list[float]:
    """--burn-schedule of the two clustering mains: a Julia vector literal of kT multipliers."""
    try:
        return julia_vector(pargs["burn-schedule"])
    except (ValueError, SyntaxError):
        raise ReferenceError_(f"burn-schedule '{pargs['burn-schedule']}' not understood")


def common_params(pargs: dict, num_chains: int, chain_id0: int, device: int, energy_types: dict, precisions: dict | None) -> dict:
    """pargs -> the pstat_params fields every main sets, as keyword arguments of _lib.default_params, with the reference's
    error() branches (inc/eap_chain.jl:81-105).  `energy_types` / `precisions`: what the main allows (None: it has no
    --precision and sets the field itself); a main without --theta-step leaves that field alone."""
    resolve_seed(pargs)
    ct = {"dielectric": _lib.DIELECTRIC, "polar": _lib.POLAR}.get(pargs["chain-type"])
    if ct is None:
        raise ReferenceError_("chain-type is not understood.")                       # inc/eap_chain.jl:86
    et = energy_types.get(pargs["energy-type"])
    if et is None:
        raise ReferenceError_("energy-type is not understood.")                      # inc/eap_chain.jl:104
    own = {}
    if precisions is not None:
        own["precision"] = precisions.get(pargs["precision"])
        if own["precision"] is None:
            raise ReferenceError_(f"precision '{pargs['precision']}' not understood")
    rng = {"mwc64x": _lib.RNG_MWC64X, "xoshiro128++": _lib.RNG_XOSHIRO128PP}.get(pargs["rng"])
    if rng is None:
        raise ReferenceError_(f"rng '{pargs['rng']}' not understood")
    if "theta-step" in pargs:
        own["theta_step"] = pargs["theta-step"]
    return dict(
        E0=pargs["E0"], K1=pargs["K1"], K2=pargs["K2"], mu=pargs["mu"], kT=pargs["kT"],
        Fz=pargs["Fz"], Fx=pargs["Fx"], b=pargs["mlen"], phi_step=pargs["phi-step"],
        adj_lb=pargs["step-adjust-lb"], adj_ub=pargs["step-adjust-ub"], adj_scale=pargs["step-adjust-scale"],
        steps_per_adjust=pargs["steps-per-adjust"], n=pargs["num-monomers"], num_chains=num_chains,
        seed=pargs["seed"], chain_id0=chain_id0, chain_type=ct, energy_type=et,
        umbrella=1 if pargs["umbrella-sampling"] else 0, device=device, rng=rng,
        uniform_bits=int(pargs.get("uniform-bits", 0)), **own)


# ---------------------------------------------------------------------------------------------- averagers
@dataclass
class Averager:
    """What the caller of mcmc() gets back in place of a StandardAverager (inc/average.jl:8-48)."""
    value: object
    stderr: object

    def get_avg(self):
        return self.value


def get_avg(a: Averager):
    return a.get_avg()


def _averagers(s):
    avg, se = np.array(s.avg), np.array(s.stderr)
    sas = [Averager(avg[6], se[6]), Averager(avg[13], se[13]), Averager(avg[14], se[14]), Averager(avg[15], se[15])]
    vas = [Averager(avg[0:3], se[0:3]), Averager(avg[3:6], se[3:6]), Averager(avg[7:10], se[7:10]),
           Averager(avg[10:13], se[10:13])]
    return sas, vas, s.acceptance_ratio


# ---------------------------------------------------------------------------------------------- the pool
class _Pool:
    """The cases of one ensemble -- one for the command line, many for a sweep (polymer_stats_amd/sweep.py; they differ only
    in their physics scalars, pstat_create) --, every case's chains sharded over one or more devices in this process;
    reductions merged on the host (every entry of the reduction vector is additive).  `factory` is the main's
    params_from_pargs.  As a context manager it closes its handles, and on success leaves the kernel's name in `info`."""

    def __init__(self, pargs, factory, planar=False, info=None):
        self.plist = plist = pargs if isinstance(pargs, list) else [pargs]
        self.info = info
        for p in plist:
            resolve_seed(p)      # before the shards are made: every device gets the same seed, disjoint chain ids
        p0 = plist[0]
        self.numeric_type = p0.get("numeric-type", "float64")
        if self.numeric_type != "float64":
            # mcmc_eap_chain.jl:186-197 switches the averagers' accumulation type.  Here the per-chain sums are
            # Float64 on the device (the reference's default); what the option changes is the merge over chains.
            _log(p0, 2, "Warning", f"--numeric-type {self.numeric_type}: per-chain sums are Float64 on the device; the "
                                   f"merge over chains is carried out in {WIDE_TYPES[self.numeric_type]}")
        devices = [int(d) for d in str(p0["devices"]).split(",") if d != ""]
        total = int(p0["num-chains"])
        if total < 1:
            raise ReferenceError_("num-chains must be >= 1")
        devices = devices[:total] or [0]
        base, extra = divmod(total, len(devices))
        self.parts, self.counts = [], []
        first = 0
        for i, dev in enumerate(devices):
            cnt = base + (1 if i < extra else 0)
            self.parts.append(Ensemble([factory(p, cnt, first, dev) for p in plist], planar=planar))
            self.counts.append(cnt)
            first += cnt
        self.steps = 0

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        try:
            if exc_type is None and self.info is not None:
                self.info["kernel"] = self.kernel()
        finally:
            self.close()

    def advance(self, n):
        for e in self.parts:
            e.advance(n)            # asynchronous: the devices run concurrently
        self.steps += n

    def reinit(self, force):
        for e in self.parts:
            e.reinit(force)

    def burn_in(self, nsteps, multipliers):
        """Run the temperature ladder (every case's own kT times the rung's multiplier) without keeping anything it records."""
        for mult in multipliers:
            for e in self.parts:
                e.scale_kT(mult)
            for e in self.parts:
                e.advance(nsteps)
        for e in self.parts:
            e.scale_kT(1.0)
            e.reset_averages()
        self.steps = 0

    def stage(self, mult):
        """Start of a fresh mcmc(nsteps, pargs, chain) call of the clustering main: new temperature (kT x mult),
        default step sizes, empty acceptor cache and averagers (mcmc_clustering_eap_chain.jl:172-181)."""
        for e in self.parts:
            e.scale_kT(mult)
            e.reset_sampler()
            e.reset_averages()
        self.steps = 0

    def recorded(self, nsteps, stepout, angles=False, tick=None):
        """advance(nsteps), yielding after every `stepout`-th step (step, micro, ang, summaries): per case the microstate
        [7] of its first chain, with `angles` that chain's theta[n] then phi[n], and its pooled summary.  The rows are
        recorded on the device for all cases at once (Ensemble.advance_series) and come back a chunk at a time: shard
        vectors are added as in summary(), the microstate is shard 0's.  `tick(step)` is called once per chunk.
        --numeric-type other than float64 needs every chain's means at every row (summary()): it takes the per-row calls."""
        ncases = len(self.plist)
        nrows = nsteps // stepout if stepout > 0 else 0
        if self.numeric_type != "float64":
            for r in range(1, nrows + 1):
                self.advance(stepout)
                if tick:
                    tick(r * stepout)
                st = [self.chain0(k) for k in range(ncases)] if angles else None
                yield (r * stepout, [self.microstate(k) for k in range(ncases)],
                       [np.concatenate([c["theta"], c["phi"]]) for c in st] if angles else None,
                       [self.summary(k) for k in range(ncases)])
        elif nrows:
            n = self.parts[0].n
            row_bytes = 8 * ncases * (_lib.NRED + 7 + (2 * n if angles else 0))
            chunk = min(nrows, max(1, SERIES_BUDGET_BYTES // row_bytes))
            series = [e.open_series(chunk, angles=angles and i == 0) for i, e in enumerate(self.parts)]
            try:
                done = 0
                while done < nrows:
                    m = min(chunk, nrows - done)
                    for e, s in zip(self.parts, series):
                        e.advance_series(s, m * stepout, stepout)      # asynchronous: the devices run concurrently
                    self.steps += m * stepout
                    reads = [s.read() for s in series]
                    for s in series:
                        s.clear()
                    steps, _, micro, ang = reads[0]
                    red = np.zeros((m, ncases, _lib.NRED))
                    for rd in reads:
                        red += rd[1]
                    if tick:
                        tick((done + m) * stepout)
                    for r in range(m):
                        yield ((done + r + 1) * stepout, micro[r], ang[r] if angles else None,
                               [summary_from_reduction(red[r, k], int(steps[r])) for k in range(ncases)])
                    done += m
            finally:
                for s in series:
                    s.close()
        rest = nsteps - nrows * stepout      # not recorded
        if rest > 0:
            self.advance(rest)
            if tick:
                tick(nsteps)

    def record(self, nsteps, rec):
        """advance(nsteps), made TWICE from the same state: first recorded on the device the way `rec` (a Recording) says -- as the
        records its row of RECORDING_KINDS counts, so many steps apart (error_bars: exactly N batches of nsteps // N steps; the others:
        a record after every --stepout-th step; a remainder belongs to no record), into the recorder the row opens, by the row's
        Ensemble.advance_* --; then, from a checkpoint taken before it, as the one launch of advance(nsteps), which leaves the
        handle -- and so the averages the caller prints -- exactly as a run without a recording does.  (Recording leaves
        trajectories alone, but N launches add the running sums in another order than one launch: the step kernels fold them in
        blocks that start at a launch's first step.)  Returns what the row reads at the end (error_bars: the blocked standard
        errors of every case, Series.error_bars; hist: HistResult; corr, shape: (CorrResult | ShapeResult, ErrorBars of the rows)).
        Called where the averages are empty (after burn_in / stage / creation), so an error_bars row's differences are the batch
        means.  The chains are on one device only: the shards of a case hold different chains, and their records are not merged.
        The recorder is closed whatever happens; the checkpoint is put back also when the recorded run failed, so that the handle
        is never left mid-run (error_bars alone leaves a failed run where it stopped)."""
        check_recording(self.plist[0], rec, devices=len(self.parts))
        row = RECORDING_KINDS[rec.kind]
        nrec, stepout = row.records(nsteps, rec.spec, int(self.plist[0]["stepout"]))
        e = self.parts[0]
        image = e.checkpoint()
        recorder = row.open(e, rec.spec, nrec)
        done = False
        try:
            row.advance(e, recorder, nrec * stepout, stepout)
            res = row.read(recorder)
            done = True
        finally:
            recorder.close()
            if done or row.restore_after_failure:
                e.restore(image)
        self.advance(nsteps)
        return res

    def chain0(self, k=0):
        return self.parts[0].chain_state(k * self.counts[0])      # the first chain of case k

    def microstate(self, k=0):
        return self.parts[0].microstate(k * self.counts[0])

    def summary(self, k=0):
        red = np.zeros(_lib.NRED)
        for e in self.parts:
            red += e.reduce_host(k)
        s = summary_from_reduction(red, self.steps)
        if self.numeric_type != "float64":
            # --numeric-type: pooled mean and across-chain standard error re-done in the wide type from the per-chain
            # means (the same quantities the device reduction folds in Float64)
            m = np.concatenate([e.chain_means(k) for e in self.parts], axis=1).astype(np.longdouble)
            C = m.shape[1]
            mean = m.sum(axis=1) / C
            se = np.sqrt(((m - mean[:, None]) ** 2).sum(axis=1) / (C - 1) / C) if C > 1 else np.zeros_like(mean)
            for q in range(_lib.NOBS):
                s.avg[q], s.stderr[q] = float(mean[q]), float(se[q])
            s.acceptance_ratio, s.ar_stderr = float(mean[16]), float(se[16])
            for q in range(2):
                s.extra_avg[q], s.extra_stderr[q] = float(mean[17 + q]), float(se[17 + q])
        return s

    def report_failures(self, k, s):
        """stderr only (stdout stays the reference's lines): what the reference hides -- proposals it rejected because
        their energy was NaN/Inf, and chains sitting in a 1/r^3 singularity (no excluded volume, inc/eap_chain.jl:200-207)."""
        pargs = self.plist[k]
        who = f"{os.path.basename(pargs['prefix'])}: " if len(self.plist) > 1 else ""
        if s.nan_rejects:
            _log(pargs, 2, "Warning", f"{who}{s.nan_rejects} proposals had a non-finite energy and were rejected "
                                      f"({s.nan_rejects / max(1.0, s.attempted_updates):.3g} of all attempts)")
        if s.chains_collapsed:
            _log(pargs, 2, "Warning", f"{who}{s.chains_collapsed} of {s.num_chains} chains have collapsed "
                                      f"(|U| a thousand times beyond field + force + thermal energy: monomers on top of each other)")

    def kernel(self) -> str:
        return self.parts[0].launch_info().kernel.decode()

    def close(self):
        for e in self.parts:
            e.close()


# ---------------------------------------------------------------------------------------------- the two CSV files
class CsvFiles:
    """The `<prefix>_trajectory.csv` / `<prefix>_rolling.csv` pair of every case of an ensemble.  The reference holds its two
    files open for the whole run (mcmc_eap_chain.jl:256-258,372-373); a batched sweep has thousands of cases, so the handles
    stay open only while two per case fit the process's descriptor limit with room to spare -- beyond that every row is
    appended by open/write/close (same bytes on disk)."""

    def __init__(self, prefixes, traj_headers, roll_header):
        try:
            import resource
            limit = resource.getrlimit(resource.RLIMIT_NOFILE)[0]
        except Exception:
            limit = 256
        self.paths = [(f"{p}_trajectory.csv", f"{p}_rolling.csv") for p in prefixes]
        self.keep_open = 2 * len(self.paths) <= max(0, limit - 64) // 2
        self.handles = []
        for (tp, rp), th in zip(self.paths, traj_headers):
            ft, fr = open(tp, "w"), open(rp, "w")
            ft.write(th + "\n")
            fr.write(roll_header + "\n")
            if self.keep_open:
                self.handles.append((ft, fr))
            else:
                ft.close()
                fr.close()

    def __len__(self):
        return len(self.paths)

    def rows(self, k, traj_row, roll_row):
        if self.keep_open:
            ft, fr = self.handles[k]
            ft.write(traj_row + "\n")
            fr.write(roll_row + "\n")
        else:
            for path, row in zip(self.paths[k], (traj_row, roll_row)):
                with open(path, "a") as f:
                    f.write(row + "\n")

    def close(self):
        for ft, fr in self.handles:
            ft.close()
            fr.close()
        self.handles = []


def recorded_stage(pool, nsteps, write: bool, traj_header, roll_header, rows, angles=False, runs=(None,), report=None,
                   record=None):
    """One recorded run of `nsteps` for every case of the pool, the body of the reference's mcmc(nsteps, pargs[, chain]):
    with `write` the two CSV files of every case (headers `traj_header(pargs)` and `roll_header`, a row per --stepout
    steps: `rows(pargs, step, micro, ang, summary)` -> the case's (trajectory row, rolling row)), then the summaries, the
    total time and the acceptance rates on stderr (`report(k, summary)` right after case k's rate).  `runs` yields the
    progress line of each run of `nsteps` into the same files (the fixed-force main's inits; it is resumed after the run).
    `record` = a Recording (without `write`): the run is recorded its way instead (_Pool.record) and the pool's `info` gets what
    that returns under the recording's kind ("error_bars" | "hist" | "corr" | "shape")."""
    plist = pool.plist
    pargs = plist[0]
    stepout = int(pargs["stepout"]) if write else 0
    files = None
    try:
        if write:
            files = CsvFiles([p["prefix"] for p in plist], [traj_header(p) for p in plist], roll_header)
        start = time.time()
        last_update = [start]
        for progress in runs:
            def tick(step):                                             # per chunk of rows
                if time.time() - last_update[0] > pargs["update-freq"]:
                    _log(pargs, 3, "Info", f"elapsed: {time.time() - start}")
                    if progress:
                        _log(pargs, 3, "Info", progress)
                    _log(pargs, 3, "Info", f"step:    {step} / {nsteps}")
                    last_update[0] = time.time()
            if record:
                res = pool.record(nsteps, record)
                if pool.info is not None:
                    pool.info[record.kind] = res
                continue
            for step, micro, ang, sums in pool.recorded(nsteps, stepout, angles=angles, tick=tick):
                for k in range(len(files)):
                    files.rows(k, *rows(plist[k], step, micro[k], ang[k] if angles else None, sums[k]))
        out = [pool.summary(k) for k in range(len(plist))]
        _log(pargs, 3, "Info", f"total time elapsed: {time.time() - start}")
        for k, s in enumerate(out):
            _log(plist[k], 3, "Info", f"acceptance rate: {s.acceptance_ratio}")
            if report:
                report(k, s)
        return out
    finally:
        if files:
            files.close()


# ---------------------------------------------------------------------------------------------- stdout
def error_summary(eb, k: int):
    """The blocked standard errors of case k laid out like the summary of its averages (a main's `averagers` and
    `summary_lines` then print them under the names of the quantities they belong to)."""
    s = _lib.Summary()
    se = eb.stderr[k]
    for q in range(_lib.NOBS):
        s.avg[q] = se[q]
    s.acceptance_ratio = se[16]
    s.extra_avg[0], s.extra_avg[1] = se[17], se[18]
    return s


def error_lines(main, eb, k: int, pargs) -> list[str]:
    """`<case>.err`: the left-hand names of the `.out` (the main's own summary_lines) with the blocked standard errors as
    right-hand sides, then the batch count and, over the 19 quantities of _lib.EB_NAMES, inefficiency and converged."""
    return [*main.summary_lines(*main.averagers(error_summary(eb, k)), pargs),
            f"batches = {eb.nbatches}",
            f"inefficiency = {jl_vector(eb.inefficiency[k])}",
            f"converged = {jl_vector(eb.converged[k].astype(float))}"]


def hist_lines(res, specs, k: int, chains: int) -> list[str]:
    """`<case>.hist`: per histogram a header line naming channel, lo, hi, nbins, records and chains, the `bin_lo,bin_hi,count`
    rows, then the three tails."""
    out = []
    for i, (channel, lo, hi, nbins) in enumerate(specs):
        edges = res.edges(i, k)
        out.append(f"# channel={channel} lo={lo!r} hi={hi!r} nbins={nbins} records={res.records} chains={chains}")
        out += [f"{float(edges[j])!r},{float(edges[j + 1])!r},{int(c)}" for j, c in enumerate(res.counts[i][k])]
        out += [f"{name},{int(c)}" for name, c in zip(("below", "above", "not_finite"), res.tails[k, i])]
    return out


def corr_lines(res, eb, k: int) -> list[str]:
    """`<case>.corr`: CSV `k,<ch>,<ch>_stderr,...`, a row per lag: the mean over records and chains and its blocked standard
    error from the records' rows."""
    w = res.max_lag + 1
    out = ["k," + ",".join(f"{ch},{ch}_stderr" for ch in res.channels)]
    for lag in range(w):
        out.append(f"{lag}," + ",".join(f"{float(res.mean[ch][k, lag])!r},{float(eb.stderr[k, i * w + lag])!r}"
                                        for i, ch in enumerate(res.channels)))
    return out


def shape_lines(res, eb, k: int) -> list[str]:
    """`<case>.shape`: CSV `name,qx,qy,qz,value,stderr`: the eight gyration rows (no wave-vector), then a row `sq` per
    wave-vector: the mean over records and chains and its blocked standard error from the records' rows."""
    out = ["name,qx,qy,qz,value,stderr"]
    for i, name in enumerate(_lib.SHAPE_NAMES):
        out.append(f"{name},,,,{float(res.mean[k, i])!r},{float(eb.stderr[k, i])!r}")
    for j, v in enumerate(res.q):
        i = len(_lib.SHAPE_NAMES) + j
        out.append(f"sq,{float(v[0])!r},{float(v[1])!r},{float(v[2])!r},{float(res.mean[k, i])!r},{float(eb.stderr[k, i])!r}")
    return out


def pdist_lines(res, eb, k: int) -> list[str]:
    """`<case>.pdist`: CSV `name,x,value,stderr`: a row `msd` per separation (x = s), `rmin` (no x), a row `hist` per bin (x = the
    bin's centre, value = the density P(r)), `above` (the share of the counted pairs at or beyond rmax) and a row `sq` per Debye
    magnitude (x = q): the mean over records and chains and its blocked standard error from the records' rows (the histogram's
    in the units of its value)."""
    out = ["name,x,value,stderr"]
    row = lambda name, x, v, e: f"{name},{x},{float(v)!r},{float(e)!r}"
    for s in range(1, res.max_sep + 1):
        out.append(row("msd", s, res.mean[k, s - 1], eb.stderr[k, s - 1]))
    out.append(row("rmin", "", res.rmin[k], eb.stderr[k, res.max_sep]))
    h0 = res.max_sep + 1
    if res.nbins:
        width, centers, density = float(res.rmax[k]) / res.nbins, res.centers(k), res.density(k)
        for j in range(res.nbins):     # a row's column is the chains' mean count: / (pairs * width) turns it into the density
            out.append(row("hist", repr(float(centers[j])), density[j], eb.stderr[k, h0 + j] / (res.pairs * width)))
        share = res.above[k] / (res.records * res.num_chains * res.pairs)
        out.append(row("above", "", share, eb.stderr[k, h0 + res.nbins] / res.pairs))
        h0 += res.nbins + 1
    for j, v in enumerate(res.q):
        out.append(row("sq", repr(float(v)), res.mean[k, h0 + j], eb.stderr[k, h0 + j]))
    return out


def energy_lines(res, eb, model_eb, k: int) -> list[str]:
    """`<case>.energy`: CSV `name,x,value,stderr`: `field`, `work`, `bend` (no x), a row `pair` per separation (x = s), `rest`,
    `within` (x = the radius in monomer lengths; only with the column) and `model`, the energy the case's own step carries: the
    mean over records and chains and its blocked standard error from the records' rows -- `model`'s from the rows' combined
    column."""
    out = ["name,x,value,stderr"]
    row = lambda name, x, v, e: f"{name},{x},{float(v)!r},{float(e)!r}"
    for i, name in enumerate(_lib.ENERGY_NAMES):
        out.append(row(name, "", res.mean[k, i], eb.stderr[k, i]))
    for s in range(1, res.max_sep + 1):
        out.append(row("pair", s, res.mean[k, 2 + s], eb.stderr[k, 2 + s]))
    out.append(row("rest", "", res.rest[k], eb.stderr[k, 3 + res.max_sep]))
    if res.has_within:
        out.append(row("within", repr(float(res.cutoff[k])), res.within[k], eb.stderr[k, 4 + res.max_sep]))
    out.append(row("model", "", res.model[k], model_eb.stderr[k]))
    return out


def summary_lines(sas, vas, ar, pargs, extra=()) -> list[str]:
    """The println lines every main ends with (mcmc_eap_chain.jl:386-395); `extra`: a main's own lines in front of AR."""
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
        *extra,
        f"AR     =   {jl_float(ar)}",
    ]


def main(pargs: dict, profile_message: str, run, lines) -> int:
    """What a main does with its parsed command line: `run(pargs)` -> (scalar_averagers, vector_averagers, ar), printed."""
    if pargs["profile"]:
        raise ReferenceError_(profile_message)
    sas, vas, ar = run(pargs)
    for line in lines(sas, vas, ar, pargs):
        print(line)
    return 0
