"""What the reference's sweep drivers do with `pmap` over subprocesses, as batched launches.

A `run/*.jl` script (run/interacting_dielectric_study.jl, run/Ising_2025-12-18.jl, run/K1_E0-kT-phase.jl, ...) builds a
list of cases (dicts of E0, K1, K2, kT, Fz, Fx, n, b, kappa, run ...), and for every case starts
`julia mcmc_[clustering_]eap_chain.jl <fixed flags> <the case's flags> --prefix workdir/<name>` in a worker process,
writes the ten (twelve) stdout lines to `workdir/<name>.out` unless that file already exists, where
`<name>` = `E0-0001000_K1-0000000_..._b-0001000[_run-001]` (every value x 1000, `%07d`).  scripts/aggregate_mcmc.jl
then reads the values back out of the file NAMES and the stdout lines.

Here the cases of a sweep that share everything but their physics scalars become ONE ensemble (`pstat_create` with
ncases > 1) and one launch per stage of the main's protocol -- the hosts' own `run_cases`, which the command
line calls with one case --; cases are dealt to ranks round-robin (independent work, no exchange: `pmap`'s own partitioning),
and every case's `.out` holds the lines the single-case host prints for the same options, seed and chains.

What "the same" means: a chain's TRAJECTORY depends on its (seed, chain id) and its case's options only -- in f64 bit for bit
whatever else shares the ensemble, however many ranks there are and whatever is already finished.  The printed f64 averages
agree to ~1e-10 relative, not to the last bit: how a launch is cut into time segments (and, in f32, where the chains live)
depends on how many chains are co-batched, and the running sums are folded in 128-step blocks that start at segment
boundaries (the f64 clustering main also re-derives its cached n-hat there).  f32 / q16 cases are statistically equivalent
across partitions, not trajectory-identical, once an ensemble is large enough to change the kernel's home
(tests/test_gpu_sweep.py::test_a_case_does_not_depend_on_what_shares_its_ensemble_even_past_the_resident_slots).

    python tools/run_sweep.py WORKDIR --main mcmc_clustering_eap_chain --num-chains 64 \
        --axis run=1:5 --axis kT='10^(-2:0.2:2)' --axis E0=0:0.2:5 --axis K1=1 --axis K2=0 --axis Fz=0 --axis Fx=0 \
        --axis n=100 --axis b=1 --axis kappa=0 --name E0,K1,K2,kT,Fz,Fx,n,b,kappa,run:raw \
        -- --chain-type dielectric --energy-type Ising --num-steps 2500000 --burn-in 100000 -v 2

The planar main's sweeps (2D/run/*.jl) are the same thing with `--main mcmc_clustering_eap_chain_2d`.
"""
from __future__ import annotations

import ast
import itertools
import json
import os
import time

import numpy as np

from . import _lib          # (tools/run_sweep.py counts the devices through it)
from . import mcmc_clustering_eap_chain as cluster_main
from . import mcmc_clustering_eap_chain_2d as planar_main
from . import mcmc_eap_chain as fixed_main
from ._host import RECORDING_KINDS, Recording, ReferenceError_, arith, check_recording, fresh_seed, number
from ._host import parse_corr, parse_energy, parse_hist, parse_pdist, parse_shape      # (reached through this module too)

# (the planar main: 2D/run/Ising_2024-11-06.jl and its siblings launch 2D/mcmc_clustering_eap_chain.jl the same way)
MAINS = {"mcmc_eap_chain": fixed_main, "mcmc_clustering_eap_chain": cluster_main, "mcmc_clustering_eap_chain_2d": planar_main}

# how the reference's run scripts turn a case's keys into flags of the main (run/K1_E0-kT-phase.jl:45)
KEY_FLAG = {"E0": "--E0", "K1": "--K1", "K2": "--K2", "mu": "--mu", "kT": "--kT", "Fz": "--Fz", "Fx": "--Fx",
            "n": "--num-monomers", "b": "--mlen", "kappa": "--bend-mod", "run": None}
NAME_ORDER = ["E0", "K1", "K2", "mu", "kT", "Fz", "Fx", "n", "b", "kappa", "run"]
# pargs entries that may differ between the cases of one ensemble (pstat_create: "differ only in physics scalars")
PER_CASE = {"E0", "K1", "K2", "mu", "kT", "Fz", "Fx", "mlen", "bend-mod", "bend-angle", "cluster-prob", "cutoff-radius",
            "prefix", "seed"}


# ---------------------------------------------------------------------------------------------- the case list
def julia_range(text: str) -> list:
    """`a:b` or `a:s:b` the way Julia enumerates it: a, a+s, ... while <= b (count from the rounded quotient, values
    as a + k*s -- Julia's own StepRangeLen is a shade more careful, equal to this to an ulp; names are rounded to 1e-3)."""
    parts = [number(p) for p in text.split(":")]
    if len(parts) == 2:
        a, s, b = parts[0], 1, parts[1]
    elif len(parts) == 3:
        a, s, b = parts
    else:
        raise ValueError(f"range '{text}' not understood")
    if s == 0:
        raise ValueError(f"range '{text}' has step 0")
    cnt = int(np.floor((b - a) / s + 1e-9)) + 1
    vals = [a + k * s for k in range(max(cnt, 0))]
    if all(isinstance(p, int) for p in (a, s, b)):
        return [int(v) for v in vals]
    return [float(np.round(v, 12)) for v in vals]


def axis_values(text: str) -> list:
    """`1,5,10` | `0:0.2:5` | `10^(-2:0.2:2)` (run/K1_E0-kT-phase.jl:22-27) | `0:0.05:1,1.5:0.5:5` (vcat of ranges,
    run/noninteracting-compare-with-clustering_2021-09-24.jl:21) -> values."""
    t = text.strip()
    if t.startswith("10^(") and t.endswith(")"):
        return [float(10.0 ** x) for x in julia_range(t[4:-1])]
    out = []
    for item in t.split(","):
        if item.strip():
            out += julia_range(item) if ":" in item else [number(item)]
    return out


def product_cases(axes: list[tuple[str, list]]) -> list[dict]:
    """`for a in As, b in Bs, ...` (first axis outermost, run/interacting_dielectric_study.jl:28)."""
    keys = [k for k, _ in axes]
    return [dict(zip(keys, combo)) for combo in itertools.product(*[v for _, v in axes])]


_CMP = {ast.Eq: lambda a, b: a == b, ast.NotEq: lambda a, b: a != b, ast.Lt: lambda a, b: a < b,
        ast.LtE: lambda a, b: a <= b, ast.Gt: lambda a, b: a > b, ast.GtE: lambda a, b: a >= b}


def _cond(node, case):
    if isinstance(node, ast.BoolOp):
        vals = [_cond(v, case) for v in node.values]
        return all(vals) if isinstance(node.op, ast.And) else any(vals)
    if isinstance(node, ast.UnaryOp) and isinstance(node.op, ast.Not):
        return not _cond(node.operand, case)
    if isinstance(node, ast.Compare):
        left = _cond(node.left, case)
        for op, right in zip(node.ops, node.comparators):
            r = _cond(right, case)
            if not _CMP[type(op)](left, r):
                return False
            left = r
        return True
    if isinstance(node, ast.Name):
        if node.id not in case:
            raise ValueError(f"--skip names '{node.id}', which is not a key of the cases")
        return case[node.id]
    return arith(node)


def skip_case(expr: str, case: dict) -> bool:
    """`K1==K2` (run/interacting_dielectric_study.jl:29): comparisons of case keys and numbers, and/or/not."""
    return bool(_cond(ast.parse(expr.replace("&&", " and ").replace("||", " or "), mode="eval").body, case))


def fmt(x) -> str:
    """`@sprintf("%07d", round(Int, 1e3*x))` (run/interacting_dielectric_study.jl:12)."""
    return "%07d" % int(round(1e3 * x))


def name_spec(text: str | None, keys) -> list[tuple[str, str]]:
    """`E0,K1,...,run:int` -> [(key, kind)], kind in milli (%07d of 1000 x) | int (%03d) | raw."""
    if not text:
        order = [k for k in NAME_ORDER if k in keys] + [k for k in keys if k not in NAME_ORDER]
        return [(k, "int" if k == "run" else "milli") for k in order]       # run/Ising_2025-12-18.jl:15: `_run-$(fmt_int(run))`
    out = []
    for tok in text.split(","):
        k, _, kind = tok.strip().partition(":")
        kind = kind or "milli"
        if kind not in ("milli", "int", "raw"):
            raise ValueError(f"name kind '{kind}' not understood (milli | int | raw)")
        out.append((k, kind))
    return out


def case_name(case: dict, spec) -> str:
    toks = []
    for k, kind in spec:
        v = case[k]
        toks.append(f"{k}-" + (fmt(v) if kind == "milli" else "%03d" % int(v) if kind == "int" else str(v)))
    return "_".join(toks)


def case_argv(case: dict) -> list[str]:
    argv = []
    for k, v in case.items():
        flag = KEY_FLAG.get(k, f"--{k}")
        if flag is not None:
            whole = isinstance(v, int) or (flag == "--num-monomers" and float(v).is_integer())
            argv += [flag, repr(int(v)) if whole else repr(float(v))]      # (an integer option of the main may be an axis too)
    return argv


# ---------------------------------------------------------------------------------------------- the sweep
def plan(main_name: str, fixed_argv: list[str], cases: list[dict], workdir: str, *, name=None, num_chains: int = 64,
         seed: int | None = None, precision: str | None = None, rng: str | None = None, device: int = 0) -> list[dict]:
    """Every case's parsed options (the dict the main's own parser returns) with its prefix, its `.out` path and its
    seed = base seed + position in the FULL case list (so a case's result depends neither on which other cases still
    have to be run nor on how many ranks share them)."""
    main = MAINS[main_name]
    if not cases:
        return []
    spec = name_spec(name, list(cases[0].keys()))
    base = fresh_seed() & 0x7FFFFFFFFFFF if seed is None else int(seed)
    extra = ["--num-chains", str(int(num_chains)), "--devices", str(int(device))]
    if precision:
        extra += ["--precision", precision]
    if rng:
        extra += ["--rng", rng]
    out, seen = [], set()
    for k, case in enumerate(cases):
        nm = case_name(case, spec)
        if nm in seen:
            raise ValueError(f"two cases share the file name '{nm}': add the key that tells them apart to --name")
        seen.add(nm)
        pargs = main.parse_args(list(fixed_argv) + case_argv(case) + extra +
                                ["--prefix", os.path.join(workdir, nm), "--seed", str(base + k)])
        if pargs["profile"]:
            raise ReferenceError_("not implemented for the HPC env")
        pargs["_case"], pargs["_name"], pargs["_out"], pargs["_index"] = case, nm, os.path.join(workdir, nm + ".out"), k
        out.append(pargs)
    return out


def recording(main_name: str, fixed_argv: list[str], cases: list[dict], *, error_bars: int = 0, hist=None, corr=None, shape=None,
              pdist=None, energy=None, write_csv: bool = False, world: int = 1) -> Recording | None:
    """--error-bars N | --hist SPEC ... | --corr SPEC | --shape [SPEC] | --pdist SPEC | --energy SPEC of tools/run_sweep.py (the texts as the
    command line gives them; shape "" is the bare flag, None its absence) -> the Recording of the production run, or None where none is asked for.
    Parses the flag that is given and refuses what it cannot be combined with -- another of the six, more than one rank, and
    what _host.check_recording refuses, judged from the options every case shares and from every chain and monomer length
    among the cases; no GPU is touched."""
    given = [(kind, text) for kind, text in (("error_bars", error_bars or None), ("hist", hist or None), ("corr", corr or None),
                                             ("shape", shape), ("pdist", pdist or None), ("energy", energy or None)) if text is not None]
    if not given:
        return None
    row = RECORDING_KINDS[given[0][0]]
    rec = Recording(given[0][0], row.parse(given[0][1]))
    if len(given) > 1:
        raise ReferenceError_(f"{RECORDING_KINDS[given[1][0]].flag} cannot be combined with {row.flag}: each records the production run "
                              "in its own way")
    if world > 1:
        raise ReferenceError_(f"{row.flag} needs one device, not --gpus {world}")
    main = MAINS[main_name]
    if rec.kind == "shape" and main is planar_main and any(v[1] != 0.0 for v in rec.spec[1]):
        raise ReferenceError_("--shape: the planar main's chains lie in the x-z plane: no wave-vectors along y")
    sizes = {}
    for case in cases or [{}]:
        sizes.setdefault(repr((case.get("n", case.get("num-monomers")), case.get("b", case.get("mlen")))), case)
    for case in sizes.values():
        check_recording(main.parse_args(list(fixed_argv) + case_argv(case)), rec, write_csv)
    return rec


def _signature(pargs: dict):
    return tuple(sorted((k, repr(v)) for k, v in pargs.items() if k not in PER_CASE and not k.startswith("_")))


def run_sweep(main_name: str, fixed_argv: list[str], cases: list[dict], workdir: str, *, name=None, num_chains: int = 64,
              seed: int | None = None, precision: str | None = None, rng: str | None = None, rank: int = 0, world: int = 1,
              device: int = 0, overwrite: bool = False, write_csv: bool = False, max_chains: int = 262144, log=None,
              error_bars: int = 0, hist=None, corr=None, shape=None, pdist=None, energy=None) -> dict:
    """Runs the cases whose `.out` does not exist yet (run/interacting_dielectric_study.jl:39) and that fall to this rank
    (position in the full case list modulo `world`).  `write_csv` also writes every case's two time-series files (rows
    recorded on the device for the whole ensemble, _Pool.recorded).  `error_bars` = N | `hist` = ["CHANNEL:LO:HI:NBINS", ...] | `corr` =
    "MAXLAG[:nn,zz,mm]" | `shape` = "[AXIS:QMAX:NQ,...]" ("" for the gyration block alone; None: no shape) | `pdist` =
    "RMAX:NBINS[,sep=..][,min=..][,q=QMAX:NQ]" | `energy` = "MAXSEP[,cut=RCUT]", the command line's six options and at most one of them (recording): the production run is recorded that way (_Pool.record: N batches | every chain
    histogrammed | the lag correlations | the gyration tensor and the form factor at those wave-vectors | the pair distances | the energy by term and separation, every --stepout steps)
    and every `<case>.out` gets a `<case>.err` | `.hist` | `.corr` | `.shape` | `.pdist` | `.energy` beside it (_host.error_lines: blocked standard
    errors under the .out's names | hist_lines | corr_lines | shape_lines | pdist_lines | energy_lines); the .out files are those of a run without it, and a
    case whose file beside the .out is missing is run again.  Returns {"ran": [...], "skipped": [...], "launches": k}."""
    main = MAINS[main_name]
    rec = recording(main_name, fixed_argv, cases, error_bars=error_bars, hist=hist, corr=corr, shape=shape, pdist=pdist, energy=energy,
                    write_csv=write_csv, world=world)
    os.makedirs(workdir, exist_ok=True)
    todo_all = plan(main_name, fixed_argv, cases, workdir, name=name, num_chains=num_chains, seed=seed, precision=precision,
                    rng=rng, device=device)
    # a recorded case is complete when the recording's file is there too (a directory first swept without it: run again)
    beside = lambda p: p["_out"][:-len(".out")] + RECORDING_KINDS[rec.kind].ext
    done = lambda p: os.path.isfile(p["_out"]) and (rec is None or os.path.isfile(beside(p)))
    skipped = [p["_name"] for p in todo_all if done(p) and not overwrite]
    todo = [p for p in todo_all if overwrite or not done(p)]
    mine = [p for p in todo if p["_index"] % world == rank]     # by position in the full list: ranks need not agree on what is done
    groups: dict = {}
    for p in mine:
        groups.setdefault(_signature(p), []).append(p)
    ran, launches = [], 0
    per_launch = max(1, int(max_chains) // max(1, int(num_chains)))
    for plist_all in groups.values():
        for i in range(0, len(plist_all), per_launch):
            plist = plist_all[i:i + per_launch]
            t0 = time.time()
            info = {}
            # the main's own protocol, every case of the ensemble at once
            res = main.run_cases(plist, write_csv=write_csv, info=info, record=rec)
            for k, (p, (sas, vas, ar)) in enumerate(zip(plist, res)):
                texts = [(p["_out"], main.summary_lines(sas, vas, ar, p))]      # println x 10 (12)
                if rec:      # (first: a case whose .out is there is complete)
                    texts.insert(0, (beside(p), RECORDING_KINDS[rec.kind].lines(main, info[rec.kind], rec.spec, k, p)))
                for path, lines in texts:           # complete or absent: an interrupted sweep re-runs the case
                    tmp = path + f".tmp{os.getpid()}"
                    with open(tmp, "w") as f:
                        f.write("\n".join(lines) + "\n")
                    os.replace(tmp, path)
                ran.append(p["_name"])
            launches += 1
            if log:
                log(f"rank {rank}: {len(plist)} cases x {num_chains} chains, n = {plist[0]['num-monomers']}, "
                    f"{info.get('kernel', '?')}: {time.time() - t0:.2f} s")
    return {"ran": ran, "skipped": skipped, "launches": launches}


def load_cases(path: str) -> list[dict]:
    """An explicit case list (what run/Ising_2025-12-18.jl spells out push! by push!): a JSON array of objects."""
    with open(path) as f:
        cases = json.load(f)
    if not isinstance(cases, list) or not all(isinstance(c, dict) for c in cases):
        raise ValueError(f"{path}: expected a JSON array of objects")
    return cases
