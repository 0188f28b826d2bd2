"""Generates tests/golden/host_tables.json: what the three hosts (polymer_stats_amd/mcmc_eap_chain.py,
mcmc_clustering_eap_chain.py, mcmc_clustering_eap_chain_2d.py) state about their command lines, recorded from the commit
BEFORE their shared text moved to polymer_stats_amd/_host.py, so that tests/test_host.py can hold the hosts to it.  For
each main:

  options   the parser's actions in order: option strings, dest, action class, type name, default, help
  params    every field of the pstat_params that params_from_pargs(parse_args(argv + ["--seed", "11"]), 5, 2, 0) returns,
            for the empty command line and for command lines that together set every option the main maps into the struct
  errors    the exception type and message of every error() branch of params_from_pargs, of mcmc() / run() in front of
            the pool, and of main(), with what reached stderr before it
  summary   summary_lines for one fixed set of averagers

Only names every version of the hosts has are used (mcmc / run, not run_cases).  Needs the built libpstat.so (the struct's
defaults come out of it), no GPU.

Run:  python tests/golden/make_host_tables.py [CHECKOUT]   (imports CHECKOUT's package, default: this tree's, and
      rewrites the JSON next to this file)
"""
import contextlib
import importlib
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MAINS = ["mcmc_eap_chain", "mcmc_clustering_eap_chain", "mcmc_clustering_eap_chain_2d"]

COMMON = ["-e", "1.5", "-J", "0.7", "-K", "0.2", "-m", "0.3", "-k", "2.0", "-F", "0.5", "-G", "0.25", "-b", "1.5", "-n", "37",
          "-p", "0.9", "-L", "0.1", "-U", "0.6", "-A", "1.2", "-S", "1000", "--uniform-bits", "23"]
PARAMS = {
    "mcmc_eap_chain": [
        [],
        COMMON + ["-T", "polar", "-u", "Ising", "-q", "0.4", "--do-flips", "-B", "--rng", "xoshiro128++", "--precision", "f32"],
        ["-u", "interacting", "--precision", "q16", "--uniform-bits", "53", "-n", "12"],
    ],
    "mcmc_clustering_eap_chain": [
        [],
        COMMON + ["-T", "polar", "-u", "cutoff", "--cutoff-radius", "3.5", "-q", "0.4", "-a", "2.0", "-g", "0.1", "--cluster-prob", "0.25",
                  "-B", "--rng", "xoshiro128++", "--precision", "f32", "--x0", "[0.3; 1.2]", "--dx0", "[pi/2, 2^-3]"],
        ["-u", "interacting", "-n", "3", "--x0", "[0.1; 0.2; 0.3; 0.4; 0.5; 0.6]"],
        ["-u", "noninteracting", "--x0", "[π/2; -0.3]"],
    ],
    "mcmc_clustering_eap_chain_2d": [
        [],
        COMMON + ["-T", "polar", "-u", "Ising", "--cluster-prob", "0.25", "-B", "--rng", "xoshiro128++"],
        ["-u", "interacting", "--uniform-bits", "53", "--carry-burn-in"],
    ],
}
# (where, argv): where the branch is -- params_from_pargs | run (mcmc / run, in front of the pool) | main
ERRORS = {
    "mcmc_eap_chain": [
        ("params", ["-T", "rod"]), ("params", ["-u", "cutoff"]), ("params", ["--precision", "f16"]), ("params", ["--rng", "lcg"]),
        ("params", ["-T", "rod", "-u", "x", "--precision", "x", "--rng", "x"]), ("params", ["-u", "x", "--precision", "x", "--rng", "x"]),
        ("params", ["--precision", "x", "--rng", "x"]),
        ("run", ["-a", "kawasaki"]), ("run", ["--numeric-type", "float16"]), ("run", ["-E", "end-to-end"]),
        ("run", ["-a", "kawasaki", "--numeric-type", "float16", "-E", "end-to-end"]), ("run", ["--numeric-type", "float16", "-E", "end-to-end"]),
        ("main", ["--profile"]), ("main", ["-Z", "-E", "end-to-end", "-v", "2"]),
    ],
    "mcmc_clustering_eap_chain": [
        ("params", ["-T", "rod"]), ("params", ["-u", "x"]), ("params", ["--precision", "q16"]), ("params", ["--rng", "lcg"]),
        ("params", ["-T", "rod", "-u", "x", "--precision", "x", "--rng", "x", "--x0", "[a]"]), ("params", ["--rng", "x", "--x0", "[a]"]),
        ("params", ["--x0", "[1; 2; 3]"]), ("params", ["--x0", "[a]"]), ("params", ["--x0", "1, 2"]), ("params", ["--x0", "[1; 2]", "--dx0", "[1]"]),
        ("params", ["--x0", "[1; 2]", "--dx0", "[f(1), 2]"]), ("params", ["--x0", "[__import__('os'); 2]"]),
        ("run", ["--numeric-type", "float16"]), ("run", ["--burn-schedule", "10; 1"]), ("run", ["--burn-schedule", "[10; x]"]),
        ("run", ["--numeric-type", "float16", "--burn-schedule", "[x]"]),
        ("main", ["--profile"]),
    ],
    "mcmc_clustering_eap_chain_2d": [
        ("params", ["-T", "rod"]), ("params", ["-u", "cutoff"]), ("params", ["--rng", "lcg"]),
        ("params", ["-T", "rod", "-u", "x", "--rng", "x"]), ("params", ["-u", "x", "--rng", "x"]),
        ("parse", ["--precision", "f64"]),
        ("run", ["--numeric-type", "float16"]), ("run", ["--burn-schedule", "10; 1"]), ("run", ["--burn-schedule", "[10; x]"]),
        ("run", ["--numeric-type", "float16", "--burn-schedule", "[x]"]),
        ("main", ["--profile"]),
    ],
}


def _options(mod):
    return [dict(flags=a.option_strings, dest=a.dest, action=type(a).__name__, type=getattr(a.type, "__name__", None),
                 default=a.default, help=a.help) for a in mod.build_parser()._actions]


def _params(mod, argv):
    p = mod.params_from_pargs(mod.parse_args(argv + ["--seed", "11"]), 5, 2, 0)
    return {f: getattr(p, f) for f, _ in p._fields_}


def _error(mod, where, argv):
    err = io.StringIO()
    try:
        with contextlib.redirect_stderr(err), contextlib.redirect_stdout(io.StringIO()):
            if where == "main":
                mod.main(argv)
            else:
                pargs = mod.parse_args(argv + ["--seed", "11"])
                if where == "params":
                    mod.params_from_pargs(pargs, 5, 2, 0)
                elif where == "run":
                    mod.mcmc(10, pargs) if hasattr(mod, "mcmc") else mod.run(pargs)
    except SystemExit as e:                     # argparse: the usage text depends on the terminal, the exit code does not
        return dict(type="SystemExit", message=str(e.code))
    except Exception as e:
        return dict(type=type(e).__name__, message=str(e), stderr=err.getvalue())
    return dict(type=None, message=None, stderr=err.getvalue())


def _summary(mod, name):
    A = mod.Averager
    planar = name.endswith("_2d")
    scalars = [57.25, 1.5e-7, -3.0, 9.0e6] + ([0.4, 1.2] if name == "mcmc_clustering_eap_chain" else [])
    vectors = [[1.0, 2.0, 3.0], [4.0, 5.5, 6.0], [0.1, 0.2, 1e7], [7.0, 1e-5, 9.0]]
    vas = [A(np.array(v)[[0, 2]] if planar else np.array(v), None) for v in vectors]
    return mod.summary_lines([A(x, None) for x in scalars], vas, 0.3125, mod.default_pargs(**{"num-monomers": 40, "mlen": 0.5}))


def tables(package="polymer_stats_amd") -> dict:
    out = {}
    for name in MAINS:
        mod = importlib.import_module(f"{package}.{name}")
        out[name] = dict(options=_options(mod),
                         params=[dict(argv=argv, fields=_params(mod, argv)) for argv in PARAMS[name]],
                         errors=[dict(where=w, argv=argv, **_error(mod, w, argv)) for w, argv in ERRORS[name]],
                         summary=_summary(mod, name))
    return out


def dumps(t: dict) -> str:
    """One option (one command line, one error, one stdout line) per line."""
    main_texts = []
    for name, sections in t.items():
        parts = []
        for key, rows in sections.items():
            body = ",\n".join("      " + json.dumps(r, ensure_ascii=False) for r in rows)
            parts.append(f"    {json.dumps(key)}: [\n{body}\n    ]")
        main_texts.append(f"  {json.dumps(name)}: {{\n" + ",\n".join(parts) + "\n  }")
    return "{\n" + ",\n".join(main_texts) + "\n}\n"


if __name__ == "__main__":
    sys.path.insert(0, os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(HERE)))
    with open(os.path.join(HERE, "host_tables.json"), "w") as f:
        f.write(dumps(tables()))
