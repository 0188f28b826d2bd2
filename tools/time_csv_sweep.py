#!/usr/bin/env python3
"""End-to-end time of a sweep that writes its time-series files (what `tools/run_sweep.py --csv` runs), and the share of it
spent formatting text.  The grid of run/K1_E0-kT-phase.jl, fixed-force main, Ising, f64:

    python tools/time_csv_sweep.py WORKDIR                      # 546 cases x 16 chains, n = 100, 250 000 steps, --stepout 250
    python tools/time_csv_sweep.py WORKDIR --tree OTHER_CHECKOUT  # the same sweep through another checkout's package

`--tree` names a checkout (with a built libpstat.so) whose polymer_stats_amd is imported instead of this one's: the two are
compared by running them one after the other.  jl_row -- every row of both files goes through it -- is wrapped with a clock
in every module of the imported package that holds it, wherever that checkout formats its rows.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workdir")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--chains", type=int, default=16)
    ap.add_argument("-n", type=int, default=100)
    ap.add_argument("--steps", type=int, default=250000)
    ap.add_argument("--stepout", type=int, default=250)
    ap.add_argument("--main", default="mcmc_eap_chain", choices=["mcmc_eap_chain", "mcmc_clustering_eap_chain", "mcmc_clustering_eap_chain_2d"])
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    from polymer_stats_amd import sweep as sw, julia_fmt

    spent = [0.0, 0]
    inner = julia_fmt.jl_row

    def timed_row(values):
        t0 = time.perf_counter()
        out = inner(values)
        spent[0] += time.perf_counter() - t0
        spent[1] += 1
        return out

    for name, mod in list(sys.modules.items()):
        if name.startswith("polymer_stats_amd.") and hasattr(mod, "jl_row"):
            mod.jl_row = timed_row
    cases = sw.product_cases([("kT", sw.axis_values("10^(-2:0.2:2)")), ("E0", sw.axis_values("0:0.2:5")), ("K1", [1]), ("K2", [0]),
                              ("n", [args.n])])
    fixed = ["--chain-type", "dielectric", "--energy-type", "Ising", "--num-steps", str(args.steps), "--stepout", str(args.stepout),
             "-v", "0"]
    t0 = time.perf_counter()
    res = sw.run_sweep(args.main, fixed, cases, args.workdir, num_chains=args.chains, seed=1, write_csv=True, overwrite=True)
    total = time.perf_counter() - t0
    print(json.dumps(dict(tree=os.path.abspath(args.tree), main=args.main, cases=len(res["ran"]), chains=args.chains, n=args.n,
                          steps=args.steps, stepout=args.stepout, seconds=round(total, 2), jl_row_seconds=round(spent[0], 2),
                          jl_row_calls=spent[1], text_share=round(spent[0] / total, 3))))


if __name__ == "__main__":
    main()
