#!/usr/bin/env python3
"""What the stepout time series costs, library level, no text.

Three legs on fresh handles of the same ensemble, alternated in one process, each ending in a synchronise:
  P  the per-row loop the hosts used: advance(stepout), then microstate and reduce_host of every case, row after row;
  S  advance_series in chunks of --chunk rows, each chunk read back once;
  0  the same steps unrecorded, in launches of `stepout` (advance x rows, one sync at the end): S - 0 is the recorder.
Prints one JSON line: seconds per leg and repetition, their medians and spreads, S against P and against 0.

    python tools/time_series.py                       # 546 cases x 16 chains, n = 100, Ising, f64, 250 000 steps, stepout 250
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=546)
    ap.add_argument("--chains", type=int, default=16)
    ap.add_argument("-n", type=int, default=100)
    ap.add_argument("--steps", type=int, default=250000)
    ap.add_argument("--stepout", type=int, default=250)
    ap.add_argument("--chunk", type=int, default=1000, help="rows per read-back of leg S")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2000, help="steps every handle takes before its leg is timed")
    ap.add_argument("--legs", default="P,S,0")
    args = ap.parse_args()

    import polymer_stats_amd as ps
    cases = [ps.default_params(n=args.n, E0=0.2 * (k % 26), kT=10.0 ** (-2 + 0.2 * (k // 26)), K1=1.0, K2=0.0,
                               num_chains=args.chains, seed=1 + k, energy_type=ps.ISING, precision=ps.F64)
             for k in range(args.cases)]
    rows = args.steps // args.stepout

    def leg_P(e):
        for _ in range(rows):
            e.advance(args.stepout)
            for k in range(e.ncases):
                e.microstate(k * e.num_chains)
                e.reduce_host(k)

    def leg_S(e):
        s = e.open_series(min(args.chunk, rows))
        done = 0
        while done < rows:
            m = min(args.chunk, rows - done)
            e.advance_series(s, m * args.stepout, args.stepout)
            s.read()
            s.clear()
            done += m
        s.close()

    def leg_0(e):
        for _ in range(rows):
            e.advance(args.stepout)
        e.sync()

    legs = {"P": leg_P, "S": leg_S, "0": leg_0}
    names = [x for x in args.legs.split(",") if x]
    times = {x: [] for x in names}
    kernel = ""
    for _ in range(args.reps):
        for x in names:
            with ps.Ensemble(cases) as e:
                kernel = e.launch_info().kernel.decode()
                e.advance(args.warmup)
                e.sync()
                t0 = time.perf_counter()
                legs[x](e)
                e.sync()
                times[x].append(time.perf_counter() - t0)
                print(f"# leg {x}: {times[x][-1]:.3f} s", file=sys.stderr, flush=True)
    out = dict(cases=args.cases, chains=args.chains, n=args.n, steps=args.steps, stepout=args.stepout, rows=rows, chunk=args.chunk,
               kernel=kernel, seconds={x: [round(t, 4) for t in v] for x, v in times.items()},
               median={x: round(statistics.median(v), 4) for x, v in times.items()},
               spread={x: round(max(v) - min(v), 4) for x, v in times.items()})
    med = out["median"]
    if "P" in med and "S" in med:
        out["P_over_S"] = round(med["P"] / med["S"], 2)
    if "0" in med and "S" in med:
        out["S_excess_over_0"] = round(med["S"] / med["0"] - 1.0, 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
