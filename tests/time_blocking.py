#!/usr/bin/env python3
"""What error bars cost, device against host: for one recorded series of --cases single-chain cases x --rows
rows, the wall time of Series.error_bars() (two kernels, 6 + 24 doubles per column come back) beside that of Series.read() +
the numpy twin (tests/blocking_ref.py: the whole series comes back and is blocked on the host).  One warm-up and --reps
repetitions of each; prints one JSON line per shape.  It lives under tests/ because it uses the twin.

    python tests/time_blocking.py --cases 546 2730
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, nargs="+", default=[546, 2730])
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--stepout", type=int, default=10)
    ap.add_argument("-n", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()

    import numpy as np
    import blocking_ref as br
    import polymer_stats_amd as ps
    from bench import kernel_source_hash

    for ncases in args.cases:
        cases = [ps.default_params(n=args.n, E0=0.2 * (k % 26), kT=10.0 ** (-2 + 0.2 * ((k // 26) % 21)), K1=1.0, K2=0.0, num_chains=1,
                                   seed=1 + k, energy_type=ps.ISING, precision=ps.F64) for k in range(ncases)]
        with ps.Ensemble(cases) as e:
            s = e.open_series(args.rows)
            e.advance_series(s, args.rows * args.stepout, args.stepout)
            e.sync()

            def device():
                return s.error_bars(levels=True)

            def host():
                steps, red, _, _ = s.read()
                return br.blocking(br.batches(steps, red))

            times = {"device": [], "host": []}
            for name, leg in (("device", device), ("host", host)):
                for rep in range(args.reps + 1):
                    t0 = time.perf_counter()
                    got = leg()
                    if rep:
                        times[name].append(time.perf_counter() - t0)
                if name == "device":
                    dev = got
            same = bool(np.allclose(dev.stderr.reshape(-1), got["stderr"], rtol=1e-9, atol=0, equal_nan=True))
            s.close()
        print(json.dumps(dict(cases=ncases, rows=args.rows, n=args.n, series_bytes=8 * args.rows * ncases * (ps.NRED + 7),
                              kernel_source_sha256_16=kernel_source_hash(),
                              seconds={k: [round(t, 5) for t in v] for k, v in times.items()},
                              median={k: round(statistics.median(v), 5) for k, v in times.items()},
                              spread={k: round(max(v) - min(v), 5) for k, v in times.items()},
                              host_over_device=round(statistics.median(times["host"]) / statistics.median(times["device"]), 1),
                              stderr_agrees_1e9=same)), flush=True)


if __name__ == "__main__":
    main()
