#!/usr/bin/env python3
"""What one shape record costs beside advancing the same handle one sweep (n steps):
  bench shape        one case of 65 536 chains, n = 100, f64, at nq = 0, 64 and 256 wave-vectors;
  phase-scan shape   2 730 cases of one chain, n = 200, the clustering main, at nq = 64.
The wave-vectors are equally spaced along z up to |q| b = 6.

Timed with HIP events on the handle's stream, after a warm-up round, per shape and nq:
  record   R back-to-back pstat_shape_record calls between two events: the launch pair on its own, microseconds per record;
  sweep    R calls of advance(n) between two events: microseconds per n steps.
Writes profiles/shape/time_shape.json (and prints it): medians over --reps, record / sweep, and for nq > 0 the sincos of the
hot loop per second (chains * n * nq phases per record, one sincos each; the 2 n per chain of the unit vectors are not counted).

    python tools/time_shape.py
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, cases, chains, n, wave-vector counts, the clustering main)
SHAPES = [("bench", 1, 65536, 100, (0, 64, 256), False), ("phase scan", 2730, 1, 200, (64,), True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shape", "time_shape.json"))
    args = ap.parse_args()

    import torch
    import polymer_stats_amd as ps
    from bench import kernel_source_hash

    stream = torch.cuda.Stream()
    R = args.records

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b) * 1e3      # microseconds

    results = []
    for name, ncases, chains, n, counts, cluster in SHAPES:
        extra = dict(move_set=ps.MOVES_CLUSTER, energy_type=ps.ISING) if cluster else {}
        cases = [ps.default_params(n=n, E0=0.2 * (k % 26), kT=10.0 ** (-1 + 0.1 * ((k // 26) % 21)), K1=1.0, K2=0.0, Fz=0.5,
                                   num_chains=chains, seed=1 + k, precision=ps.F64, **extra) for k in range(ncases)]
        with ps.Ensemble(cases, stream=stream.cuda_stream) as e:
            e.advance(5 * n)
            for nq in counts:
                q = np.zeros((nq, 3))
                q[:, 2] = 6.0 * np.arange(1, nq + 1) / max(nq, 1)
                g = e.open_shape(q)

                def leg_record():
                    for _ in range(R):
                        g.record()

                def leg_sweep():
                    for _ in range(R):
                        e.advance(n)

                legs = {"record": leg_record, "sweep": leg_sweep}
                times = {k: [] for k in legs}
                for rep in range(args.reps + 1):            # the first round warms up
                    for k, leg in legs.items():
                        t = timed(leg)
                        if rep:
                            times[k].append(t / R)
                e.sync()
                got = g.read()
                assert got.records == R * (args.reps + 1) and np.all(got.rg2 > 0) and np.all(np.isfinite(got.sum))
                g.close()
                med = {k: statistics.median(v) for k, v in times.items()}
                pairs = ncases * chains * n * nq
                results.append(dict(shape=name, cases=ncases, chains=chains, n=n, nq=nq, records=R,
                                    kernel=e.launch_info().kernel.decode(),
                                    us={k: [round(t, 2) for t in v] for k, v in times.items()},
                                    record_us=round(med["record"], 2), sweep_us=round(med["sweep"], 2),
                                    record_over_sweep=round(med["record"] / max(med["sweep"], 1e-9), 4),
                                    sincos_per_record=pairs,
                                    sincos_per_second=round(pairs / (med["record"] * 1e-6), 0) if nq else None))
                print("# " + json.dumps(results[-1]), file=sys.stderr, flush=True)
    out = dict(kernel_source_sha256_16=kernel_source_hash(), device=torch.cuda.get_device_name(0), shapes=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
