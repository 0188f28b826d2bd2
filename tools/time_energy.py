#!/usr/bin/env python3
"""What one energy record costs, on two shapes: one case of 65 536 chains of n = 100 (max_sep 99: a column per
separation, 3.2e8 pair terms per record) and one of 4 096 chains of n = 64, f64, with a `within` column at 1.5 monomer lengths.
Beside each, in the same process on the same ensemble's shape, the yardstick: a pair-distance record with no histogram and no
Debye magnitude (R2(s) and the closest approach: the same positions and the same pairs, a square root per pair and no dipole).
Both pair mappings of pstat_energy.hip are timed, each on a handle of its own (PSTAT_ENERGY_MAP is read when a handle is made):
  paired    separations s and n - s share a wavefront pass (the default);
  single    a separation per wavefront pass, pdist's R2(s) mapping.
`lane_use` is the share of the pair phase's lane slots that hold a pair under the mapping.

Timed with HIP events on the handle's stream: after one warm-up record, three records, each between its own pair of events.
Writes profiles/energy/time_energy.json (and prints it).

    python tools/time_energy.py
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(65536, 100), (4096, 64)]
CUTOFF = 1.5


def lane_use(n, paired):
    """Pairs over lane slots of the pair phase: a pass takes ceil(pairs / 64) strides of 64 lanes."""
    if paired:
        slots = sum(64 * -(-(n if n - u != u else n - u) // 64) for u in range(1, n // 2 + 1))
    else:
        slots = sum(64 * -(-(n - s) // 64) for s in range(1, n))
    return (n * (n - 1) // 2) / slots


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "energy", "time_energy.json"))
    args = ap.parse_args()

    import torch
    import polymer_stats_amd as ps
    from bench import kernel_source_hash

    stream = torch.cuda.Stream()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b) * 1e3      # microseconds

    results = []
    kernel = ""
    for chains, n in SHAPES:
        pairs = chains * (n * (n - 1) // 2)
        p = ps.default_params(n=n, E0=1.0, K1=1.0, K2=0.0, Fz=0.5, kT=1.0, num_chains=chains, seed=1, precision=ps.F64)
        sums = {}
        for name, env, open_ in (("energy paired", "p", lambda e: e.open_energy(-1, CUTOFF)),
                                 ("energy single", "s", lambda e: e.open_energy(-1, CUTOFF)),
                                 ("pdist", None, lambda e: e.open_pdist())):
            if env:
                os.environ["PSTAT_ENERGY_MAP"] = env
            else:
                os.environ.pop("PSTAT_ENERGY_MAP", None)
            with ps.Ensemble(p, stream=stream.cuda_stream) as e:
                e.advance(5 * n)
                g = open_(e)
                g.record()                                          # warms up
                e.sync()
                us = [timed(g.record) for _ in range(args.records)]
                e.sync()
                got = g.read()
                assert got.records == args.records + 1 and np.all(np.isfinite(got.sum))
                sums[name] = got.sum
                g.close()
                kernel = e.launch_info().kernel.decode()
            med = statistics.median(us)
            results.append(dict(config=name, chains=chains, n=n, max_sep=n - 1, records=args.records, us=[round(t, 1) for t in us],
                                median_us=round(med, 1), spread_us=round(max(us) - min(us), 1), pairs_per_record=pairs,
                                pairs_per_second=round(pairs / (med * 1e-6), 0),
                                lane_use=round(lane_use(n, name == "energy paired"), 4) if env else None))
            print("# " + json.dumps(results[-1]), file=sys.stderr, flush=True)
        a, b = sums["energy paired"], sums["energy single"]         # the two mappings: the same sums to rounding
        assert np.allclose(a, b, rtol=1e-9, atol=1e-9 * np.abs(a).max())
    os.environ.pop("PSTAT_ENERGY_MAP", None)
    out = dict(kernel_source_sha256_16=kernel_source_hash(), device=torch.cuda.get_device_name(0), step_kernel=kernel,
               configs=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
