#!/usr/bin/env python3
"""What one pair-distance record costs, on the bench shape: one case of 65 536 chains, n = 100, f64, that is
3.2e8 pairs per record, in three configurations of the object, and the shape recorder in the same process as the yardstick:
  hist     nbins = 128 below rmax = 30, no Debye magnitudes: the pair loop with its LDS integer add;
  debye    nq = 16 magnitudes up to q b = 6, no histogram: 16 sines per pair, n / 2 times what the shape recorder takes per
           wave-vector;
  both     the two together (one walk over the pairs: the first block of q shares it with the histogram);
  shape    pstat_shape_record at nq = 16 wave-vectors along z up to |q| b = 6.
Every object also has its default R2(s) columns, s = 1 .. 99 (the shape object: its gyration block).

Timed with HIP events on the handle's stream: after one warm-up record, three records, each between its own pair of events.
Writes profiles/pdist/time_pdist.json (and prints it): the three times, their median and spread (max - min), pairs per second
and sines per second (chains * pairs * nq per record; the 2 n per chain of the unit vectors are not counted).

    python tools/time_pdist.py
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHAINS, N = 65536, 100
NBINS, RMAX, NQ, QMAX = 128, 30.0, 16, 6.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=3)
    ap.add_argument("--chains", type=int, default=CHAINS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pdist", "time_pdist.json"))
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

    q = QMAX * np.arange(1, NQ + 1) / NQ
    qz = np.zeros((NQ, 3))
    qz[:, 2] = q
    pairs = args.chains * (N * (N - 1) // 2)
    # name: (how the object is opened, pairs per record, sines per record)
    configs = {
        "hist": (lambda e: e.open_pdist(bins=(NBINS, RMAX)), pairs, 0),
        "debye": (lambda e: e.open_pdist(q=q), pairs, pairs * NQ),
        "both": (lambda e: e.open_pdist(bins=(NBINS, RMAX), q=q), pairs, pairs * NQ),
        "shape": (lambda e: e.open_shape(qz), 0, args.chains * N * NQ),
    }
    results = []
    p = ps.default_params(n=N, E0=1.0, K1=1.0, K2=0.0, Fz=0.5, kT=1.0, num_chains=args.chains, seed=1, precision=ps.F64)
    with ps.Ensemble(p, stream=stream.cuda_stream) as e:
        e.advance(5 * N)
        for name, (open_, npairs, nsines) in configs.items():
            g = open_(e)
            g.record()                                          # warms up
            e.sync()
            us = [timed(g.record) for _ in range(args.records)]
            e.sync()
            got = g.read()
            assert got.records == args.records + 1 and np.all(np.isfinite(got.sum))
            if name != "shape":
                assert np.all(got.rmin > 0)
                if got.nbins:
                    assert got.counts.sum() + got.above.sum() == got.records * pairs
            g.close()
            med = statistics.median(us)
            results.append(dict(config=name, chains=args.chains, n=N, nbins=NBINS if name in ("hist", "both") else 0,
                                nq=0 if name == "hist" else NQ, records=args.records, us=[round(t, 1) for t in us],
                                median_us=round(med, 1), spread_us=round(max(us) - min(us), 1),
                                pairs_per_record=npairs, pairs_per_second=round(npairs / (med * 1e-6), 0) if npairs else None,
                                sines_per_record=nsines, sines_per_second=round(nsines / (med * 1e-6), 0) if nsines else None))
            print("# " + json.dumps(results[-1]), file=sys.stderr, flush=True)
        kernel = e.launch_info().kernel.decode()
    out = dict(kernel_source_sha256_16=kernel_source_hash(), device=torch.cuda.get_device_name(0), step_kernel=kernel,
               configs=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
