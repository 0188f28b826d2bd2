#!/usr/bin/env python3
"""What one histogram record costs beside one recorded series row, at the three shapes a handle is used at:
one case of 65 536 chains, 2 730 single-chain cases (a phase scan), 546 cases of 128 chains.

Both recorders read the same DevState::obs rows between step launches; the series row (launch_record) does the heavier
reduction, the histogram the atomics.  Timed with HIP events on the handle's stream, after warm-up, per shape:
  record    R back-to-back pstat_hist_record calls between two events: the launch on its own;
  H, S, 0   R single-step launches each followed by a histogram record (pstat_advance_hist, stepout 1), by a series row
            (pstat_advance_series, stepout 1), by nothing: (H - 0) / R and (S - 0) / R are what a record and a row add to a run.
Writes profiles/hist/time_hist.json (and prints it): microseconds per record / row, medians over --reps.

    python tools/time_hist.py
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1, 65536), (2730, 1), (546, 128)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-n", type=int, default=8)
    ap.add_argument("--records", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nbins", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hist", "time_hist.json"))
    args = ap.parse_args()

    import torch
    import polymer_stats_amd as ps
    from bench import kernel_source_hash

    stream = torch.cuda.Stream()
    R = args.records
    specs = [ps.hist_spec("r3", args.nbins, -args.n, args.n), ps.hist_spec("U", args.nbins, -2.0 * args.n, 2.0 * args.n),
             ps.hist_spec("rmag", args.nbins, 0.0, args.n)]

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b) * 1e3      # microseconds

    results = []
    for ncases, chains in SHAPES:
        cases = [ps.default_params(n=args.n, E0=0.2 * (k % 26), kT=10.0 ** (-1 + 0.1 * ((k // 26) % 21)), K1=1.0, K2=0.0, Fz=0.5,
                                   num_chains=chains, seed=1 + k, precision=ps.F64) for k in range(ncases)]
        with ps.Ensemble(cases, stream=stream.cuda_stream) as e:
            h = e.open_hist(specs)
            s = e.open_series(R)
            e.advance(500)

            def leg_record():
                for _ in range(R):
                    h.record()

            def leg_H():
                e.advance_hist(h, R, 1)

            def leg_S():
                s.clear()
                e.advance_series(s, R, 1)

            def leg_0():
                for _ in range(R):
                    e.advance(1)

            legs = {"record": leg_record, "H": leg_H, "S": leg_S, "0": leg_0}
            times = {k: [] for k in legs}
            for rep in range(args.reps + 1):            # the first round warms up
                for k, leg in legs.items():
                    t = timed(leg)
                    if rep:
                        times[k].append(t / R)
            e.sync()
            got = h.read()
            assert all(int(c.sum()) + int(got.tails[:, i].sum()) == got.samples * ncases for i, c in enumerate(got.counts))
            med = {k: statistics.median(v) for k, v in times.items()}
            results.append(dict(cases=ncases, chains=chains, n=args.n, specs=len(specs), nbins=args.nbins, records=R,
                                kernel=e.launch_info().kernel.decode(),
                                us_per_launch={k: [round(t, 3) for t in v] for k, v in times.items()},
                                median_us={k: round(t, 3) for k, t in med.items()},
                                hist_record_us=round(med["record"], 3), hist_added_us=round(med["H"] - med["0"], 3),
                                series_row_added_us=round(med["S"] - med["0"], 3),
                                record_over_row=round((med["H"] - med["0"]) / max(med["S"] - med["0"], 1e-9), 3)))
            print("# " + json.dumps(results[-1]), file=sys.stderr, flush=True)
    out = dict(kernel_source_sha256_16=kernel_source_hash(), device=torch.cuda.get_device_name(0), shapes=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
