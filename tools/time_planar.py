#!/usr/bin/env python3
"""Proposals per second of the planar main's kernel (pstat_planar.hip) and, beside each figure, of the 3D clustering main
at the same chain length, chain count and energy in the same process: HIP-event time of warmed launches through torch on
the stream the library launches on; three timed launches after the warm-up, median and spread (min .. max) reported.

    python tools/time_planar.py [--quick] [--only SUBSTRING] [--json OUT]

Shapes: Ising dielectric at n = 25 and n = 100 with 65 536 chains; the 880 cases of 2D/run/Ising_2024-11-06.jl
(n = 25, E0 = 0.1, K1 in 0.01 .. 0.4, Fz in 0 .. 50) with 1 and with 64 chains per case.  The 3D twin runs on its default
home and, f64 cells in LDS (PSTAT_F64_STATE=l), on ClusterLds; cluster_prob = 0.5 on both sides (the planar main reads it
as the probability of flipping, the 3D one as that of not trying: at 0.5 the same).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FZS = [0, 0.1, 0.2, 0.3, 0.4, 0.5, 1, 2, 3, 4, 5, 7.5, 10, 12.5, 15, 20, 25, 30, 35, 40, 45, 50]
K1S = [0.01, 0.04, 0.1, 0.4]


def timed(ps, torch, name, make, planar, nsteps, warm, env=None):
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            e = ps.Ensemble(make(), stream=stream.cuda_stream, planar=planar)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    with torch.cuda.stream(stream):
        e.advance(warm)                        # warm-up: also leaves the adaptation in its regime
        torch.cuda.synchronize()
        times = []
        for _ in range(3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            e.advance(nsteps)
            b.record(stream)
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b))
        info = e.launch_info()
        s = e.summary(0)
        chains = e.num_chains * e.ncases
        e.close()
    med = statistics.median(times)
    out = dict(config=name, chains=chains, n=e.n, steps=nsteps, ms_median=round(med, 3), ms_min=round(min(times), 3),
               ms_max=round(max(times), 3), proposals_per_s=chains * nsteps / (med * 1e-3), kernel=info.kernel.decode(),
               lanes=info.lanes_per_block, wg_per_cu=info.blocks_per_cu, lds_bytes=info.lds_bytes, packed=info.packed_cases,
               AR=s.acceptance_ratio, nan_rejects=s.nan_rejects)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="a tenth of the steps")
    ap.add_argument("--only", default="", help="substring filter on the configuration name")
    ap.add_argument("--json", default="", help="also write the list of results here")
    args = ap.parse_args()
    import torch
    import polymer_stats_amd as ps
    q = 10 if args.quick else 1
    res = []

    def both(name, kw, chains, cases, nsteps, warm):
        """the planar kernel, then the 3D clustering main on its default home and on ClusterLds"""
        if args.only and args.only not in name:
            return
        grid = cases or [dict()]
        res.append(timed(ps, torch, name + " [planar]",
                         lambda: [ps.default_planar_params(**{**dict(num_chains=chains, cluster_prob=0.5, seed=6), **kw, **g})
                                  for g in grid], True, nsteps, warm))
        three = lambda: [ps.default_params(**{**dict(num_chains=chains, move_set=ps.MOVES_CLUSTER, cluster_prob=0.5, adj_ub=0.40,
                                                     seed=6), **kw, **g}) for g in grid]
        res.append(timed(ps, torch, name + " [3D, default home]", three, False, nsteps, warm))
        res.append(timed(ps, torch, name + " [3D, ClusterLds]", three, False, nsteps, warm, env={"PSTAT_F64_STATE": "l"}))

    ising = dict(E0=0.1, K1=0.04, K2=0.0, kT=1.0, Fz=1.0, energy_type=ps.ISING)
    both("Ising dielectric n=25 x 65536", dict(n=25, **ising), 65536, None, 20000 // q, 2500)
    both("Ising dielectric n=100 x 65536", dict(n=100, **ising), 65536, None, 5000 // q, 2500)
    grid = [dict(Fz=float(f), K1=k, seed=1000 + 10 * (4 * i + j) + r) for i, f in enumerate(FZS) for j, k in enumerate(K1S)
            for r in range(10)]
    sweep = dict(n=25, E0=0.1, K2=0.0, kT=1.0, energy_type=ps.ISING)
    both("Ising_2024-11-06 880 cases x 1", sweep, 1, grid, 50000 // q, 2500)
    both("Ising_2024-11-06 880 cases x 64", sweep, 64, grid, 20000 // q, 2500)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
