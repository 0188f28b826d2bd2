#!/usr/bin/env python3
"""BASELINE configs[4]: (E0, kT) phase-diagram scan at n = 200 (grid of run/K1_E0-kT-phase.jl:21-24:
E0 in 0:0.2:5, kT in 10^(-2:0.2:2), K1 = 1, K2 = 0, b = 1, F = 0), all 546 grid points in ONE
batched launch per GPU.  The reference farms the grid points out to worker processes with `pmap`
(run/K1_E0-kT-phase.jl:19-45); here the chains of every grid point are sharded over the ranks by global chain id
and the only exchange is one all-reduce(SUM) of the [points x 41] reduction tensor (RCCL; nothing at all for one GPU).

    python tools/phase_scan.py --chains 128 --steps 50000 --burn-in 20000 --energy Ising --out scan.csv
    python tools/phase_scan.py --main clustering --burn-schedule "1000,100,10,2,1" ...   # what the reference's
        # run/K1_E0-kT-phase.jl:45 launches per grid point: mcmc_clustering_eap_chain.jl with its annealed ladder
    python tools/phase_scan.py --chains 1 --steps 2500000 --error-bars 1000 ...   # error bars from ONE chain per point: the
        # production run is recorded on the device as 1000 batches; their blocked standard errors (Flyvbjerg-Petersen,
        # Series.error_bars) are the columns r3_blocked ... converged (0: the run is too short for r3, p3 or U at that point)
    python tools/phase_scan.py --exchange 50 ...                 # replica exchange along kT: every column of equal E0 is a
        # ladder, one exchange round after every 50 steps of the burn-in rungs and of the production run; adds the column
        # swap_acceptance (Ensemble.open_tempering)
    python tools/phase_scan.py --gpus 8 ...                      # starts its own 8 ranks, one per GPU (RCCL)
    python tools/phase_scan.py --gpus 2 --backend gloo ...       # rehearsal: ranks may share a GPU, all-reduce via host
    python -m torch.distributed.run --nproc-per-node 8 tools/phase_scan.py --gpus 8 ...   (also fine)

`--chains` is chains per grid point PER RANK: rank r owns global chain ids [r * chains, (r + 1) * chains) of every
point, so N ranks x C chains pool exactly the chains of one rank x N*C (tests/test_gpu_dist.py).
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def grid_points(points: int):
    g = [(0.2 * i, 10.0 ** (-2 + 0.2 * j)) for i in range(26) for j in range(21)]   # run/K1_E0-kT-phase.jl:21-24
    if points and points < len(g):      # an evenly spread subset (tests, rehearsals)
        g = [g[(k * len(g)) // points] for k in range(points)]
    return g


def _all_reduced(dist, host, backend):
    """SUM over the ranks of a host tensor (nccl reduces device tensors, gloo host ones)."""
    if backend == "gloo":
        dist.all_reduce(host)
        return host
    dev = host.cuda()
    dist.all_reduce(dev)
    return dev.cpu()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200)
    ap.add_argument("--chains", type=int, default=128, help="chains per grid point per rank")
    ap.add_argument("--steps", type=int, default=50000)
    ap.add_argument("--burn-in", type=int, default=20000)
    ap.add_argument("--energy", choices=["noninteracting", "Ising"], default="Ising")
    ap.add_argument("--precision", choices=["f32", "f64", "q16"], default="f64", help="f64 = the reference's arithmetic (default); f32 / q16 = fast paths")
    ap.add_argument("--main", choices=["fixed-force", "clustering"], default="fixed-force",
                    help="which main's step: mcmc_eap_chain.jl or mcmc_clustering_eap_chain.jl (cluster flips)")
    ap.add_argument("--burn-schedule", default="1", help="kT multipliers of the burn-in ladder, comma-separated")
    ap.add_argument("--bend-mod", type=float, default=0.0)
    ap.add_argument("--cluster-prob", type=float, default=0.5)
    ap.add_argument("--points", type=int, default=0, help="use only this many grid points, evenly spread (0 = all 546)")
    ap.add_argument("--seed", type=int, default=20260501)
    ap.add_argument("--gpus", type=int, default=1, help="ranks; > 1 from a bare shell starts them (one per GPU)")
    ap.add_argument("--backend", choices=["nccl", "gloo"], default="nccl",
                    help="collective backend; gloo (through host memory, ranks may share a GPU) to rehearse N > 1 on a box with fewer GPUs")
    ap.add_argument("--error-bars", type=int, default=0, metavar="N",
                    help="record the production run as N batches of steps / N steps and add their blocked standard errors as the columns "
                         "r3_blocked, p3_blocked, U_blocked, r3_ineff, U_ineff, converged (one rank only; a remainder steps %% N is run and belongs to no batch)")
    ap.add_argument("--exchange", type=int, default=0, metavar="EVERY",
                    help="replica exchange between the grid points of equal E0 (a ladder along kT): one round after every EVERY steps of "
                         "the burn-in rungs and of the production run; adds the column swap_acceptance = accepted / attempted exchanges "
                         "the point took part in during production (0: off; each rank exchanges among its own chains)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    if args.exchange < 0:
        raise SystemExit(f"--exchange {args.exchange}: a number of steps between exchange rounds, or 0 for none")
    if args.exchange and args.error_bars:
        raise SystemExit("--exchange cannot be combined with --error-bars yet: exchanges interleaved with the recorded rows of a "
                         "series are the follow-up to this option")
    if args.error_bars:
        if args.gpus > 1:       # the ranks hold different chains of the same point; their series are not merged
            raise SystemExit(f"--error-bars needs one rank, not --gpus {args.gpus}")
        if args.error_bars < 32 or args.steps < args.error_bars:
            raise SystemExit(f"--error-bars {args.error_bars}: at least 32 batches of at least one step each (--steps {args.steps})")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # start the ranks BEFORE anything touches the GPU; this process never imports torch
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from rank_spawn import spawn_ranks
        rc, out0 = spawn_ranks(os.path.abspath(__file__), sys.argv[1:], args.gpus)
        sys.stdout.write(out0)
        sys.exit(rc)

    import torch
    import torch.distributed as dist
    import polymer_stats_amd as ps

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("phase_scan.py needs a GPU: libpstat has no CPU path")
    ndev = torch.cuda.device_count()
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.backend == "nccl" and local >= ndev:
        raise SystemExit(f"rank {rank}: LOCAL_RANK {local} but only {ndev} GPU(s) visible (use --backend gloo to rehearse)")
    local %= ndev
    torch.cuda.set_device(local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29512")
        if args.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)
    prec = {"f32": ps.F32, "f64": ps.F64, "q16": ps.Q16}[args.precision]
    en = ps.ISING if args.energy == "Ising" else ps.NONINTERACTING
    grid = grid_points(args.points)
    cases = [ps.default_params(n=args.n, E0=E0, kT=kT, K1=1.0, K2=0.0, b=1.0, num_chains=args.chains,
                               chain_id0=rank * args.chains, seed=args.seed + k, precision=prec,
                               energy_type=en, device=local,
                               **(dict(move_set=ps.MOVES_CLUSTER, bend_mod=args.bend_mod, cluster_prob=args.cluster_prob,
                                       adj_ub=0.40) if args.main == "clustering" else {}))
             for k, (E0, kT) in enumerate(grid)]
    stream = torch.cuda.Stream()
    red = torch.zeros(len(grid), ps.NRED, dtype=torch.float64, device="cuda")
    with torch.cuda.stream(stream):
        e = ps.Ensemble(cases, stream=stream.cuda_stream)
        temper = e.open_tempering(ps.ladders_by(cases), seed=args.seed) if args.exchange else None
        advance = (lambda nsteps: e.advance_tempered(temper, nsteps, args.exchange)) if temper else e.advance
        t0 = time.perf_counter()
        ladder = [float(x) for x in args.burn_schedule.split(",") if x.strip()]
        rungs = 0
        if args.burn_in > 0:
            for mult in ladder:             # every rung is a fresh mcmc() call in the clustering main
                e.scale_kT(mult)
                if args.main == "clustering":
                    e.reset_sampler()
                advance(args.burn_in)
                rungs += 1
            e.scale_kT(1.0)
            if args.main == "clustering":
                e.reset_sampler()
            e.reset_averages()
        swaps0 = temper.stats() if temper else None     # what the burn-in exchanged is not the production run's acceptance
        eb = None
        if args.error_bars:
            series = e.open_series(args.error_bars)
            try:        # exactly N rows of steps // N steps; the remainder is advanced and belongs to no batch
                q = args.steps // args.error_bars
                e.advance_series(series, args.error_bars * q, q)
                e.advance(args.steps - args.error_bars * q)
                eb = series.error_bars()
            finally:
                series.close()
        else:
            advance(args.steps)
        for k in range(len(grid)):
            e.reduce_into(red[k].data_ptr(), icase=k)
        if world > 1:
            if args.backend == "nccl":
                dist.all_reduce(red)
            else:
                host = red.cpu()
                dist.all_reduce(host)
                red.copy_(host)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        e.sync()
        info = e.launch_info()
        swaps = None
        if temper:
            # counted on the lower rung of a pair: a point took part in the pairs with its neighbour above and below
            att, acc, rounds = temper.stats()
            att, acc, rounds = att - swaps0[0], acc - swaps0[1], rounds - swaps0[2]
            swaps = torch.zeros(2, len(grid), dtype=torch.float64)
            ids = ps.ladders_by(cases)
            for l in set(ids.tolist()):
                rung = sorted((k for k in range(len(grid)) if ids[k] == l), key=lambda k: (grid[k][1], k))
                for lo, up in zip(rung, rung[1:]):
                    for k in (lo, up):
                        swaps[0, k] += float(att[lo])
                        swaps[1, k] += float(acc[lo])
            if world > 1:
                swaps = _all_reduced(dist, swaps, args.backend)
    if rank == 0:
        host = red.cpu().numpy()
        rows = ["E0,kT,chains,r3,r3_stderr,rsq,p3,p3_stderr,psq,U,U_stderr,AR" +
                (",r3_blocked,p3_blocked,U_blocked,r3_ineff,U_ineff,converged" if eb else "") + (",swap_acceptance" if swaps is not None else "")]
        R3, P3, U = (ps.EB_NAMES.index(q) for q in ("r3", "p3", "U"))
        for k, ((E0, kT), v) in enumerate(zip(grid, host)):
            s = ps.summary_from_reduction(v, args.steps)
            blocked = (eb.stderr[k, R3], eb.stderr[k, P3], eb.stderr[k, U], eb.inefficiency[k, R3], eb.inefficiency[k, U],
                       int(eb.converged[k, [R3, P3, U]].min())) if eb else ()
            if swaps is not None:       # (a point without a partner, or a run shorter than --exchange, attempted none: 0)
                blocked += (float(swaps[1, k] / swaps[0, k]) if swaps[0, k] > 0 else 0.0,)
            rows.append(",".join(f"{x:.12g}" for x in (E0, kT, s.num_chains, s.avg[2], s.stderr[2], s.avg[6], s.avg[9],
                                                        s.stderr[9], s.avg[13], s.avg[14], s.stderr[14], s.acceptance_ratio, *blocked)))
        text = "\n".join(rows) + "\n"
        if args.out:
            open(args.out, "w").write(text)
        else:
            sys.stdout.write(text[:2000] + ("...\n" if len(text) > 2000 else ""))
        upd = world * len(grid) * args.chains * (args.steps + rungs * args.burn_in)
        print(f"# {len(grid)} grid points x {world * args.chains} chains, n={args.n}, {args.main} main, {args.energy}, {args.precision}, "
              f"{world} rank(s) [{args.backend if world > 1 else 'no collective'}]: {wall:.3f} s wall, {upd / wall:.3e} attempted updates/s; "
              f"{info.kernel.decode()}, {info.lanes_per_block} lanes x {info.blocks_per_cu} per CU", file=sys.stderr)
        if swaps is not None:
            print(f"# exchange every {args.exchange} steps: {rounds} rounds in production, {int(swaps[0].sum()) // 2} exchanges attempted, "
                  f"{int(swaps[1].sum()) // 2} accepted", file=sys.stderr)
    e.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
