#!/usr/bin/env python3
"""A whole parameter sweep of the reference's run/*.jl kind in batched launches: the cases that `pmap` hands to worker
processes one `julia mcmc_*.jl` at a time (run/interacting_dielectric_study.jl:37-47) become the cases of one ensemble
per chain length, dealt round-robin to the ranks; every case gets its `<name>.out` exactly as the run script would have
written it (polymer_stats_amd/sweep.py), ready for scripts/aggregate_mcmc.jl (or `--aggregate`, its twin).

    # run/interacting_dielectric_study.jl
    python tools/run_sweep.py out/ --main mcmc_eap_chain --axis b=0.5,1,2 --axis n=100,200 --axis Fx=0,0.5,1,2 \
        --axis Fz=0,0.5,1,2 --axis kT=1 --axis E0=0.1,1,10 --axis K1=0,0.1,0.5,1,2 --axis K2=0,0.1,0.5,1,2 --skip 'K1==K2' \
        --num-chains 16 -- --chain-type dielectric --energy-type interacting --num-steps 500000 -v 2
    # run/K1_E0-kT-phase.jl: 546 grid points x 5 runs of the clustering main, on 8 GPUs
    python tools/run_sweep.py out/ --gpus 8 --main mcmc_clustering_eap_chain --axis b=1 --axis n=100 --axis Fx=0 --axis Fz=0 \
        --axis kT='10^(-2:0.2:2)' --axis E0=0:0.2:5 --axis K1=1 --axis K2=0 --axis kappa=0 --axis run=1:5 \
        --name E0,K1,K2,kT,Fz,Fx,n,b,kappa,run:raw \
        -- --chain-type dielectric --energy-type Ising --num-steps 2500000 --burn-in 100000 -v 2 --stepout 250

    # 2D/run/Ising_2024-11-06.jl: the planar main, 4 x 22 grid points x 10 runs = 880 single-chain cases of 1e7 steps
    python tools/run_sweep.py out/ --main mcmc_clustering_eap_chain_2d --num-chains 1 --axis b=1 --axis n=25 --axis Fx=0 \
        --axis Fz=0,0.1,0.2,0.3,0.4,0.5,1,2,3,4,5,7.5,10,12.5,15,20,25,30,35,40,45,50 --axis kT=1 --axis E0=0.1 \
        --axis K1=0.01,0.04,0.1,0.4 --axis K2=0 --axis run=1:10 --name E0,K1,K2,kT,Fz,Fx,n,b,run:raw \
        -- --chain-type dielectric --energy-type Ising --num-steps 10000000 --burn-in 200000 -v 2

The first --axis is the outermost loop (`for b in bs, n in ns, ...`).  Everything after `--` goes to the main unchanged.
A case whose .out exists is not run again (the run scripts' `isfile(outfile)`); --overwrite runs it anyway.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    argv = sys.argv[1:]
    fixed = []
    if "--" in argv:
        k = argv.index("--")
        argv, fixed = argv[:k], argv[k + 1:]
    ap = argparse.ArgumentParser()
    ap.add_argument("workdir")
    ap.add_argument("--main", choices=["mcmc_eap_chain", "mcmc_clustering_eap_chain", "mcmc_clustering_eap_chain_2d"],
                    default="mcmc_eap_chain")
    ap.add_argument("--axis", action="append", default=[], metavar="KEY=VALUES",
                    help="values: a,b,c | start:step:stop (also several, comma-separated) | 10^(start:step:stop); first axis = outermost loop")
    ap.add_argument("--cases", default="", help="JSON array of case objects instead of (or appended to) the axes' product")
    ap.add_argument("--skip", default="", help="leave out the cases for which this holds, e.g. 'K1==K2'")
    ap.add_argument("--name", default="", help="file-name tokens, e.g. E0,K1,K2,kT,Fz,Fx,n,b,run:int (kinds: milli [default] | int | raw)")
    ap.add_argument("--num-chains", type=int, default=64, help="independent chains per case, pooled (1 = literally one reference run)")
    ap.add_argument("--seed", type=int, default=None, help="base seed; case k of the full list runs on seed + k (default: fresh entropy)")
    ap.add_argument("--precision", choices=["f64", "f32", "q16"], default=None)
    ap.add_argument("--rng", choices=["mwc64x", "xoshiro128++"], default=None)
    ap.add_argument("--gpus", type=int, default=1, help="ranks; > 1 from a bare shell starts them (one per GPU)")
    ap.add_argument("--share-gpu", action="store_true", help="rehearsal: ranks beyond the visible GPUs share them")
    ap.add_argument("--overwrite", action="store_true")
    ap.add_argument("--csv", action="store_true", help="also write every case's _trajectory.csv and _rolling.csv, one row per --stepout steps: the rows of all cases are "
                         "recorded on the device by one launch each and read back in chunks (formatting their text is then the larger part of a big run)")
    ap.add_argument("--error-bars", type=int, default=0, metavar="N",
                    help="record the production run as N batches (of num-steps / N steps) on the device and write, next to every <case>.out, "
                         "a <case>.err: the same names with the blocked standard errors (Flyvbjerg-Petersen) as values, then batches, "
                         "inefficiency and converged over the 19 quantities.  One device, --num-inits 1, float64, no --csv, no umbrella sampling.  "
                         "ROUGHLY DOUBLES the production time: the stage is run recorded for the .err and then again, from a checkpoint, as "
                         "the one launch of a plain run, so that the .out is byte for byte the plain run's (the two runs' means agree to "
                         "~1e-15; a remainder num-steps %% N belongs to no batch).  A case whose .out is there but whose .err is not is run again")
    ap.add_argument("--hist", action="append", default=[], metavar="CHANNEL:LO:HI:NBINS",
                    help="repeatable: histogram CHANNEL (r1 r2 r3 p1 p2 p3 U rmag pmag) of EVERY chain every --stepout steps of the "
                         "production run, on the device, and write next to every <case>.out a <case>.hist: per histogram a header line "
                         "(channel, lo, hi, nbins, records, chains), bin_lo,bin_hi,count rows and the three tails; tools/free_energy.py "
                         "turns a force sweep's into A(r).  Refused where --error-bars is, and with it; the .out files stay byte for "
                         "byte a plain run's, at the same doubled production time")
    ap.add_argument("--corr", default="", metavar="MAXLAG[:nn,zz,mm]",
                    help="record the lag correlations of EVERY chain's orientations (nn: tangent, zz: along the field) and dipoles (mm) "
                         "for lags 0 .. MAXLAG every --stepout steps of the production run, on the device, and write next to every "
                         "<case>.out a <case>.corr: CSV k,<ch>,<ch>_stderr,... with the blocked standard errors of the records (at least "
                         "32 records).  Default channel: nn.  Refused where --hist is, with it and with --error-bars; the .out files stay "
                         "byte for byte a plain run's, at the same doubled production time")
    ap.add_argument("--shape", nargs="?", const="", default=None, metavar="AXIS:QMAX:NQ[,AXIS:QMAX:NQ...]",
                    help="record the gyration tensor of EVERY chain (gxx gyy gzz gxy gxz gyz rg2 trg2) and its form factor S(q) at NQ "
                         "wave-vectors QMAX (1 .. NQ) / NQ along AXIS (x, y or z) per entry, every --stepout steps of the production "
                         "run, on the device, and write next to every <case>.out a <case>.shape: CSV name,qx,qy,qz,value,stderr with "
                         "the blocked standard errors of the records (at least 32 records).  A bare --shape records the gyration "
                         "block only.  Refused where --corr is, and with it; the .out files stay byte for byte a plain run's, at the "
                         "same doubled production time")
    ap.add_argument("--pdist", default="", metavar="RMAX:NBINS[,sep=MAXSEP][,min=MINSEP][,q=QMAX:NQ]",
                    help="record the distances between two monomers of EVERY chain every --stepout steps of the production run, on "
                         "the device: the mean-square internal distance R2(s) for s = 1 .. MAXSEP (default n - 1), the closest "
                         "approach and the distribution P(r) below RMAX in NBINS bins over the pairs at least MINSEP apart along the "
                         "chain (default 1; NBINS 0: no histogram), and the Debye S(q) at NQ magnitudes QMAX (1 .. NQ) / NQ; write "
                         "next to every <case>.out a <case>.pdist: CSV name,x,value,stderr with the blocked standard errors of the "
                         "records (at least 32 records).  Refused where --shape is, and with it; the .out files stay byte for byte "
                         "a plain run's, at the same doubled production time")
    ap.add_argument("--energy", default="", metavar="MAXSEP[,cut=RCUT]",
                    help="record what EVERY chain's energy is made of every --stepout steps of the production run, on the device: "
                         "the field term, the work of the force, the bending term, the dipole-dipole sum by separation s = 1 .. "
                         "MAXSEP along the chain (-1: n - 1) whatever --energy-type is, the separations beyond MAXSEP in one column "
                         "and, with cut=RCUT (monomer lengths; default under --energy-type cutoff: --cutoff-radius), the sum inside "
                         "that radius; write next to every <case>.out a <case>.energy: CSV name,x,value,stderr with the blocked "
                         "standard errors of the records (at least 32 records), the last row `model` the energy the step itself "
                         "carries.  Refused where --pdist is, and with it; the .out files stay byte for byte a plain run's, at the "
                         "same doubled production time")
    ap.add_argument("--max-chains", type=int, default=262144, help="chains per launch (cases per ensemble = this / num-chains)")
    ap.add_argument("--dry-run", action="store_true", help="print the plan (cases, file names, ensembles) and stop: no GPU needed")
    ap.add_argument("--aggregate", default="", help="afterwards write scripts/aggregate_mcmc.jl's CSV of the whole directory here")
    ap.add_argument("--aggregate-args", default="*.out,dielectric", help="pattern,dielectric|polar[,kappaflag[,runflag]]")
    args = ap.parse_args(argv)

    from polymer_stats_amd import sweep as sw          # (no GPU call on import)
    axes = []
    for a in args.axis:
        key, _, vals = a.partition("=")
        axes.append((key.strip(), sw.axis_values(vals)))
    cases = sw.product_cases(axes) if axes else []
    if args.cases:
        cases += sw.load_cases(args.cases)
    if args.skip:
        cases = [c for c in cases if not sw.skip_case(args.skip, c)]
    if not cases:
        raise SystemExit("no cases: give --axis and/or --cases")

    recording = dict(error_bars=args.error_bars, hist=args.hist, corr=args.corr, shape=args.shape, pdist=args.pdist, energy=args.energy)
    try:
        sw.recording(args.main, fixed, cases, write_csv=args.csv, world=args.gpus, **recording)
    except sw.ReferenceError_ as e:
        raise SystemExit(str(e))
    if args.dry_run:
        pl = sw.plan(args.main, fixed, cases, args.workdir, name=args.name or None, num_chains=args.num_chains,
                     seed=0 if args.seed is None else args.seed, precision=args.precision, rng=args.rng)
        groups = {}
        for p in pl:
            groups.setdefault(sw._signature(p), []).append(p)
        done = sum(os.path.isfile(p["_out"]) for p in pl)
        print(f"{len(pl)} cases ({done} already there), {len(groups)} ensemble(s) per rank at most, {args.num_chains} chain(s) per case, "
              f"{args.gpus} rank(s); main {args.main}; seed {'fresh entropy' if args.seed is None else args.seed} + position")
        for g in groups.values():
            p0 = g[0]
            print(f"  n = {p0['num-monomers']}, {p0['energy-type']}, {p0['chain-type']}, {p0['num-steps']} steps: {len(g)} cases, "
                  f"{len(g) * args.num_chains} chains")
        for p in pl[:3] + (pl[-1:] if len(pl) > 3 else []):
            print("  " + os.path.basename(p["_out"]))
        return
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # the ranks are started before anything touches the GPU; this process never does.  A fresh default seed has to be
        # drawn HERE: every rank must name the same seed for case k
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from rank_spawn import spawn_ranks
        extra = [] if args.seed is not None else ["--seed", str(sw.fresh_seed() & 0x7FFFFFFFFFFF)]
        pre = sys.argv[1:sys.argv.index("--")] if "--" in sys.argv else sys.argv[1:]
        agg = bool(args.aggregate)              # the ranks only run; the parent aggregates when all of them are done
        kept, skip = [], False
        for a in pre:                           # drop `--aggregate X` and `--aggregate=X` from what the ranks are given
            if skip:
                skip = False
            elif a == "--aggregate":
                skip = True
            elif not a.startswith("--aggregate="):
                kept.append(a)
        pre = kept
        rc, out0 = spawn_ranks(os.path.abspath(__file__), pre + extra + (["--"] + fixed if fixed else []), args.gpus)
        sys.stdout.write(out0)
        if rc == 0 and agg:
            rc = aggregate(args)
        sys.exit(rc)

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if world > 1 and args.seed is None:
        # started by an external launcher: every rank would draw its own fresh base seed, and case k's seed = base + k must
        # be the same whichever rank runs it
        raise SystemExit("run_sweep.py under an external launcher (WORLD_SIZE preset) needs --seed: all ranks must name the same one")
    lib = sw._lib.load()
    ndev = lib.pstat_device_count()
    if ndev < 1:
        raise SystemExit("run_sweep.py needs a GPU: libpstat has no CPU path")
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if local >= ndev and not args.share_gpu:
        raise SystemExit(f"rank {rank}: LOCAL_RANK {local} but only {ndev} GPU(s) visible (--share-gpu to rehearse)")
    t0 = time.time()
    res = sw.run_sweep(args.main, fixed, cases, args.workdir, name=args.name or None, num_chains=args.num_chains, seed=args.seed,
                       precision=args.precision, rng=args.rng, rank=rank, world=world, device=local % ndev,
                       overwrite=args.overwrite, write_csv=args.csv, max_chains=args.max_chains, **recording,
                       log=lambda m: print("# " + m, file=sys.stderr, flush=True))
    print(f"# rank {rank} of {world}: {len(res['ran'])} cases run in {res['launches']} ensembles, {len(res['skipped'])} already "
          f"there; {time.time() - t0:.2f} s", file=sys.stderr, flush=True)
    if world == 1 and args.aggregate:
        sys.exit(aggregate(args))


def aggregate(args) -> int:
    from polymer_stats_amd import aggregate_mcmc as ag
    parts = args.aggregate_args.split(",")
    flag = lambda i: len(parts) > i and parts[i].strip() == "true"
    return ag.aggregate(args.aggregate, args.workdir, parts[0], parts[1] if len(parts) > 1 else "dielectric", flag(2), flag(3))


if __name__ == "__main__":
    main()
