#!/usr/bin/env python3
"""A(r) from a force sweep: the `.hist` files that tools/run_sweep.py --hist left in a directory, stitched by WHAM
(polymer_stats_amd/free_energy.py).  No GPU.

    python tools/run_sweep.py out/ --axis n=8 --axis Fz=0:0.5:3 --num-chains 64 --hist r3:-8:8:64 -- --num-steps 100000 --stepout 100
    python tools/free_energy.py out/ --component r3

The files are grouped by everything in their name but the force along the component (Fz for r3, Fx for r1) and `run`; a group's
cases must differ in nothing else.  Per group one `<group>_A_<component>.csv` with the columns x,A,sigma,samples: bin centre,
the free energy along the component at zero force (min = 0) -- the fixed-extension Helmholtz free energy up to its constant --,
its counting error kT / sqrt(samples), and the samples all cases put in the bin; bins nobody visited are left out.  kT is the
group's kT token (milli or raw, as run_sweep.py names files), or --kT.
"""
import argparse
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORCE_OF = {"r3": "Fz", "r1": "Fx"}


def token_value(text: str) -> float:
    """A file-name token's value: `%07d` of 1000 x (run_sweep.py's default kind), or the number as written (kind raw)."""
    return int(text) / 1e3 if re.fullmatch(r"-?\d{7}|-\d{6}", text) else float(text)


def read_hist(path: str) -> list[dict]:
    """The histograms of one .hist file: dicts of channel, lo, hi, nbins, records, chains, edges, counts, tails."""
    import numpy as np
    out = []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line.startswith("#"):
                kv = dict(t.split("=", 1) for t in line[1:].split())
                out.append(dict(channel=kv["channel"], lo=float(kv["lo"]), hi=float(kv["hi"]), nbins=int(kv["nbins"]),
                                records=int(kv["records"]), chains=int(kv["chains"]), rows=[], tails={}))
            elif line:
                a = line.split(",")
                if len(a) == 3:
                    out[-1]["rows"].append((float(a[0]), float(a[1]), int(a[2])))
                else:
                    out[-1]["tails"][a[0]] = int(a[1])
    for h in out:
        rows = h.pop("rows")
        if len(rows) != h["nbins"] or set(h["tails"]) != {"below", "above", "not_finite"}:
            raise ValueError(f"{path}: histogram of {h['channel']} is incomplete")
        h["edges"] = np.array([r[0] for r in rows] + [rows[-1][1]])
        h["counts"] = np.array([r[2] for r in rows], dtype=np.int64)
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--component", choices=sorted(FORCE_OF), default="r3")
    ap.add_argument("--kT", type=float, default=None, help="default: the kT token of the file names, or 1")
    ap.add_argument("--out", default=None, help="directory of the CSVs (default: DIR)")
    ap.add_argument("--tol", type=float, default=1e-10)
    args = ap.parse_args(argv)

    import numpy as np
    from polymer_stats_amd.free_energy import wham_force

    force_key = FORCE_OF[args.component]
    groups: dict = {}
    for path in sorted(glob.glob(os.path.join(args.dir, "*.hist"))):
        toks = [t.split("-", 1) for t in os.path.basename(path)[:-len(".hist")].split("_")]
        if any(len(t) != 2 for t in toks) or force_key not in [t[0] for t in toks]:
            raise SystemExit(f"{path}: the name has no {force_key}-<value> token to read the force from")
        named = dict(toks)
        key = "_".join(f"{k}-{v}" for k, v in toks if k not in (force_key, "run"))
        hs = [h for h in read_hist(path) if h["channel"] == args.component]
        if not hs:
            raise SystemExit(f"{path}: holds no histogram of {args.component}")
        kT = args.kT if args.kT is not None else (token_value(named["kT"]) if "kT" in named else 1.0)
        groups.setdefault(key, []).append((token_value(named[force_key]), kT, hs[0], path))
    if not groups:
        raise SystemExit(f"no .hist files in {args.dir}")
    outdir = args.out or args.dir
    os.makedirs(outdir, exist_ok=True)
    for key, members in groups.items():
        first = members[0][2]
        for _, kT, h, path in members:
            if (h["lo"], h["hi"], h["nbins"]) != (first["lo"], first["hi"], first["nbins"]) or kT != members[0][1]:
                raise SystemExit(f"{path}: its bins or kT differ from {members[0][3]}'s")
        counts = np.array([m[2]["counts"] for m in members])
        A, sigma, f, iterations, converged = wham_force(counts, first["edges"], members[0][1], [m[0] for m in members], tol=args.tol)
        x = 0.5 * (first["edges"][:-1] + first["edges"][1:])
        col = counts.sum(axis=0)
        dest = os.path.join(outdir, f"{key}_A_{args.component}.csv")
        with open(dest, "w") as fh:
            fh.write("x,A,sigma,samples\n")
            for j in np.flatnonzero(col > 0):
                fh.write(f"{float(x[j])!r},{float(A[j])!r},{float(sigma[j])!r},{int(col[j])}\n")
        lost = sum(sum(m[2]["tails"].values()) for m in members)
        print(f"# {dest}: {len(members)} cases, forces {sorted({m[0] for m in members})}, {int(col.sum())} samples "
              f"({lost} outside the bins), WHAM {'converged' if converged else 'NOT converged'} in {iterations} iterations",
              file=sys.stderr)
        if not converged:
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
