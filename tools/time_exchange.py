"""One replica-exchange round against the steps between two rounds, on a phase-scan ensemble:
    python tools/time_exchange.py [main=fixed-force|clustering] [per_case=16] [n=100] [every=50] [rounds=200]
    rocprofv3 --kernel-trace --stats -d out -- python3 tools/time_exchange.py ...      # the kernels' own times, in a run of its own
The (E0, kT) grid of run/K1_E0-kT-phase.jl (26 x 21 points x 5 runs, Ising, K1 = 1), `per_case` chains per case; every column of
equal E0 of every run is a ladder of 21 rungs.  Prints the wall time of `rounds` x advance(every) with and without the exchange
round after each, and the swap acceptance."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import polymer_stats_amd as ps

main = sys.argv[1] if len(sys.argv) > 1 else "fixed-force"
per = int(sys.argv[2]) if len(sys.argv) > 2 else 16
n = int(sys.argv[3]) if len(sys.argv) > 3 else 100
every = int(sys.argv[4]) if len(sys.argv) > 4 else 50
rounds = int(sys.argv[5]) if len(sys.argv) > 5 else 200
extra = dict(move_set=ps.MOVES_CLUSTER, cluster_prob=0.5) if main == "clustering" else {}
cases, ladder = [], []
for rep in range(5):
    for i in range(26):
        for j in range(21):
            cases.append(ps.default_params(n=n, E0=0.2 * i, K1=1.0, K2=0.0, kT=10 ** (-2 + 0.2 * j), num_chains=per, precision=ps.F64,
                                           seed=1000 + len(cases), energy_type=ps.ISING, **extra))
            ladder.append(26 * rep + i)
with ps.Ensemble(cases) as e:
    t = e.open_tempering(ladder, seed=1)
    e.advance_tempered(t, 4 * every, every)     # warm-up of both paths
    e.sync()
    wall = {}
    for what in ("plain", "tempered", "plain", "tempered"):
        t0 = time.perf_counter()
        if what == "plain":
            for _ in range(rounds):
                e.advance(every)
        else:
            e.advance_tempered(t, rounds * every, every)
        e.sync()
        wall.setdefault(what, []).append(time.perf_counter() - t0)
    att, acc, r = t.stats()
    info = e.launch_info()
print(f"{len(cases)} cases x {per} chains, n = {n}, {main} main, Ising; {info.kernel.decode()}; {rounds} x advance({every})")
for what, ts in wall.items():
    print(f"  {what:9s} " + " / ".join(f"{x * 1e3:8.2f} ms" for x in ts) + f"   = {min(ts) / rounds * 1e6:8.2f} us per advance({every})"
          + (" + exchange round" if what == "tempered" else ""))
print(f"  one exchange round costs {(min(wall['tempered']) - min(wall['plain'])) / rounds * 1e6:.2f} us of wall time; "
      f"{r} rounds, swap acceptance over all pairs {acc.sum() / max(att.sum(), 1):.3f} "
      f"(per ladder position, coldest pair first: {np.round((acc.reshape(-1, 21).sum(0) / np.maximum(att.reshape(-1, 21).sum(0), 1))[:-1], 2).tolist()})")
