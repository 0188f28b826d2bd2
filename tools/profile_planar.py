"""The workload of the planar main's profiles (profiles/planar/): Ising dielectric, n = 25, 65 536 chains, the coupling of
2D/run/Ising_2024-11-06.jl.  Run under rocprofv3 (one --kernel-trace --stats run; one --pmc run of its own):
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o t -- python3 tools/profile_planar.py [steps=5000] [n=25] [chains=65536]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import polymer_stats_amd as ps

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 5000
n = int(sys.argv[2]) if len(sys.argv) > 2 else 25
chains = int(sys.argv[3]) if len(sys.argv) > 3 else 65536
p = ps.default_planar_params(n=n, E0=0.1, K1=0.04, K2=0.0, kT=1.0, Fz=1.0, energy_type=ps.ISING, num_chains=chains, seed=6)
with ps.Ensemble(p, planar=True) as e:
    e.advance(steps)
    e.sync()
    info, s = e.launch_info(), e.summary()
    print("%s: n=%d chains=%d steps=%d, %d lanes x %d per CU, LDS %d B; AR %.4f r3 %.5f nan_rejects %d" %
          (info.kernel.decode(), n, chains, steps, info.lanes_per_block, info.blocks_per_cu, info.lds_bytes, s.acceptance_ratio,
           s.avg[2], s.nan_rejects), flush=True)
