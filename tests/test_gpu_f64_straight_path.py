"""The step loop of the f64 sweep with its cells in memory keeps its common path straight: the literal log/exp/division
evaluation of an undecided Metropolis draw (metropolis_filter<STRAIGHT>, pstat_math.h) sits behind the loop, entered
through a not-taken scalar branch on "(accept mask | reject mask) != exec".  The verdicts are the same by construction;
this file requires them to be the same in fact -- the oracle's trajectory bit for bit: final angles, generator words,
step sizes and acceptance counts -- at the smallest in-memory size (n = 41) and at the benchmark's (n = 100) with none and
with all 39 rows of its LDS share, under both generators; and, because the filter is one template for both homes, on the LDS
home too (n = 20, and the Ising instantiation once at n = 8), which keeps the plain form of the branch.  The in-memory
main loop runs three steps per iteration and hands the rest to a tail, so every run length modulo 3 is covered (20 000,
20 001, 20 002 steps); adaptation is on with a window of 700 steps (no multiple of 3: the chunks end at every remainder),
and every launch is split into three time segments (spill and refill).

How often the cold path runs: about 1e-5 of all draws are undecided, so the 65 x 20 000 = 1.3e6 draws
of one case enter the literal evaluation about 13 times -- no case expects fewer than 10 -- and the cases of this file
together well over 100 times.  One wrong verdict moves a chain off the oracle's trajectory for good."""
import numpy as np
import pytest

from helpers import both

pytestmark = pytest.mark.gpu

NCHAINS = 65           # one full wave and a one-lane wave
LENGTHS = (20000, 20001, 20002)
SPA = 700              # adaptation window: 700 = 3 * 233 + 1

# (n, PSTAT_F64_LDS_ROWS or None, "state in L2" expected)
SHAPES = {
    "n41": (41, None, True),
    "n100_rows0": (100, 0, True),
    "n100_rows39": (100, 39, True),
    "n20_lds": (20, None, False),
}


@pytest.fixture(scope="module")
def ps():
    import polymer_stats_amd as ps
    assert ps._lib.load().pstat_device_count() >= 1, "no HIP device visible"
    return ps


def run_and_compare(ps, oracle, monkeypatch, nsteps, rows, in_memory, check_collapse=False, **kw):
    monkeypatch.delenv("PSTAT_F64_STATE", raising=False)
    if rows is None:
        monkeypatch.delenv("PSTAT_F64_LDS_ROWS", raising=False)
    else:
        monkeypatch.setenv("PSTAT_F64_LDS_ROWS", str(rows))  # read once, at create
    monkeypatch.setenv("PSTAT_SEGMENTS", "3")
    monkeypatch.setenv("PSTAT_MAX_SPINS", str(1 << 22))      # a stuck job queue fails instead of hanging
    assert NCHAINS * nsteps * 1e-5 >= 10                     # expected entries into the cold path, this case
    op, pp = both(nsteps, num_chains=NCHAINS, precision=ps.F64, steps_per_adjust=SPA, **kw)
    with ps.Ensemble(pp) as e:
        info = e.launch_info()
        assert "sweep_kernel<double" in info.kernel.decode(), info.kernel
        assert ("state in L2" in info.kernel.decode()) == in_memory, info.kernel
        if rows is not None:
            assert info.lds_bytes == (rows + 1) * 64 * 16, (info.lds_bytes, rows)
        e.advance(nsteps)
        e.sync()
        for c in range(NCHAINS):
            o = oracle.run(op, chain_id=c, mode="fast", trace=True)
            g = e.chain_state(c)
            ctx = (kw.get("n"), rows, nsteps, c)
            if check_collapse:
                assert abs(o.U) < 1e3 * kw["n"] * kw["kT"], "collapsed: not a trajectory-parity case"
            assert np.array_equal(g["theta"], o.final_theta), ctx
            assert np.array_equal(g["phi"], o.final_phi), ctx
            assert np.array_equal(g["rng"], o.rng), ctx
            assert g["phi_step"] == o.phi_step and g["theta_step"] == o.theta_step, ctx
            assert g["nacc_total"] == o.nacc_total, ctx
        assert e.summary().nan_rejects == 0


@pytest.mark.parametrize("nsteps", LENGTHS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_f64_straight_path_bit_parity(ps, oracle, monkeypatch, shape, nsteps):
    n, rows, in_memory = SHAPES[shape]
    # the generator alternates over the grid, so every shape and every remainder sees both
    rng = ps.RNG_XOSHIRO128PP if (sorted(SHAPES).index(shape) + nsteps) % 2 else ps.RNG_MWC64X
    run_and_compare(ps, oracle, monkeypatch, nsteps, rows, in_memory, n=n, E0=1.0, K1=1.0, K2=0.0, Fz=1.0, kT=1.0,
                    seed=20261019 + n, rng=rng)


@pytest.mark.parametrize("rng_name", ["RNG_MWC64X", "RNG_XOSHIRO128PP"])
def test_f64_straight_path_both_generators_at_the_benchmark_shape(ps, oracle, monkeypatch, rng_name):
    """n = 100 with the default LDS share, the kernel bench.py measures, under each generator (20 001 steps: tail of one)."""
    run_and_compare(ps, oracle, monkeypatch, 20001, None, True, n=100, E0=1.0, K1=1.0, K2=0.0, Fz=1.0, kT=1.0,
                    seed=20261020, rng=getattr(ps, rng_name))


def test_f64_straight_path_ising_n8(ps, oracle, monkeypatch):
    """The Ising instantiation shares the filter template; warm enough that no chain collapses onto the 1/r^3 singularity."""
    run_and_compare(ps, oracle, monkeypatch, 20002, None, False, check_collapse=True, n=8, E0=0.2, K1=1.0, K2=0.0, b=1.0,
                    kT=10.0 ** 0.6, seed=20261021, energy_type=ps.ISING)
