"""The f64 sweep with its cells in memory fetches the row of step s + 2 BEHIND the stores of step s (run_segment, ST = 2,
PSTAT_GM_LATE) and forwards one commit, that of step s + 1, into it at its first use.  What breaks if the order is
wrong: a step sees a stale cell when it hits the monomer of the step before it (the forwarded commit, fw1), or the monomer of
the step two before it (no forwarding any more: the hardware's store -> load order of one wave alone).  The shortest chains make
both collisions frequent -- at n = 1 every step collides, at n = 2 half of the step-two-before pairs do, at n = 3 with one row
in LDS one home is LDS and two are memory -- so they run here with 0 and with 1 row in LDS, with and without step-size
adaptation, in one launch and split 1 + 2 + 2 997 (prologue and tail loop of the pipeline), against the CPU oracle's trajectory.

Tolerances, as tests/test_gpu_parity.py states them for the f64 kernel: angles, generator, acceptance counts and step sizes bit
for bit; running sums to 1e-9 relative (1e-7 absolute)."""
import numpy as np
import pytest

from helpers import both

pytestmark = pytest.mark.gpu

NSTEPS, NCHAINS = 3000, 128
PHYS = dict(E0=1.0, K1=1.0, K2=0.0, Fz=1.0, kT=1.0)      # the bench instantiation: dielectric, non-interacting, no Fx, no flips
ADAPT = {"adapt": dict(steps_per_adjust=500, adj_scale=1.1), "fixed-steps": dict(adj_scale=1.0)}


@pytest.fixture(scope="module")
def ps():
    import polymer_stats_amd as ps
    assert ps._lib.load().pstat_device_count() >= 1, "no HIP device visible"
    return ps


_reference = {}


def reference(oracle, ps, nsteps, nchains, **kw):
    """The oracle's trajectories of one configuration, computed once and shared by the cases that differ only in where the
    device keeps its rows and how it splits the run."""
    key = (nsteps, nchains, tuple(sorted(kw.items())))
    if key not in _reference:
        op, _ = both(nsteps, num_chains=nchains, precision=ps.F64, **kw)
        _reference[key] = [oracle.run(op, chain_id=c, mode="fast", trace=True) for c in range(nchains)]
    return _reference[key]


def check(e, ref, nchains):
    for c in range(nchains):
        o, g = ref[c], e.chain_state(c)
        assert np.array_equal(g["theta"], o.final_theta), f"theta differs, chain {c}"
        assert np.array_equal(g["phi"], o.final_phi), f"phi differs, chain {c}"
        assert np.array_equal(g["rng"], o.rng), f"rng differs, chain {c}"
        assert g["nacc_total"] == o.nacc_total, f"acceptance count differs, chain {c}"
        assert g["phi_step"] == o.phi_step and g["theta_step"] == o.theta_step, f"step sizes differ, chain {c}"
        np.testing.assert_allclose(g["sums"], o.sums, rtol=1e-9, atol=1e-7)
    assert e.summary().nan_rejects == 0


@pytest.mark.parametrize("split", [(NSTEPS,), (1, 2, NSTEPS - 3)], ids=["one-launch", "split-1-2-rest"])
@pytest.mark.parametrize("adapt", sorted(ADAPT))
@pytest.mark.parametrize("rows", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_short_chains_in_memory_match_the_oracle(ps, oracle, monkeypatch, n, rows, adapt, split):
    kw = dict(n=n, seed=20260701 + n, **PHYS, **ADAPT[adapt])
    ref = reference(oracle, ps, NSTEPS, NCHAINS, **kw)
    monkeypatch.setenv("PSTAT_F64_STATE", "global")
    monkeypatch.setenv("PSTAT_F64_LDS_ROWS", str(rows))
    _, pp = both(NSTEPS, num_chains=NCHAINS, precision=ps.F64, **kw)
    with ps.Ensemble(pp) as e:
        assert "state in L2" in e.launch_info().kernel.decode()
        for part in split:
            e.advance(part)
        e.sync()
        check(e, ref, NCHAINS)


def test_headline_shape_matches_the_oracle(ps, oracle, monkeypatch):
    """n = 100 with 39 rows in LDS, the shape bench.py times: one full wave, adaptation at its default."""
    kw = dict(n=100, seed=20260702, **PHYS)
    ref = reference(oracle, ps, 2000, 64, **kw)
    monkeypatch.delenv("PSTAT_F64_STATE", raising=False)
    monkeypatch.setenv("PSTAT_F64_LDS_ROWS", "39")
    _, pp = both(2000, num_chains=64, precision=ps.F64, **kw)
    with ps.Ensemble(pp) as e:
        assert "state in L2" in e.launch_info().kernel.decode()
        e.advance(2000)
        e.sync()
        check(e, ref, 64)
