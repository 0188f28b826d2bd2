"""The f64 sweep with its cells in memory steers every access by address arithmetic on the cell's byte offset
(run_segment, ST = 2): LDS address min(cell, trash row), buffer offset cell - (bytes of the LDS rows) into a resource
that spans the memory rows only.  The edges of that arithmetic are the split between the two homes, so this file runs
the kernel at every split the knob PSTAT_F64_LDS_ROWS can reach at its ends -- 0 rows in LDS (no LDS part: the trash
row is row 0, the resource spans all rows), 1 row, and the default 39 -- for n = 41 (39 rows leave a resource of two
rows) and n = 100 (the benchmark's chain length), and requires the oracle's trajectory bit for bit: angles, generator
words, step sizes and acceptance counts, after a launch that is split into time segments and into two advances."""
import numpy as np
import pytest

from helpers import both

pytestmark = pytest.mark.gpu

NSTEPS = 4000          # adaptation windows of 2500 steps: one adjustment inside the run
NCHAINS = 70           # one full wave and one 6-lane wave


@pytest.fixture(scope="module")
def ps():
    import polymer_stats_amd as ps
    assert ps._lib.load().pstat_device_count() >= 1, "no HIP device visible"
    return ps


def case_params(ps, n):
    return both(NSTEPS, num_chains=NCHAINS, precision=ps.F64, n=n, E0=1.0, K1=1.0, K2=0.0, Fz=1.0, kT=1.0,
                seed=20261016 + n)


@pytest.mark.parametrize("n", [41, 100])
@pytest.mark.parametrize("rows", [0, 1, 39])
def test_f64_in_memory_bit_parity_at_every_lds_split(ps, oracle, monkeypatch, rows, n):
    monkeypatch.delenv("PSTAT_F64_STATE", raising=False)
    monkeypatch.setenv("PSTAT_F64_LDS_ROWS", str(rows))      # read once, at create
    monkeypatch.setenv("PSTAT_SEGMENTS", "3")
    monkeypatch.setenv("PSTAT_MAX_SPINS", str(1 << 19))      # a stuck job queue fails within ~1 s instead of hanging
    op, pp = case_params(ps, n)
    with ps.Ensemble(pp) as e:
        info = e.launch_info()
        assert "state in L2" in info.kernel.decode()
        assert info.lds_bytes == (rows + 1) * 64 * 16, (info.lds_bytes, rows)   # the knob took: `rows` rows + the trash row
        e.advance(1500); e.advance(NSTEPS - 1500)            # 2 launches x 3 segments: five spills and refills
        e.sync()
        for c in range(NCHAINS):
            o = oracle.run(op, chain_id=c, mode="fast", trace=True)
            g = e.chain_state(c)
            ctx = (rows, n, c)
            assert np.array_equal(g["theta"], o.final_theta), ctx
            assert np.array_equal(g["phi"], o.final_phi), ctx
            assert np.array_equal(g["rng"], o.rng), ctx
            assert g["phi_step"] == o.phi_step and g["theta_step"] == o.theta_step, ctx
            assert g["nacc_total"] == o.nacc_total, ctx
        assert e.summary().nan_rejects == 0
