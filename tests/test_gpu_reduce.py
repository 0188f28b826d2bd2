"""The ensemble reduction, restated on the host from the public read-outs and held to `==`.

A. pstat_chain_means: every chain's mean vector v[0..18] recomputed from pstat_chain_state (sums, normalizer, nacc_total,
   steps_recorded) and pstat_chain_extras (sums): inv = 1 / norm (0 when norm is 0), v[q] = sums[q] * inv for the 16
   observables, v[16] = nacc / steps (0 when no step was taken), v[17], v[18] = the two extra sums * inv.
B. pstat_reduce_host: red[1..38] folded from that [19, chains] array in the device's order.  Thread t of block b takes
   chains 256 b + t + 65536 j (counted from the first chain reduced) in order of j, m1 += v and m2 = fma(v, v, m2); within
   each wave of 64 the tree x[i] += x[i + off], off = 32 ... 1; a block's waves 0..3 are added in order from 0.0; stage-2
   lane i adds the partials of blocks i, i + 64, i + 128, i + 192 in that order from 0.0, and the same tree follows.
   m1 is float64 additions; the fma is computed exactly in rationals and rounded once.  Slots that hold no chain carry
   +0.0, and adding +0.0 changes no sum here (no accumulator is ever -0.0: each starts from +0.0).
The energies are non-interacting, so nothing is rejected as non-finite and nothing collapses: red[39] == red[40] == 0."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NQ, BLOCKS, THREADS = 19, 256, 256
SLOTS = BLOCKS * THREADS


@pytest.fixture(scope="module")
def ps():
    import polymer_stats_amd as ps
    ps._lib.load()
    return ps


def P(ps, **kw):
    base = dict(n=6, E0=1.0, Fz=0.5, Fx=0.2, precision=ps.F64, steps_per_adjust=150, seed=11)
    base.update(kw)
    return ps.default_params(**base)


def host_means(e, chains):
    """v[NQ, len(chains)] from pstat_chain_state and pstat_chain_extras (no angles, no generator words: fewer copies)."""
    dp, L = C.POINTER(C.c_double), e._L
    v = np.zeros((NQ, len(chains)))
    sums, cnt, steps, extra = np.zeros(16), np.zeros(4, dtype=np.int64), np.zeros(3), np.zeros(2)
    for k, c in enumerate(chains):
        assert L.pstat_chain_state(e._h, c, None, sums.ctypes.data_as(dp), cnt.ctypes.data_as(C.POINTER(C.c_int64)),
                                   steps.ctypes.data_as(dp), None) == 0
        assert L.pstat_chain_extras(e._h, c, extra.ctypes.data_as(dp), None) == 0
        norm, nacc, nsteps = float(steps[2]), int(cnt[0]), int(cnt[1])
        inv = 1.0 / norm if norm != 0.0 else 0.0
        v[:16, k] = sums * inv
        v[16, k] = nacc / nsteps if nsteps > 0 else 0.0
        v[17:, k] = extra * inv
    return v


def tree(x):
    """lane 0 of the shfl_down tree over the last axis (64 lanes)"""
    for off in (32, 16, 8, 4, 2, 1):
        x = x[..., :off] + x[..., off:2 * off]
    return x[..., 0]


def stages(acc):
    """acc[NQ, SLOTS], the threads' accumulators (slot = 256 block + thread) -> the NQ outputs"""
    waves = tree(acc.reshape(-1, BLOCKS, THREADS // 64, 64))
    partial = np.zeros(waves.shape[:2])
    for w in range(THREADS // 64):
        partial = partial + waves[:, :, w]
    strided = partial.reshape(-1, BLOCKS // 64, 64)          # [q, r, i] = block i + 64 r
    lanes = np.zeros((strided.shape[0], 64))
    for r in range(BLOCKS // 64):
        lanes = lanes + strided[:, r]
    return tree(lanes)


def fold_m1(v):
    m = v.shape[1]
    passes = -(-m // SLOTS)
    padded = np.zeros((NQ, passes * SLOTS))
    padded[:, :m] = v
    acc = np.zeros((NQ, SLOTS))
    for j in range(passes):
        acc = acc + padded[:, j * SLOTS:(j + 1) * SLOTS]
    return stages(acc)


def fold_m2(v):
    acc = np.zeros((NQ, SLOTS))
    for c in range(v.shape[1]):                              # ascending c is ascending j in every slot
        for q in range(NQ):
            x = Fraction(v[q, c])
            acc[q, c % SLOTS] = float(x * x + Fraction(acc[q, c % SLOTS]))
    return stages(acc)


def check(e, icase, m2=True):
    per = e.num_chains
    chains = range(e.ncases * per) if icase < 0 else range(icase * per, (icase + 1) * per)
    v = host_means(e, chains)
    got = e.chain_means(icase)
    assert got.shape == v.shape and np.array_equal(got, v), (icase, np.argwhere(got != v)[:5])
    red = e.reduce_host(icase)
    assert red[0] == len(chains) and red[39] == 0.0 and red[40] == 0.0, (icase, red[0], red[39:])
    want = fold_m1(v)
    assert np.array_equal(red[1:1 + NQ], want), (icase, "m1", red[1:1 + NQ], want)
    if m2:
        want = fold_m2(v)
        assert np.array_equal(red[1 + NQ:1 + 2 * NQ], want), (icase, "m2", red[1 + NQ:1 + 2 * NQ], want)
    return v


def run(ps, cases, steps=400, **kw):
    with ps.Ensemble(cases) as e:
        if steps:
            e.advance(steps)
        e.sync()
        return [check(e, icase, **kw) for icase in ([0] if e.ncases == 1 else list(range(e.ncases)) + [-1])]


@pytest.mark.parametrize("chains", [1, 5, 64, 65, 257, 300])
def test_one_case(ps, chains):
    """a single lane, a partial wave, the 64 / 65 boundary of the recorder's two kernels, the second block, a partial last one"""
    v, = run(ps, P(ps, num_chains=chains))
    assert np.all(v[0:3] != 0.0) and np.all(v[16] > 0.0)     # the run recorded something


def test_three_cases_each_and_pooled(ps):
    """the pooled reduction crosses case boundaries inside a block and looks the case of every chain up"""
    run(ps, [P(ps, num_chains=65, Fz=fz, seed=20 + i) for i, fz in enumerate((0.0, 0.5, 2.0))])


def test_umbrella(ps):
    """the norm is each chain's own wnorm"""
    with ps.Ensemble(P(ps, num_chains=48, umbrella=1)) as e:
        e.advance(400)
        e.sync()
        norms = [e.chain_state(c)["normalizer"] for c in range(48)]
        assert len(set(norms)) > 1 and all(x > 0 for x in norms)
        check(e, 0)


def test_clustering_main_extras(ps):
    v, = run(ps, P(ps, n=8, num_chains=12, move_set=ps.MOVES_CLUSTER, bend_mod=0.4))
    assert np.all(v[17] != 0.0) and np.all(v[18] != 0.0)


def test_no_steps_taken(ps):
    """steps = 0: the norm is 0 and every mean exactly 0"""
    v, = run(ps, P(ps, num_chains=70), steps=0)
    assert not v.any()


def test_second_pass_of_block_0(ps):
    """chains 65 536 ... are the j = 1 pass; the m2 half is held at the small sizes (1.2 M exact fractions here)"""
    run(ps, P(ps, n=2, num_chains=65600, precision=ps.F32), steps=120, m2=False)
