"""tests/pair_ref.py judged on the CPU: the literal pair sum against 200-bit mpmath and against the oracle, the ring's class
rule against a lane-by-lane replay of the ring, and the CONDITIONS the GPU census (tests/test_gpu_pair_census.py) relies on:
every class of pairs is there, every judged pair stands at least RESOLVE x above the bound, no injected chain brings two
monomers closer than 0.3 b (family A) / 0.5 b (family B), the cutoff sits inside the spread of distances with at most 1 % of
the pairs undecided, and the position errors stay inside the cutoff margin.  These are conditions, not measurements."""
import math

import numpy as np
import pytest

import pair_ref as pr
import step_judge as sj

PRECS = [(pr.F32, "f32"), (pr.F64, "f64")]


def _small_configs():
    g = np.random.default_rng(31)
    out = []
    for n, chain, cut in ((2, "diel", False), (5, "polar", False), (7, "diel", True), (12, "polar", True), (12, "diel", False)):
        p = dict(pr.B_PARAMS[chain], n=n, energy_type=pr.CUTOFF if cut else pr.INTERACTING, cutoff_radius=2.1)
        out.append((p, g.uniform(0.3, math.pi - 0.3, n), g.uniform(0, 2 * math.pi, n)))
    return out


@pytest.mark.parametrize("prec,pname", PRECS, ids=[p[1] for p in PRECS])
def test_literal_sum_against_mpmath_and_the_oracle(oracle, prec, pname):
    """The long double sum lies within 2^-58 sum |terms| of the 200-bit value (the f64 bounds start at ~2^-46 sum |terms|), and
    the oracle's f64 eap_chain_energy of the same radians within 2^-44."""
    for p, th_rad, ph_rad in _small_configs():
        th, ph = pr.stored(th_rad, ph_rad, prec)
        lit = pr.literal(p, th, ph, prec)
        rad_th, rad_ph = pr.radians_ld(th, prec).astype(np.float64), pr.radians_ld(ph, prec).astype(np.float64)
        scale = sj.term_sums(p, rad_ph, rad_th)[0][6]
        want = pr.literal_mp(p, th, ph, prec)
        err = abs(float(want - lit.U))
        print(f"n = {p['n']} {pname}: U = {lit.U!r}, |literal - mpmath| / sum |terms| = {err / scale:.2e}")
        # (lit.U is the long double rounded to a double: half an ulp of U on top of the sum's own error)
        assert err <= 2.0 ** -58 * scale + 2.0 ** -53 * abs(lit.U)
        if prec == pr.F64:
            Uo, _, _ = oracle.chain_energy(oracle.make_params(num_steps=0, stepout=0, **p), rad_ph, rad_th)
            assert abs(Uo - lit.U) <= 2.0 ** -44 * scale


@pytest.mark.parametrize("n", [2, 3, 6, 63, 64, 65, 66, 127, 130, 253, 257, 264])
def test_class_rule_against_a_replay_of_the_ring(n):
    """pstat_wave.h read lane by lane: lane l of the L in the ring meets, at rotation k = 1 .. L/2, the M entries at ring
    entry l + L - k (the first copy holds lane e at e, the second at e + L), rotation L/2 at weight 1/2; pairs inside a lane
    directly.  Every pair of real monomers must come out with total weight 1, in the class pair_classes names."""
    M, L = pr.ring(n)
    assert L % 2 == 0 and L <= 64 and (L - 2) * M < n <= L * M
    weight, seen = {}, {}
    for lane in range(L):
        for j in range(M):
            for jp in range(j + 1, M):
                a, b = lane * M + j, lane * M + jp
                if b < n:
                    weight[(a, b)] = weight.get((a, b), 0) + 1.0
                    seen.setdefault((a, b), set()).add((0, j, jp, 0))
        for k in range(1, L // 2 + 1):
            entry = lane + L - k
            partner, copy = entry % L, 2 if entry >= L else 1
            for j in range(M):
                for jp in range(M):
                    a, b = lane * M + j, partner * M + jp
                    if a < n and b < n:
                        key = (min(a, b), max(a, b))
                        weight[key] = weight.get(key, 0) + (0.5 if k == L // 2 else 1.0)
                        cls = (k, j, jp, copy) if k < L // 2 else (k, *((j, jp) if a < b else (jp, j)), 3)
                        seen.setdefault(key, set()).add(cls)
    ii, jj = np.triu_indices(n, 1)
    assert set(weight) == set(zip(ii.tolist(), jj.tolist()))
    assert all(w == 1.0 for w in weight.values())
    k, own, other, order = pr.pair_classes(n, ii, jj)
    for q, key in enumerate(zip(ii.tolist(), jj.tolist())):
        assert seen[key] == {(int(k[q]), int(own[q]), int(other[q]), int(order[q]))}, (key, seen[key])


def _special_monomers(n):
    M, _ = pr.ring(n)
    return {0, n - 1} | (set(range((n // M) * M, n)) if n % M else set())


@pytest.mark.parametrize("prec,pname", PRECS, ids=[p[1] for p in PRECS])
@pytest.mark.parametrize("n", pr.CENSUS_N)
def test_family_a_conditions(n, prec, pname):
    M, L = pr.ring(n)
    rc = pr.choose_cutoff_radius(n, prec)
    total = n * (n - 1) // 2
    for cut in (False, True):
        fa = pr.family_a(n, prec, cut, rc)
        K = len(fa.i)
        assert K <= pr.MAX_CHAINS and fa.theta.shape == (K, n)
        assert fa.dmin >= pr.MIN_DIST_A, fa.dmin
        hi = 0.5 if prec == pr.F32 else math.pi
        assert np.all((fa.theta > 0) & (fa.theta < hi)) and np.all((fa.phi >= 0) & (fa.phi < 2 * hi))
        # every offered pair is judged -- or, with a cutoff, within its margin (at most 1 % of the judged ones)
        ids = fa.i.astype(np.int64) * n + fa.j
        judged_ids, und_ids = np.unique(ids[fa.judged]), np.unique(ids[fa.undecided])
        assert len(np.union1d(judged_ids, und_ids)) == fa.offered == min(total, pr.MAX_CHAINS)
        assert len(und_ids) <= 0.01 * len(judged_ids) or not cut and len(und_ids) == 0
        assert np.all(np.abs(fa.t[fa.judged]) >= pr.RESOLVE * fa.bound[fa.judged])
        # zero missing classes
        required = pr.required_classes(n)
        if total <= pr.MAX_CHAINS:
            ii, jj = np.triu_indices(n, 1)
            required = np.unique(pr.class_key(*pr.pair_classes(n, ii, jj)))
        missing = np.setdiff1d(required, np.unique(fa.keys[fa.judged]))
        assert len(missing) == 0, [pr.class_name(n, int(k)) for k in missing]
        for m in _special_monomers(n):
            assert np.any(fa.judged & ((fa.i == m) | (fa.j == m))), m
        if cut:
            # the cutoff sits inside the spread: pairs on both sides (one distance only at n = 2 with equal tilts: both there)
            assert fa.live[fa.judged].any() and (~fa.live[fa.judged]).any(), rc
            assert np.all(fa.U[~fa.live & ~fa.undecided] == 0.0)             # its pair part is 0, not small
            assert fa.pos_rel <= pr.CUT_MARGIN, fa.pos_rel
        # the vectorised reference is the literal sum (which also holds the dust: f64's is carried in the bound here; in f32
        # the long double cos(2 pi / 4) = 2.5e-20 leaves < 1e-13 where the device has an exact zero)
        for q in sorted({0, K // 3, K - 1}):
            lit = pr.literal(fa.params, fa.theta[q], fa.phi[q], prec)
            assert abs(lit.U - fa.U[q]) <= 0.5 * fa.bound[q] + 1e-13, (q, lit.U, fa.U[q], fa.bound[q])
            assert lit.dmin >= fa.dmin - 1e-9
        ratio = np.abs(fa.t[fa.judged]) / np.maximum(fa.bound[fa.judged], 1e-300)
        print(f"family A n = {n} (M = {M}, L = {L}) {pname}{' cutoff %.3f b' % rc if cut else ''}: chains {K}, pairs judged "
              f"{len(judged_ids)}, undecided {len(und_ids)}, classes {len(required)}, smallest |t| / bound {ratio.min():.1f}, "
              f"closest approach {fa.dmin:.3f} b")


@pytest.mark.parametrize("prec,pname", PRECS, ids=[p[1] for p in PRECS])
@pytest.mark.parametrize("n", (2, 3, 64, 65, 100, 130, 200, 257, 400, 512))
def test_family_b_conditions(n, prec, pname):
    """Every monomer lit.  Prints the share of single pairs with |t| >= RESOLVE x the chain's bound per shape; in f64 without a
    cutoff every pair of the dielectric chains is resolved (their dipoles stand along z and no pair direction of these shapes
    comes near the zero of 1 - 3 cos^2); the polar chains' dipoles lie along the chain, where that angular factor does vanish
    for some pairs -- a property of the geometry, not of the bound: at least 99 % there.  (The GPU census asserts the
    distance and margin conditions at every chain length it runs and prints the shares.)"""
    rc = pr.choose_cutoff_radius(n)
    for chain in pr.B_PARAMS:
        for cut in (False, True):
            p, th, ph, lits, names = pr.family_b(n, prec, chain, cut, rc)
            assert len(lits) == 2 * pr.chains_per_shape(n) <= pr.MAX_CHAINS
            assert min(l.dmin for l in lits) >= pr.MIN_DIST_B
            assert max(l.pos_rel for l in lits) <= pr.CUT_MARGIN
            live = sum(int((l.live & ~l.undecided).sum()) for l in lits)
            und = sum(int(l.undecided.sum()) for l in lits)
            assert und <= 0.01 * max(live, 1), (und, live)
            share = {s: float(np.mean([pr.resolved_share(l) for l, nm in zip(lits, names) if nm == s])) for s in pr.B_SHAPES}
            print(f"family B n = {n} {pname} {chain}{' cutoff %.3f b' % rc if cut else ''}: chains {len(lits)}, pairs inside "
                  f"{live}, undecided {und}, resolved single pairs " + ", ".join(f"{s} {100 * v:.2f} %" for s, v in share.items()))
            if prec == pr.F64 and not cut:
                for s, v in share.items():
                    assert v == 1.0 if chain == "diel" else v >= 0.99, (chain, s, v)
