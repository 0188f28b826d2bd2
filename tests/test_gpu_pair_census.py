"""The pair census of the all-pairs kernels -- run with -m gpu.

interacting_kernel (U_interaction) and cluster_wave_kernel (U_interaction and UCutoff), f64 and f32, at the edges of the ring
for every M (tests/pair_ref.py: CENSUS_N).  Per (kernel, type, n) three handles, one at a time, each one launch and a
read-back:
  family A   up to 4096 chains with TWO lit monomers each (every other monomer at theta = 1/4 turn, its dipole dark): the
             kernel's U is the two self terms plus ONE pair term, which stands at least 8 x above the bound on |U - U_ref|.  A
             pair that the ring sum drops, doubles, weighs wrongly or puts on the wrong side of the cutoff fails its chain, and the
             failure names the pair's class (rotation, slots, which copy of the ring);
  family B   jittered compact rods and helices with every monomer lit, dielectric and polar, forces on: the whole sum within the
             bound -- which sees a wrong weight and, in f64, every single pair.
The reference is the literal sum over i < j in long double from the stored angles; bounds and configurations are derived in
tests/pair_ref.py and their conditions checked on the CPU by tests/test_pair_census_cpu.py (and again here, where cheap).
"""
import numpy as np
import pytest

import pair_ref as pr

pytestmark = pytest.mark.gpu

KERNELS = [("interacting", "interacting_kernel", False, False),
           ("cluster-interacting", "cluster_wave_kernel", True, False),
           ("cluster-cutoff", "cluster_wave_kernel", True, True)]
PRECS = [(pr.F32, "float"), (pr.F64, "double")]


@pytest.fixture(scope="module")
def ps():
    import polymer_stats_amd as ps
    assert ps._lib.load().pstat_device_count() >= 1, "no HIP device visible"
    return ps


def _device_U(ps, p, theta, phi, precision, cluster, kernel):
    """U of every chain of one handle holding the configurations (theta, phi)[C, n]."""
    C = len(theta)
    with ps.Ensemble(pr.device_params(ps, p, C, precision, cluster)) as e:
        name = e.launch_info().kernel.decode()
        assert kernel in name, name
        pr.set_chain_angles(e, theta, phi)
        U = np.array([e.microstate(c)[6] for c in range(C)])
        th, ph = pr.read_chain_angles(e)
        assert np.array_equal(th, theta) and np.array_equal(ph, phi), "the launch moved an injected configuration"
    return U


def _ratio(err, bound):
    """err / bound; a bound of 0 (f32, a lone pair beyond the cutoff: every term an exact zero) allows no error at all."""
    return np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))


@pytest.mark.parametrize("kname,kernel,cluster,cut", KERNELS, ids=[k[0] for k in KERNELS])
@pytest.mark.parametrize("prec,tname", PRECS, ids=["f32", "f64"])
@pytest.mark.parametrize("n", pr.CENSUS_N)
def test_pair_census(ps, n, prec, tname, kname, kernel, cluster, cut):
    M, L = pr.ring(n)
    kernel = f"{kernel}<{tname}>"
    rc = pr.choose_cutoff_radius(n, prec) if cut else None

    # ---- family A
    fa = pr.family_a(n, prec, cut, rc)
    assert fa.dmin >= pr.MIN_DIST_A and len(fa.i) <= pr.MAX_CHAINS
    U = _device_U(ps, fa.params, fa.theta, fa.phi, prec, cluster, kernel)
    err = np.abs(U - fa.U)
    ra = _ratio(err, fa.bound)
    bad = np.nonzero(~(ra <= 1.0))[0]
    pairs = fa.judged_pairs()
    und = len(np.unique((fa.i.astype(np.int64) * n + fa.j)[fa.undecided]))
    print(f"\nCENSUS {kernel} {kname} M={M} n={n} family A: chains {len(fa.i)}, pairs judged {pairs}, undecided by the cutoff "
          f"margin {und}, largest |err| / bound {ra[np.isfinite(ra)].max() if np.isfinite(ra).any() else np.inf:.3g}, wrong chains {len(bad)}")
    if len(bad):
        classes = sorted({pr.class_name(n, int(k)) for k in fa.keys[bad]})
        lines = [f"pair ({fa.i[q]}, {fa.j[q]}) [{pr.class_name(n, int(fa.keys[q]))}]: U = {U[q]!r}, reference {fa.U[q]!r}, "
                 f"pair term {fa.t[q]!r}{'' if fa.live[q] else ' (beyond the cutoff)'}, |err| / bound {ra[q]:.3g}" for q in bad[:6]]
        pytest.fail(f"{kernel} n = {n}: {len(bad)} of {len(fa.i)} two-lit chains off their reference; classes: "
                    + "; ".join(classes[:12]) + (" ..." if len(classes) > 12 else "") + "\n" + "\n".join(lines))

    # ---- family B
    for chain in pr.B_PARAMS:
        p, th, ph, lits, names = pr.family_b(n, prec, chain, cut, rc)
        assert min(l.dmin for l in lits) >= pr.MIN_DIST_B and max(l.pos_rel for l in lits) <= pr.CUT_MARGIN
        U = _device_U(ps, p, th, ph, prec, cluster, kernel)
        want, bound = np.array([l.U for l in lits]), np.array([l.bound for l in lits])
        rb = _ratio(np.abs(U - want), bound)
        share = {s: float(np.mean([pr.resolved_share(l) for l, nm in zip(lits, names) if nm == s])) for s in pr.B_SHAPES}
        live = sum(int((l.live & ~l.undecided).sum()) for l in lits)
        undb = sum(int(l.undecided.sum()) for l in lits)
        print(f"CENSUS {kernel} {kname} M={M} n={n} family B {chain}: chains {len(lits)}, pairs inside {live}, undecided {undb}, "
              f"largest |err| / bound {rb.max():.3g}, single pairs resolved "
              + ", ".join(f"{s} {100 * v:.2f} %" for s, v in share.items()))
        q = int(np.argmax(rb))
        assert rb[q] <= 1.0, (f"{kernel} n = {n} {chain} {names[q]} chain {q}: U = {U[q]!r}, reference {want[q]!r}, "
                              f"|err| / bound {rb[q]:.3g}")
