"""tests/math_ref.py judged on the CPU: its long-double references against 200-bit mpmath, its error measure, its argument
classes, and how much of the Metropolis families its reference verdict leaves open.  (The device side: test_gpu_math.py.)"""
import numpy as np
import pytest

import math_ref as mr

import mpmath as mp

REF_BOUND = 2.0 ** -10        # ulp of a double: what the long-double references may be off by (a condition of their use)
SAMPLE = 4000


def _sample(args, keep, nspecial):
    """The leading specials and an even stride of the rest, restricted to `keep`."""
    args = np.asarray(args)
    idx = np.concatenate([np.arange(nspecial), np.linspace(nspecial, args.size - 1, SAMPLE).astype(int)])
    x = args[idx]
    return x[keep(x)]


@pytest.mark.parametrize("cls, fn, keep", [
    ("sincos", "sin", np.isfinite), ("sincos", "cos", np.isfinite),
    ("exp", "exp", lambda x: np.isfinite(x) & (x < 709.7)),
    ("log", "log", lambda x: np.isfinite(x) & (x > 0)),
    ("acos", "acos", np.isfinite), ("rsqrt", "rsqrt", lambda x: x > 0)])
def test_long_double_references_against_mpmath(cls, fn, keep):
    """Every class, huge sincos arguments and the neighbours of k pi/2 included: the long double lies within 2^-10 ulp of the
    double nearest the 200-bit value."""
    x = _sample(mr.CLASSES[cls](), keep, mr.SPECIALS[cls].size)
    assert x.size > SAMPLE // 2
    got = mr.REFS[fn](x)
    worst = max(mr.mp_ulps(got[i], mr.mp_value(fn, x[i])) for i in range(x.size))
    print("%s on the %s class: long double within %.2e ulp of mpmath over %d points" % (fn, cls, worst, x.size))
    assert worst <= REF_BOUND


def test_pi_and_fold_constants():
    assert float(mr.PI_LD) == np.pi and mr.PI_LD != np.longdouble(np.pi)
    assert abs(mr.mp_ulps(mr.PI_LD, mp.pi)) <= REF_BOUND
    assert 0 < mr.fold_residual() < 2.0 ** -53 * 2.5e-16            # what two doubles leave of 2 pi


def test_ulps_flags_two_ulp_and_passes_point_four():
    g = np.random.default_rng(5)
    x = np.concatenate([g.uniform(-4, 4, 1000), np.ldexp(g.uniform(1, 2, 1000), g.integers(-1000, 1000, 1000)), [1.0, 2.0 ** -1022]])
    want = x.astype(np.longdouble)
    moved = np.nextafter(np.nextafter(x, np.inf), np.inf)
    e2 = mr.ulps(moved, want)
    assert np.all(e2 >= 1.0) and np.all(e2 <= 2.0) and np.all(e2[np.abs(x) != 1.0] == 2.0)   # (a power of two: the ulp doubles above)
    down = mr.ulps(np.nextafter(np.nextafter(x, -np.inf), -np.inf), want)
    assert np.all(down[np.abs(x) != 1.0] == 2.0) and np.all(down >= 1.0)      # (below a power of two the spacing halves)
    ulp = np.abs(np.nextafter(x, np.inf) - x).astype(np.longdouble)
    e04 = mr.ulps(x, want + 0.4 * ulp)
    assert np.all(e04 < 0.45) and np.all(e04 > 0.35)
    # floats
    f = g.uniform(-4, 4, 1000).astype(np.float32)
    f2 = np.nextafter(np.nextafter(f, np.float32(9)), np.float32(9))
    assert np.all(mr.ulps(f2.astype(np.float64), f.astype(np.float64), bits=24) >= 1.0)
    assert np.all(mr.ulps(f.astype(np.float64), f.astype(np.float64) * (1 + 0.2 * 2.0 ** -24), bits=24) < 0.5)
    # the rules
    inf, nan = np.inf, np.nan
    got = np.array([0.0, 1e-300, nan, 1.0, inf, -inf, inf, 1.0, 2.0 ** -1074])
    want = np.array([0.0, 0.0, nan, nan, inf, inf, 1.0, inf, 0.0]).astype(np.longdouble)
    assert list(mr.ulps(got, want)) == [0.0, inf, 0.0, inf, 0.0, inf, inf, inf, inf]
    assert mr.ulps(np.array([np.inf]), np.array([np.longdouble(np.finfo(np.float64).max) * 2]))[0] == 0.0   # overflow wants inf
    assert mr.ulps(np.array([2.0 ** -1074]), np.array([np.longdouble(2.0) ** -1076]))[0] == pytest.approx(0.75)
    # the hot-loop metric: absolute next to a zero
    assert mr.ulps_or_abs(np.array([1e-20]), np.array([np.longdouble(3e-20)]))[0] < 1e-3
    assert mr.ulps_or_abs(np.array([1.0]), np.array([np.longdouble(1.0) + 2.0 ** -51]))[0] == pytest.approx(2.0)


@pytest.mark.parametrize("cls", sorted(mr.CLASSES))
def test_classes_hold_their_specials_and_repeat(cls):
    a, b = mr.CLASSES[cls](), mr.CLASSES[cls]()
    assert a.dtype == np.float64 and np.array_equal(a, b, equal_nan=True)
    sp = mr.SPECIALS[cls]
    head = a[: sp.size]
    assert np.array_equal(head, sp, equal_nan=True) and np.array_equal(np.signbit(head), np.signbit(sp))
    assert 1 << 15 <= a.size <= 1 << 20


def test_class_contents():
    x = mr.sincos_args()
    f = x[np.isfinite(x)]
    k = np.rint(f[(f >= 0) & (f <= np.pi)] * 2 / np.pi)
    assert set(np.unique(k)) == {0.0, 1.0, 2.0}
    for fold in (mr.F64_FOLD, mr.PHI_FOLD):
        for v in (np.nextafter(fold, 0), fold, np.nextafter(fold, np.inf), -fold):
            assert v in f
    assert f.max() == 7e9 and f.min() == -7e9 and np.any((np.abs(f) > 0) & (np.abs(f) < 2.0 ** -58))
    assert np.isin(np.nextafter(40 * mr.HALF_PI, np.inf), f)
    lg = mr.log_args()
    assert np.any((lg > 0) & (lg < 2.0 ** -1022)) and np.any(lg < 0) and np.isin(1 + 2.0 ** -52, lg) and np.isin(1 - 2.0 ** -52, lg)
    ac = mr.acos_args()
    assert np.all(np.abs(ac) <= 1) and np.any((ac < 1) & (ac > 1 - 2.0 ** -50))
    pa = mr.pair_args()
    assert pa.shape[1] == 9 and np.all(pa[0, :3] == 0)
    r2 = (pa[1:, :3] ** 2).sum(1)
    assert r2.min() < 1e-11 and r2.max() > 1e11
    val, scale = mr.ref_pair(pa[1:])
    assert np.mean(np.abs(val) < 1e-6 * scale) > 0.1                # the cancelling third is there
    p32 = mr.pair_args(f32=True)
    assert np.array_equal(p32, p32.astype(np.float32).astype(np.float64))
    th = mr.sc32_theta_args()
    assert th.size == (1 << 23) + 1 and th[0] == 0.25 and th[-1] == 0.5
    pn = mr.positive_normal_floats()
    assert pn.min() == 2.0 ** -126 and pn.max() == float(np.finfo(np.float32).max)
    w = mr.words()
    assert w.size >= 2 * 65536 and w.max() == 0xFFFFFFFF


def test_metropolis_families_and_reference_verdict():
    """The families are what they say, the reference verdict follows the rules, and at most 0.5 % of all generated cases
    (the cap of the step judge) are left undecided by the reference alone."""
    near, far, edges = mr.metropolis_near(), mr.metropolis_far(), mr.metropolis_edges()
    assert near.shape[0] % 64 == 0 and far.shape[0] % 64 == 0 and np.array_equal(near, mr.metropolis_near(), equal_nan=True)
    allrows = np.concatenate([near, far, edges, mr.metropolis_near("floor", waves=32), mr.metropolis_near("subnormal", waves=32)])
    verdict, decided = mr.metropolis_reference(allrows)
    share = 1 - decided.mean()
    print("Metropolis families: %d rows, %.3f %% undecided by the reference alone" % (allrows.shape[0], 100 * share))
    assert share <= 0.005
    # far: every lane at least 1e-3 from the threshold, both verdicts present
    vf, df = verdict[near.shape[0]: near.shape[0] + far.shape[0]], decided[near.shape[0]: near.shape[0] + far.shape[0]]
    assert df.all() and 0.3 < vf.mean() < 0.7
    x = -far[:, 0] / far[:, 1] + far[:, 4]
    z = x + np.log(far[:, 2] / far[:, 3]) - np.log(mr.eps_of(*(far[:, j] for j in range(5, 10))) * 2.0 ** -53)
    assert np.abs(z).min() >= 0.999e-3
    # near: a third inside +-3 m of the threshold, verdicts on both sides
    vn = verdict[: near.shape[0]]
    assert 0.3 < vn.mean() < 0.7
    xn = -near[:, 0] / near[:, 1] + near[:, 4]
    zn = xn + np.log(near[:, 2] / near[:, 3]) - np.log(mr.eps_of(*(near[:, j] for j in range(5, 10))) * 2.0 ** -53)
    assert np.mean(np.abs(zn) <= 3 * mr.filter_margin(xn)) > 0.6
    # rules
    rows = np.array([[0.0, 1.0, 0.0, 0.5, 0.0, 0, 1 << 20, 0, 0, 0],        # st1 = 0: reject
                     [0.0, 1.0, 0.5, 0.0, 0.0, 0, 1 << 20, 0, 0, 0],        # st0 = 0: accept
                     [0.0, 1.0, 0.0, 0.0, 0.0, 0, 1 << 20, 0, 0, 0],        # both: reject
                     [np.nan, 1.0, 0.5, 0.5, 0.0, 0, 1 << 20, 0, 0, 0],     # NaN: reject
                     [-np.inf, 1.0, 0.5, 0.5, 0.0, 0, 1 << 20, 0, 0, 0],    # x = +inf: accept
                     [np.inf, 1.0, 0.5, 0.5, 0.0, 0, 1 << 20, 0, 0, 0],     # x = -inf: reject
                     [50.0, 1.0, 0.5, 0.5, 0.0, 0, 0, 0, 0, 0],             # eps = 0: accept
                     [0.0, 1.0, 0.5, 0.5, 0.0, 0, 1 << 31, 0, 0, 0],        # delta = 0: accept
                     [1.0, 1.0, 0.5, 0.5, 0.0, 0, 1 << 31, 0, 0, 0],        # e^-1 < 1/2: reject
                     [0.5, 1.0, 0.5, 0.5, 0.0, 0, 1 << 31, 0, 0, 0]],       # e^-1/2 > 1/2: accept
                    dtype=np.float64)
    v, d = mr.metropolis_reference(rows)
    assert list(v) == [False, True, False, False, True, False, True, True, False, True] and d.all()
    # the two contracts of eps
    assert int(mr.eps_of(1, 0xFFFFFFFF, 7, 511, 511)) == (1 << 53) - 1 and int(mr.eps_of(0, 0xFFFFFFFF, 7, 511, 511)) == ((1 << 23) - 1) << 30
