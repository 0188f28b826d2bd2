"""High-precision references and argument classes for the device arithmetic of polymer_stats_amd/csrc/pstat_math.h and
pstat_math_tab.h, and the ctypes door to the probe that runs one of those functions per launch (tests/probe/math_probe.hip,
built by polymer_stats_amd/csrc/Makefile as libmathprobe_off.so and libmathprobe_fast.so).  Written from the mathematics,
sharing no code with the library.

REFERENCES.  f64 functions: numpy longdouble (the x86 64-bit mantissa: 2^-11 of a double's ulp), f32 functions: float64.
tests/test_math_ref_cpu.py holds the long-double values to within 2^-10 ulp of a 200-bit mpmath evaluation on a sample of
every argument class, so an error measured against them is the device's to three digits.

ERRORS.  ulps(got, want): |got - want| in units of one ulp of the double (bits = 53) or float (bits = 24) nearest the true
value, 2^(e - bits) with want = m 2^e, 1/2 <= |m| < 1, and never below the subnormal spacing.  A true value beyond the largest
finite number wants inf, NaN wants NaN, 0 wants 0 exactly.  ulps_or_abs is the metric of the hot-loop sincos: the smaller of
that and |err| / 2^-53 -- next to a zero of the function the absolute error is what the energy sees.

ARGUMENT CLASSES are the smallest sets that reach every branch of each function; the generators are seeded, two calls give
the same arrays, and the specials stand first (SPECIALS names them)."""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

LD = np.longdouble
HERE = os.path.dirname(os.path.abspath(__file__))
PI, HALF_PI = math.pi, math.pi / 2
PHI_FOLD = 1.0e9            # PSTAT_PHI_FOLD: sincos_fast_f64 and sincos_tab fold by whole turns from here on
F64_FOLD = 1.0e5            # sincos_f64 folds from here on
U53 = 2.0 ** -53

# fn -> (code, columns in, columns out): the enum and the table of tests/probe/math_probe.hip
FN = {name: (code, ic, oc) for code, (name, ic, oc) in enumerate([
    ("sincos_f64", 1, 2), ("sincos_fast_bounded", 1, 2), ("sincos_fast_fold", 1, 2), ("sincos_fast_nofold", 1, 2),
    ("sincos_tab", 1, 2),
    ("exp_f64", 1, 1), ("log_f64", 1, 1), ("acos_f64", 1, 1), ("acos_tab", 1, 1), ("rsqrt_f64", 1, 1),
    ("pair_term_f64", 9, 1), ("pair_term_fast_f64", 9, 1), ("pair_term_tab", 9, 1),
    ("sc_f32", 1, 2), ("exp2f", 1, 1), ("rcpf", 1, 1), ("rsqf", 1, 1), ("acos_f32", 1, 1), ("pair_term_fast_f32", 9, 1),
    ("u01_f32", 1, 1), ("sym11_f32", 1, 1), ("sym11_f64", 1, 1), ("bits12", 1, 1), ("bits24", 1, 1),
    ("q16_theta_turns", 1, 1), ("q16_phi_turns", 1, 1), ("q16_disp", 2, 1), ("eps_uniform", 5, 1),
    ("metropolis", 10, 3), ("metropolis_straight", 10, 3)])}
FLAVOURS = ("off", "fast")
_libs = {}


def probe_path(flavour: str) -> str:
    # PSTAT_MATH_PROBE_DIR: probes built from an altered copy of the headers (the evidence that a test bites), like PSTAT_LIB
    return os.path.join(os.environ.get("PSTAT_MATH_PROBE_DIR") or os.path.join(HERE, "probe"), "libmathprobe_%s.so" % flavour)


def probe(flavour: str, fn: str, args) -> np.ndarray:
    """Run device function `fn` on the rows of `args` ([n] or [n, columns in]) in the probe built with the `flavour` flags;
    returns [n, columns out] doubles.  Rows are padded to whole waves with copies of the last row.  A missing probe library
    is an error (the normal build makes both), as is any HIP error."""
    code, ic, oc = FN[fn]
    if flavour not in _libs:
        lib = C.CDLL(probe_path(flavour))
        lib.pstat_probe.restype = C.c_int
        lib.pstat_probe.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_long]
        _libs[flavour] = lib
    a = np.ascontiguousarray(np.asarray(args, dtype=np.float64).reshape(-1, ic))
    n = a.shape[0]
    pad = (-n) % 64
    if pad:
        a = np.ascontiguousarray(np.concatenate([a, np.repeat(a[-1:], pad, axis=0)]))
    out = np.full((n + pad, oc), np.nan)
    rc = _libs[flavour].pstat_probe(code, a.ctypes.data, ic, out.ctypes.data, oc, n + pad)
    if rc != 0:
        raise RuntimeError("pstat_probe(%s, %s) failed with code %d" % (flavour, fn, rc))
    return out[:n]


# ------------------------------------------------------------------------------------------------------------ errors

def ulps(got, want, bits: int = 53) -> np.ndarray:
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want)
    emin, big = (-1022, LD(np.finfo(np.float64).max)) if bits == 53 else (-126, LD(np.finfo(np.float32).max))
    w = want.astype(LD)
    with np.errstate(all="ignore"):
        half_top = big * (LD(2) ** -(bits + 1))             # beyond max + half an ulp the nearest number is inf
        w = np.where(np.abs(w) > big + half_top, np.sign(w) * LD(np.inf), w)
        _, e = np.frexp(w)
        e = np.maximum(np.where(np.isfinite(w), e, 0).astype(np.int64), emin + 1)
        err = np.abs(got.astype(LD) - w) / np.ldexp(LD(1), (e - bits).astype(np.int32))
        err = np.where(w == 0, np.where(got == 0, LD(0), LD(np.inf)), err)
        err = np.where(np.isnan(w), np.where(np.isnan(got), LD(0), LD(np.inf)), err)
        err = np.where(np.isinf(w), np.where(got == w.astype(np.float64), LD(0), LD(np.inf)), err)
        err = np.where(np.isnan(got) & ~np.isnan(w), LD(np.inf), err)
    return err.astype(np.float64)


def ulps_or_abs(got, want) -> np.ndarray:
    with np.errstate(all="ignore"):
        a = (np.abs(np.asarray(got, dtype=np.float64).astype(LD) - np.asarray(want).astype(LD)) / LD(U53)).astype(np.float64)
    u = ulps(got, want)
    return np.where(np.isfinite(u), np.minimum(u, a), u)


# -------------------------------------------------------------------------------------------------------- references

def _ld(x):
    return np.asarray(x, dtype=np.float64).astype(LD)


def ref_sin(x):
    with np.errstate(all="ignore"):
        return np.sin(_ld(x))


def ref_cos(x):
    with np.errstate(all="ignore"):
        return np.cos(_ld(x))


def ref_exp(x):
    with np.errstate(all="ignore"):
        return np.exp(_ld(x))


def ref_log(x):
    with np.errstate(all="ignore"):
        return np.log(_ld(x))


def ref_acos(x):
    with np.errstate(all="ignore"):
        return np.arccos(_ld(x))


def ref_rsqrt(x):
    with np.errstate(all="ignore"):
        return LD(1) / np.sqrt(_ld(x))


REFS = {"sin": ref_sin, "cos": ref_cos, "exp": ref_exp, "log": ref_log, "acos": ref_acos, "rsqrt": ref_rsqrt}


def ref_pair(a):
    """One dipole-dipole term (m_i . m_j - 3 (m_i . rhat)(m_j . rhat)) / (4 pi r^3) and the scale its rounding errors are
    measured in, S = (sum_a |m_ia m_ja| + 3 (sum_a |m_ia rhat_a|)(sum_a |m_ja rhat_a|)) / (4 pi r^3); both long double."""
    a = _ld(a)
    r, mi, mj = a[:, 0:3], a[:, 3:6], a[:, 6:9]
    with np.errstate(all="ignore"):
        r2 = (r * r).sum(1)
        rm = np.sqrt(r2)
        h = r / rm[:, None]
        den = LD(4) * PI_LD * r2 * rm
        val = ((mi * mj).sum(1) - 3 * (mi * h).sum(1) * (mj * h).sum(1)) / den
        scale = (np.abs(mi * mj).sum(1) + 3 * np.abs(mi * h).sum(1) * np.abs(mj * h).sum(1)) / den
    return val, scale


def mp_value(name: str, x: float):
    """The function at the double x in 200-bit mpmath arithmetic (the judge of the long-double references)."""
    import mpmath as mp
    mp.mp.prec = 200
    v = mp.mpf(float(x))
    if name == "rsqrt":
        return 1 / mp.sqrt(v)
    return getattr(mp, name)(v)


def mp_ulps(got_ld, want_mp, bits: int = 53) -> float:
    """|got - want| in ulps of the double nearest want; got a long double, want an mpf."""
    import mpmath as mp
    mp.mp.prec = 200
    m, e = np.frexp(got_ld)
    g = mp.mpf(int(np.ldexp(m, 64))) * mp.mpf(2) ** (int(e) - 64)           # the long double, exactly
    if want_mp == 0:
        return 0.0 if g == 0 else math.inf
    ew = max(int(mp.floor(mp.log(abs(want_mp), 2))) + 1, -1021)
    return float(abs(g - want_mp) / mp.mpf(2) ** (ew - bits))


def _pi_ld():
    import mpmath as mp
    mp.mp.prec = 200
    hi = float(mp.pi)
    return LD(hi) + LD(float(mp.pi - mp.mpf(hi)))


PI_LD = _pi_ld()             # pi to the long double's 64 bits (np.pi is a double)


# --------------------------------------------------------------------------------------------------- argument classes

def _rng(seed):
    return np.random.default_rng(seed)


SINCOS_SPECIALS = np.array([0.0, -0.0, PI, HALF_PI, np.nextafter(PI, 0.0), 1e-300, np.nan, np.inf, -np.inf,
                            PI / 4, 3 * PI / 4, -PI, 2 * PI, 1.0])


def _near_multiples(ks):
    base = np.asarray(ks, dtype=np.float64) * HALF_PI
    out = [base]
    for _ in range(8):
        out.append(np.nextafter(out[-1], np.inf))
    lo = base
    for _ in range(8):
        lo = np.nextafter(lo, -np.inf)
        out.append(lo)
    return np.concatenate(out)


def sincos_args() -> np.ndarray:
    """The sincos class: one set for every form (sincos_f64 folds by whole turns at 1e5, the hot-loop and table forms at 1e9)."""
    g = _rng(20240611)
    n = 1 << 15
    th = g.uniform(0.0, PI, 3 * n)                                  # k = 0, 1, 2 of the bounded form
    k_small = np.arange(-40, 41)
    k_big = np.concatenate([np.rint(2 / PI * v) + np.arange(-2, 3) for v in (1e5, -1e5, 9e8, -9e8)])
    folds = []
    for f in (F64_FOLD, PHI_FOLD):                                   # both sides of each fold bound
        edge = np.array([np.nextafter(f, 0.0), f, np.nextafter(f, np.inf)])
        folds += [edge, -edge, g.uniform(0.99 * f, f, 512), g.uniform(f, 1.01 * f, 512), -g.uniform(0.99 * f, 1.01 * f, 512)]
    scaled = np.ldexp(g.uniform(0.0, PI, n), -(1 + np.arange(n) % 60))
    parts = [SINCOS_SPECIALS, th, _near_multiples(k_small), _near_multiples(k_big), g.uniform(-2000, 2000, n),
             g.uniform(-9.9e4, 9.9e4, n), *folds, g.uniform(-9.0e8, 9.0e8, n), g.uniform(-7e9, 7e9, n // 2),
             np.array([7e9, -7e9]), scaled, -scaled[: n // 4]]
    return np.concatenate(parts)


def exp_args() -> np.ndarray:
    g = _rng(20240612)
    n = 1 << 16
    cut = np.array([-745.2, 709.8])
    edges = np.concatenate([np.nextafter(cut, -np.inf), cut, np.nextafter(cut, np.inf)])
    x = sincos_args()
    x = x[np.isfinite(x) & (np.abs(x) < 1e5)]
    return np.concatenate([EXP_SPECIALS, edges, g.uniform(-745.2, 0.0, 2 * n), g.uniform(0.0, 709.8, n // 2),
                           -np.abs(x[:n]) * 0.007])


EXP_SPECIALS = np.array([-np.inf, np.nan, 0.0, -0.0, -745.2, 709.8])
LOG_SPECIALS = np.array([0.0, -0.0, 1.0, -1.0, -1e-300, np.inf, np.nan, -np.inf, 5e-324, 2.2250738585072014e-308])


def log_args() -> np.ndarray:
    g = _rng(20240613)
    n = 1 << 16
    m = np.concatenate([g.uniform(1.0, 2.0, n), math.sqrt(2.0) * (1 + g.uniform(-1e-3, 1e-3, n // 2)),
                        math.sqrt(2.0) * (1 + g.uniform(-4, 4, n // 4) * 2.0 ** -52)])
    e = g.integers(-1022, 1024, m.size)
    k = np.arange(1, 53)
    ones = np.concatenate([1 + 2.0 ** -k, 1 - 2.0 ** -k, 1 + g.uniform(-1, 1, n // 4) * 2.0 ** -g.integers(1, 53, n // 4)])
    sub = np.ldexp(g.uniform(0.5, 1.0, n // 8), g.integers(-1073, -1021, n // 8))
    return np.concatenate([LOG_SPECIALS, np.ldexp(m, e), m, ones, sub, -g.uniform(0, 10, 16)])


ACOS_SPECIALS = np.array([1.0, -1.0, 0.0, -0.0, 0.5, -0.5, np.nextafter(0.5, 0), np.nextafter(0.5, 1), np.nextafter(-0.5, 0),
                          np.nextafter(-0.5, -1), np.nextafter(1.0, 0), np.nextafter(-1.0, 0)])


def acos_args() -> np.ndarray:
    g = _rng(20240614)
    n = 1 << 16
    k = np.arange(n) % 53
    near1 = 1 - np.ldexp(g.uniform(0, 1, n), -k)
    nearm1 = -1 + np.ldexp(g.uniform(0, 1, n), -k)
    return np.concatenate([ACOS_SPECIALS, g.uniform(-1, 1, 2 * n), near1, nearm1])


RSQRT_SPECIALS = np.array([0.0, 1.0, 4.0, 1e-12, 1e12])


def rsqrt_args() -> np.ndarray:
    g = _rng(20240615)
    return np.concatenate([RSQRT_SPECIALS, np.exp(g.uniform(math.log(1e-12), math.log(1e12), 1 << 18))])


def _unit(g, n):
    v = g.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def pair_args(f32: bool = False) -> np.ndarray:
    """[n, 9]: bond vector r, dipoles m_i, m_j.  |r|^2 log-uniform in 1e-12 ... 1e12; dipoles of both chain types with the
    magnitudes of the step-judge configurations (tests/test_step_judge_cpu.py: E0 = 1.2, K1 = 1, K2 = 0.3, mu = 0.9):
    dielectric m = (K1 - K2) E0 n_z n + K2 E0 z, polar m = mu n; a third of the rows sit where m_i . m_j - 3 (m_i . rhat)
    (m_j . rhat) cancels (m_i = m_j at the angle cos^2 = 1/3 to r, up to a relative 2^-k).  Row 0 has r = 0.
    f32: every entry is a float."""
    g = _rng(20240616)
    n = 1 << 16
    E0, K1, K2, mu = 1.2, 1.0, 0.3, 0.9

    def dip(nh, polar):
        diel = (K1 - K2) * E0 * nh[:, 2:3] * nh + np.array([0.0, 0.0, K2 * E0])
        return np.where(polar[:, None], mu * nh, diel)

    rmag = np.exp(0.5 * g.uniform(math.log(1e-12), math.log(1e12), 3 * n))
    rh = _unit(g, 3 * n)
    polar = g.integers(0, 2, 3 * n).astype(bool)
    mi, mj = dip(_unit(g, 3 * n), polar), dip(_unit(g, 3 * n), polar)
    # the cancelling third: m at the magic angle to rhat, m_j = m_i (1 + 2^-k)
    c = slice(2 * n, 3 * n)
    perp = np.cross(rh[c], _unit(g, n))
    perp /= np.linalg.norm(perp, axis=1)[:, None]
    m = 0.9 * (rh[c] / math.sqrt(3.0) + perp * math.sqrt(2.0 / 3.0))
    mi[c] = m
    mj[c] = m * (1 + np.ldexp(g.uniform(-1, 1, n), -(np.arange(n) % 40))[:, None])
    a = np.concatenate([rh * rmag[:, None], mi, mj], axis=1)
    a[0, 0:3] = 0.0
    if f32:
        a = a.astype(np.float32).astype(np.float64)
    return a


SC32_SPECIALS = np.array([0.0, 0.25, 0.5, 0.75, 2.0 ** -149, 2.0 ** -127, 2.0 ** -126, 1e-30, 1e-10])


def sc32_theta_args() -> np.ndarray:
    """Every float of [1/4, 1/2] (turns): theta of the upper hemisphere."""
    lo, hi = np.float32(0.25).view(np.uint32), np.float32(0.5).view(np.uint32)
    return np.arange(lo, hi + 1, dtype=np.uint32).view(np.float32).astype(np.float64)


def sc32_phi_args() -> np.ndarray:
    """The specials, a stride over the floats of [0, 1) (phi, and theta of the lower hemisphere), subnormal and tiny ones."""
    g = _rng(20240617)
    top = int(np.float32(1.0).view(np.uint32))
    bits = np.arange(0, top, 4093, dtype=np.uint32)
    sub = g.integers(1, 1 << 23, 4096).astype(np.uint32)
    return np.concatenate([SC32_SPECIALS, bits.view(np.float32).astype(np.float64), sub.view(np.float32).astype(np.float64),
                           g.uniform(0, 1, 1 << 16).astype(np.float32).astype(np.float64)])


EXP2_SPECIALS = np.array([0.0, 1.0, -1.0, -126.0, -127.0, -149.0, -150.0, 127.0, 128.0])


def exp2_args() -> np.ndarray:
    g = _rng(20240618)
    return np.concatenate([EXP2_SPECIALS, g.uniform(-150, 128, 1 << 18).astype(np.float32).astype(np.float64)])


def positive_normal_floats() -> np.ndarray:
    """A stride over all positive normal floats, ends included."""
    bits = np.concatenate([np.arange(0x00800000, 0x7F800000, 8191, dtype=np.uint32), np.array([0x7F7FFFFF, 0x3F800000], np.uint32)])
    return bits.view(np.float32).astype(np.float64)


ACOS32_SPECIALS = np.array([1.0, -1.0, 0.0, 0.5, -0.5])


def acos32_args() -> np.ndarray:
    g = _rng(20240619)
    n = 1 << 16
    k = np.arange(n) % 24
    a = np.concatenate([ACOS32_SPECIALS, g.uniform(-1, 1, 2 * n), 1 - np.ldexp(g.uniform(0, 1, n), -k),
                        -1 + np.ldexp(g.uniform(0, 1, n), -k)])
    return np.clip(a.astype(np.float32).astype(np.float64), -1.0, 1.0)


def words() -> np.ndarray:
    """32-bit words: the edges, all 65 536 values of a 16-bit pattern in the high half, and 2^16 random words."""
    g = _rng(20240620)
    edge = np.array([0, 1, 511, 512, 0xFFFFFFFF, 0xFFFFFE00, 0x80000000, 0x7FFFFFFF, 0x00000200], dtype=np.uint64)
    return np.concatenate([edge, np.arange(65536, dtype=np.uint64) << np.uint64(16), g.integers(0, 1 << 32, 1 << 16, dtype=np.uint64)])


SPECIALS = {"sincos": SINCOS_SPECIALS, "exp": EXP_SPECIALS, "log": LOG_SPECIALS, "acos": ACOS_SPECIALS, "rsqrt": RSQRT_SPECIALS,
            "sc32": SC32_SPECIALS, "exp2": EXP2_SPECIALS, "acos32": ACOS32_SPECIALS}
CLASSES = {"sincos": sincos_args, "exp": exp_args, "log": log_args, "acos": acos_args, "rsqrt": rsqrt_args,
           "sc32": sc32_phi_args, "exp2": exp2_args, "acos32": acos32_args}


# ------------------------------------------------------------------------------------------------ derived bounds

def fold_residual() -> float:
    """|2 pi - HI2 - LO2| of the fold by whole turns (the two constants of sincos_f64 / sincos_fast_f64 / sincos_tab)."""
    import mpmath as mp
    mp.mp.prec = 200
    return float(abs(2 * mp.pi - mp.mpf(6.28318530717958623200e+00) - mp.mpf(2.44929359829470641435e-16)))


def fold_abs_bound(x, own_ulps: float) -> np.ndarray:
    """Absolute error bound of a folded sincos at |x| >= the fold bound.  The fold is x' = fma(-t, LO2, fma(-t, HI2, x)),
    t = rint(x / 2 pi): t HI2 and t LO2 are exact inside their fused multiply-adds, each of which rounds once a number of
    magnitude <= pi (+ 2 pi times the 2^-52 |t| by which the rounded x / 2 pi can miss: < 4 in all), so by <= 2^-52; what
    the two constants leave of 2 pi enters t times.  sin and cos have slope <= 1, and the form's own error on the folded
    argument is own_ulps of a result <= 1."""
    t = np.abs(np.asarray(x, dtype=np.float64)) / (2 * PI)
    return 2 * 2.0 ** -52 + t * fold_residual() + own_ulps * U53


# pair terms: K 2^-53 S with S of ref_pair.  Rounded operations of pair_term_fast(double), in units of u = 2^-53 relative
# (1 ulp <= 2 u):  r2 three (its terms are positive: 3 u); y = rsqrt_f64(r2): its own <= 3 ulp = 6 u plus half of r2's: 7.5 u;
# ir2 = y y: 16 u;  -3 ir2: 17 u;  m_i.r and m_j.r three each on their absolute sums, their product: 7 u;  the second term of
# num: 24 u, the first (m_i.m_j, three operations): 3 u, the fma's own rounding: 1 u -- 25 u of S r^3 4 pi;  ir2 y: 24.5 u;  the
# two last products and the rounded 1 / 4 pi: 3 u.  First order 52.5 u; the literal pair_term<double> (sqrt, four divisions,
# all correctly rounded) counts to 24 u and the table form is the fast one.  The next power of two:
K_PAIR = 64.0
# pair_term_fast(float), u = 2^-24: v_rsq_f32 at 1 ulp (2 u) instead of 6 u: y 3.5 u, ir2 8 u, -3 ir2 9 u, second term 16 u,
# num 17 u, ir2 y 12.5 u, the tail 3 u: 32.5 u.  The next power of two:
K_PAIR_F32 = 64.0


def acos32_bound(x) -> np.ndarray:
    """|acos_r(float) - acos| <=, from its operations (u = 2^-24).  p: seven fused steps on values below 2, each off by <= u,
    propagated with |a| <= 1, and eight coefficients rounded to float (sum of magnitudes 1.98: 2 u): 9 u absolute on p >= 1.41,
    6.4 u relative.  1 - a: exact for a >= 1/2, else u / 2 relative; v_sqrt_f32 halves that and adds its 1 ulp = 2 u; the
    product rounds once: together < 10 u of r = acos |x|.  The polynomial's truncation (the header: 2e-8, Abramowitz & Stegun
    4.4.46).  For x < 0 the float constant pi is off by 8.75e-8 and the subtraction rounds a number below 4: 2^-23."""
    x = np.asarray(x, dtype=np.float64)
    r = np.arccos(np.abs(x))
    return 10 * 2.0 ** -24 * r + 2e-8 + np.where(x < 0, 8.75e-8 + 2.0 ** -23, 0.0)


# -------------------------------------------------------------------------------------------- the Metropolis test

MET_COLS = ("dU", "kT", "st1", "st0", "extra", "wide", "weps", "w0", "wphi", "wth")
FILTER_FLOOR = 2.0 ** -96      # the filter's domain (pstat_math.h): num, den in {0} U [2^-96, 16]
FILTER_TOP = 16.0


def eps_of(wide, weps, w0, wphi, wth) -> np.ndarray:
    """eps of include/pstat.h's two stream contracts as an exact integer numerator over 2^53."""
    weps, w0, wphi, wth = (np.asarray(v).astype(np.uint64) for v in (weps, w0, wphi, wth))
    lo = ((wth & np.uint64(511)) << np.uint64(12)) | ((wphi & np.uint64(511)) << np.uint64(3)) | (w0 & np.uint64(7))
    e53 = (weps << np.uint64(21)) + lo
    e23 = (weps >> np.uint64(9)) << np.uint64(30)
    return np.where(np.asarray(wide) != 0, e53, e23)


def filter_margin(x) -> np.ndarray:
    """m of metropolis_filter as a double (the f32 value differs in its last bits: the generators only aim with it)."""
    return 2e-6 + 1e-6 * np.abs(x)


def _aim(a, target):
    """Set dU of the rows a so that delta - log eps is `target`, up to the rounding of dU to a double."""
    ld = a.astype(LD)
    eps = eps_of(*(a[:, j] for j in range(5, 10))).astype(LD) * LD(2) ** -53
    with np.errstate(all="ignore"):
        dU = (np.log(ld[:, 2] / ld[:, 3]) + ld[:, 4] - np.log(eps) - np.asarray(target).astype(LD)) * ld[:, 1]
    a[:, 0] = dU.astype(np.float64)
    return a


def _met_rows(g, n, target, kind, wide=None, min_weps=1 << 9):
    """n rows whose exact delta - log eps is (up to the rounding of dU) `target`; kind: 'sweep' (sines), 'floor' (num, den at
    the bottom of the filter's domain) or 'subnormal' (below it)."""
    wide = g.integers(0, 2, n) if wide is None else np.full(n, wide)
    weps = g.integers(min_weps, 1 << 32, n, dtype=np.uint64)
    w0, wphi, wth = (g.integers(0, 1 << 32, n, dtype=np.uint64) for _ in range(3))
    if kind == "sweep":
        st1, st0 = np.sin(g.uniform(1e-3, PI - 1e-3, n)), np.sin(g.uniform(1e-3, PI - 1e-3, n))
    else:
        lo, hi = (-96, -90) if kind == "floor" else (-149, -96)
        st1 = np.ldexp(g.uniform(1, 2, n), g.integers(lo, hi, n))
        st0 = np.ldexp(g.uniform(1, 2, n), g.integers(lo, hi, n))
        if kind == "subnormal":        # keep x inside [-80, 80]: the ratio decides, not an exponent out of range
            st0 = np.where(np.abs(np.log(st1 / st0)) > 30, st1 * g.uniform(0.3, 3, n), st0)
    kT = g.uniform(0.3, 3.0, n)
    extra = np.where(g.integers(0, 4, n) == 0, g.uniform(-300, 300, n), g.uniform(-3, 3, n))
    a = np.stack([np.zeros(n), kT, st1, st0, extra, wide.astype(np.float64), weps.astype(np.float64),
                  w0.astype(np.float64), wphi.astype(np.float64), wth.astype(np.float64)], axis=1)
    return _aim(a, target)


def _signed(g, mag):
    return mag * np.where(g.integers(0, 2, mag.size) == 0, -1.0, 1.0)


def metropolis_near(kind: str = "sweep", waves: int = 144, seed: int = 20240621) -> np.ndarray:
    """waves * 64 rows around the threshold, in thirds: delta = +-10^U(-17, -3); dense in +-3 m, where the filter hands over
    to the literal test; and eps inside the interval [u, u + 2^-23) that the filter sees only the lower end of, with random
    low bits under the 53-bit contract (delta within +-2^-23 / u of the threshold)."""
    g = _rng(seed)
    n = waves * 64 // 3
    a = _met_rows(g, n, _signed(g, 10.0 ** g.uniform(-17, -3, n)), kind)
    b = _met_rows(g, n, g.uniform(-3, 3, n) * 3e-6, kind)
    # the interval third: the threshold E (accept iff eps < E) at u + t 2^-23, t in (-1.5, 2.5): below, inside and above
    # the interval, the 53-bit eps anywhere inside it
    nc = waves * 64 - 2 * n
    c = _met_rows(g, nc, np.zeros(nc), kind, wide=1)
    c[:, 6] = np.maximum(c[:, 6], 2048.0)          # u >= 4 * 2^-23, so that E > 0
    u = np.floor(c[:, 6] / 512.0) * 2.0 ** -23
    E = (u + g.uniform(-1.5, 2.5, nc) * 2.0 ** -23).astype(LD)
    eps = eps_of(*(c[:, j] for j in range(5, 10))).astype(LD) * LD(2) ** -53
    c = _aim(c, np.log(E) - np.log(eps))
    out = np.concatenate([a, b, c])
    return out[g.permutation(out.shape[0])]


def metropolis_far(waves: int = 4096, seed: int = 20240622) -> np.ndarray:
    """Whole waves with |delta - log eps| >= 1e-3 in every lane: the filter must decide all of them by itself.  What it may
    leave to the literal test is a draw within m = 2e-6 + 1e-6 |x| of the threshold plus the interval it cannot see into,
    2^-23 / u relative: with |x| < 350 and u >= 2^-10 that is below 4.7e-4."""
    g = _rng(seed)
    n = waves * 64
    mag = np.where(g.integers(0, 2, n) == 0, 10.0 ** g.uniform(-3, 0, n), g.uniform(1, 40, n))
    return _met_rows(g, n, _signed(g, mag), "sweep", min_weps=1 << 22)


def metropolis_edges(seed: int = 20240623) -> np.ndarray:
    """Zero and sin(fl pi) densities, u = 0 and u = 1 - 2^-23, x at +-inf, NaN and where v_exp_f32 under- and overflows,
    |extra| up to 300: each edge with a spread of the other arguments, every num and den inside the filter's domain."""
    g = _rng(seed)
    rows = []
    sinpi = math.sin(PI)

    def block(n=256, target=None):
        return _met_rows(g, n, _signed(g, 10.0 ** g.uniform(-8, 1, n)) if target is None else target, "sweep")

    for st1, st0 in ((None, 0.0), (0.0, None), (0.0, 0.0), (sinpi, None), (None, sinpi), (sinpi, sinpi)):
        tg = _signed(g, 10.0 ** g.uniform(-8, 1, 256))
        b = block(256, tg)
        if st1 is not None:
            b[:, 2] = st1
        if st0 is not None:
            b[:, 3] = st0
        rows.append(_aim(b, tg) if 0.0 not in (st1, st0) else b)
    for weps in (0.0, 511.0, float(0xFFFFFFFF), float(0xFFFFFE00), 512.0):     # u = 0 (twice), 1 - 2^-23 (twice), 2^-23
        tg = _signed(g, 10.0 ** g.uniform(-8, 1, 256))
        b = block(256, tg)
        b[:, 6] = weps
        pos = eps_of(*(b[:, j] for j in range(5, 10))) > 0          # (eps = 0 has no threshold to aim at)
        b[pos] = _aim(b[pos], tg[pos])
        rows.append(b)
    for x in (np.inf, -np.inf, np.nan, *np.arange(-104.0, -86.5, 0.5), *np.arange(88.0, 90.5, 0.25)):
        b = block(64)
        b[:, 4] = g.uniform(-3, 3, 64)
        b[:, 0] = -(x - b[:, 4]) * b[:, 1] if np.isfinite(x) else (-x if not np.isnan(x) else np.nan)
        rows.append(b)
    b = block(1024)
    b[:, 4] = _signed(g, g.uniform(250, 300, 1024))
    rows.append(b)
    target = _signed(g, 10.0 ** g.uniform(-8, 1, 1024))
    b = block(1024, target)
    b[:, 4] = _signed(g, g.uniform(250, 300, 1024))          # ... and around the threshold
    rows.append(_aim(b, target))
    # the corner of the domain where x is lowest around the threshold: num at the top, den at the floor, u = 1 ... 3 * 2^-23
    b = block(1024, target)
    b[:, 2], b[:, 3] = g.uniform(1, FILTER_TOP, 1024), FILTER_FLOOR * g.uniform(1, 2, 1024)
    b[:, 6] = g.integers(512, 2048, 1024).astype(np.float64)
    rows.append(_aim(b, target))
    return np.concatenate(rows)


def metropolis_reference(a: np.ndarray):
    """(verdict, decided) of the reference's expression  (delta >= 0) or (eps < exp(delta)),  delta = -dU/kT + log(st1/st0) +
    extra, evaluated exactly on the doubles of each row: z = delta - log eps in long double, and in 200-bit mpmath wherever
    the long double's own error (2^-60 of the terms) could reach z.  decided: |z| exceeds 16 * 2^-53 (1 + |dU/kT| +
    |log(st1/st0)| + |extra|), the room a double evaluation of the expression may use; rows the rules below settle are
    always decided.  Rules (IEEE arithmetic of the literal expression, the reject-on-NaN logic of the callers): NaN anywhere
    or st1 = 0: reject (log 0 = -inf, 0/0 = NaN); st0 = 0 < st1: accept; dU = -+inf: accept / reject; eps = 0: accept
    (undecided where delta < -700: exp underflows)."""
    import mpmath as mp
    mp.mp.prec = 200
    a = np.asarray(a, dtype=np.float64)
    dU, kT, st1, st0, extra = (a[:, j] for j in range(5))
    epsn = eps_of(*(a[:, j] for j in range(5, 10)))
    n = a.shape[0]
    verdict = np.zeros(n, dtype=bool)
    decided = np.ones(n, dtype=bool)
    nan = np.isnan(dU) | np.isnan(extra) | np.isnan(st1) | np.isnan(st0)
    rule = nan | (st1 == 0) | (st0 == 0) | np.isinf(dU)
    verdict[(st0 == 0) & (st1 > 0) & ~nan & ~(dU == np.inf)] = True
    verdict[(dU == -np.inf) & (st1 > 0) & ~nan] = True
    with np.errstate(all="ignore"):
        t1, t2, t3 = -dU.astype(LD) / kT.astype(LD), np.log(st1.astype(LD) / st0.astype(LD)), extra.astype(LD)
        delta = t1 + t2 + t3
        mag = 1 + np.abs(t1) + np.abs(t2) + np.abs(t3)
        z = delta - np.log(epsn.astype(LD) * LD(2) ** -53)
    gen = ~rule
    zero = gen & (epsn == 0)
    verdict[zero] = True
    decided[zero & (delta < -700)] = False
    gen &= epsn != 0
    with np.errstate(all="ignore"):
        logeps = np.abs(np.log(epsn.astype(LD) * LD(2) ** -53))
    verdict[gen] = (z[gen] > 0) | (delta[gen] >= 0)
    decided[gen] = (np.abs(z[gen]) > 16 * U53 * mag[gen]).astype(bool)
    close = gen & (np.abs(z) <= 2.0 ** -50 * (mag + logeps))
    for i in np.nonzero(close)[0]:
        d = -mp.mpf(dU[i]) / mp.mpf(kT[i]) + mp.log(mp.mpf(st1[i]) / mp.mpf(st0[i])) + mp.mpf(extra[i])
        zi = d - mp.log(mp.mpf(int(epsn[i])) / mp.mpf(2) ** 53)
        verdict[i] = bool(zi > 0 or d >= 0)
        decided[i] = bool(abs(zi) > 16 * U53 * float(mag[i]))
    return verdict, decided
