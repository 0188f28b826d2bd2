// pstat_math_tab.h -- the table-driven copy of the f64 step arithmetic of pstat_math.h, for the chain-per-wavefront
// clustering kernel (pstat_cluster_cw.hip); not part of the public ABI.  tests/test_gpu_math.py holds each form here to the
// form of pstat_math.h it restates (tests/probe/math_probe.hip stages KINIT into LDS the way the kernel does).
#pragma once

#include "pstat_math.h"

namespace pstat {

namespace {

// ---- Polynomial coefficients of the step's trigonometry, read from LDS where they are used.  A double constant cannot be an
// operand of an f64 instruction: it is built in a register pair first -- by two vector moves if the instruction wants it as
// its accumulator, which is what the Horner forms below compile to, or parked in scalar registers across the loop, which
// spills the step's own scalars (the kernel needs ~60 such constants).  One broadcast ds_read_b128 delivers two coefficients
// to where the fused multiply-add wants them and costs the vector ALU nothing.  The arithmetic is that of sincos_fast_f64
// (general form), pair_term_fast and acos_r in pstat_math.h, operation for operation.
enum { K_2OPI = 0, K_PIO2_HI, K_PIO2_MID, K_S6, K_S5, K_S4, K_S3, K_S2, K_S1, K_C6, K_C5, K_C4, K_C3, K_C2, K_C1, K_R375, K_M3, K_INV4PI,
       K_A0, K_PIO2 = K_A0 + 13, K_PI, NK };
__constant__ double KINIT[NK] = {
    6.36619772367581382433e-01, 1.57079632679489655800e+00, 6.12323399573676603587e-17,
    1.58969099521155010221e-10, -2.50507602534068634195e-08, 2.75573137070700676789e-06, -1.98412698298579493134e-04,
    8.33333333332248946124e-03, -1.66666666666666324348e-01,
    -1.13596475577881948265e-11, 2.08757232129817482790e-09, -2.75573143513906633035e-07, 2.48015872894767294178e-05,
    -1.38888888888741095749e-03, 4.16666666666666019037e-02,
    0.375, -3.0, 0.0795774715459476679,
    2.87578513674215663354e-02, -1.48518870712472036977e-02, 1.74008794426940213707e-02, 5.45750671864035814818e-03,
    1.03228143501857792808e-02, 1.14791774151849056834e-02, 1.39712129735529329289e-02, 1.73523927208699725588e-02,
    2.23721729421498885526e-02, 3.03819441385312465076e-02, 4.46428571463554288434e-02, 7.49999999999843292020e-02,
    1.66666666666666685170e-01,
    1.57079632679489661923, 3.14159265358979323846};

__device__ __forceinline__ void sincos_tab(double x, const double *kt, double *s, double *c) {
  if (!(fabs(x) < PSTAT_PHI_FOLD)) {   // fold by whole turns (no chain gets here: see sincos_fast_f64)
    const double t = rint(x * 1.59154943091895345609e-01);
    x = __builtin_fma(-t, 2.44929359829470641435e-16, __builtin_fma(-t, 6.28318530717958623200e+00, x));
  }
  const double k = rint(x * kt[K_2OPI]);
  const double r = __builtin_fma(-k, kt[K_PIO2_MID], __builtin_fma(-k, kt[K_PIO2_HI], x));
  const double z = r * r;
  const double ps = __builtin_fma(z, __builtin_fma(z, __builtin_fma(z, __builtin_fma(z, __builtin_fma(z, kt[K_S6], kt[K_S5]), kt[K_S4]), kt[K_S3]), kt[K_S2]), kt[K_S1]);
  const double pc = __builtin_fma(z, __builtin_fma(z, __builtin_fma(z, __builtin_fma(z, __builtin_fma(z, kt[K_C6], kt[K_C5]), kt[K_C4]), kt[K_C3]), kt[K_C2]), kt[K_C1]);
  const uint32_t q = (uint32_t)(int)k;
  const uint32_t odd = q << 31;
  const uint32_t m_kc = (q >> 1) << 31;
  const uint32_t m_ks = m_kc ^ odd;
  const double rs = __hiloint2double((int)(__double2hiint(r) ^ m_ks), __double2loint(r));
  const double ks = __builtin_fma(rs * z, ps, rs);
  const double kc0 = __builtin_fma(z, __builtin_fma(z, pc, -0.5), 1.0);
  const double kc = __hiloint2double((int)(__double2hiint(kc0) ^ m_kc), __double2loint(kc0));
  const bool swap = (int)odd < 0;
  *s = swap ? kc : ks;
  *c = swap ? ks : kc;
}
__device__ __forceinline__ double pair_term_tab(double rx, double ry, double rz, double mix, double miy, double miz, double mjx,
                                                double mjy, double mjz, const double *kt) {
  const double r2 = __builtin_fma(rz, rz, __builtin_fma(ry, ry, rx * rx));
  const double y0 = __builtin_amdgcn_rsq(r2);
  const double e = __builtin_fma(-(r2 * y0), y0, 1.0);
  const double y = __builtin_fma(y0 * e, __builtin_fma(e, kt[K_R375], 0.5), y0);       // rsqrt_f64
  const double ir2 = y * y;
  const double mimj = __builtin_fma(miz, mjz, __builtin_fma(miy, mjy, mix * mjx));
  const double mir = __builtin_fma(miz, rz, __builtin_fma(miy, ry, mix * rx));
  const double mjr = __builtin_fma(mjz, rz, __builtin_fma(mjy, ry, mjx * rx));
  const double num = __builtin_fma(kt[K_M3] * ir2, mir * mjr, mimj);
  return num * (ir2 * y) * kt[K_INV4PI];
}
__device__ __forceinline__ double acos_tab(const double x, const double *kt) {
  const double a = fabs(x);
  const bool big = a >= 0.5;
  const double z = big ? __builtin_fma(a, -0.5, 0.5) : a * a;
  double p = kt[K_A0];
#pragma unroll
  for (int i = 1; i < 13; ++i) p = __builtin_fma(p, z, kt[K_A0 + i]);
  const double zp = z * p;
  const double y = __builtin_amdgcn_rsq(z);
  const double s0 = z * y, h0 = 0.5 * y;
  const double r = __builtin_fma(-s0, h0, 0.5);
  const double s1 = __builtin_fma(s0, r, s0), h1 = __builtin_fma(h0, r, h0);
  double sq = __builtin_fma(__builtin_fma(-s1, s1, z), h1, s1);
  sq = z == 0.0 ? 0.0 : sq;
  const double t = big ? sq : x;
  const double as = __builtin_fma(t, zp, t);
  const double small = kt[K_PIO2] - as;
  const double two = as + as;
  const double bigv = x < 0.0 ? kt[K_PI] - two : two;
  return big ? bigv : small;
}

}  // namespace

}  // namespace pstat
