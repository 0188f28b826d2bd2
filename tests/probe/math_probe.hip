// math_probe.hip -- test infrastructure: one device function of polymer_stats_amd/csrc/pstat_math.h or pstat_math_tab.h per
// launch, one row of arguments in, one row of results out.  Built by polymer_stats_amd/csrc/Makefile into two shared objects
// next to this file, libmathprobe_off.so (the Makefile's FLAGS: -ffp-contract=off) and libmathprobe_fast.so (the flags of
// pstat_cluster_cw.o: -ffp-contract=fast, machine LICM off), so that tests/test_gpu_math.py measures the arithmetic under the
// contraction settings the kernels are built with.  Not part of libpstat.so and not a public interface.
//
//   int pstat_probe(int fn, const void *in, int in_cols, void *out, int out_cols, long n)
//
// in[n][in_cols] and out[n][out_cols] are HOST arrays of doubles, row-major.  Every argument and result travels as a double:
// a float argument is the double of that float (converted exactly on the device), a 32-bit word is its value as a double, a
// float or integer result is widened exactly.  n is a multiple of 64 (the Metropolis filter ballots over whole waves).
// Returns 0, the first HIP error code, or -1 for arguments that do not fit `fn` (tests/math_ref.py: FN has the column counts).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <utility>

#include "../../polymer_stats_amd/csrc/pstat_math.h"
#include "../../polymer_stats_amd/csrc/pstat_math_tab.h"

namespace {

using namespace pstat;

enum Fn {
  F_SINCOS = 0, F_SINCOS_BOUNDED, F_SINCOS_FOLD, F_SINCOS_NOFOLD, F_SINCOS_TAB,
  F_EXP, F_LOG, F_ACOS, F_ACOS_TAB, F_RSQRT, F_PAIR, F_PAIR_FAST, F_PAIR_TAB,
  F_SC_F32, F_EXP2F, F_RCPF, F_RSQF, F_ACOS_F32, F_PAIR_FAST_F32,
  F_U01_F32, F_SYM11_F32, F_SYM11_F64, F_BITS12, F_BITS24, F_Q16_THETA, F_Q16_PHI, F_Q16_DISP, F_EPS,
  F_METROPOLIS, F_METROPOLIS_STRAIGHT, F_COUNT
};
// columns in, columns out
constexpr int COLS[F_COUNT][2] = {
    {1, 2}, {1, 2}, {1, 2}, {1, 2}, {1, 2},
    {1, 1}, {1, 1}, {1, 1}, {1, 1}, {1, 1}, {9, 1}, {9, 1}, {9, 1},
    {1, 2}, {1, 1}, {1, 1}, {1, 1}, {1, 1}, {9, 1},
    {1, 1}, {1, 1}, {1, 1}, {1, 1}, {1, 1}, {1, 1}, {1, 1}, {2, 1}, {5, 1},
    {10, 3}, {10, 3}};

template <int FN>
__global__ __launch_bounds__(256) void probe_kernel(const double *__restrict__ in, double *__restrict__ out, const long n) {
  constexpr int IC = COLS[FN][0], OC = COLS[FN][1];
  constexpr bool TAB = FN == F_SINCOS_TAB || FN == F_ACOS_TAB || FN == F_PAIR_TAB;
  __shared__ double KT[NK];
  const double *kt = nullptr;
  if constexpr (TAB) {   // the table in LDS and its opaque index, as cluster_cw_kernel stages and addresses it
    if (threadIdx.x < NK) KT[threadIdx.x] = KINIT[threadIdx.x];
    __syncthreads();
    int kz = 0;
    asm volatile("" : "+v"(kz));
    kt = &KT[kz];
  }
  (void)kt;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;    // (n is a multiple of 64: whole waves leave)
  const double *a = in + i * IC;
  double *o = out + i * OC;
  auto word = [&](int j) -> uint32_t { return (uint32_t)a[j]; };
  if constexpr (FN == F_SINCOS) sincos_f64(a[0], &o[0], &o[1]);
  else if constexpr (FN == F_SINCOS_BOUNDED) sincos_fast_f64<true>(a[0], &o[0], &o[1]);
  else if constexpr (FN == F_SINCOS_FOLD) sincos_fast_f64<false, true>(a[0], &o[0], &o[1]);
  else if constexpr (FN == F_SINCOS_NOFOLD) sincos_fast_f64<false, false>(a[0], &o[0], &o[1]);
  else if constexpr (FN == F_SINCOS_TAB) sincos_tab(a[0], kt, &o[0], &o[1]);
  else if constexpr (FN == F_EXP) o[0] = exp_f64(a[0]);
  else if constexpr (FN == F_LOG) o[0] = log_f64(a[0]);
  else if constexpr (FN == F_ACOS) o[0] = acos_r(a[0]);
  else if constexpr (FN == F_ACOS_TAB) o[0] = acos_tab(a[0], kt);
  else if constexpr (FN == F_RSQRT) o[0] = rsqrt_f64(a[0]);
  else if constexpr (FN == F_PAIR) o[0] = pair_term<double>(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8]);
  else if constexpr (FN == F_PAIR_FAST) o[0] = pair_term_fast(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8]);
  else if constexpr (FN == F_PAIR_TAB) o[0] = pair_term_tab(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], kt);
  else if constexpr (FN == F_SC_F32) {
    float s, c;
    Ang<float>::sc((float)a[0], &s, &c);
    o[0] = (double)s; o[1] = (double)c;
  } else if constexpr (FN == F_EXP2F) o[0] = (double)__builtin_amdgcn_exp2f((float)a[0]);
  else if constexpr (FN == F_RCPF) o[0] = (double)__builtin_amdgcn_rcpf((float)a[0]);
  else if constexpr (FN == F_RSQF) o[0] = (double)__builtin_amdgcn_rsqf((float)a[0]);
  else if constexpr (FN == F_ACOS_F32) o[0] = (double)acos_r((float)a[0]);
  else if constexpr (FN == F_PAIR_FAST_F32)
    o[0] = (double)pair_term_fast((float)a[0], (float)a[1], (float)a[2], (float)a[3], (float)a[4], (float)a[5], (float)a[6],
                                  (float)a[7], (float)a[8]);
  else if constexpr (FN == F_U01_F32) o[0] = (double)u01<float>(word(0));
  else if constexpr (FN == F_SYM11_F32) o[0] = (double)sym11<float>(word(0));
  else if constexpr (FN == F_SYM11_F64) o[0] = sym11<double>(word(0));
  else if constexpr (FN == F_BITS12) o[0] = (double)bits12(word(0));
  else if constexpr (FN == F_BITS24) o[0] = (double)bits24(word(0));
  else if constexpr (FN == F_Q16_THETA) o[0] = (double)q16_theta_turns(word(0));
  else if constexpr (FN == F_Q16_PHI) o[0] = (double)q16_phi_turns(word(0));
  else if constexpr (FN == F_Q16_DISP) o[0] = (double)q16_disp((float)a[0], (float)a[1]);
  else if constexpr (FN == F_EPS) o[0] = eps_uniform(a[0] != 0.0, word(1), word(2), word(3), word(4));
  else {
    // the Metropolis test as metropolis_f64 poses it: x = dU (-1 / kT) + extra, num = st1, den = st0
    const double dU = a[0], kT = a[1], st1 = a[2], st0 = a[3], extra = a[4];
    const bool wide = a[5] != 0.0;
    const uint32_t weps = word(6), w0 = word(7), wphi = word(8), wth = word(9);
    const double ninv_kT = -1.0 / kT;
    bool called = false;
    const bool ok = metropolis_filter<FN == F_METROPOLIS_STRAIGHT>(dU * ninv_kT + extra, st1, st0, weps, [&]() -> bool {
      called = true;
      return metropolis_literal(dU, kT, st1, st0, extra, wide, weps, w0, wphi, wth);
    });
    o[0] = ok ? 1.0 : 0.0;
    o[1] = metropolis_literal(dU, kT, st1, st0, extra, wide, weps, w0, wphi, wth) ? 1.0 : 0.0;
    o[2] = called ? 1.0 : 0.0;
  }
}

template <int FN>
void launch(const double *in, double *out, long n) {
  hipLaunchKernelGGL(probe_kernel<FN>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, in, out, n);
}
using Launcher = void (*)(const double *, double *, long);
template <int... I> constexpr Launcher launcher_of(int fn, std::integer_sequence<int, I...>) {
  Launcher l = nullptr;
  ((fn == I ? (void)(l = &launch<I>) : (void)0), ...);
  return l;
}

}  // namespace

extern "C" int pstat_probe(int fn, const void *in, int in_cols, void *out, int out_cols, long n) {
  if (fn < 0 || fn >= F_COUNT || !in || !out || n <= 0 || n % 64 != 0 || n > (1L << 26)) return -1;
  if (in_cols != COLS[fn][0] || out_cols != COLS[fn][1]) return -1;
  const size_t bi = (size_t)n * in_cols * sizeof(double), bo = (size_t)n * out_cols * sizeof(double);
  double *din = nullptr, *dout = nullptr;
  hipError_t e = hipMalloc(&din, bi);
  if (e == hipSuccess) e = hipMalloc(&dout, bo);
  if (e == hipSuccess) e = hipMemcpy(din, in, bi, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    launcher_of(fn, std::make_integer_sequence<int, F_COUNT>{})(din, dout, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, dout, bo, hipMemcpyDeviceToHost);
  if (din) (void)hipFree(din);
  if (dout) (void)hipFree(dout);
  return (int)e;
}
