// pstat_blocking.hip -- blocked standard errors (Flyvbjerg-Petersen) of batch means, on the device.
//
// Two kernels and their launchers; the estimator they state is the normative one of DESIGN.md section 3.12 (its numpy twin
// is tests/blocking_ref.py):
//   series_batches    the recorded rows of a series (cumulative reduction vectors, launch_record) -> the compact matrix of
//                     batch means x[N][ncases * PSTAT_NQ]: differences of consecutive rows' sums, per chain and step;
//   blocking_columns  x[N][ncols] -> per column the mean, the blocked standard error picked by the maximum rule, its own
//                     uncertainty, the statistical inefficiency, the level picked and the convergence flag, and se_l of
//                     every level.
// One wavefront owns one column: lanes stride over the batches, sums are per-lane partials in order of the batch index
// followed by wave_sum's tree, so a result depends on the input only.  Level 0 is read from memory twice (mean, then
// deviations) and folded into level 1 in LDS while it is read; every further level is folded in place.  Up to four adjacent
// columns share a workgroup (their strided level-0 reads share cache lines) when the LDS for N / 2 doubles per column
// allows.  Built with -ffp-contract=off: a batch mean is the same double here and in the twin.  No inline assembly.
#include <hip/hip_runtime.h>

#include "../../include/pstat.h"
#include "pstat_device.h"

namespace pstat {

namespace {

constexpr int NQ = PSTAT_NQ;
constexpr int BLOCKING_LDS = 160 * 1024;   // LDS of a CU: level 1 of one column must fit it
constexpr int BLOCKING_WAVES = 4;          // columns per workgroup, at most
constexpr int BATCH_THREADS = 256;

struct BatchArgs {
  int64_t row0;       // the row of batch 0
  int64_t nbatches;
  int64_t ncases;
  int64_t steps0;     // steps recorded at row0
  int64_t d;          // the rows' common spacing in steps
  int32_t zero_base;  // batch 0's baseline is the empty average (S = 0), not row0 - 1
};

// thread e = (b, k, q), q fastest: consecutive threads read along the PSTAT_NRED doubles of one (row, case)
__global__ __launch_bounds__(BATCH_THREADS) void series_batches(const double *__restrict__ red, BatchArgs a,
                                                                double *__restrict__ x) {
  const int64_t ncols = a.ncases * NQ;
  const int64_t e = (int64_t)blockIdx.x * BATCH_THREADS + threadIdx.x;
  if (e >= a.nbatches * ncols) return;
  const int64_t b = e / ncols, col = e - b * ncols;
  const int64_t k = col / NQ;
  const int q = (int)(col - k * NQ);
  const int64_t r = a.row0 + b;
  const double *now = red + (r * a.ncases + k) * PSTAT_NRED;
  const double s_now = now[1 + q] * (double)(a.steps0 + b * a.d);
  double s_prev = 0.0;
  if (b > 0 || !a.zero_base) s_prev = (now - a.ncases * PSTAT_NRED)[1 + q] * (double)(a.steps0 + (b - 1) * a.d);
  x[e] = (s_now - s_prev) / ((double)a.d * now[0]);
}

// every lane's stores to LDS are visible to every lane of the wave afterwards
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ double wave_total(const double partial) { return __shfl(wave_sum(partial), 0, 64); }

// The choice among the levels, fed in order of l: the eligible level of largest se, the lowest on ties;
// `below` is the se of the level under the one picked.
struct Choice {
  double se0 = 0.0, se = -1.0, n = 0.0, below = 0.0, prev = 0.0;
  int level = -1, last = -1, bad = 0;
  __device__ void level_done(const int l, const int64_t nl, const double se_l, const int min_blocks) {
    if (l == 0) se0 = se_l;
    if (nl >= min_blocks) {
      last = l;
      if (not_finite(se_l)) bad = 1;
      if (se_l > se) { se = se_l; level = l; n = (double)nl; below = prev; }
    }
    prev = se_l;
  }
  // 0: the level picked is the last eligible one and the curve was still rising into it by more than its own uncertainty
  // (or it is the only one: nothing to judge by)
  __device__ bool converged(const double dse) const { return !(level == last && (level == 0 || se - below > dse)); }
};

__global__ __launch_bounds__(64 * BLOCKING_WAVES) void blocking_columns(const double *__restrict__ x, const int64_t N,
                                                                        const int64_t ncols, const int64_t stride,
                                                                        const int min_blocks, double *__restrict__ out,
                                                                        double *__restrict__ levels) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t c = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
  if (c >= ncols) return;   // (waves never meet at a workgroup barrier)
  const int64_t n1 = N / 2;
  double *const v = lds + (int64_t)wave * n1;   // this column's level l >= 1, v[0 .. N_l)
  const double *const col = x + c;
  Choice ch;

  // level 0, pass 1: the mean, and level 1 into LDS
  double p = 0.0;
  for (int64_t j = lane; j < n1; j += 64) {
    const double a = col[2 * j * stride], b = col[(2 * j + 1) * stride];
    p += a;
    p += b;
    v[j] = 0.5 * (a + b);
  }
  if ((N & 1) && lane == 0) p += col[(N - 1) * stride];
  const double mean0 = wave_total(p) / (double)N;
  // pass 2: the deviations
  p = 0.0;
  for (int64_t j = lane; j < N; j += 64) {
    const double dx = col[j * stride] - mean0;
    p += dx * dx;
  }
  double se = sqrt(wave_total(p) / (double)(N - 1) / (double)N);
  ch.level_done(0, N, se, min_blocks);
  if (levels && lane == 0) levels[c * PSTAT_BLOCK_LEVELS] = se;
  wave_sync();

  int l = 1;
  for (int64_t nl = n1; l < PSTAT_BLOCK_LEVELS; ++l) {
    if (nl < 2) break;
    p = 0.0;
    for (int64_t j = lane; j < nl; j += 64) p += v[j];
    const double m = wave_total(p) / (double)nl;
    p = 0.0;
    for (int64_t j = lane; j < nl; j += 64) {
      const double dx = v[j] - m;
      p += dx * dx;
    }
    se = sqrt(wave_total(p) / (double)(nl - 1) / (double)nl);
    ch.level_done(l, nl, se, min_blocks);
    if (levels && lane == 0) levels[c * PSTAT_BLOCK_LEVELS + l] = se;
    // fold in place: the 64 values written in one round lie below everything a later round reads, and within a round
    // every lane has read before any lane writes
    const int64_t nn = nl / 2;
    for (int64_t base = 0; base < nn; base += 64) {
      const int64_t j = base + lane;
      double f = 0.0;
      if (j < nn) f = 0.5 * (v[2 * j] + v[2 * j + 1]);
      wave_sync();
      if (j < nn) v[j] = f;
      wave_sync();
    }
    nl = nn;
  }
  if (levels && lane == 0)
    for (; l < PSTAT_BLOCK_LEVELS; ++l) levels[c * PSTAT_BLOCK_LEVELS + l] = 0.0;

  if (lane == 0) {
    double *o = out + c * PSTAT_EB_FIELDS;
    const double nan = __builtin_nan("");
    o[PSTAT_EB_MEAN] = mean0;
    if (ch.bad) {
      o[PSTAT_EB_STDERR] = nan; o[PSTAT_EB_STDERR_ERR] = nan; o[PSTAT_EB_INEFFICIENCY] = nan;
      o[PSTAT_EB_LEVEL] = -1.0; o[PSTAT_EB_CONVERGED] = 0.0;
    } else if (ch.se0 == 0.0) {   // a constant column
      o[PSTAT_EB_STDERR] = 0.0; o[PSTAT_EB_STDERR_ERR] = 0.0; o[PSTAT_EB_INEFFICIENCY] = 1.0;
      o[PSTAT_EB_LEVEL] = 0.0; o[PSTAT_EB_CONVERGED] = 1.0;
    } else {
      const double ratio = ch.se / ch.se0;
      const double dse = ch.se / sqrt(2.0 * (ch.n - 1.0));
      o[PSTAT_EB_STDERR] = ch.se;
      o[PSTAT_EB_STDERR_ERR] = dse;
      o[PSTAT_EB_INEFFICIENCY] = ratio * ratio;
      o[PSTAT_EB_LEVEL] = (double)ch.level;
      o[PSTAT_EB_CONVERGED] = ch.converged(dse) ? 1.0 : 0.0;
    }
  }
}

}  // namespace

// level 1 of the longest column is the whole LDS of a CU
static_assert(PSTAT_BLOCK_MAX_BATCHES / 2 * sizeof(double) <= BLOCKING_LDS, "PSTAT_BLOCK_MAX_BATCHES of include/pstat.h");
int64_t blocking_max_batches() { return PSTAT_BLOCK_MAX_BATCHES; }

hipError_t launch_series_batches(const double *red, int64_t row0, int64_t nbatches, int64_t ncases, int64_t steps0, int64_t d,
                                 int zero_base, double *x, hipStream_t stream) {
  const BatchArgs a{row0, nbatches, ncases, steps0, d, zero_base};
  const int64_t elems = nbatches * ncases * NQ;
  hipLaunchKernelGGL(series_batches, dim3((unsigned)((elems + BATCH_THREADS - 1) / BATCH_THREADS)), dim3(BATCH_THREADS), 0,
                     stream, red, a, x);
  return hipGetLastError();
}

hipError_t launch_blocking(const double *x, int64_t nbatches, int64_t ncols, int64_t stride, int min_blocks, double *out,
                           double *levels, hipStream_t stream) {
  const int64_t col_bytes = (nbatches / 2) * (int64_t)sizeof(double);   // >= 8: nbatches >= 2
  if (nbatches < 2 || nbatches > blocking_max_batches()) return hipErrorInvalidValue;
  int64_t waves = BLOCKING_LDS / col_bytes;
  if (waves > BLOCKING_WAVES) waves = BLOCKING_WAVES;
  if (waves > ncols) waves = ncols;
  const size_t lds = (size_t)(waves * col_bytes);
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void *)blocking_columns, hipFuncAttributeMaxDynamicSharedMemorySize, BLOCKING_LDS);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(blocking_columns, dim3((unsigned)((ncols + waves - 1) / waves)), dim3((unsigned)(64 * waves)), lds, stream,
                     x, nbatches, ncols, stride, min_blocks, out, levels);
  return hipGetLastError();
}

}  // namespace pstat
