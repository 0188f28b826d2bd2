// pstat_series.hip -- the device-side recorder of the stepout time series (pstat_series_*, include/pstat.h).
//
// One launch appends one row for EVERY case of a handle: per case the PSTAT_NRED reduction vector that
// pstat_reduce_host would return, the 7 doubles of pstat_microstate for the case's first chain and, when asked for,
// that chain's 2n angles as pstat_chain_state returns them.  It reads the spilled DevState only and writes the series'
// own buffers only.
//
// The reduction vector is equal AS DOUBLES to what reduce_stage1 / reduce_stage2 (pstat_kernels.hip) produce for the
// same case, so the summation order is theirs:
//   stage 1   thread t of block b folds chains c0 + 256 b + t + 65536 j in order of j (m1 += v, m2 = fma(v, v, m2)),
//             wave_sum's shfl_down tree, then the block's four waves in order;
//   stage 2   lane i adds the partials of blocks i, i + 64, i + 128, i + 192 in that order, then the same tree.
// What is left out is additions of +0.0 only: a block (wave, lane) that holds no chain of the case contributes +0.0, and
// no sum here can be -0.0 (every accumulator starts from +0.0, and under round-to-nearest x + y is -0.0 only when both
// are), so x + 0.0 == x for every x that occurs.  Built like pstat_kernels.o, with -ffp-contract=off: the per-chain
// means are products rounded before they are added.
#include <hip/hip_runtime.h>

#include "../../include/pstat.h"
#include "pstat_device.h"

namespace pstat {

namespace {

constexpr int RED_BLOCKS = 256;    // the grid of reduce_stage1
constexpr int RED_THREADS = 256;   // and its workgroup: the chain -> (block, thread, j) map is part of the result
constexpr int NQ = PSTAT_NQ;
constexpr int NX = PSTAT_NX;
constexpr int NP = 2 * NQ + NX;
static_assert(1 + NP == PSTAT_NRED, "reduction layout of include/pstat.h");

struct RecordArgs {
  int64_t steps;             // the handle's steps_recorded at this row
  int64_t chains_per_case;
  int64_t ncases;
  int64_t n;
  int32_t umbrella;
  int32_t precision;         // storage format of DevState::ang
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// One chain's contribution, folded into a thread's accumulators exactly as the loop body of reduce_stage1 does.
__device__ __forceinline__ void fold_chain(const DevState &S, const RecordArgs &a, const CaseConst &cc, const int64_t c,
                                           double (&m1)[NQ], double (&m2)[NQ], double (&mx)[NX]) {
  const int64_t C = S.C;
  const double norm = a.umbrella ? S.wnorm[c] : (double)a.steps;
  const double inv = norm != 0.0 ? 1.0 / norm : 0.0;
  double v[NQ];
  v[PSTAT_R1] = S.sums[S_R1 * C + c]; v[PSTAT_R2] = S.sums[S_R2 * C + c]; v[PSTAT_R3] = S.sums[S_R3 * C + c];
  v[PSTAT_R1SQ] = S.sums[S_R1SQ * C + c]; v[PSTAT_R2SQ] = S.sums[S_R2SQ * C + c];
  v[PSTAT_R3SQ] = S.sums[S_R3SQ * C + c];
  v[PSTAT_RSQ] = v[PSTAT_R1SQ] + v[PSTAT_R2SQ] + v[PSTAT_R3SQ];
  v[PSTAT_P1] = S.sums[S_P1 * C + c]; v[PSTAT_P2] = S.sums[S_P2 * C + c]; v[PSTAT_P3] = S.sums[S_P3 * C + c];
  v[PSTAT_P1SQ] = S.sums[S_P1SQ * C + c]; v[PSTAT_P2SQ] = S.sums[S_P2SQ * C + c];
  v[PSTAT_P3SQ] = S.sums[S_P3SQ * C + c];
  v[PSTAT_PSQ] = v[PSTAT_P1SQ] + v[PSTAT_P2SQ] + v[PSTAT_P3SQ];
  v[PSTAT_U] = S.sums[S_U * C + c]; v[PSTAT_USQ] = S.sums[S_USQ * C + c];
#pragma unroll
  for (int q = 0; q < PSTAT_NOBS; ++q) v[q] *= inv;
  v[16] = a.steps > 0 ? (double)S.nacc_total[c] / (double)a.steps : 0.0;
  v[17] = S.sums[S_C2 * C + c] * inv;
  v[18] = S.sums[S_PSI * C + c] * inv;
#pragma unroll
  for (int q = 0; q < NQ; ++q) { m1[q] += v[q]; m2[q] = fma(v[q], v[q], m2[q]); }
  mx[0] += (double)S.nanrej[c];
  const double mu_max = fmax(fmax(fabs(cc.K1), fabs(cc.K2)) * fabs(cc.E0), fabs(cc.mu));
  const double per_monomer = cc.kT + 0.5 * fabs(cc.E0) * mu_max + fabs(cc.b) * (fabs(cc.Fx) + fabs(cc.Fz));
  mx[1] += !(fabs(S.obs[OBS_U * C + c]) <= 1e3 * (double)a.n * per_monomer) ? 1.0 : 0.0;
}

// angle j (theta for j < n, then phi) of chain c in radians: the conversions of pstat_chain_state, each one exact scaling
__device__ __forceinline__ double angle_radians(const DevState &S, const RecordArgs &a, const int64_t j, const int64_t c) {
  const int64_t at = j * S.C + c;
  if (a.precision == PSTAT_F64) return ((const double *)S.ang)[at];
  if (a.precision == PSTAT_F32) return (double)((const float *)S.ang)[at] * 6.28318530717958647692;
  return (j < a.n ? 3.14159265358979323846 : 6.28318530717958647692) * ((double)((const uint16_t *)S.ang)[at] + 0.5) / 65536.0;
}

// microstate and angles of chain c0, the case's first: `nthreads` threads of which this is `t` write case k's slices
__device__ __forceinline__ void record_chain(const DevState &S, const RecordArgs &a, const int64_t k, const int64_t c0, const int t,
                                             const int nthreads, double *__restrict__ micro, double *__restrict__ angles) {
  if (t < 7) micro[k * 7 + t] = S.obs[(int64_t)t * S.C + c0];   // OBS_R1 .. OBS_U: the order of pstat_microstate
  if (angles)
    for (int64_t j = t; j < 2 * a.n; j += nthreads) angles[k * 2 * a.n + j] = angle_radians(S, a, j, c0);
}

// Cases of up to 64 chains (the sweeps: 1-25 chains per case): one wavefront per case, four cases per workgroup.  Lane t
// holds chain t of the case, which is thread t of block 0, wave 0 of reduce_stage1; every other wave and block is empty.
__global__ __launch_bounds__(RED_THREADS) void record_wave_per_case(DevState S, RecordArgs a, const CaseConst *__restrict__ cases,
                                                                    double *__restrict__ red, double *__restrict__ micro,
                                                                    double *__restrict__ angles) {
  const int lane = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * (RED_THREADS / 64) + (threadIdx.x >> 6);
  if (k >= a.ncases) return;
  const int64_t c0 = k * a.chains_per_case;
  double m1[NQ], m2[NQ], mx[NX] = {0, 0};
#pragma unroll
  for (int q = 0; q < NQ; ++q) { m1[q] = 0; m2[q] = 0; }
  if (lane < a.chains_per_case) fold_chain(S, a, cases[k], c0 + lane, m1, m2, mx);
  // lane 1 + q keeps output q, so that the row leaves in one contiguous store
  double mine = (double)a.chains_per_case;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const double s1 = __shfl(wave_sum(m1[q]), 0, 64), s2 = __shfl(wave_sum(m2[q]), 0, 64);
    if (lane == 1 + q) mine = s1;
    if (lane == 1 + NQ + q) mine = s2;
  }
#pragma unroll
  for (int q = 0; q < NX; ++q) {
    const double s = __shfl(wave_sum(mx[q]), 0, 64);
    if (lane == 1 + 2 * NQ + q) mine = s;
  }
  if (lane < PSTAT_NRED) red[k * PSTAT_NRED + lane] = mine;
  record_chain(S, a, k, c0, lane, 64, micro, angles);
}

// Larger cases: one workgroup per case plays the blocks of reduce_stage1 that hold chains of it one after the other and
// keeps reduce_stage2's 64 strided sums in LDS as the partials arrive (block b goes to lane b % 64, in order of b).
__global__ __launch_bounds__(RED_THREADS) void record_group_per_case(DevState S, RecordArgs a, const CaseConst *__restrict__ cases,
                                                                     double *__restrict__ red, double *__restrict__ micro,
                                                                     double *__restrict__ angles) {
  __shared__ double waves[RED_THREADS / 64][NP];
  __shared__ double strided[64][NP];
  __shared__ double row[PSTAT_NRED];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int64_t k = blockIdx.x;
  const int64_t c0 = k * a.chains_per_case, c1 = c0 + a.chains_per_case;
  const CaseConst cc = cases[k];
  for (int i = t; i < 64 * NP; i += RED_THREADS) (&strided[0][0])[i] = 0.0;
  const int64_t want = (a.chains_per_case + RED_THREADS - 1) / RED_THREADS;
  const int nblocks = (int)(want < RED_BLOCKS ? want : RED_BLOCKS);
  for (int b = 0; b < nblocks; ++b) {
    double m1[NQ], m2[NQ], mx[NX] = {0, 0};
#pragma unroll
    for (int q = 0; q < NQ; ++q) { m1[q] = 0; m2[q] = 0; }
    for (int64_t c = c0 + (int64_t)b * RED_THREADS + t; c < c1; c += (int64_t)RED_BLOCKS * RED_THREADS)
      fold_chain(S, a, cc, c, m1, m2, mx);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const double s1 = wave_sum(m1[q]), s2 = wave_sum(m2[q]);
      if (lane == 0) { waves[wave][q] = s1; waves[wave][NQ + q] = s2; }
    }
#pragma unroll
    for (int q = 0; q < NX; ++q) {
      const double s = wave_sum(mx[q]);
      if (lane == 0) waves[wave][2 * NQ + q] = s;
    }
    __syncthreads();
    if (t < NP) {
      double partial = 0;
#pragma unroll
      for (int w = 0; w < RED_THREADS / 64; ++w) partial += waves[w][t];
      strided[b & 63][t] += partial;
    }
    __syncthreads();   // `waves` is rewritten by the next block
  }
  for (int q = wave; q < NP; q += RED_THREADS / 64) {
    const double s = wave_sum(strided[lane][q]);
    if (lane == 0) row[1 + q] = s;
  }
  if (t == 0) row[0] = (double)a.chains_per_case;
  __syncthreads();
  if (t < PSTAT_NRED) red[k * PSTAT_NRED + t] = row[t];
  record_chain(S, a, k, c0, t, RED_THREADS, micro, angles);
}

}  // namespace

hipError_t launch_record(const LaunchCfg &cfg, const SweepArgs &a, const DevState &s, const CaseConst *cases,
                         int64_t steps_recorded, double *red, double *micro, double *angles, hipStream_t stream) {
  const RecordArgs r{steps_recorded, a.chains_per_case, a.ncases, a.n, cfg.umbrella, cfg.precision};
  if (a.chains_per_case <= 64)
    hipLaunchKernelGGL(record_wave_per_case, dim3((unsigned)((a.ncases + 3) / 4)), dim3(RED_THREADS), 0, stream, s, r, cases,
                       red, micro, angles);
  else
    hipLaunchKernelGGL(record_group_per_case, dim3((unsigned)a.ncases), dim3(RED_THREADS), 0, stream, s, r, cases, red, micro,
                       angles);
  return hipGetLastError();
}

}  // namespace pstat
