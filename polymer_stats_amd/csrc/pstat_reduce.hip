// pstat_reduce.hip -- the ensemble reduction: per-chain running sums -> the PSTAT_NRED vector of include/pstat.h.
//
// Three readers share the statements of this file: launch_reduce (reduce_stage1 / reduce_stage2: pstat_reduce_host, summaries),
// launch_record (the device-side recorder of the stepout time series, pstat_series_*: one launch appends, for EVERY case of a
// handle, the vector launch_reduce would give, the 7 doubles of pstat_microstate for the case's first chain and, when asked
// for, that chain's 2n angles) and the host loops of pstat_chain_means / pstat_chain_state.  The kernels read the spilled
// DevState only; the recorder writes the series' own buffers only.
//
// The summation order is part of the result and is stated by the shared code below: fold_chain, wave_partials,
// block_partial, stage2_*.  A recorded row is equal AS DOUBLES to launch_reduce's vector although the recorder skips the
// blocks, waves and lanes that hold no chain of the case: what it leaves out is additions of +0.0 only, and no sum here can
// be -0.0 (every accumulator starts from +0.0, and under round-to-nearest x + y is -0.0 only when both are), so
// x + 0.0 == x for every x that occurs.  Built with -ffp-contract=off: the per-chain means are products rounded before
// they are added.
#include <hip/hip_runtime.h>

#include "../../include/pstat.h"
#include "pstat_device.h"
#include "pstat_math.h"

namespace pstat {

namespace {

constexpr int RED_BLOCKS = 256;    // the grid of reduce_stage1
constexpr int RED_THREADS = 256;   // and its workgroup: the chain -> (block, thread, j) map is part of the result
constexpr int NQ = PSTAT_NQ;       // 16 observables + acceptance ratio + the clustering main's two extras
constexpr int NX = PSTAT_NX;       // plain sums: non-finite-energy rejections, collapsed chains (pstat.h)
constexpr int NP = 2 * NQ + NX;    // one partial: m1[NQ] (sum of v), m2[NQ] (sum of v^2), mx[NX]; out[1 + i] = sum of p[i]
static_assert(1 + NP == PSTAT_NRED, "reduction layout of include/pstat.h");

struct ReduceArgs {
  int64_t c0, c1;            // reduce_stage1: the chains [c0, c1) to fold (the recorder folds each case's own)
  int64_t steps;             // the handle's steps_recorded
  int64_t chains_per_case;
  int64_t ncases;
  int64_t n;
  int32_t umbrella;
  int32_t elem;              // the recorder's angles: bytes per stored angle of DevState::ang
};

// the 16 sums in the order of include/pstat.h from the S_* rows of a [NSUMS][stride] array; r.r and p.p are the sums of
// their components
__host__ __device__ __forceinline__ void abi_sums(const double *sums, const int64_t stride, double *v) {
  v[PSTAT_R1] = sums[S_R1 * stride]; v[PSTAT_R2] = sums[S_R2 * stride]; v[PSTAT_R3] = sums[S_R3 * stride];
  v[PSTAT_R1SQ] = sums[S_R1SQ * stride]; v[PSTAT_R2SQ] = sums[S_R2SQ * stride]; v[PSTAT_R3SQ] = sums[S_R3SQ * stride];
  v[PSTAT_RSQ] = v[PSTAT_R1SQ] + v[PSTAT_R2SQ] + v[PSTAT_R3SQ];
  v[PSTAT_P1] = sums[S_P1 * stride]; v[PSTAT_P2] = sums[S_P2 * stride]; v[PSTAT_P3] = sums[S_P3 * stride];
  v[PSTAT_P1SQ] = sums[S_P1SQ * stride]; v[PSTAT_P2SQ] = sums[S_P2SQ * stride]; v[PSTAT_P3SQ] = sums[S_P3SQ * stride];
  v[PSTAT_PSQ] = v[PSTAT_P1SQ] + v[PSTAT_P2SQ] + v[PSTAT_P3SQ];
  v[PSTAT_U] = sums[S_U * stride]; v[PSTAT_USQ] = sums[S_USQ * stride];
}

// one chain's mean vector v[NQ]: what the reduction folds and pstat_chain_means returns
__host__ __device__ __forceinline__ void chain_mean(const double *sums, const int64_t stride, const double norm,
                                                    const int64_t steps, const int64_t nacc, double *v) {
  const double inv = norm != 0.0 ? 1.0 / norm : 0.0;
  abi_sums(sums, stride, v);
#pragma unroll
  for (int q = 0; q < PSTAT_NOBS; ++q) v[q] *= inv;
  v[16] = steps > 0 ? (double)nacc / (double)steps : 0.0;
  v[17] = sums[S_C2 * stride] * inv;    // sum cos^2(theta)
  v[18] = sums[S_PSI * stride] * inv;   // mean bond angle
}

// chain c of case `cc`, folded into a thread's partial
__device__ __forceinline__ void fold_chain(const DevState &S, const ReduceArgs &a, const CaseConst &cc, const int64_t c,
                                           double (&p)[NP]) {
  const int64_t C = S.C;
  double v[NQ];
  chain_mean(S.sums + c, C, a.umbrella ? S.wnorm[c] : (double)a.steps, a.steps, S.nacc_total[c], v);
#pragma unroll
  for (int q = 0; q < NQ; ++q) { p[q] += v[q]; p[NQ + q] = fma(v[q], v[q], p[NQ + q]); }
  p[2 * NQ] += (double)S.nanrej[c];
  // collapsed: |U| of the current configuration is 1e3 times beyond what n separated monomers can hold in field,
  // force and thermal energy -- only a 1/r^3 contact gets there (pstat.h, pstat_summary.chains_collapsed)
  const double mu_max = fmax(fmax(fabs(cc.K1), fabs(cc.K2)) * fabs(cc.E0), fabs(cc.mu));
  const double per_monomer = cc.kT + 0.5 * fabs(cc.E0) * mu_max + fabs(cc.b) * (fabs(cc.Fx) + fabs(cc.Fz));
  p[2 * NQ + 1] += !(fabs(S.obs[OBS_U * C + c]) <= 1e3 * (double)a.n * per_monomer) ? 1.0 : 0.0;
}

// a block's threads' partials -> its four waves' sums (shfl_down tree, lane 0 writes); __syncthreads, then threads
// t < NP take block_partial: the waves in order, from 0.0
__device__ __forceinline__ void wave_partials(const double (&p)[NP], double (&waves)[RED_THREADS / 64][NP]) {
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const double s = wave_sum(p[i]);
    if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6][i] = s;
  }
}
__device__ __forceinline__ double block_partial(const double (&waves)[RED_THREADS / 64][NP], const int t) {
  double s = 0;
#pragma unroll
  for (int w = 0; w < RED_THREADS / 64; ++w) s += waves[w][t];
  return s;
}

// Stage 2: lane i adds the partials of blocks i, i + 64, i + 128, i + 192 in that order, from 0.0; wave_sum's tree over the
// 64 lanes follows.  stage2_read takes all partials at the end (reduce_stage2), stage2_add is handed them in order of b.
__device__ __forceinline__ double stage2_read(const double *__restrict__ partial, const int q, const int lane) {
  double s = 0;
  for (int b = lane; b < RED_BLOCKS; b += 64) s += partial[b * NP + q];
  return s;
}
__device__ __forceinline__ void stage2_add(double (&strided)[64][NP], const int b, const int q, const double partial) {
  strided[b & 63][q] += partial;
}

// stage 1: thread t of block b folds chains c0 + 256 b + t + 65536 j in order of j; partial[block][NP] (deterministic)
__global__ __launch_bounds__(RED_THREADS) void reduce_stage1(DevState S, ReduceArgs a, const CaseConst *__restrict__ cases,
                                                             double *__restrict__ partial) {
  __shared__ double waves[RED_THREADS / 64][NP];
  double p[NP] = {};
  for (int64_t c = a.c0 + (int64_t)blockIdx.x * RED_THREADS + threadIdx.x; c < a.c1; c += (int64_t)RED_BLOCKS * RED_THREADS)
    fold_chain(S, a, cases[c / a.chains_per_case], c, p);
  wave_partials(p, waves);
  __syncthreads();
  if (threadIdx.x < NP) partial[blockIdx.x * NP + threadIdx.x] = block_partial(waves, threadIdx.x);
}

// stage 2: one wave per output folds the RED_BLOCKS partials
__global__ __launch_bounds__(64) void reduce_stage2(const double *__restrict__ partial, int64_t nchains,
                                                    double *__restrict__ out) {
  const int q = blockIdx.x;  // 0 .. NP-1
  const double s = wave_sum(stage2_read(partial, q, threadIdx.x));
  if (threadIdx.x == 0) {
    out[1 + q] = s;
    if (q == 0) out[0] = (double)nchains;
  }
}

// microstate and angles of chain c0, the case's first: `nthreads` threads of which this is `t` write case k's slices
__device__ __forceinline__ void record_chain(const DevState &S, const ReduceArgs &a, const int64_t k, const int64_t c0, const int t,
                                             const int nthreads, double *__restrict__ micro, double *__restrict__ angles) {
  if (t < 7) micro[k * 7 + t] = S.obs[(int64_t)t * S.C + c0];   // OBS_R1 .. OBS_U: the order of pstat_microstate
  if (angles)   // theta for j < n, then phi, as pstat_chain_state returns them
    for (int64_t j = t; j < 2 * a.n; j += nthreads) angles[k * 2 * a.n + j] = load_angle(S.ang, j * S.C + c0, a.elem, j < a.n);
}

// Cases of up to 64 chains (the sweeps: 1-25 chains per case): one wavefront per case, four cases per workgroup.  Lane t
// holds chain t of the case, which is thread t of block 0, wave 0 of reduce_stage1; every other wave and block is empty.
__global__ __launch_bounds__(RED_THREADS) void record_wave_per_case(DevState S, ReduceArgs a, const CaseConst *__restrict__ cases,
                                                                    double *__restrict__ red, double *__restrict__ micro,
                                                                    double *__restrict__ angles) {
  const int lane = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * (RED_THREADS / 64) + (threadIdx.x >> 6);
  if (k >= a.ncases) return;
  const int64_t c0 = k * a.chains_per_case;
  double p[NP] = {};
  if (lane < a.chains_per_case) fold_chain(S, a, cases[k], c0 + lane, p);
  // lane 1 + i keeps output 1 + i, so that the row leaves in one contiguous store
  double mine = (double)a.chains_per_case;
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const double s = __shfl(wave_sum(p[i]), 0, 64);
    if (lane == 1 + i) mine = s;
  }
  if (lane < PSTAT_NRED) red[k * PSTAT_NRED + lane] = mine;
  record_chain(S, a, k, c0, lane, 64, micro, angles);
}

// Larger cases: one workgroup per case plays the blocks of reduce_stage1 that hold chains of it one after the other and
// keeps reduce_stage2's 64 strided sums in LDS as the partials arrive.
__global__ __launch_bounds__(RED_THREADS) void record_group_per_case(DevState S, ReduceArgs a, const CaseConst *__restrict__ cases,
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
    double p[NP] = {};
    for (int64_t c = c0 + (int64_t)b * RED_THREADS + t; c < c1; c += (int64_t)RED_BLOCKS * RED_THREADS)
      fold_chain(S, a, cc, c, p);
    wave_partials(p, waves);
    __syncthreads();
    if (t < NP) stage2_add(strided, b, t, block_partial(waves, t));
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

size_t reduce_scratch_doubles() { return (size_t)RED_BLOCKS * NP; }

hipError_t launch_reduce(const DevState &s, int64_t c0, int64_t c1, int64_t steps_recorded,
                         int umbrella, const CaseConst *cases, int64_t chains_per_case, int64_t n,
                         double *partial, double *out, hipStream_t stream) {
  const ReduceArgs r{c0, c1, steps_recorded, chains_per_case, 0, n, umbrella, 0};
  hipLaunchKernelGGL(reduce_stage1, dim3(RED_BLOCKS), dim3(RED_THREADS), 0, stream, s, r, cases, partial);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(reduce_stage2, dim3(NP), dim3(64), 0, stream, partial, c1 - c0, out);
  return hipGetLastError();
}

hipError_t launch_record(const LaunchCfg &cfg, const SweepArgs &a, const DevState &s, const CaseConst *cases,
                         int64_t steps_recorded, double *red, double *micro, double *angles, hipStream_t stream) {
  const int32_t elem = cfg.precision == PSTAT_F64 ? 8 : (cfg.precision == PSTAT_Q16 ? 2 : 4);
  const ReduceArgs r{0, 0, steps_recorded, a.chains_per_case, a.ncases, a.n, cfg.umbrella, elem};
  if (a.chains_per_case <= 64)
    hipLaunchKernelGGL(record_wave_per_case, dim3((unsigned)((a.ncases + 3) / 4)), dim3(RED_THREADS), 0, stream, s, r, cases,
                       red, micro, angles);
  else
    hipLaunchKernelGGL(record_group_per_case, dim3((unsigned)a.ncases), dim3(RED_THREADS), 0, stream, s, r, cases, red, micro,
                       angles);
  return hipGetLastError();
}

void sums_in_abi_order(const double *sums, int64_t stride, double out[PSTAT_NOBS]) { abi_sums(sums, stride, out); }

void chain_means_host(const double *sums, const double *wnorm, const int64_t *nacc, int64_t steps, int64_t m, double *out) {
  for (int64_t k = 0; k < m; ++k) {
    double v[NQ];
    chain_mean(sums + k, m, wnorm ? wnorm[k] : (double)steps, steps, nacc[k], v);
    for (int q = 0; q < NQ; ++q) out[q * m + k] = v[q];
  }
}

}  // namespace pstat
