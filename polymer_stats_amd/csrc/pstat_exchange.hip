// pstat_exchange.hip -- replica exchange (parallel tempering) between the cases of one handle, on the device.
//
// THE EXCHANGE CONTRACT (restated, not shared, in tests/tempering_ref.py).
//   Ladder     a set of cases that differ in nothing but kT, seed and chain_id0.  Its rungs are the cases ordered by kT
//              ascending at open time, ties broken by case index.
//   Pairing    round t pairs rungs (2j + (t & 1), 2j + 1 + (t & 1)), j = 0, 1, ...; a rung without a partner sits the round
//              out.  Chain k of the lower rung's case a pairs with chain k of the upper rung's case b.  The round counter
//              starts at 0, advances by one per exchange call and is 32-bit.
//   Criterion  in f64, every operation rounded on its own:  d = (1 / kT_a - 1 / kT_b) * (U_a - U_b);
//              accept iff U_a and U_b are finite and (d >= 0 or u < exp(d)).  kT is the cases' CURRENT temperature.
//   Stream     o = Philox4x32-10(key = (seed_lo, seed_hi), ctr = (k, a, 0x7e3a9e0d, t)) with the tempering object's own
//              seed;  u = ((o[0] << 21) | (o[1] >> 11)) * 2^-53.  Nothing is drawn from the chains' generators: between
//              exchanges every trajectory is the step kernel's own.
//   Counters   attempted[a] += 1 for every (pair, k) of a round, accepted[a] += 1 for every accepted one: on the LOWER rung.
//
// What an accepted exchange moves between global chains a * per + k and b * per + k: every row of DevState::ang (both
// planes, in the handle's element size) and every row of DevState::obs -- a chain's whole configuration between launches
// (each home fills its LDS / DevState::work / registers from these two and spills back to them; a checkpoint image holds no
// more of a configuration than they do).  DevState::lag of both chains becomes 0: an accepted exchange is an accepted move of
// the acceptor with alpha = 1, whose cached log(pi) is the new configuration's own.  What stays with the temperature slot
// (the case): sums, wnorm, rng, stepsz, win, nacc_total, nanrej, uref.
//
// Two launches per round, ordered by the stream: exchange_decide writes one flag per (pair, k); exchange_swap reads the flags
// (never recomputes them: the swap changes the U they were computed from).  Lane t of either grid owns (pair, k) =
// (t / per, t % per), so consecutive lanes touch consecutive chains of both cases: every access to obs and ang is coalesced
// along C.  Pure memory traffic: no LDS, plain vector loads and stores, vector atomics for the counters (one per wave and
// case).  Built with -ffp-contract=off (there is nothing to contract in d, and it stays so).
#include <hip/hip_runtime.h>

#include "pstat_device.h"

namespace pstat {

namespace {

constexpr int XTHREADS = 64;

// one wave's contribution to counter[icase]: lanes of equal icase are folded before one of them adds
__device__ __forceinline__ void count_per_case(int64_t *counter, const int icase, const bool on) {
  // lanes of a wave span few cases (consecutive t): peel them off one case at a time
  uint64_t todo = __ballot(on);
  while (todo) {
    const int leader = __ffsll((unsigned long long)todo) - 1;
    const int which = __shfl(icase, leader, 64);
    const uint64_t same = __ballot(on && icase == which);
    if ((int)(threadIdx.x & 63) == leader)
      atomicAdd(reinterpret_cast<unsigned long long *>(counter + which), (unsigned long long)__popcll(same));
    todo &= ~same;
  }
}

__global__ __launch_bounds__(XTHREADS) void exchange_decide(const ExchangeArgs a, const double *__restrict__ obs,
                                                            const CaseConst *__restrict__ cases,
                                                            const int32_t *__restrict__ pairs, unsigned char *__restrict__ flags,
                                                            int64_t *__restrict__ attempted, int64_t *__restrict__ accepted) {
  const int64_t t = (int64_t)blockIdx.x * XTHREADS + threadIdx.x;
  const bool live = t < a.npairs * a.per;
  int ca = 0;
  bool ok = false;
  if (live) {
    const int64_t pair = t / a.per, k = t - pair * a.per;
    ca = pairs[2 * pair];
    const int cb = pairs[2 * pair + 1];
    const double Ua = obs[(int64_t)OBS_U * a.C + ca * a.per + k];
    const double Ub = obs[(int64_t)OBS_U * a.C + cb * a.per + k];
    const double d = (1.0 / cases[ca].kT - 1.0 / cases[cb].kT) * (Ua - Ub);
    uint32_t o[4];
    philox4x32_10((uint32_t)k, (uint32_t)ca, 0x7e3a9e0du, a.round, a.seed_lo, a.seed_hi, o);
    const double u = (double)(((uint64_t)o[0] << 21) | (uint64_t)(o[1] >> 11)) * 0x1p-53;
    ok = !not_finite(Ua) && !not_finite(Ub) && (d >= 0.0 || u < exp(d));
    flags[t] = ok ? 1 : 0;
  }
  count_per_case(attempted, ca, live);
  count_per_case(accepted, ca, ok);
}

// E: the unsigned integer of the handle's angle element (8, 4 or 2 bytes): a swap moves bits, whatever they encode
template <typename E>
__global__ __launch_bounds__(XTHREADS) void exchange_swap(const ExchangeArgs a, E *__restrict__ ang, double *__restrict__ obs,
                                                          double *__restrict__ lag, const int32_t *__restrict__ pairs,
                                                          const unsigned char *__restrict__ flags) {
  const int64_t t = (int64_t)blockIdx.x * XTHREADS + threadIdx.x;
  if (t >= a.npairs * a.per || !flags[t]) return;
  const int64_t pair = t / a.per, k = t - pair * a.per;
  const int64_t ga = pairs[2 * pair] * a.per + k, gb = pairs[2 * pair + 1] * a.per + k;   // < C: pairs hold case indices
  const int64_t nang = 2 * a.n, nrows = nang + NOBS_STATE;
  for (int64_t row = blockIdx.y; row < nrows; row += gridDim.y) {
    if (row < nang) {
      E *p = ang + row * a.C;
      const E x = p[ga], y = p[gb];
      p[ga] = y; p[gb] = x;
    } else {
      double *p = obs + (row - nang) * a.C;
      const double x = p[ga], y = p[gb];
      p[ga] = y; p[gb] = x;
    }
    if (row == 0) { lag[ga] = 0.0; lag[gb] = 0.0; }
  }
}

}  // namespace

hipError_t launch_exchange(const ExchangeArgs &a, const DevState &s, const CaseConst *cases, const int32_t *pairs,
                           unsigned char *flags, int64_t *attempted, int64_t *accepted, size_t elem, hipStream_t stream) {
  const int64_t lanes = a.npairs * a.per;
  if (lanes <= 0) return hipSuccess;   // a round in which no rung has a partner
  const unsigned blocks = (unsigned)((lanes + XTHREADS - 1) / XTHREADS);
  exchange_decide<<<dim3(blocks), dim3(XTHREADS), 0, stream>>>(a, s.obs, cases, pairs, flags, attempted, accepted);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int64_t nrows = 2 * a.n + NOBS_STATE;
  const dim3 grid(blocks, (unsigned)(nrows < 65535 ? nrows : 65535));
  if (elem == 8) exchange_swap<uint64_t><<<grid, dim3(XTHREADS), 0, stream>>>(a, (uint64_t *)s.ang, s.obs, s.lag, pairs, flags);
  else if (elem == 4) exchange_swap<uint32_t><<<grid, dim3(XTHREADS), 0, stream>>>(a, (uint32_t *)s.ang, s.obs, s.lag, pairs, flags);
  else exchange_swap<uint16_t><<<grid, dim3(XTHREADS), 0, stream>>>(a, (uint16_t *)s.ang, s.obs, s.lag, pairs, flags);
  return hipGetLastError();
}

}  // namespace pstat
