// pstat_hist.hip -- per-case histograms of the chains' current configurations, on the device.
//
// THE BINNING CONTRACT (restated, not shared, in tests/hist_ref.py).  It is the formula, not the real
// interval [lo, hi):
//   Host       inv = (double)nbins / (hi - lo), computed once when the histogram is opened.
//   Device     t = (x - lo) * inv: a subtraction and a product, each rounded on its own (f64).
//              x not finite     tails[2] += 1
//              t < 0            tails[0] += 1
//              t >= nbins       tails[1] += 1
//              otherwise        bin (int)t += 1            (truncation)
//              So lo falls in bin 0, hi in the upper tail, -0.0 where +0.0 does; an x within an ulp of an interior edge goes
//              where the two rounded operations put it, which the twin reproduces because it performs the same two.
//   Channels   0..6 = rows OBS_R1 .. OBS_U of DevState::obs, the seven doubles of pstat_microstate.  7 (PSTAT_HC_RMAG) =
//              sqrt(r1 * r1 + r2 * r2 + r3 * r3), 8 (PSTAT_HC_PMAG) the same over p: every product rounded, added left to
//              right, then a correctly rounded square root.  For pstat_histogram_device a channel is a column of the caller's
//              matrix and there are no magnitudes.
//   Counts     64-bit integers, counts[ncases][total_bins] with the specs' bins concatenated in order, tails[ncases][nspecs][3]
//              beside them.  Integer sums do not depend on order: the result is exact whatever the mapping below does.
//
// One launch per record for every case and spec.  It reads the source (DevState::obs, or the matrix) only and writes the
// histogram's buffers only.
//   Cases of up to 64 chains (the reference's sweeps run 1-25 per case): one wavefront per case, four cases per workgroup, as
//       record_wave_per_case in pstat_reduce.hip.  Lane t takes chain t, so loads are coalesced along C; a lane adds its
//       sample straight to the case's 64-bit counter in memory (at most 64 adds per case and spec).
//   Larger cases, and the matrix: 256-thread workgroups of GROUP_SAMPLES samples each, several per case when a case has more.
//       A workgroup keeps the case's bins and tails privately in LDS as 32-bit counters (it adds at most GROUP_SAMPLES to any of
//       them) and ends with one 64-bit atomicAdd per non-zero counter.  PSTAT_HIST_MAX_BINS = 8192 bins and 48 tails are
//       32.2 KiB of LDS: several workgroups per CU.
// Plain HIP C++: vector loads, atomicAdd on LDS and on global memory.  Built with -ffp-contract=off: t and the magnitudes are
// made of singly rounded operations.
#include <hip/hip_runtime.h>

#include "../../include/pstat.h"
#include "pstat_device.h"

namespace pstat {

namespace {

constexpr int HTHREADS = 256;
constexpr int64_t GROUP_SAMPLES = 1024;   // samples per workgroup of hist_group: four per thread

// value of channel `ch` for the sample whose first channel is at p; consecutive channels are `stride` doubles apart
__device__ __forceinline__ double channel_value(const double *__restrict__ p, const int64_t stride, const int ch, const bool matrix) {
  if (matrix || ch < PSTAT_HC_RMAG) return p[(int64_t)ch * stride];
  const double *v = p + (ch == PSTAT_HC_RMAG ? (int64_t)OBS_R1 : (int64_t)OBS_P1) * stride;
  const double a = v[0], b = v[stride], c = v[2 * stride];
  return sqrt(a * a + b * b + c * c);
}

// where a sample of value x goes under spec s: its bin, or nbins + (0 below | 1 above | 2 not finite)
__device__ __forceinline__ int slot_of(const HistSpec &s, const double x) {
  if (not_finite(x)) return s.nbins + 2;
  const double t = (x - s.lo) * s.inv;
  if (t < 0.0) return s.nbins;
  if (t >= (double)s.nbins) return s.nbins + 1;
  return (int)t;
}

// Cases of up to 64 samples: wave w of the grid takes case w, lane t its sample t.
__global__ __launch_bounds__(HTHREADS) void hist_wave_per_case(const HistArgs a, const double *__restrict__ src,
                                                               const HistSpec *__restrict__ specs,
                                                               unsigned long long *__restrict__ counts,
                                                               unsigned long long *__restrict__ tails) {
  const int lane = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * (HTHREADS / 64) + (threadIdx.x >> 6);
  if (k >= a.ncases || lane >= a.per) return;
  const double *p = src + (k * a.per + lane) * a.pitch;
  const HistSpec *mine = specs + (a.per_case ? k * a.nspecs : 0);
  for (int i = 0; i < a.nspecs; ++i) {
    const HistSpec s = mine[i];
    const int slot = slot_of(s, channel_value(p, a.stride, s.channel, a.matrix != 0));
    if (slot < s.nbins) atomicAdd(counts + k * a.total_bins + s.offset + slot, 1ull);
    else atomicAdd(tails + (k * a.nspecs + i) * 3 + (slot - s.nbins), 1ull);
  }
}

// Larger cases: workgroup (k, g) takes samples [g * GROUP_SAMPLES, (g + 1) * GROUP_SAMPLES) of case k.
// Dynamic LDS: total_bins + 3 * nspecs 32-bit counters, the tails behind the bins.
__global__ __launch_bounds__(HTHREADS) void hist_group(const HistArgs a, const int64_t groups, const double *__restrict__ src,
                                                       const HistSpec *__restrict__ specs,
                                                       unsigned long long *__restrict__ counts,
                                                       unsigned long long *__restrict__ tails) {
  extern __shared__ unsigned int bins[];
  const int t = threadIdx.x;
  const int64_t k = (int64_t)blockIdx.x / groups, g = (int64_t)blockIdx.x % groups;
  const int nslots = a.total_bins + 3 * a.nspecs;
  for (int i = t; i < nslots; i += HTHREADS) bins[i] = 0u;
  __syncthreads();
  const int64_t first = g * GROUP_SAMPLES;
  const int64_t last = first + GROUP_SAMPLES < a.per ? first + GROUP_SAMPLES : a.per;
  const HistSpec *mine = specs + (a.per_case ? k * a.nspecs : 0);
  for (int i = 0; i < a.nspecs; ++i) {
    const HistSpec s = mine[i];
    for (int64_t j = first + t; j < last; j += HTHREADS) {
      const int slot = slot_of(s, channel_value(src + (k * a.per + j) * a.pitch, a.stride, s.channel, a.matrix != 0));
      atomicAdd(&bins[slot < s.nbins ? s.offset + slot : a.total_bins + 3 * i + (slot - s.nbins)], 1u);
    }
  }
  __syncthreads();
  for (int i = t; i < nslots; i += HTHREADS) {
    const unsigned int c = bins[i];
    if (!c) continue;
    if (i < a.total_bins) atomicAdd(counts + k * a.total_bins + i, (unsigned long long)c);
    else atomicAdd(tails + k * 3 * a.nspecs + (i - a.total_bins), (unsigned long long)c);
  }
}

}  // namespace

hipError_t launch_hist(const HistArgs &a, const double *src, const HistSpec *specs, int64_t *counts, int64_t *tails,
                       hipStream_t stream) {
  if (a.ncases <= 0 || a.per <= 0) return hipSuccess;   // an empty matrix
  unsigned long long *c = reinterpret_cast<unsigned long long *>(counts), *t = reinterpret_cast<unsigned long long *>(tails);
  if (a.per <= 64) {
    const int64_t blocks = (a.ncases + HTHREADS / 64 - 1) / (HTHREADS / 64);
    hist_wave_per_case<<<dim3((unsigned)blocks), dim3(HTHREADS), 0, stream>>>(a, src, specs, c, t);
  } else {
    const int64_t groups = (a.per + GROUP_SAMPLES - 1) / GROUP_SAMPLES;
    const int64_t blocks = a.ncases * groups;
    if (blocks > 0x7fffffffll) return hipErrorInvalidConfiguration;
    const size_t lds = (size_t)(a.total_bins + 3 * a.nspecs) * sizeof(unsigned int);
    hist_group<<<dim3((unsigned)blocks), dim3(HTHREADS), lds, stream>>>(a, groups, src, specs, c, t);
  }
  return hipGetLastError();
}

}  // namespace pstat
