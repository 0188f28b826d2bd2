// pstat_pdist.hip -- pair distances on the device: per case the mean-square internal distance R^2(s), the closest approach,
// the distribution P(r) of the distances between two monomers of one chain and the orientationally averaged (Debye) S(q).
//
// THE CONTRACT (restated, not shared, in tests/pdist_ref.py; include/pstat.h).  Everything is f64, from the
// doubles load_angle gives for the stored angles (radians | turns | lattice index), whatever the handle's precision:
//   positions       exactly the shape recorder's: x_i = b (sum_{j <= i} n_j - n_i / 2), i = 0 .. n - 1, with the case's own b; a
//                   planar handle's n_i = (cos phi_i, sin phi_i) sits in the x and z slots, y = 0.
//   pair distance   for i < j: d = x_j - x_i;  r2 = (d_x d_x + d_y d_y) + d_z d_z (planar: d_x d_x + d_z d_z), every product rounded
//                   (built with -ffp-contract=off);  r = sqrt(r2), the correctly rounded square root.
//   options         max_sep in 0 .. n - 1 (-1: n - 1); min_sep in 1 .. n - 1; nbins >= 0; rmax > 0, finite (absolute units, one for
//                   all cases or one per case), as inv = nbins / rmax computed once on the host; q[nq] >= 0, absolute units.
//   columns per chain, in this order (ncols = max_sep + 1 + (nbins ? nbins + 1 : 0) + nq):
//     msd    max_sep columns, s = 1 .. max_sep:  R2(s) = (1 / (n - s)) sum_{i = 0}^{n - 1 - s} r2_{i,i+s}.
//     rmin   one column: min r_ij over the pairs with j - i >= min_sep.
//     hist   nbins + 1 columns (none when nbins = 0): COUNTS, as doubles, of the pairs with j - i >= min_sep:  t = r * inv; bin
//            (int)t if t < nbins, else the last column, "above".  r = 0 is in bin 0, r = rmax in "above"; a chain's columns add
//            up to (n - min_sep)(n - min_sep + 1) / 2.
//     debye  nq columns:  S(q) = 1 + (2 / n) sum_{i < j} sinc(q r_ij) over ALL pairs whatever min_sep;  x = q r rounded once,
//            sinc(0) = 1 exactly, else sin(x) / x with sincos_f64's sine.  q = 0 gives exactly n.  A planar handle uses the same
//            formula (the flat chain oriented at random in space; the in-plane average would need J0).
//   Per case and column one record adds sum_c v to `sum` and sum_c v * v to `sumsq`; a row, when the object keeps rows, is
//   sum_c v / num_chains.
//
// The order of every floating-point addition is fixed by (ncases, num_chains, n, the object's options) alone -- no floating-point
// atomics, nothing that depends on the number of CUs or on which workgroup arrives first:
//   pdist_stage1  workgroup (case, tile) of 256 threads takes `tile_chains` consecutive chains of one case, as corr_stage1 does.
//       Phase 1 (tile_unit_vectors) and phase 2 (tile_positions, the shape recorder's prefix sum) leave the positions in LDS.
//       Phase 3, R2(s): wavefront w takes the separations s = 1 + w, 5 + w, ... and for each walks the tile's chains in chain
//       order: lanes strided over i, wave_sum, one division, and the chain's value joins the column's (sum, sumsq) in registers.
//       Phase 4, the pairs, one chain of the tile after the other with the 256 threads sharing its n (n - 1) / 2 pairs: the pairs
//       are numbered row by row, p = (i, j) with j fastest, and thread t takes p = t, t + 256, ..., stepping (i, j) on with integer
//       adds alone.  So every lane has work until the chain's last 256 pairs (rows of lanes, j = i + 1 + lane, leave 43 % of
//       the lane slots empty at n = 100: 21.8 ms against 13.7 ms per record of 65 536 chains at nq = 16); a
//       wavefront's 64 consecutive pairs span few rows, so its x_i are a few LDS broadcasts and its x_j runs of consecutive 8-byte
//       words.  From one (r2, r) a lane updates its running minimum, adds 1 to the chain's bin counter in LDS (an INTEGER add:
//       order-free) and adds sinc(q r) to its accumulators for a block of PDIST_QB = 8 magnitudes held in registers; further
//       blocks of q walk the pairs again and recompute r (15 flops and a square root beside 8 sines).  Per block, wave_sum gives
//       the wavefront's sums; behind a barrier thread k adds the four wavefronts' in order of w from 0.0 and S_k joins column
//       k's (sum, sumsq) in its registers; thread 0 does the same with the minimum, and thread t with the counters t, t + 256,
//       t + 512, which it zeroes for the next chain.  So every column is folded over the tile's chains in chain order from 0.0,
//       and the tile's partial leaves as partial[tile][sum | sumsq][column].
//   tile_fold     (pstat_corr.hip) the fold over the tiles per (case, column).
// LDS: the tile frame's 4 KiB of scratch (here: the wavefronts' minima and sums), the positions, and ONE chain's nbins + 1 32-bit
// counters behind them (a chain has at most n (n - 1) / 2 <= 3.3e6 pairs).  pstat_pdist_open refuses a chain whose positions and
// counters do not fit: n <= pdist_max_n(planar, nbins) = (61440 - 8 ceil((nbins + 1) / 2)) / (24 | 16 planar).
// It reads DevState::ang and the case table only and writes the pdist object's own buffers only.  Plain HIP C++.
#include <hip/hip_runtime.h>

#include "../../include/pstat.h"
#include "pstat_device.h"
#include "pstat_math.h"
#include "pstat_tile.h"

namespace pstat {

namespace {

#ifndef PSTAT_PDIST_QB
#define PSTAT_PDIST_QB 8
#endif
constexpr int PDIST_QB = PSTAT_PDIST_QB;           // Debye magnitudes per walk over a chain's pairs (8, measured)
constexpr int PDIST_WAVES = TILE_THREADS / 64;
constexpr int PDIST_HSLOTS = (PSTAT_PDIST_MAX_BINS + 1 + TILE_THREADS - 1) / TILE_THREADS;   // bin columns per thread
static_assert(PSTAT_PDIST_MAX_Q <= 64 && 8 + PDIST_WAVES * PSTAT_PDIST_MAX_Q <= 2 * TILE_THREADS, "the wavefronts' sums fit the scratch");

template <bool PLANAR>
__device__ __forceinline__ double pair_r2(const double *x, const double *y, const double *z, const double xi, const double yi,
                                          const double zi, const int j) {
  const double dx = x[j] - xi, dz = z[j] - zi;
  double r2 = dx * dx;
  if constexpr (!PLANAR) {
    const double dy = y[j] - yi;
    r2 += dy * dy;
  }
  return r2 + dz * dz;
}

template <bool PLANAR>
__global__ __launch_bounds__(TILE_THREADS) void pdist_stage1(const PdistArgs a, const void *__restrict__ ang,
                                                             const CaseConst *__restrict__ cases, const double *__restrict__ qtab,
                                                             const double *__restrict__ invtab, double *__restrict__ partial) {
  extern __shared__ double lds[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const Tile w = tile_of(a, lds);
  const int n = (int)a.n, tc = w.tc, ns = w.ns;
  tile_unit_vectors<PLANAR>(a, w, ang);
  tile_positions<PLANAR>(a, w, cases[w.kcase].b);

  const int ncols = a.ncols, nbins = a.nbins, nq = a.nq;
  const int ncnt = nbins > 0 ? nbins + 1 : 0;
  const int col_rmin = a.max_sep, col_hist = a.max_sep + 1, col_sq = col_hist + ncnt;
  double *out = partial + (int64_t)blockIdx.x * 2 * ncols;

  // phase 3: R2(s), a wavefront per separation, the tile's chains in order
  for (int s = 1 + wave; s <= a.max_sep; s += PDIST_WAVES) {
    const double d = (double)(n - s);
    double r1 = 0.0, r2 = 0.0;
    for (int q = 0; q < tc; ++q) {
      const double *x = w.x + q * ns, *z = w.z + q * ns, *y = w.y + q * ns;
      double sum = 0.0;
      for (int i = lane; i < n - s; i += 64) sum += pair_r2<PLANAR>(x, y, z, x[i], PLANAR ? 0.0 : y[i], z[i], i + s);
      const double v = wave_sum(sum) / d;                           // (lane 0's is the wavefront's)
      r1 += v;
      r2 += v * v;
    }
    if (lane == 0) {
      out[s - 1] = r1;
      out[ncols + s - 1] = r2;
    }
  }

  // phase 4: the pairs.  Scratch: wmin[4] at lds[0], wsum[4][64] at lds[8]; the counters lie behind the positions
  double *wmin = lds, *wsum = lds + 8;
  unsigned int *cnt = (unsigned int *)(w.x + (int64_t)(PLANAR ? 2 : 3) * a.tile_chains * ns);
  for (int c = t; c < ncnt; c += TILE_THREADS) cnt[c] = 0u;
  __syncthreads();
  const double inv = nbins > 0 ? invtab[w.kcase] : 0.0;
  const double dn = (double)n;
  double m1 = 0.0, m2 = 0.0, d1 = 0.0, d2 = 0.0;                     // rmin's (thread 0) and S_t's (thread t < nq) sums
  double h1[PDIST_HSLOTS], h2[PDIST_HSLOTS];                         // those of the bin columns t, t + 256, ...
#pragma unroll
  for (int k = 0; k < PDIST_HSLOTS; ++k) h1[k] = h2[k] = 0.0;
  const int npairs = n * (n - 1) / 2;
  const int nblocks = nq > 0 ? (nq + PDIST_QB - 1) / PDIST_QB : 1;  // (one walk even without a q: minimum and counters)
  for (int q = 0; q < tc; ++q) {                                     // uniform: every thread meets every barrier
    const double *x = w.x + q * ns, *z = w.z + q * ns, *y = w.y + q * ns;
    for (int kb = 0; kb < nblocks; ++kb) {
      const bool first = kb == 0;
      double qv[PDIST_QB], acc[PDIST_QB];
#pragma unroll
      for (int u = 0; u < PDIST_QB; ++u) {
        acc[u] = 0.0;
        qv[u] = kb * PDIST_QB + u < nq ? qtab[kb * PDIST_QB + u] : 0.0;
      }
      double lo = __builtin_inf();
      // pair p = (i, j) in row-major order of the upper triangle; a lane's next pair is 256 further on
      int i = 0, j = 1 + t;
      for (int p = t; p < npairs; p += TILE_THREADS, j += TILE_THREADS) {
        while (j >= n) {                                             // past the end of row i: its n - 1 - i pairs lie behind
          j -= n - 2 - i;
          ++i;
        }
        const double r = sqrt(pair_r2<PLANAR>(x, y, z, x[i], PLANAR ? 0.0 : y[i], z[i], j));
        if (first && j - i >= a.min_sep) {
          lo = r < lo ? r : lo;
          if (nbins > 0) {
            const double tt = r * inv;
            atomicAdd(&cnt[tt < (double)nbins ? (int)tt : nbins], 1u);
          }
        }
#pragma unroll
        for (int u = 0; u < PDIST_QB; ++u) {
          if (kb * PDIST_QB + u < nq) {                              // uniform
            const double ph = qv[u] * r;
            double sn, cs;
            sincos_f64(ph, &sn, &cs);
            acc[u] += ph == 0.0 ? 1.0 : sn / ph;
          }
        }
      }
      if (first) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const double other = __shfl_down(lo, off, 64);
          lo = other < lo ? other : lo;
        }
        if (lane == 0) wmin[wave] = lo;
      }
#pragma unroll
      for (int u = 0; u < PDIST_QB; ++u) {
        if (kb * PDIST_QB + u < nq) {                                // uniform
          const double s = wave_sum(acc[u]);
          if (lane == 0) wsum[wave * 64 + kb * PDIST_QB + u] = s;
        }
      }
    }
    __syncthreads();
    if (t == 0) {
      double m = wmin[0];
      for (int v = 1; v < PDIST_WAVES; ++v) m = wmin[v] < m ? wmin[v] : m;
      m1 += m;
      m2 += m * m;
    }
    if (t < nq) {
      double s = 0.0;
      for (int v = 0; v < PDIST_WAVES; ++v) s += wsum[v * 64 + t];
      const double S = 1.0 + (2.0 * s) / dn;                         // (q = 0: s = n (n - 1) / 2 and S = n, exactly)
      d1 += S;
      d2 += S * S;
    }
#pragma unroll
    for (int k = 0; k < PDIST_HSLOTS; ++k) {
      const int c = t + k * TILE_THREADS;
      if (c < ncnt) {
        const double v = (double)cnt[c];
        h1[k] += v;
        h2[k] += v * v;
        cnt[c] = 0u;
      }
    }
    __syncthreads();                                                 // the scratch and the counters are the next chain's
  }
  if (t == 0) {
    out[col_rmin] = m1;
    out[ncols + col_rmin] = m2;
  }
  if (t < nq) {
    out[col_sq + t] = d1;
    out[ncols + col_sq + t] = d2;
  }
#pragma unroll
  for (int k = 0; k < PDIST_HSLOTS; ++k) {
    const int c = t + k * TILE_THREADS;
    if (c < ncnt) {
      out[col_hist + c] = h1[k];
      out[ncols + col_hist + c] = h2[k];
    }
  }
}

}  // namespace

size_t pdist_counter_bytes(const int nbins) { return nbins > 0 ? 8 * (((size_t)nbins + 2) / 2) : 0; }

int64_t pdist_max_n(const int planar, const int nbins) {
  return (int64_t)((TILE_LDS - TILE_SCRATCH - pdist_counter_bytes(nbins)) / ((planar ? 2 : 3) * sizeof(double)));
}

void pdist_layout(PdistArgs &a) {
  tile_layout(a, 64);                                                // (lpc, groups: the frame's; the pair phase has its own mapping)
  while (a.tile_chains > 1 && tile_lds_bytes(a.n, a.tile_chains, a.planar) + pdist_counter_bytes(a.nbins) > TILE_LDS) --a.tile_chains;
  a.tiles = (a.per + a.tile_chains - 1) / a.tile_chains;
}

hipError_t launch_pdist(const PdistArgs &a, const void *ang, const CaseConst *cases, const double *q, const double *inv,
                        double *partial, double *totals, double *row, hipStream_t stream) {
  int64_t blocks;
  size_t lds;
  hipError_t e = tile_launch_shape(a, &blocks, &lds);
  if (e != hipSuccess || blocks == 0) return e;
  lds += pdist_counter_bytes(a.nbins);
  if (lds > TILE_LDS || a.nq > PSTAT_PDIST_MAX_Q || a.nbins > PSTAT_PDIST_MAX_BINS || a.nbins < 0 || a.nq < 0 || a.n < 2 ||
      a.max_sep < 0 || a.max_sep > a.n - 1 || a.min_sep < 1 || a.ncols != a.max_sep + 1 + (a.nbins ? a.nbins + 1 : 0) + a.nq)
    return hipErrorInvalidConfiguration;
  const dim3 grid((unsigned)blocks), block(TILE_THREADS);
  if (a.planar) pdist_stage1<true><<<grid, block, lds, stream>>>(a, ang, cases, q, inv, partial);
  else pdist_stage1<false><<<grid, block, lds, stream>>>(a, ang, cases, q, inv, partial);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_tile_fold(a, partial, totals, row, stream);
}

}  // namespace pstat
