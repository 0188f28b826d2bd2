// pstat_corr.hip -- chain structure on the device: per-case lag correlations of the monomers' orientations and dipoles.
//
// THE CONTRACT (restated, not shared, in tests/corr_ref.py; include/pstat.h).  Everything is f64, from the
// doubles load_angle gives for the stored angles (radians | turns | lattice index), whatever the handle's precision:
//   3D handles      n_i = (cos phi_i sin theta_i, sin phi_i sin theta_i, cos theta_i); the field axis z is component 3.
//                   dielectric  mu_i = (K1 - K2) E0 cos theta_i n_i + K2 E0 z
//                   polar       mu_i = mu n_i                                  (E0, K1, K2, mu: the case's own, CaseConst)
//   planar handles  n_i = (cos phi_i, sin phi_i); the field axis is component 2.
//                   dielectric  mu_i = (K1 - K2) E0 sin phi_i n_i + (0, K2 E0);  polar as above.
//                   Here a planar unit vector is kept as (x, z) = (cos phi, sin phi): with y = 0 every formula below is the 3D one.
//   Per chain c and lag k = 0 .. max_lag:  v(c, k) = (1 / (n - k)) sum_{i = 0}^{n - 1 - k} of
//                   PSTAT_CORR_NN  n_i . n_{i+k}        PSTAT_CORR_ZZ  n_{i,z} n_{i+k,z}        PSTAT_CORR_MM  mu_i . mu_{i+k}
//                   added in order of i from 0.0, every product rounded (built with -ffp-contract=off), one division at the end.
//   Per case and column (channels in the order NN, ZZ, MM, each max_lag + 1 wide) one record adds sum_c v to `sum` and
//   sum_c v * v to `sumsq`; a row, when the object keeps rows, is sum_c v / num_chains.
//
// The order of every addition is fixed by (ncases, num_chains, n, max_lag) alone -- no floating-point atomics, nothing that
// depends on the number of CUs or on which workgroup arrives first -- so two identical runs give identical bits:
//   corr_stage1   workgroup (case, tile) of 256 threads takes `tile_chains` consecutive chains of one case (16, fewer where a
//       case has fewer or LDS is short).  Phase 1: the threads load the tile's angles with the chain index fastest, so a row of
//       16 chains is one 128-byte segment of DevState::ang, take two sincos per monomer (one for a planar handle) and leave the
//       unit vectors in LDS, component by component (24 n bytes per chain, 16 n planar).  Phase 2: the 256 threads are `groups`
//       groups of `lpc` = min(256, 2^ceil(log2(max_lag + 1))) threads; thread s of a group takes the lags s, s + lpc, ... and group
//       g the tile's chains g, g + groups, ... in that order, keeping sum v and sum v * v of its own (lag, chains) in registers.
//       A thread reads n_i (the same word for the whole group: a broadcast) and n_{i+k} (consecutive words over the group:
//       conflict-free) and forms mu on the fly, so LDS holds nothing but the unit vectors.  The groups' sums are then added in
//       order of g from 0.0 by group 0 through 4 KiB of LDS, and the tile's partial leaves as partial[tile][sum | sumsq][column].
//   tile_fold     one wavefront per (case, column): lane l adds the partials of the case's tiles l, l + 64, ... in order from
//       0.0, wave_sum's tree follows, lane 0 adds the two results to the running totals it alone owns and writes the row's mean.
// A chain's vectors must fit the 64 KiB a workgroup is given beside the 4 KiB of scratch: n <= 2560 for a 3D handle, n <= 3840
// for a planar one (tile_max_n); pstat_corr_open refuses longer chains.
// The tile frame -- the layout rule, phase 1, the groups' fold and tile_fold -- is the shape recorder's too: pstat_tile.h states
// the device pieces, this file defines the host ones and the fold kernel.
// It reads DevState::ang and the case table only and writes the correlation object's own buffers only.
// Plain HIP C++; sincos_f64 (pstat_math.h) is the < 1 ulp one the initialisation kernels use.
#include <hip/hip_runtime.h>

#include "../../include/pstat.h"
#include "pstat_device.h"
#include "pstat_math.h"
#include "pstat_tile.h"

namespace pstat {

namespace {

template <bool PLANAR, bool MM>
__global__ __launch_bounds__(TILE_THREADS) void corr_stage1(const CorrArgs a, const void *__restrict__ ang,
                                                            const CaseConst *__restrict__ cases, double *__restrict__ partial) {
  extern __shared__ double lds[];
  const int t = threadIdx.x;
  const Tile w = tile_of(a, lds);
  tile_unit_vectors<PLANAR>(a, w, ang);
  const int64_t kcase = w.kcase;
  const int n = (int)a.n, tc = w.tc, ns = w.ns;
  const double *vx = w.x, *vz = w.z, *vy = w.y;

  // mu = f n + mb z with f = ma * n_z (dielectric) or mu (polar)
  double ma = 0.0, mb = 0.0;
  if constexpr (MM) {
    const CaseConst cc = cases[kcase];
    if (a.polar) { ma = cc.mu; }
    else { ma = (cc.K1 - cc.K2) * cc.E0; mb = cc.K2 * cc.E0; }
  }
  const int sub = t % a.lpc, g = t / a.lpc;
  const int ncols = a.ncols, width = a.max_lag + 1;
  double *mine = partial + (int64_t)blockIdx.x * 2 * ncols;
  for (int j = 0; j < a.nslots; ++j) {                               // uniform: every thread meets every barrier
    const int k = sub + j * a.lpc;
    const bool active = k <= a.max_lag;
    double a1[3] = {0.0, 0.0, 0.0}, a2[3] = {0.0, 0.0, 0.0};
    if (active) {
      const double d = (double)(n - k);
      for (int q = g; q < tc; q += a.groups) {
        const double *x = vx + q * ns, *z = vz + q * ns, *y = vy + q * ns;
        double snn = 0.0, szz = 0.0, smm = 0.0;
        for (int i = 0; i < n - k; ++i) {
          const double xi = x[i], xj = x[i + k], zi = z[i], zj = z[i + k];
          double yi = 0.0, yj = 0.0;
          if constexpr (!PLANAR) { yi = y[i]; yj = y[i + k]; }
          double dot = xi * xj;
          if constexpr (!PLANAR) dot += yi * yj;
          dot += zi * zj;
          snn += dot;
          szz += zi * zj;
          if constexpr (MM) {
            const double fi = a.polar ? ma : ma * zi, fj = a.polar ? ma : ma * zj;
            double m = (fi * xi) * (fj * xj);
            if constexpr (!PLANAR) m += (fi * yi) * (fj * yj);
            m += (fi * zi + mb) * (fj * zj + mb);
            smm += m;
          }
        }
        const double v0 = snn / d, v1 = szz / d, v2 = smm / d;
        a1[0] += v0; a2[0] += v0 * v0;
        a1[1] += v1; a2[1] += v1 * v1;
        a1[2] += v2; a2[2] += v2 * v2;
      }
    }
    int col = 0;
    for (int ch = 0; ch < 3; ++ch) {
      if (!(a.channels & (1 << ch))) continue;
      double r1 = a1[ch], r2 = a2[ch];
      tile_group_fold(a, lds, sub, g, active, r1, r2);
      if (g == 0 && active) {
        mine[col * width + k] = r1;
        mine[ncols + col * width + k] = r2;
      }
      ++col;
    }
  }
}

}  // namespace

// wave w of the grid takes (case, column) w
__global__ __launch_bounds__(TILE_THREADS) void tile_fold(const int64_t ncases, const int64_t ncols, const int64_t tiles,
                                                          const int64_t per, const double *__restrict__ partial,
                                                          double *__restrict__ totals, double *__restrict__ row) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * (TILE_THREADS / 64) + (threadIdx.x >> 6);
  if (w >= ncases * ncols) return;
  const int64_t kcase = w / ncols, col = w % ncols;
  const double *p = partial + kcase * tiles * 2 * ncols + col;
  double r1 = 0.0, r2 = 0.0;
  for (int64_t tile = lane; tile < tiles; tile += 64) {
    r1 += p[tile * 2 * ncols];
    r2 += p[tile * 2 * ncols + ncols];
  }
  r1 = wave_sum(r1);
  r2 = wave_sum(r2);
  if (lane == 0) {
    totals[w] += r1;                     // sum[ncases][ncols]
    totals[ncases * ncols + w] += r2;    // sumsq[ncases][ncols]
    if (row) row[w] = r1 / (double)per;
  }
}

hipError_t launch_tile_fold(const TileArgs &a, const double *partial, double *totals, double *row, hipStream_t stream) {
  const int64_t waves = a.ncases * a.ncols;
  tile_fold<<<dim3((unsigned)((waves + TILE_THREADS / 64 - 1) / (TILE_THREADS / 64))), dim3(TILE_THREADS), 0, stream>>>(
      a.ncases, a.ncols, a.tiles, a.per, partial, totals, row);
  return hipGetLastError();
}

int64_t tile_max_n(int planar) { return (int64_t)((TILE_LDS - TILE_SCRATCH) / ((planar ? 2 : 3) * sizeof(double))); }

void tile_layout(TileArgs &a, const int width) {
  int tc = (int)(a.per < TILE_CHAINS ? a.per : TILE_CHAINS);
  while (tc > 1 && tile_lds_bytes(a.n, tc, a.planar) > TILE_LDS) --tc;
  a.tile_chains = tc;
  a.tiles = (a.per + tc - 1) / tc;
  int lpc = 1;
  while (lpc < TILE_THREADS && lpc < width) lpc *= 2;
  a.lpc = lpc;
  a.groups = TILE_THREADS / lpc;
  a.nslots = (width + lpc - 1) / lpc;
}

size_t tile_partial_doubles(const TileArgs &a) { return (size_t)a.ncases * (size_t)a.tiles * 2 * (size_t)a.ncols; }

hipError_t tile_launch_shape(const TileArgs &a, int64_t *blocks, size_t *lds) {
  *blocks = a.ncases * a.tiles > 0 ? a.ncases * a.tiles : 0;
  *lds = tile_lds_bytes(a.n, a.tile_chains, a.planar);
  if (*blocks > 0x7fffffffll || *lds > TILE_LDS || a.tile_chains > TILE_CHAINS || a.lpc * a.groups != TILE_THREADS)
    return hipErrorInvalidConfiguration;
  return hipSuccess;
}

hipError_t launch_corr(const CorrArgs &a, const void *ang, const CaseConst *cases, double *partial, double *totals, double *row,
                       hipStream_t stream) {
  int64_t blocks;
  size_t lds;
  hipError_t e = tile_launch_shape(a, &blocks, &lds);
  if (e != hipSuccess || blocks == 0) return e;
  const bool mm = (a.channels & PSTAT_CORR_MM) != 0;
  const dim3 grid((unsigned)blocks), block(TILE_THREADS);
  if (a.planar) {
    if (mm) corr_stage1<true, true><<<grid, block, lds, stream>>>(a, ang, cases, partial);
    else corr_stage1<true, false><<<grid, block, lds, stream>>>(a, ang, cases, partial);
  } else {
    if (mm) corr_stage1<false, true><<<grid, block, lds, stream>>>(a, ang, cases, partial);
    else corr_stage1<false, false><<<grid, block, lds, stream>>>(a, ang, cases, partial);
  }
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_tile_fold(a, partial, totals, row, stream);
}

}  // namespace pstat
