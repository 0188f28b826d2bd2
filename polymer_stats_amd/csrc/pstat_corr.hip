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
//   corr_stage2   one wavefront per (case, column): lane l adds the partials of the case's tiles l, l + 64, ... in order from
//       0.0, wave_sum's tree follows, lane 0 adds the two results to the running totals it alone owns and writes the row's mean.
// A chain's vectors must fit the 64 KiB a workgroup is given beside the 4 KiB of scratch: n <= 2560 for a 3D handle, n <= 3840
// for a planar one (corr_max_n); pstat_corr_open refuses longer chains.
// It reads DevState::ang and the case table only and writes the correlation object's own buffers only.
// Plain HIP C++; sincos_f64 (pstat_math.h) is the < 1 ulp one the initialisation kernels use.
#include <hip/hip_runtime.h>

#include "../../include/pstat.h"
#include "pstat_device.h"
#include "pstat_math.h"

namespace pstat {

namespace {

constexpr int CTHREADS = 256;
constexpr int CORR_TILE = 16;                       // chains per workgroup at most
constexpr size_t CORR_LDS = 65536;                  // what a workgroup may have
constexpr size_t CORR_SCRATCH = 2 * CTHREADS * sizeof(double);   // the groups' sums on their way to group 0

// monomers of a chain as LDS keeps them: odd where several chains share a tile, so that the phase-1 stores of consecutive chains
// do not meet in one bank
__host__ __device__ inline int64_t padded_n(const int64_t n, const int tile_chains) { return tile_chains > 1 ? (n | 1) : n; }

template <bool PLANAR, bool MM>
__global__ __launch_bounds__(CTHREADS) void corr_stage1(const CorrArgs a, const void *__restrict__ ang,
                                                        const CaseConst *__restrict__ cases, double *__restrict__ partial) {
  extern __shared__ double lds[];
  double *s1 = lds, *s2 = lds + CTHREADS;
  const int t = threadIdx.x;
  const int64_t kcase = (int64_t)blockIdx.x / a.tiles, tile = (int64_t)blockIdx.x % a.tiles;
  const int64_t first = tile * a.tile_chains;                       // the tile's first chain within its case
  const int64_t left = a.per - first;
  const int tc = (int)(left < a.tile_chains ? left : a.tile_chains);  // chains this tile holds
  const int64_t c0 = kcase * a.per + first, C = a.ncases * a.per;
  const int n = (int)a.n, ns = (int)padded_n(a.n, a.tile_chains);
  // vx[q][i], (vy[q][i],) vz[q][i] for chain q of the tile
  double *vx = lds + 2 * CTHREADS;
  double *vz = vx + (int64_t)a.tile_chains * ns;
  double *vy = vz + (int64_t)a.tile_chains * ns;                    // 3D only

  for (int e = t; e < tc * n; e += CTHREADS) {
    const int q = e % tc, i = e / tc;
    double sp, cp;
    sincos_f64(load_angle(ang, ((int64_t)n + i) * C + c0 + q, (size_t)a.elem, false), &sp, &cp);
    if constexpr (PLANAR) {
      vx[q * ns + i] = cp;
      vz[q * ns + i] = sp;
    } else {
      double st, ct;
      sincos_f64(load_angle(ang, (int64_t)i * C + c0 + q, (size_t)a.elem, true), &st, &ct);
      vx[q * ns + i] = cp * st;
      vy[q * ns + i] = sp * st;
      vz[q * ns + i] = ct;
    }
  }
  __syncthreads();

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
      if (a.groups > 1) {
        s1[t] = r1; s2[t] = r2;
        __syncthreads();
        if (g == 0 && active) {
          r1 = 0.0; r2 = 0.0;
          for (int gg = 0; gg < a.groups; ++gg) { r1 += s1[sub + gg * a.lpc]; r2 += s2[sub + gg * a.lpc]; }
        }
        __syncthreads();   // the scratch is rewritten for the next channel
      }
      if (g == 0 && active) {
        mine[col * width + k] = r1;
        mine[ncols + col * width + k] = r2;
      }
      ++col;
    }
  }
}

}  // namespace

// wave w of the grid takes (case, column) w (declared in pstat_device.h: the shape recorder's fold is this kernel too)
__global__ __launch_bounds__(CTHREADS) void corr_stage2(const CorrArgs a, const double *__restrict__ partial,
                                                        double *__restrict__ totals, double *__restrict__ row) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * (CTHREADS / 64) + (threadIdx.x >> 6);
  const int64_t ncols = a.ncols;
  if (w >= a.ncases * ncols) return;
  const int64_t kcase = w / ncols, col = w % ncols;
  const double *p = partial + kcase * a.tiles * 2 * ncols + col;
  double r1 = 0.0, r2 = 0.0;
  for (int64_t tile = lane; tile < a.tiles; tile += 64) {
    r1 += p[tile * 2 * ncols];
    r2 += p[tile * 2 * ncols + ncols];
  }
  r1 = wave_sum(r1);
  r2 = wave_sum(r2);
  if (lane == 0) {
    totals[w] += r1;                       // sum[ncases][ncols]
    totals[a.ncases * ncols + w] += r2;    // sumsq[ncases][ncols]
    if (row) row[w] = r1 / (double)a.per;
  }
}

int64_t corr_max_n(int planar) { return (int64_t)((CORR_LDS - CORR_SCRATCH) / ((planar ? 2 : 3) * sizeof(double))); }

void corr_shape(CorrArgs &a) {
  const int comps = a.planar ? 2 : 3;
  int tc = (int)(a.per < CORR_TILE ? a.per : CORR_TILE);
  while (tc > 1 && CORR_SCRATCH + (size_t)tc * (size_t)padded_n(a.n, tc) * comps * sizeof(double) > CORR_LDS) --tc;
  a.tile_chains = tc;
  a.tiles = (a.per + tc - 1) / tc;
  int lpc = 1;
  while (lpc < CTHREADS && lpc < a.max_lag + 1) lpc *= 2;
  a.lpc = lpc;
  a.groups = CTHREADS / lpc;
  a.nslots = (a.max_lag + lpc) / lpc;
}

size_t corr_partial_doubles(const CorrArgs &a) { return (size_t)a.ncases * (size_t)a.tiles * 2 * (size_t)a.ncols; }

hipError_t launch_corr(const CorrArgs &a, const void *ang, const CaseConst *cases, double *partial, double *totals, double *row,
                       hipStream_t stream) {
  const int64_t blocks = a.ncases * a.tiles;
  if (blocks <= 0) return hipSuccess;
  if (blocks > 0x7fffffffll) return hipErrorInvalidConfiguration;
  const size_t lds = CORR_SCRATCH + (size_t)a.tile_chains * (size_t)padded_n(a.n, a.tile_chains) * (a.planar ? 2 : 3) * sizeof(double);
  if (lds > CORR_LDS) return hipErrorInvalidConfiguration;
  const bool mm = (a.channels & PSTAT_CORR_MM) != 0;
  const dim3 grid((unsigned)blocks), block(CTHREADS);
  if (a.planar) {
    if (mm) corr_stage1<true, true><<<grid, block, lds, stream>>>(a, ang, cases, partial);
    else corr_stage1<true, false><<<grid, block, lds, stream>>>(a, ang, cases, partial);
  } else {
    if (mm) corr_stage1<false, true><<<grid, block, lds, stream>>>(a, ang, cases, partial);
    else corr_stage1<false, false><<<grid, block, lds, stream>>>(a, ang, cases, partial);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int64_t waves = a.ncases * a.ncols;
  corr_stage2<<<dim3((unsigned)((waves + CTHREADS / 64 - 1) / (CTHREADS / 64))), block, 0, stream>>>(a, partial, totals, row);
  return hipGetLastError();
}

}  // namespace pstat
