// pstat_shape.hip -- chain shape on the device: per-case gyration tensor and form factor S(q) of the monomers' positions.
//
// THE CONTRACT (restated, not shared, in tests/shape_ref.py; include/pstat.h).  Everything is f64, from the
// doubles load_angle gives for the stored angles (radians | turns | lattice index), whatever the handle's precision:
//   3D handles      n_i = (cos phi_i sin theta_i, sin phi_i sin theta_i, cos theta_i)                (as pstat_corr.hip)
//   planar handles  n_i = (cos phi_i, sin phi_i), kept as (x, z) with y = 0: every formula below is the 3D one.
//   positions       x_i = b (sum_{j <= i} n_j - n_i / 2), i = 0 .. n - 1: the monomers' centres, with the case's own b.
//   gyration block, eight columns per chain in the order gxx, gyy, gzz, gxy, gxz, gyz, rg2, trg2 (PSTAT_SHAPE_GYR):
//                   xbar = (1 / n) sum_i x_i;  G_ab = (1 / n) sum_i (x_i - xbar)_a (x_i - xbar)_b  (centred first);
//                   rg2 = G_xx + G_yy + G_zz;  trg2 = sum_ab G_ab^2 (the off-diagonals counted twice).
//                   A planar handle's gyy, gxy, gyz are exactly 0.
//   form factor     nq >= 0 further columns, one per wave-vector of the caller's table q[nq][3] (absolute units; a planar
//                   handle ignores q[.][1]):  S(c, q) = (1 / n) [(sum_i cos(q . x_i))^2 + (sum_i sin(q . x_i))^2], so q = 0
//                   gives exactly n.  Every product is rounded (built with -ffp-contract=off).
//   Per case and column one record adds sum_c v to `sum` and sum_c v * v to `sumsq`; a row, when the object keeps rows, is
//   sum_c v / num_chains.
//
// The order of every addition is fixed by (ncases, num_chains, n, nq) alone -- no floating-point atomics, nothing that depends
// on the number of CUs or on which workgroup arrives first -- so two identical runs give identical bits:
//   shape_stage1  workgroup (case, tile) of 256 threads takes `tile_chains` consecutive chains of one case (16, fewer where a
//       case has fewer or LDS is short), as corr_stage1 does.
//       Phase 1: the threads load the tile's angles with the chain index fastest, take two sincos per monomer (one for a planar
//       handle) and leave the unit vectors in LDS, component by component (24 n bytes per chain, 16 n planar).
//       Phase 2 (tile_positions, pstat_tile.h: the pair-distance recorder's too): the prefix sum, in place.  A wavefront takes one (chain, component) sequence at a time: lane l sums its segment
//       of ceil(n / 64) consecutive monomers in order, the lanes' sums go through a 6-level shift-and-add scan, and the lane
//       rewrites its segment as b (running sum - n_i / 2).  The tree depends on n alone.
//       Phase 3: a wavefront per chain, lanes strided over i: wave_sum of the three coordinates gives the centre, wave_sum of the
//       six centred products the tensor; lane 0 leaves the chain's eight values in LDS, and thread j < 8 adds column j over the
//       tile's chains in chain order from 0.0.
//       Phase 4, the hot loop: the 256 threads are `groups` groups of `lpc` = min(256, 2^ceil(log2 nq)) threads; thread s of a
//       group takes the wave-vectors s, s + lpc, ... and group g the tile's chains g, g + groups, ...  With its q in registers a
//       thread walks i, reads x_i from LDS (the same word for the whole group: a broadcast; groups of one wave read different
//       chains, whose odd padding keeps them in different banks), forms the phase, takes ONE sincos_f64 and keeps sum cos and sum
//       sin in registers.  The groups' sums are then added in order of g from 0.0 by group 0 through 4 KiB of LDS, and the tile's
//       partial leaves as partial[tile][sum | sumsq][column].  With nq = 0 the phase is skipped.
//   tile_fold     (pstat_corr.hip) the fold over the tiles per (case, column).
// The tile frame -- the layout rule, phase 1 and the groups' fold -- is the correlation recorder's too (pstat_tile.h).
// A chain's positions take the LDS its unit vectors take in corr_stage1: n <= tile_max_n(planar); pstat_shape_open refuses longer
// chains, more than PSTAT_SHAPE_MAX_Q wave-vectors, and a wave-vector whose phase could reach 1e5 (below that sincos_f64 is the
// < 1 ulp routine).
// It reads DevState::ang and the case table only and writes the shape object's own buffers only.  Plain HIP C++.
#include <hip/hip_runtime.h>

#include "../../include/pstat.h"
#include "pstat_device.h"
#include "pstat_math.h"
#include "pstat_tile.h"

namespace pstat {

namespace {

template <bool PLANAR>
__global__ __launch_bounds__(TILE_THREADS) void shape_stage1(const ShapeArgs a, const void *__restrict__ ang,
                                                             const CaseConst *__restrict__ cases, const double *__restrict__ qtab,
                                                             double *__restrict__ partial) {
  extern __shared__ double lds[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  // px[q][i], pz[q][i], (py[q][i]) for chain q of the tile: unit vectors first, positions after phase 2
  const Tile w = tile_of(a, lds);
  const int n = (int)a.n, tc = w.tc, ns = w.ns;
  double *px = w.x, *pz = w.z, *py = w.y;
  const double b = cases[w.kcase].b;
  tile_unit_vectors<PLANAR>(a, w, ang);

  tile_positions<PLANAR>(a, w, b);                                  // phase 2 (pstat_tile.h)

  // phase 3: centre and gyration tensor, a wavefront per chain; the chain's eight values go to gy[q][8]
  double *gy = lds;                                                 // TILE_CHAINS * 8 doubles of the scratch
  const double dn = (double)n;
  for (int q = wave; q < tc; q += TILE_THREADS / 64) {
    const double *x = px + q * ns, *z = pz + q * ns, *y = py + q * ns;
    double mx = 0.0, my = 0.0, mz = 0.0;
    for (int i = lane; i < n; i += 64) {
      mx += x[i];
      mz += z[i];
      if constexpr (!PLANAR) my += y[i];
    }
    mx = __shfl(wave_sum(mx), 0, 64) / dn;
    mz = __shfl(wave_sum(mz), 0, 64) / dn;
    if constexpr (!PLANAR) my = __shfl(wave_sum(my), 0, 64) / dn;
    double xx = 0.0, yy = 0.0, zz = 0.0, xy = 0.0, xz = 0.0, yz = 0.0;
    for (int i = lane; i < n; i += 64) {
      const double dx = x[i] - mx, dz = z[i] - mz;
      xx += dx * dx;
      zz += dz * dz;
      xz += dx * dz;
      if constexpr (!PLANAR) {
        const double dy = y[i] - my;
        yy += dy * dy;
        xy += dx * dy;
        yz += dy * dz;
      }
    }
    xx = wave_sum(xx) / dn;
    zz = wave_sum(zz) / dn;
    xz = wave_sum(xz) / dn;
    if constexpr (!PLANAR) {
      yy = wave_sum(yy) / dn;
      xy = wave_sum(xy) / dn;
      yz = wave_sum(yz) / dn;
    }
    if (lane == 0) {
      double *o = gy + q * PSTAT_SHAPE_GYR;
      o[0] = xx; o[1] = yy; o[2] = zz; o[3] = xy; o[4] = xz; o[5] = yz;
      o[6] = (xx + yy) + zz;
      o[7] = ((xx * xx + yy * yy) + zz * zz) + 2.0 * ((xy * xy + xz * xz) + yz * yz);
    }
  }
  __syncthreads();
  const int ncols = a.ncols;
  double *out = partial + (int64_t)blockIdx.x * 2 * ncols;
  if (t < PSTAT_SHAPE_GYR) {
    double r1 = 0.0, r2 = 0.0;
    for (int q = 0; q < tc; ++q) {
      const double v = gy[q * PSTAT_SHAPE_GYR + t];
      r1 += v;
      r2 += v * v;
    }
    out[t] = r1;
    out[ncols + t] = r2;
  }
  if (a.nq == 0) return;                                            // uniform
  __syncthreads();                                                  // the scratch is rewritten below

  // phase 4: thread (g, sub) takes the wave-vectors sub, sub + lpc, ... of the chains g, g + groups, ...
  const int sub = t % a.lpc, g = t / a.lpc;
  for (int j = 0; j < a.nslots; ++j) {                               // uniform: every thread meets every barrier
    const int k = sub + j * a.lpc;
    const bool active = k < a.nq;
    double r1 = 0.0, r2 = 0.0;
    if (active) {
      const double qx = qtab[3 * k], qy = qtab[3 * k + 1], qz = qtab[3 * k + 2];
      for (int q = g; q < tc; q += a.groups) {
        const double *x = px + q * ns, *z = pz + q * ns, *y = py + q * ns;
        double sc = 0.0, ss = 0.0;
        for (int i = 0; i < n; ++i) {
          double ph = qx * x[i];
          if constexpr (!PLANAR) ph += qy * y[i];
          ph += qz * z[i];
          double sn, cs;
          sincos_f64(ph, &sn, &cs);
          sc += cs;
          ss += sn;
        }
        const double v = (sc * sc + ss * ss) / dn;
        r1 += v;
        r2 += v * v;
      }
    }
    tile_group_fold(a, lds, sub, g, active, r1, r2);
    if (g == 0 && active) {
      out[PSTAT_SHAPE_GYR + k] = r1;
      out[ncols + PSTAT_SHAPE_GYR + k] = r2;
    }
  }
}

}  // namespace

hipError_t launch_shape(const ShapeArgs &a, const void *ang, const CaseConst *cases, const double *q, double *partial,
                        double *totals, double *row, hipStream_t stream) {
  int64_t blocks;
  size_t lds;
  hipError_t e = tile_launch_shape(a, &blocks, &lds);
  if (e != hipSuccess || blocks == 0) return e;
  const dim3 grid((unsigned)blocks), block(TILE_THREADS);
  if (a.planar) shape_stage1<true><<<grid, block, lds, stream>>>(a, ang, cases, q, partial);
  else shape_stage1<false><<<grid, block, lds, stream>>>(a, ang, cases, q, partial);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_tile_fold(a, partial, totals, row, stream);
}

}  // namespace pstat
