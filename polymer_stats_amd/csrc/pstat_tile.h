// pstat_tile.h -- the tile frame under the correlation, the shape and the pair-distance recorder (pstat_corr.hip,
// pstat_shape.hip, pstat_pdist.hip; TileArgs and tile_layout are in pstat_device.h).  A workgroup (case, tile) of 256 threads
// takes `tile_chains` consecutive chains of one case, leaves their unit vectors in LDS behind 4 KiB of scratch, and its `groups`
// groups of `lpc` threads fold their (sum, sumsq) through that scratch; tile_fold then adds the tiles' partials per (case,
// column).  Every order below is part of the recorders' results: tests/corr_ref.py and tests/shape_ref.py restate it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pstat_device.h"
#include "pstat_math.h"

namespace pstat {

constexpr int TILE_THREADS = 256;
constexpr int TILE_CHAINS = 16;                     // chains per workgroup at most
constexpr size_t TILE_LDS = 65536;                  // what a workgroup may have
constexpr size_t TILE_SCRATCH = 2 * TILE_THREADS * sizeof(double);   // the groups' sums on their way to group 0

// monomers of a chain as LDS keeps them: odd where several chains share a tile, so that the phase-1 stores of consecutive chains
// do not meet in one bank
__host__ __device__ inline int64_t padded_n(const int64_t n, const int tile_chains) { return tile_chains > 1 ? (n | 1) : n; }

// the scratch and the unit vectors of `tile_chains` chains of n monomers
inline size_t tile_lds_bytes(const int64_t n, const int tile_chains, const int planar) {
  return TILE_SCRATCH + (size_t)tile_chains * (size_t)padded_n(n, tile_chains) * (planar ? 2 : 3) * sizeof(double);
}

// What both launchers check in front of stage 1: the grid's blocks (0: nothing to launch) and the workgroup's LDS bytes.
hipError_t tile_launch_shape(const TileArgs &a, int64_t *blocks, size_t *lds);
// The fold over the tiles of one record, one wavefront per (case, column): lane l adds the partials
// [ncases][tiles][sum | sumsq][ncols] of the case's tiles l, l + 64, ... in order from 0.0, wave_sum's tree follows, lane 0 adds
// the two results to totals[2][ncases][ncols] and writes the row's mean (unless row is null).
hipError_t launch_tile_fold(const TileArgs &a, const double *partial, double *totals, double *row, hipStream_t stream);

// A workgroup's tile: its case, its chains, and where their unit vectors lie in LDS.
struct Tile {
  int64_t kcase, first;  // its case; its first chain within the case
  int tc, ns;            // chains this tile holds; monomers of a chain as LDS keeps them
  double *x, *z, *y;     // x[q][i], z[q][i], (y[q][i]: 3D only) for chain q of the tile, one array behind the other
};

// the tile of workgroup blockIdx.x, its vectors in `lds` behind the scratch
__device__ __forceinline__ Tile tile_of(const TileArgs &a, double *lds) {
  Tile w;
  w.kcase = (int64_t)blockIdx.x / a.tiles;
  w.first = ((int64_t)blockIdx.x % a.tiles) * a.tile_chains;
  const int64_t left = a.per - w.first;
  w.tc = (int)(left < a.tile_chains ? left : a.tile_chains);
  w.ns = (int)padded_n(a.n, a.tile_chains);
  w.x = lds + 2 * TILE_THREADS;
  w.z = w.x + (int64_t)a.tile_chains * w.ns;
  w.y = w.z + (int64_t)a.tile_chains * w.ns;
  return w;
}

// Phase 1: the threads load the tile's angles with the chain index fastest, so a row of 16 chains is one 128-byte segment of
// DevState::ang, take two sincos per monomer (one for a planar handle) and leave the unit vectors in LDS.  Ends in a barrier.
template <bool PLANAR>
__device__ __forceinline__ void tile_unit_vectors(const TileArgs &a, const Tile &w, const void *__restrict__ ang) {
  const int64_t c0 = w.kcase * a.per + w.first, C = a.ncases * a.per;
  const int n = (int)a.n, tc = w.tc, ns = w.ns;
  for (int e = threadIdx.x; e < tc * n; e += TILE_THREADS) {
    const int q = e % tc, i = e / tc;
    double sp, cp;
    sincos_f64(load_angle(ang, ((int64_t)n + i) * C + c0 + q, (size_t)a.elem, false), &sp, &cp);
    if constexpr (PLANAR) {
      w.x[q * ns + i] = cp;
      w.z[q * ns + i] = sp;
    } else {
      double st, ct;
      sincos_f64(load_angle(ang, (int64_t)i * C + c0 + q, (size_t)a.elem, true), &st, &ct);
      w.x[q * ns + i] = cp * st;
      w.y[q * ns + i] = sp * st;
      w.z[q * ns + i] = ct;
    }
  }
  __syncthreads();
}

// inclusive scan over the 64 lanes: the shift-and-add tree whose order is part of every position
__device__ __forceinline__ double wave_scan(double v, const int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double up = __shfl_up(v, off, 64);
    if (lane >= off) v += up;
  }
  return v;
}

// Phase 2 of the recorders that read positions (pstat_shape.hip, pstat_pdist.hip): the prefix sum, in place, from the unit
// vectors to x_i = b (sum_{j <= i} n_j - n_i / 2).  A wavefront takes one (chain, component) sequence at a time: lane l sums its
// segment of ceil(n / 64) consecutive monomers in order, the lanes' sums go through wave_scan, and the lane rewrites its segment
// as b (running sum - n_i / 2).  The tree depends on n alone.  Ends in a barrier.
template <bool PLANAR>
__device__ __forceinline__ void tile_positions(const TileArgs &a, const Tile &w, const double b) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = (int)a.n, tc = w.tc, ns = w.ns;
  constexpr int COMPS = PLANAR ? 2 : 3;
  const int seg = (n + 63) / 64;
  for (int s = wave; s < COMPS * tc; s += TILE_THREADS / 64) {      // sequence s = (component, chain) of the tile
    double *v = w.x + (int64_t)(s / tc) * a.tile_chains * ns + (s % tc) * ns;   // x, z, y lie one behind the other
    const int i0 = lane * seg, i1 = i0 + seg < n ? i0 + seg : n;
    double mine = 0.0;
    for (int i = i0; i < i1; ++i) mine += v[i];
    const double before = __shfl_up(wave_scan(mine, lane), 1, 64);
    double run = lane ? before : 0.0;                               // what lies before this lane's segment
    for (int i = i0; i < i1; ++i) {
      const double u = v[i];
      run += u;
      v[i] = b * (run - 0.5 * u);
    }
  }
  __syncthreads();
}

// The groups' (r1, r2) of one column, added in order of g from 0.0 by group 0 through the scratch at `lds`: afterwards the
// active threads of group 0 hold the tile's.  Thread (g, sub) = (t / lpc, t % lpc); every thread of the workgroup calls it (two
// barriers where there are groups to fold).
__device__ __forceinline__ void tile_group_fold(const TileArgs &a, double *lds, const int sub, const int g, const bool active,
                                                double &r1, double &r2) {
  if (a.groups <= 1) return;
  double *s1 = lds, *s2 = lds + TILE_THREADS;
  const int t = threadIdx.x;
  s1[t] = r1; s2[t] = r2;
  __syncthreads();
  if (g == 0 && active) {
    r1 = 0.0; r2 = 0.0;
    for (int gg = 0; gg < a.groups; ++gg) { r1 += s1[sub + gg * a.lpc]; r2 += s2[sub + gg * a.lpc]; }
  }
  __syncthreads();   // the scratch is rewritten for the next column
}

}  // namespace pstat
