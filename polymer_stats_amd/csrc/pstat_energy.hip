// pstat_energy.hip -- what a chain's energy is made of, on the device: per case the field term, the work of the force, the bending
// term and the dipole-dipole sum by separation along the chain, with the part beyond max_sep and the part within a radius.
//
// THE CONTRACT (restated, not shared, in tests/energy_ref.py; include/pstat.h).  Everything is f64, from the
// doubles load_angle gives for the stored angles (radians | turns | lattice index), whatever the handle's precision:
//   unit vectors,   exactly the correlation recorder's: n_i = (cos phi_i sin theta_i, sin phi_i sin theta_i, cos theta_i);
//   dipoles         dielectric mu_i = (K1 - K2) E0 cos theta_i n_i + K2 E0 z, polar mu_i = mu n_i, as f n_i + mb z with
//                   f = ((K1 - K2) E0) n_{i,z} | mu and mb = K2 E0 | 0, every product rounded.  A planar handle's
//                   n_i = (cos phi_i, sin phi_i) sits in the x and z slots, y = 0: sin phi_i stands where cos theta_i does and
//                   the field axis is the second component.
//   positions       exactly the shape recorder's: x_i = b (sum_{j <= i} n_j - n_i / 2) by tile_positions, whose scan order is
//                   part of the result.
//   pair term       for i < j: d = x_j - x_i;  r2 = (d_x d_x + d_y d_y) + d_z d_z (planar: d_x d_x + d_z d_z);  r = sqrt(r2),
//                   correctly rounded;  mm = (mu_ix mu_jx + mu_iy mu_jy) + mu_iz mu_jz, a = mu_i . d and c = mu_j . d added the
//                   same way (planar: without the y product);
//                       t_ij = (mm - 3 ((a c) / r2)) / (FOURPI (r2 r)),   FOURPI = 4.0 * 3.14159265358979323846 as a double.
//                   Every operation is rounded (built with -ffp-contract=off), the divisions are IEEE.  r = 0 gives 0 / 0: a
//                   non-finite term, which reaches the totals of the columns it belongs to and nothing else (the reference's own
//                   0 * inf, inc/eap_chain.jl:200-207).
//   options         max_sep in 0 .. n - 1 (-1: n - 1); cutoff >= 0 in monomer lengths, one for all cases or one per case, 0: no
//                   `within` column.  On the device crad = cutoff * b, crad2 = crad * crad, both products rounded in f64, and a
//                   pair counts unless r2 > crad2: the comparison of the cutoff step kernel (pstat_wave.h, `r2 > crad2 ? 0 : t`)
//                   and its crad2 = (cutoff_radius b)(cutoff_radius b) of pstat_cluster_wave.hip, which an f64 handle rounds at
//                   the same places (an f32 handle rounds that product to float once more; this recorder does not).
//                   n >= 1: a chain of one monomer has no pair columns beyond rest = 0.
//   columns per chain, in this order (ncols = 3 + max_sep + 1 + (cutoff ? 1 : 0)):
//     field   sum_i (-E0 / 2) mu_{i,z}                       (planar: the second component)
//     work    -(Fx R_x + Fz R_z),  R = x_{n-1} + (b / 2) n_{n-1}
//     bend    sum_{i < n-1} ((kappa / 2) (psi_i - psi0)) (psi_i - psi0),  psi_i = acos_r(min(1, max(-1, n_i . n_{i+1}))), the dot
//             product added as mm is.  Exactly 0.0, with no acos evaluated, when the case's kappa (bend_mod) is 0.
//     pair[s] s = 1 .. max_sep:  sum_{i = 0}^{n-1-s} t_{i,i+s}
//     rest    sum_{s > max_sep} pair[s]; exactly 0.0 when max_sep = n - 1
//     within  sum_{i<j, r2 <= crad2} t_ij; only when cutoff is set
//   The pair columns hold the dipole-dipole sum whatever the handle's energy type.  The energy the handle's own step carries:
//     non-interacting  field + work + bend;   Ising  that + pair[1];   interacting  that + sum_s pair[s] + rest;
//     cutoff  within alone, at the case's cutoff_radius (the reference's UCutoff: no field, no force).
//   Per case and column one record adds sum_c v to `sum` and sum_c v * v to `sumsq`; a row, when the object keeps rows, is
//   sum_c v / num_chains.
//
// The order of every floating-point addition is fixed by (ncases, num_chains, n, the object's options) alone -- no floating-point
// atomics, nothing that depends on the number of CUs or on which workgroup arrives first:
//   energy_stage1  workgroup (case, tile) of 256 threads takes `tile_chains` consecutive chains of one case, as corr_stage1 does.
//       Phase 1 (tile_unit_vectors) leaves the unit vectors in LDS; each thread then writes its monomers' dipoles into a second
//       array of the same layout behind them (48 n bytes per chain, 32 n planar) and the chain's last unit vector into the
//       scratch.  field and bend: wavefront w takes the tile's chains w, w + 4, ...; lane l adds the terms i = l, l + 64, ... in
//       order from 0.0, wave_sum's tree follows.  Phase 2 (tile_positions) rewrites the vectors as positions; thread q then
//       forms chain q's work.  The pairs: wavefront w takes u = 1 + w, 5 + w, ... up to floor(n / 2) and with u the TWO
//       separations s = u and s' = n - u (one when they coincide), which have n pairs together: for each chain of the tile in
//       chain order, lane l takes p = l, l + 64, ... of 0 .. n - 1; p < n - u is the pair (p, p + u) of s, any other the pair
//       (p - (n - u), p + s' - (n - u)) of s'.  A lane adds its terms of s and of s' apart, in order of p from 0.0; wave_sum gives
//       the chain's pair[s] and pair[s'].  (A separation per wavefront pass, as pdist's R2(s) has it, leaves 42 % of the lane
//       slots empty at n = 100, the pairing 22 %: 4.09 ms against 3.53 ms per record of 65 536 chains)  A column s <= max_sep joins its
//       (sum, sumsq) in lane 0's registers, so it is folded over the tile's chains in chain order from 0.0; a separation
//       beyond max_sep is added to the wavefront's `rest` of that chain in LDS, in the order the wavefront meets it (u
//       ascending, s before s'), and the same with the terms inside the radius for `within`.  Behind a barrier thread k < 5
//       folds column k of (field, work, bend, rest, within) over the tile's chains in chain order from 0.0, where a chain's
//       rest and within are its four wavefronts' added in order of w from 0.0.  The tile's partial leaves as
//       partial[tile][sum | sumsq][column].
//   tile_fold      (pstat_corr.hip) the fold over the tiles per (case, column).
// LDS: the tile frame's 4 KiB of scratch, the positions and the dipoles.  pstat_energy_open refuses a chain whose two arrays do
// not fit: n <= energy_max_n(planar) = 61440 / (48 | 32 planar) = 1280 | 1920.
// It reads DevState::ang and the case table only and writes the energy object's own buffers only.  Plain HIP C++.
#include <hip/hip_runtime.h>

#include "../../include/pstat.h"
#include "pstat_device.h"
#include "pstat_math.h"
#include "pstat_tile.h"

namespace pstat {

namespace {

constexpr int ENERGY_WAVES = TILE_THREADS / 64;
// the scratch, in doubles: the chains' last unit vectors, their five O(n) / folded values, the wavefronts' rest and within
constexpr int EN_LAST = 0, EN_VAL = 3 * TILE_CHAINS, EN_PART = EN_VAL + 5 * TILE_CHAINS;
static_assert(EN_PART + 2 * ENERGY_WAVES * TILE_CHAINS <= 2 * TILE_THREADS, "the energy recorder's scratch fits the frame's");

constexpr double FOURPI = 4.0 * 3.14159265358979323846;

template <bool PLANAR>
__global__ __launch_bounds__(TILE_THREADS) void energy_stage1(const EnergyArgs a, const void *__restrict__ ang,
                                                              const CaseConst *__restrict__ cases,
                                                              const double *__restrict__ cuttab, double *__restrict__ partial) {
  extern __shared__ double lds[];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const Tile w = tile_of(a, lds);
  const int n = (int)a.n, tc = w.tc, ns = w.ns;
  constexpr int COMPS = PLANAR ? 2 : 3;
  const CaseConst cc = cases[w.kcase];
  tile_unit_vectors<PLANAR>(a, w, ang);

  double *const mx = w.x + (int64_t)COMPS * a.tile_chains * ns;      // the dipoles, laid out as the vectors are
  double *const mz = mx + (int64_t)a.tile_chains * ns, *const my = mz + (int64_t)a.tile_chains * ns;
  double *const last = lds + EN_LAST, *const val = lds + EN_VAL, *const part = lds + EN_PART;
  {
    double ma, mb = 0.0;                                             // mu = f n + mb z, f = ma n_z (dielectric) or mu (polar)
    if (a.polar) ma = cc.mu;
    else { ma = (cc.K1 - cc.K2) * cc.E0; mb = cc.K2 * cc.E0; }
    for (int e = t; e < tc * n; e += TILE_THREADS) {
      const int at = (e % tc) * ns + e / tc;
      const double f = a.polar ? ma : ma * w.z[at];
      mx[at] = f * w.x[at];
      if constexpr (!PLANAR) my[at] = f * w.y[at];
      mz[at] = f * w.z[at] + mb;
    }
    if (t < tc) {
      last[t] = w.x[t * ns + n - 1];
      last[TILE_CHAINS + t] = w.z[t * ns + n - 1];
      last[2 * TILE_CHAINS + t] = PLANAR ? 0.0 : w.y[t * ns + n - 1];
    }
    for (int e = t; e < 2 * ENERGY_WAVES * TILE_CHAINS; e += TILE_THREADS) part[e] = 0.0;
  }
  __syncthreads();

  // field and bend: a wavefront per chain
  const double mhalfE0 = -0.5 * cc.E0, khalf = cc.kappa / 2, psi0 = cc.psi0;
  for (int q = wave; q < tc; q += ENERGY_WAVES) {
    const double *x = w.x + q * ns, *z = w.z + q * ns, *y = w.y + q * ns;
    double f = 0.0, bd = 0.0;
    for (int i = lane; i < n; i += 64) f += mhalfE0 * mz[q * ns + i];
    if (cc.kappa != 0.0) {
      for (int i = lane; i < n - 1; i += 64) {
        double dot = x[i] * x[i + 1];
        if constexpr (!PLANAR) dot += y[i] * y[i + 1];
        dot += z[i] * z[i + 1];
        const double dpsi = acos_r(fmin(1.0, fmax(-1.0, dot))) - psi0;
        bd += (khalf * dpsi) * dpsi;
      }
      bd = wave_sum(bd);
    }
    f = wave_sum(f);
    if (lane == 0) {
      val[0 * TILE_CHAINS + q] = f;
      val[2 * TILE_CHAINS + q] = bd;
    }
  }
  __syncthreads();                                                   // the vectors are read; they become positions
  tile_positions<PLANAR>(a, w, cc.b);
  if (t < tc) {
    const double hb = cc.b / 2;
    const double Rx = w.x[t * ns + n - 1] + hb * last[t], Rz = w.z[t * ns + n - 1] + hb * last[TILE_CHAINS + t];
    val[1 * TILE_CHAINS + t] = -(cc.Fx * Rx + cc.Fz * Rz);
  }

  // the pairs: wavefront w takes u = 1 + w, 5 + w, ... and with it the separations u and n - u (a.paired; else u alone, up to n - 1)
  const int ncols = a.ncols, max_sep = a.max_sep;
  const bool cut = a.cut != 0;
  double crad2 = 0.0;
  if (cut) {
    const double crad = cuttab[w.kcase] * cc.b;
    crad2 = crad * crad;
  }
  double *out = partial + (int64_t)blockIdx.x * 2 * ncols;
  const int umax = a.paired ? n / 2 : n - 1;
  for (int u = 1 + wave; u <= umax; u += ENERGY_WAVES) {
    const int s2 = a.paired && n - u != u ? n - u : 0;               // the second separation (0: none) has u pairs
    const int cnt1 = n - u, cnt = cnt1 + (s2 ? u : 0);
    double p1 = 0.0, p2 = 0.0, o1 = 0.0, o2 = 0.0;                   // (sum, sumsq) of the columns u and s2, in lane 0
    for (int q = 0; q < tc; ++q) {
      const double *x = w.x + q * ns, *z = w.z + q * ns, *y = w.y + q * ns;
      const double *ux = mx + q * ns, *uz = mz + q * ns, *uy = my + q * ns;
      double sa = 0.0, sb = 0.0, ia = 0.0, ib = 0.0;                 // the lane's terms of u and of s2; those inside the radius
      for (int p = lane; p < cnt; p += 64) {
        const bool second = p >= cnt1;
        const int i = second ? p - cnt1 : p, j = i + (second ? s2 : u);
        const double dx = x[j] - x[i], dz = z[j] - z[i];
        double r2 = dx * dx, mm = ux[i] * ux[j], ai = ux[i] * dx, cj = ux[j] * dx;
        if constexpr (!PLANAR) {
          const double dy = y[j] - y[i];
          r2 += dy * dy;
          mm += uy[i] * uy[j];
          ai += uy[i] * dy;
          cj += uy[j] * dy;
        }
        r2 += dz * dz;
        mm += uz[i] * uz[j];
        ai += uz[i] * dz;
        cj += uz[j] * dz;
        const double r = sqrt(r2);
        const double term = (mm - 3.0 * ((ai * cj) / r2)) / (FOURPI * (r2 * r));
        const double in = r2 > crad2 ? 0.0 : term;
        if (second) { sb += term; ib += in; }
        else { sa += term; ia += in; }
      }
      const double va = wave_sum(sa), vb = s2 ? wave_sum(sb) : 0.0;  // (lane 0's is the wavefront's)
      double rest = 0.0;
      bool any_rest = false;
      if (u <= max_sep) { p1 += va; p2 += va * va; }
      else { rest += va; any_rest = true; }
      if (s2) {
        if (s2 <= max_sep) { o1 += vb; o2 += vb * vb; }
        else { rest += vb; any_rest = true; }
      }
      if (cut) {
        const double wa = wave_sum(ia), wb = s2 ? wave_sum(ib) : 0.0;
        if (lane == 0) part[(ENERGY_WAVES + wave) * TILE_CHAINS + q] += s2 ? wa + wb : wa;
      }
      if (lane == 0 && any_rest) part[wave * TILE_CHAINS + q] += rest;
    }
    if (lane == 0) {
      if (u <= max_sep) { out[2 + u] = p1; out[ncols + 2 + u] = p2; }
      if (s2 && s2 <= max_sep) { out[2 + s2] = o1; out[ncols + 2 + s2] = o2; }
    }
  }
  __syncthreads();
  if (t < 5 && (t < 4 || cut)) {
    double r1 = 0.0, r2 = 0.0;
    for (int q = 0; q < tc; ++q) {
      double v;
      if (t < 3) v = val[t * TILE_CHAINS + q];
      else {
        v = 0.0;
        for (int k = 0; k < ENERGY_WAVES; ++k) v += part[((t - 3) * ENERGY_WAVES + k) * TILE_CHAINS + q];
      }
      r1 += v;
      r2 += v * v;
    }
    const int col = t < 3 ? t : max_sep + t;                         // rest at 3 + max_sep, within behind it
    out[col] = r1;
    out[ncols + col] = r2;
  }
}

size_t energy_dipole_bytes(const EnergyArgs &a) {
  return (size_t)a.tile_chains * (size_t)padded_n(a.n, a.tile_chains) * (a.planar ? 2 : 3) * sizeof(double);
}

}  // namespace

int64_t energy_max_n(const int planar) { return (int64_t)((TILE_LDS - TILE_SCRATCH) / (2 * (planar ? 2 : 3) * sizeof(double))); }

void energy_layout(EnergyArgs &a) {
  tile_layout(a, 64);                                                // (lpc, groups: the frame's; the pairs have their own mapping)
  while (a.tile_chains > 1 && tile_lds_bytes(a.n, a.tile_chains, a.planar) + energy_dipole_bytes(a) > TILE_LDS) --a.tile_chains;
  a.tiles = (a.per + a.tile_chains - 1) / a.tile_chains;
}

hipError_t launch_energy(const EnergyArgs &a, const void *ang, const CaseConst *cases, const double *cutoff, double *partial,
                         double *totals, double *row, hipStream_t stream) {
  int64_t blocks;
  size_t lds;
  hipError_t e = tile_launch_shape(a, &blocks, &lds);
  if (e != hipSuccess || blocks == 0) return e;
  lds += energy_dipole_bytes(a);
  if (lds > TILE_LDS || a.n < 1 || a.max_sep < 0 || a.max_sep > a.n - 1 || a.ncols != 3 + a.max_sep + 1 + (a.cut ? 1 : 0) ||
      (a.cut && !cutoff))
    return hipErrorInvalidConfiguration;
  const dim3 grid((unsigned)blocks), block(TILE_THREADS);
  if (a.planar) energy_stage1<true><<<grid, block, lds, stream>>>(a, ang, cases, cutoff, partial);
  else energy_stage1<false><<<grid, block, lds, stream>>>(a, ang, cases, cutoff, partial);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_tile_fold(a, partial, totals, row, stream);
}

}  // namespace pstat
