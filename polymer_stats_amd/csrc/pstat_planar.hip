// pstat_planar.hip -- the step of the planar main, 2D/mcmc_clustering_eap_chain.jl:238-278, on gfx950 (home Planar).
//
// The planar chain has one angle per monomer: n_i = (cos phi_i, sin phi_i), the field and Fz act on the second
// component (2D/inc/energy.jl:8, 2D/inc/eap_chain.jl:64).  It is the 3D chain confined to the x-z plane with sin(phi) in
// the place of cos(theta): component 1 lives in the x slots of every observable, component 2 in the z slots, and every y
// slot stays exactly 0.  No sin(theta) Jacobian enters the target density (2D/inc/acceptance.jl:18-22).
//
// One step = ONE proposal: the single-monomer move phi_idx += dphi (move!, 2D/inc/eap_chain.jl:171-186; phi is not
// wrapped) and then cluster_flip! on the trial chain (:194-257): with probability cluster_prob the cluster grown from the
// moved monomer -- link (i, i+1) joins with probability (1 + n_i . n_{i+1}) / 2 -- is INVERTED, phi_i += pi for every
// member (flip_n!, :188-190: n -> -n, not the 3D main's reflection), and the proposal is accepted by
// Metropolis-Hastings with alpha = the ratio of the boundary probabilities after and before (:249-252).
//
// Layout: one chain per lane, phi ONLY in LDS as 8-byte cells [monomer][lane], everything else in registers, the
// persistent (block, segment) job queue of pstat_device.h.  The reference's cached cos / sin are pure functions of the
// stored phi (move! and the flip both recompute them from phi, :173-175), so deriving n from phi for every row visited is
// the reference's own arithmetic.  An inversion leaves every interior bond's pair energy unchanged (both dipoles and the
// bond vector change sign together, or -- dielectric -- the dipoles do not change at all), so the energy difference of the
// whole proposal is the single move's O(1) difference, two boundary bonds, and the members' force (and, polar, field)
// terms, which are accumulated while the cluster grows.
//
// THE PLANAR RANDOM-STREAM CONTRACT (restated, not shared, in tests/planar/planar_ref.c).  Generators and seeding as in
// pstat_device.h; u(w) = (w >> 9) 2^-23; idx = mulhi32(w, n).
//   start    n words, phi_i = 2 pi u(w_i)
//   a step   w_idx, w_phi, w_flip, [growth words], w_eps
// with flip = u(w_flip) <= cluster_prob.  Growth words are drawn only if the step flips: round t tests the link above the
// cluster, then the link below it, each with its own word while that end is still growing; an end at the end of the chain
// draws nothing.  The 53-bit eps takes its low 21 bits from the low 9 of w_phi, the low 9 of w_flip and the low 3 of
// w_idx (eps_uniform with the flip word in the place the 3D step's dphi word has and the dphi word in its dtheta word's),
// so uniform_bits 23 and 53 consume the same stream.  The reference draws idx, dphi, grows right to completion, grows
// left, then draws the flip decision and eps.  The departures keep the law of the step: the flip decision depends on
// nothing the growth produces and keeps its own iid draw; a cluster that is not flipped is thrown away by the reference
// too (alpha = 1, the trial is the single move), so not growing it changes no chain; the two ends test disjoint links
// with iid draws, so interleaving them leaves the law of (lower, upper) alone.
//
// Reference behaviour kept on purpose: the acceptor caches log(pi) + log(alpha) of the last accepted proposal
// (2D/inc/acceptance.jl:31-34), so later comparisons are offset by that log(alpha) -- `lag` below; the 1/2 in u on polar
// chains; a run records from its first step.
#include <hip/hip_runtime.h>

#include "pstat_device.h"
#include "pstat_math.h"

namespace pstat {

namespace {

struct P2 { double x, z; };
__device__ __forceinline__ double dot2(const P2 &a, const P2 &b) { return a.x * b.x + a.z * b.z; }

// dipole of one monomer, 2D/inc/dipole_response.jl:7-10 (dielectric: (K1-K2) E0 sin(phi) n + (0, K2 E0)), :25-27 (polar)
template <int CT>
__device__ __forceinline__ P2 dipole2(const double a_or_mu, const double k2e, const P2 &nh) {
  if constexpr (CT == PSTAT_DIELECTRIC) {
    const double a = a_or_mu * nh.z;
    return P2{a * nh.x, a * nh.z + k2e};
  } else {
    return P2{a_or_mu * nh.x, a_or_mu * nh.z};
  }
}

// one dipole-dipole term of neighbours (2D/inc/eap_chain.jl:156-169: the 3D kernel 1 / (4 pi r^3) on 2-vectors) for the
// bond vector r = x_i - x_j; the algebraic form of pair_term_fast (pstat_math.h).  r = 0 gives NaN, as the literal form does.
__device__ __forceinline__ double pair2(const double rx, const double rz, const P2 &mi, const P2 &mj) {
  const double r2 = __builtin_fma(rz, rz, rx * rx);
  const double y = rsqrt_f64(r2);
  const double ir2 = y * y;
  const double mimj = __builtin_fma(mi.z, mj.z, mi.x * mj.x);
  const double mir = __builtin_fma(mi.z, rz, mi.x * rx);
  const double mjr = __builtin_fma(mj.z, rz, mj.x * rx);
  const double num = __builtin_fma(-3.0 * ir2, mir * mjr, mimj);
  return num * (ir2 * y) * 0.0795774715459476679;   // 1 / (4 pi)
}

template <typename G, int CT, int EN>
__device__ __forceinline__ void run_planar_segment(const SweepArgs &A, const DevState &S, const CaseConst &cc, const int umb_on,
                                                   unsigned char *smem, const int lane, const int64_t c, int64_t step,
                                                   int64_t remaining) {
  double *ang = reinterpret_cast<double *>(smem);   // [n][lanes]: phi, radians
  const int lanes = A.lanes;
  const int64_t C = S.C;
  const int n = (int)A.n;
  constexpr double PI = 3.14159265358979323846;

  const double Fz = cc.Fz, Fx = cc.Fx, b = cc.b, kT = cc.kT;
  const double a_or_mu = (CT == PSTAT_DIELECTRIC) ? (cc.K1 - cc.K2) * cc.E0 : cc.mu;
  const double k2e = cc.K2 * cc.E0;
  const double mhalfE0 = -0.5 * cc.E0;
  const double hb = -cc.b / 2;
  const double cprob = cc.cluster_prob;

  double *gph = (double *)S.ang + (int64_t)n * C;   // the phi plane (the theta plane is zero and never read)
#pragma unroll 8
  for (int i = 0; i < n; ++i) ang[i * lanes + lane] = gph[(int64_t)i * C + c];

  G g;
  g.load(S.rng + c, C);
  double phistep = S.stepsz[0 * C + c];
  int64_t nacc_off = S.win[0 * C + c], natt_off = S.win[1 * C + c];
  int nacc_seg = 0, steps_seg = 0, nnan_seg = 0;
  double Orx = S.obs[OBS_R1 * C + c], Orz = S.obs[OBS_R3 * C + c];
  double Opx = S.obs[OBS_P1 * C + c], Opz = S.obs[OBS_P3 * C + c];
  double OU = S.obs[OBS_U * C + c], usum = S.obs[OBS_USUM * C + c];
  double lag = S.lag[c];                            // log(alpha) of the last accepted proposal of this mcmc() call
  const bool umb = umb_on != 0;
  const double wscale = umb ? umbrella_wscale(cc) : 0.0;
  double uref = umb ? S.uref[c] : 0.0;
  bool regauged = false;
  double wnorm = umb ? S.wnorm[c] : 0.0;
  // the ten running sums a planar chain records (the y slots, S_C2 and S_PSI stay 0)
  double s1[5] = {S.sums[S_R1 * C + c], S.sums[S_R3 * C + c], S.sums[S_P1 * C + c], S.sums[S_P3 * C + c], S.sums[S_U * C + c]};
  double s2[5] = {S.sums[S_R1SQ * C + c], S.sums[S_R3SQ * C + c], S.sums[S_P1SQ * C + c], S.sums[S_P3SQ * C + c],
                  S.sums[S_USQ * C + c]};

  const int64_t spa = A.steps_per_adjust;
  int64_t to_adj = A.adaptive ? spa - (step % spa) : 0;
  constexpr int FLUSH = 128;
  int left = (int)remaining;

  auto nhat_of = [](const double ph) __attribute__((always_inline)) -> P2 {
    double s, co;
    Ang<double>::sc_phi(ph, &s, &co);
    return P2{co, s};
  };
  auto load_n = [&](const int i) __attribute__((always_inline)) -> P2 { return nhat_of(ang[i * lanes + lane]); };
  // the Ising energy of bond (a, b), a the lower monomer: bond vector x_a - x_b = -b/2 (n_a + n_b)
  auto bond = [&](const P2 &na, const P2 &ma, const P2 &nb, const P2 &mb) __attribute__((always_inline)) -> double {
    if constexpr (EN == PSTAT_ISING) return pair2(hb * (na.x + nb.x), hb * (na.z + nb.z), ma, mb);
    else return 0.0;
  };
  auto neg = [](const P2 &v) __attribute__((always_inline)) -> P2 { return P2{-v.x, -v.z}; };
  // the dipole of an inverted monomer: dielectric mu is even in n, polar mu odd
  auto inv_mu = [&](const P2 &m) __attribute__((always_inline)) -> P2 {
    if constexpr (CT == PSTAT_DIELECTRIC) return m;
    else return P2{-m.x, -m.z};
  };

  while (left > 0) {
    int chunk = left < FLUSH ? left : FLUSH;
    if (A.adaptive && to_adj < chunk) chunk = (int)to_adj;
    double a1[5] = {0, 0, 0, 0, 0}, a2[5] = {0, 0, 0, 0, 0};
    double accw = 0;

    for (int s = 0; s < chunk; ++s) {
      // ---- the single-monomer part, 2D/mcmc_clustering_eap_chain.jl:239-242
      const uint32_t w0 = g.next();
      const int idx = (int)__umulhi(w0, (uint32_t)n);
      const uint32_t wphi = g.next(), wflip = g.next();
      const int cell = idx * lanes + lane;
      const double ph0 = ang[cell];
      // (the trajectory itself: the product rounded before its sum, as the restatement and Julia round it -- through an
      // opaque register, so that no build flag can fuse it)
      auto rounded = [](double v) __attribute__((always_inline)) -> double { asm volatile("" : "+v"(v)); return v; };
      const double ph1 = ph0 + rounded(phistep * sym11<double>(wphi));
      const P2 n0 = nhat_of(ph0), n1 = nhat_of(ph1);
      const P2 m0 = dipole2<CT>(a_or_mu, k2e, n0), m1 = dipole2<CT>(a_or_mu, k2e, n1);
      const bool hasL = idx > 0, hasR = idx + 1 < n;
      // the two neighbours, branch-free: at a chain end the clamped index re-reads the monomer itself and the bond's
      // contribution is masked out
      const P2 nL = load_n(max(idx - 1, 0)), nR = load_n(min(idx + 1, n - 1));
      const double du_field = mhalfE0 * (m1.z - m0.z);
      double dpair = 0;
      if constexpr (EN == PSTAT_ISING) {
        const P2 mL = dipole2<CT>(a_or_mu, k2e, nL), mR = dipole2<CT>(a_or_mu, k2e, nR);
        const double dl = bond(nL, mL, n1, m1) - bond(nL, mL, n0, m0);
        const double dr = bond(n1, m1, nR, mR) - bond(n0, m0, nR, mR);
        dpair = (hasL ? dl : 0.0) + (hasR ? dr : 0.0);
      }

      // ---- cluster_flip!(trial, idx), 2D/inc/eap_chain.jl:194-257, in the contract's order (top of the file)
      double alpha = 1;
      int upper = idx, lower = idx;
      double drx_flip = 0, drz_flip = 0, du_flip = 0, dpair_flip = 0;
      P2 dp_flip{0, 0};
      const bool flipped = u01<double>(wflip) <= cprob;                      // :233
      if (__builtin_amdgcn_ballot_w64(flipped) != 0) {     // wave-uniform: skipped only if no lane flips at all
        P2 sn = n1;                   // sum of n over the members (the moved monomer enters as proposed)
        double upper_p = 0, lower_p = 0;
        // Both ends grow in ONE loop: round t tests the link above the cluster, (idx+t, idx+t+1), then the link below it,
        // (idx-t, idx-t-1), each with its own draw while that end is still growing.  Every lane still growing at round t
        // has accepted exactly t links on that side, so the rows visited depend on t only: the n-hats shift down a
        // window (A <- B <- the next row) and the only predicated state is the generator, the extents and the sums.
        P2 Au = n1, Bu = nR, Al = n1, Bl = nL;
        bool gu = flipped && hasR, gl = flipped && hasL;
        int rowu = min(idx + 2, n - 1), rowl = max(idx - 2, 0);
        while (__builtin_amdgcn_ballot_w64(gu || gl) != 0) {
          const P2 Cu = load_n(rowu), Cl = load_n(rowl);
          rowu = min(rowu + 1, n - 1); rowl = max(rowl - 1, 0);
          {
            const double p = (1 + dot2(Au, Bu)) / 2;
            G g2 = g;
            const bool acc = gu && (u01<double>(g2.next()) <= p);
            g.pick(gu, g2);
            upper_p = gu ? p : upper_p;
            upper += acc ? 1 : 0;
            sn.x += acc ? Bu.x : 0.0; sn.z += acc ? Bu.z : 0.0;
            gu = acc && upper < n - 1;
            Au = Bu; Bu = Cu;
          }
          {
            const double p = (1 + dot2(Al, Bl)) / 2;
            G g2 = g;
            const bool acc = gl && (u01<double>(g2.next()) <= p);
            g.pick(gl, g2);
            lower_p = gl ? p : lower_p;
            lower -= acc ? 1 : 0;
            sn.x += acc ? Bl.x : 0.0; sn.z += acc ? Bl.z : 0.0;
            gl = acc && lower > 0;
            Al = Bl; Bl = Cl;
          }
        }
        upper_p = upper >= n - 1 ? 0.0 : upper_p;   // ran into the chain end: no link to test, :203-206
        lower_p = lower <= 0 ? 0.0 : lower_p;       // :220-223
        // the two boundary bonds before and after the inversion (:239-248); their monomers are read back from LDS (the
        // moved monomer enters as proposed)
        P2 cu = load_n(upper), cl = load_n(lower);
        const P2 nu = load_n(min(upper + 1, n - 1)), nl = load_n(max(lower - 1, 0));
        const bool selfu = upper == idx, selfl = lower == idx;
        cu.x = selfu ? n1.x : cu.x; cu.z = selfu ? n1.z : cu.z;
        cl.x = selfl ? n1.x : cl.x; cl.z = selfl ? n1.z : cl.z;
        const bool onu = flipped && upper < n - 1, onl = flipped && lower > 0;
        const double new_upper_p = onu ? (1 + dot2(neg(cu), nu)) / 2 : 0.0;
        const double new_lower_p = onl ? (1 + dot2(neg(cl), nl)) / 2 : 0.0;
        if constexpr (EN == PSTAT_ISING) {
          const P2 cum = dipole2<CT>(a_or_mu, k2e, cu), clm = dipole2<CT>(a_or_mu, k2e, cl);
          const P2 num = dipole2<CT>(a_or_mu, k2e, nu), nlm = dipole2<CT>(a_or_mu, k2e, nl);
          const double du_ = bond(neg(cu), inv_mu(cum), nu, num) - bond(cu, cum, nu, num);
          const double dl_ = bond(nl, nlm, neg(cl), inv_mu(clm)) - bond(nl, nlm, cl, clm);
          dpair_flip = (onu ? du_ : 0.0) + (onl ? dl_ : 0.0);
        }
        const double ratio = ((1 - new_upper_p) * (1 - new_lower_p)) / ((1 - upper_p) * (1 - lower_p));   // :249-252
        alpha = flipped ? ratio : 1.0;
        // members' own terms: n -> -n; polar mu -> -mu and with it u -> -u; dielectric mu and u do not change
        const double f2 = flipped ? -2.0 : 0.0;
        drx_flip = b * (f2 * sn.x);
        drz_flip = b * (f2 * sn.z);
        if constexpr (CT == PSTAT_POLAR) {
          dp_flip.x = f2 * (a_or_mu * sn.x);
          dp_flip.z = f2 * (a_or_mu * sn.z);
          du_flip = mhalfE0 * dp_flip.z;
        }
      }
      const uint32_t weps = g.next();   // the acceptance draw comes after the cluster's draws

      // ---- energy difference of the whole proposal, 2D/inc/energy.jl:7-23
      const double drx = b * (n1.x - n0.x) + drx_flip, drz = b * (n1.z - n0.z) + drz_flip;
      const double dus = du_field + du_flip;
      const double dU = dus + (dpair + dpair_flip) - (Fx * drx + Fz * drz);

      // ---- Metropolis-Hastings, 2D/inc/acceptance.jl:29-39: no Jacobian in the target density
      // (the f32 filter of pstat_math.h decides all but ~1e-5 of the draws; the literal expression the rest)
      const double dw = umb ? dus * wscale : 0.0;
      const bool ok = metropolis_filter(dU * (-1.0 / kT) + (dw - lag), alpha, 1.0, weps, [&]() -> bool {
        const double delta = -dU / kT + dw + log_f64(alpha) - lag;
        const double eps = eps_uniform(A.wide_eps != 0, weps, w0, wflip, wphi);
        return (delta >= 0) || (eps < exp_f64(delta));
      });
      if constexpr (EN == PSTAT_ISING) nnan_seg += not_finite(dU) ? 1 : 0;

      // ---- commit
      if (ok) {
        ang[cell] = flipped ? ph1 + PI : ph1;
        if (flipped) {
          for (int i = lower; i <= upper; ++i) {
            const double v = ang[i * lanes + lane];
            ang[i * lanes + lane] = i == idx ? v : v + PI;   // flip_n!: move!(chain, i, pi)
          }
        }
        Orx += drx; Orz += drz;
        Opx += (m1.x - m0.x) + dp_flip.x; Opz += (m1.z - m0.z) + dp_flip.z;
        OU += dU;
        usum += dus;
        lag = log_f64(alpha);
        ++nacc_seg;
      }

      // ---- record! x 8, 2D/mcmc_clustering_eap_chain.jl:277-278
      double wgt = 1;
      if (umb) {
        bool raise;
        double wrel = umbrella_logw(usum, uref, wscale, raise);
        if (__builtin_amdgcn_ballot_w64(raise) != 0) {   // the gauge rises to this configuration (pstat_math.h)
          if (raise) {
            const double f = exp_f64(-wrel);
#pragma unroll
            for (int q = 0; q < 5; ++q) { a1[q] *= f; a2[q] *= f; s1[q] *= f; s2[q] *= f; }
            accw *= f;
            wnorm *= f;
            uref = usum; regauged = true; wrel = 0;
          }
        }
        wgt = exp_f64(wrel);
      }
      accw += wgt;
      a1[0] = fma_r(wgt, Orx, a1[0]); a1[1] = fma_r(wgt, Orz, a1[1]);
      a1[2] = fma_r(wgt, Opx, a1[2]); a1[3] = fma_r(wgt, Opz, a1[3]);
      a1[4] = fma_r(wgt, OU, a1[4]);
      a2[0] = fma_r(wgt * Orx, Orx, a2[0]); a2[1] = fma_r(wgt * Orz, Orz, a2[1]);
      a2[2] = fma_r(wgt * Opx, Opx, a2[2]); a2[3] = fma_r(wgt * Opz, Opz, a2[3]);
      a2[4] = fma_r(wgt * OU, OU, a2[4]);
    }

#pragma unroll
    for (int q = 0; q < 5; ++q) { s1[q] += a1[q]; s2[q] += a2[q]; }
    wnorm += accw;
    step += chunk;
    left -= chunk;
    steps_seg += chunk;

    // ---- step-size adaptation, 2D/mcmc_clustering_eap_chain.jl:257-275: phi_step only
    if (A.adaptive) {
      to_adj -= chunk;
      if (to_adj == 0) {
        to_adj = spa;
        const Adapted a = adapt_steps<false>(nacc_off, natt_off, nacc_seg, steps_seg, A.adj_lb, A.adj_ub, A.adj_scale, phistep, 0.0);
        phistep = a.phistep; nacc_off = a.nacc_off; natt_off = a.natt_off;
      }
    }
  }

  if constexpr (EN == PSTAT_ISING) {
    // U is a running total of accepted differences, and under the Ising energy a chain can pass through a 1/r^3 contact
    // (|U| ~ 1e8 for a few steps) and come back: the total then keeps an absolute error of ~1e-16 of the LARGEST |U| it
    // has held, which the reference's full recomputation (2D/inc/eap_chain.jl:183) does not have.  So the pair sum -- the only
    // term that can be that large -- is re-derived from the angles when the segment ends: n - 1 bonds, once per segment.
    // Decisions only ever see differences dU, so no trajectory depends on this.
    double tp = 0;
    P2 pn = load_n(0), pm = dipole2<CT>(a_or_mu, k2e, pn);
    for (int i = 1; i < n; ++i) {
      const P2 nh = load_n(i), m = dipole2<CT>(a_or_mu, k2e, nh);
      tp += bond(pn, pm, nh, m);
      pn = nh; pm = m;
    }
    OU = usum + tp - (Fx * Orx + Fz * Orz);
  }
  for (int i = 0; i < n; ++i) gph[(int64_t)i * C + c] = ang[i * lanes + lane];   // ---- spill
  g.store(S.rng + c, C);
  S.stepsz[0 * C + c] = phistep;
  S.win[0 * C + c] = nacc_off + nacc_seg; S.win[1 * C + c] = natt_off + steps_seg;
  S.nacc_total[c] += nacc_seg;
  if constexpr (EN == PSTAT_ISING) S.nanrej[c] += nnan_seg;
  S.obs[OBS_R1 * C + c] = Orx; S.obs[OBS_R3 * C + c] = Orz;
  S.obs[OBS_P1 * C + c] = Opx; S.obs[OBS_P3 * C + c] = Opz;
  S.obs[OBS_U * C + c] = OU; S.obs[OBS_USUM * C + c] = usum;
  S.lag[c] = lag;
  if (umb) S.wnorm[c] = wnorm;
  if (regauged) S.uref[c] = uref;
  S.sums[S_R1 * C + c] = s1[0]; S.sums[S_R3 * C + c] = s1[1]; S.sums[S_P1 * C + c] = s1[2]; S.sums[S_P3 * C + c] = s1[3];
  S.sums[S_U * C + c] = s1[4];
  S.sums[S_R1SQ * C + c] = s2[0]; S.sums[S_R3SQ * C + c] = s2[1]; S.sums[S_P1SQ * C + c] = s2[2]; S.sums[S_P3SQ * C + c] = s2[3];
  S.sums[S_USQ * C + c] = s2[4];
}

// the persistent (block, segment) job loop of pstat_device.h around run_planar_segment
// (PACKED: chain blocks straddle cases, the case's scalars are per-lane values -- run_job_queue)
template <typename G, int CT, int EN, bool PACKED>
__global__ __launch_bounds__(64) void planar_kernel(SweepArgs A, DevState S, const CaseConst *__restrict__ cases, int umbrella,
                                                    int *__restrict__ queue) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x;
  run_job_queue<PACKED>(A, queue, lane, [&](const CaseConst &cc, int64_t chain, int64_t first, int64_t len, int) {
    run_planar_segment<G, CT, EN>(A, S, cc, umbrella, smem, lane, chain, first, len);
  }, cases);
}

using PlanarFn = void (*)(SweepArgs, DevState, const CaseConst *, int, int *);

template <typename G, bool PACKED>
PlanarFn pick_ct_en(const LaunchCfg &cfg) {
  const bool ising = cfg.energy_type == PSTAT_ISING;
  if (cfg.chain_type == PSTAT_DIELECTRIC)
    return ising ? planar_kernel<G, PSTAT_DIELECTRIC, PSTAT_ISING, PACKED> : planar_kernel<G, PSTAT_DIELECTRIC, PSTAT_NONINTERACTING, PACKED>;
  return ising ? planar_kernel<G, PSTAT_POLAR, PSTAT_ISING, PACKED> : planar_kernel<G, PSTAT_POLAR, PSTAT_NONINTERACTING, PACKED>;
}
template <typename G>
PlanarFn pick_packed(const LaunchCfg &cfg) {
  return cfg.packed ? pick_ct_en<G, true>(cfg) : pick_ct_en<G, false>(cfg);
}

// EAPChain(pargs), 2D/inc/eap_chain.jl:66-112: n draws phi ~ U(0, 2 pi), then r, p, U.  One thread per chain.  The theta
// plane of DevState::ang is zero-filled and never read.
template <typename G>
__global__ void planar_init_kernel(SweepArgs A, DevState S, const CaseConst *__restrict__ cases, int chain_type, int energy_type,
                                   double phi_step) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= S.C) return;
  const int64_t icase = c / A.chains_per_case, local = c % A.chains_per_case;
  const CaseConst cc = cases[icase];
  double *th = (double *)S.ang, *ph = (double *)S.ang + A.n * S.C;
  G g;
  g.seed(cc.seed, cc.chain_id0 + (uint64_t)local);
  for (int64_t i = 0; i < A.n; ++i) {
    ph[i * S.C + c] = store_phi<double>(u01<double>(g.next()));
    th[i * S.C + c] = 0.0;
  }
  double rx = 0, rz = 0, px = 0, pz = 0, usum = 0, upair = 0;
  P2 pn{0, 0}, pm{0, 0};
  for (int64_t i = 0; i < A.n; ++i) {
    const double f = ph[i * S.C + c];
    const P2 nh{cos(f), sin(f)};
    const P2 m = chain_type == PSTAT_DIELECTRIC ? dipole2<PSTAT_DIELECTRIC>((cc.K1 - cc.K2) * cc.E0, cc.K2 * cc.E0, nh)
                                                : dipole2<PSTAT_POLAR>(cc.mu, 0.0, nh);
    rx += cc.b * nh.x; rz += cc.b * nh.z;
    px += m.x; pz += m.z;
    usum += -0.5 * cc.E0 * m.z;
    if (energy_type == PSTAT_ISING && i > 0) {
      const double h = -cc.b / 2;
      upair += pair_term<double>(h * (pn.x + nh.x), 0.0, h * (pn.z + nh.z), pm.x, 0.0, pm.z, m.x, 0.0, m.z);
    }
    pn = nh; pm = m;
  }
  const int64_t C = S.C;
  for (int q = 0; q < NOBS_STATE; ++q) S.obs[q * C + c] = 0.0;
  S.obs[OBS_R1 * C + c] = rx; S.obs[OBS_R3 * C + c] = rz;
  S.obs[OBS_P1 * C + c] = px; S.obs[OBS_P3 * C + c] = pz;
  S.obs[OBS_U * C + c] = usum + upair - (rx * cc.Fx + rz * cc.Fz);
  S.obs[OBS_USUM * C + c] = usum;
  g.store(S.rng + c, C);
  S.stepsz[0 * C + c] = phi_step; S.stepsz[1 * C + c] = 0.0;
  S.win[0 * C + c] = 0; S.win[1 * C + c] = 0;
  S.nacc_total[c] = 0;
  for (int q = 0; q < NSUMS; ++q) S.sums[q * C + c] = 0.0;
  S.wnorm[c] = 0.0;
  S.lag[c] = 0.0;
  S.uref[c] = usum;
  S.nanrej[c] = 0;
}

}  // namespace

StepKernel planar_step_kernel(const LaunchCfg &cfg, int64_t) {
  const PlanarFn fn = cfg.rng == PSTAT_RNG_XOSHIRO128PP ? pick_packed<Xoshiro128pp>(cfg) : pick_packed<Mwc64x>(cfg);
  return {(const void *)fn, PSTAT_KERNEL_NAME(cfg, "planar_kernel<double>")};
}

hipError_t launch_planar_init(const LaunchCfg &cfg, const SweepArgs &a, const DevState &s, const CaseConst *cases,
                              double phi_step, hipStream_t stream) {
  const unsigned grid = (unsigned)((s.C + 255) / 256);
  if (cfg.rng == PSTAT_RNG_XOSHIRO128PP)
    hipLaunchKernelGGL(planar_init_kernel<Xoshiro128pp>, dim3(grid), dim3(256), 0, stream, a, s, cases, cfg.chain_type,
                       cfg.energy_type, phi_step);
  else
    hipLaunchKernelGGL(planar_init_kernel<Mwc64x>, dim3(grid), dim3(256), 0, stream, a, s, cases, cfg.chain_type,
                       cfg.energy_type, phi_step);
  return hipGetLastError();
}

}  // namespace pstat
