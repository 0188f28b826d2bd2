/*
 * planar_ref.h -- CPU restatement of the planar (2D) clustering main of grasingerm/polymer-stats:
 * 2D/mcmc_clustering_eap_chain.jl + 2D/inc/{eap_chain,dipole_response,energy,acceptance,average}.jl.
 *
 * THIS IS TEST INFRASTRUCTURE, NOT PRODUCT CODE.  Only tests/ and tools that measure or check may load
 * it.  The product (libpstat.so, polymer_stats_amd/, julia/) never links, imports or calls anything here.
 *
 * PARITY UNPINNED: the reference seeds nothing and ships no fixture, and there is no Julia interpreter to
 * run it with, so no reference output exists to pin this restatement against.  It is pinned instead by
 * hand-computable energies and Hastings ratios, and by closed-form single-monomer integrals
 * (tests/golden/planar_closed_form.json).  It is written from the Julia text as a C restatement; no
 * reference program text is copied.
 *
 * Citations "file:line" are relative to the reference tree.
 *
 * Vectors are (component 1, component 2) = what the CSV headers call (r1, r3); the 16-vectors of sums use
 * the rolling.csv order of include/pstat.h with every y entry (r2, r2sq, p2, p2sq) exactly 0.
 *
 * THE PLANAR RANDOM-STREAM CONTRACT (restated, not shared, in polymer_stats_amd/csrc/pstat_planar.hip).
 * Generators and seeding are those of the 3D mains: MWC64X with 2^40 skip-ahead per chain id, or
 * xoshiro128++ seeded through Philox4x32-10.  u(w) = (w >> 9) 2^-23; idx = mulhi32(w, n).
 *   start    n words, phi_i = 2 pi u(w_i)                                   (2D/inc/eap_chain.jl:6,67)
 *   a step   w_idx, w_phi, w_flip, [growth words], w_eps
 *     idx = mulhi32(w_idx, n);  dphi = phi_step (2 u(w_phi) - 1);  flip = u(w_flip) <= cluster_prob.
 *     Growth words are drawn ONLY IF flip: round t = 0, 1, ... tests the link above the cluster (one word,
 *     while that end is still growing), then the link below it (one word, likewise); an end that has reached
 *     the end of the chain draws nothing (2D/inc/eap_chain.jl:203-206,220-223).
 *     eps: 23 bits u(w_eps); 53 bits (w_eps 2^21 + (w_phi & 511) 2^12 + (w_flip & 511) 2^3 + (w_idx & 7)) 2^-53 --
 *     the low bits of the step's other words that nothing else uses (the planar step has no dtheta word; the
 *     flip word takes its place).  Both settings consume the same stream.
 *   Where this departs from the reference's order (idx, dphi, growth right to completion, growth left, flip
 *   draw, eps; 2D/mcmc_clustering_eap_chain.jl:239-244, 2D/inc/eap_chain.jl:199-233), and why the law of the
 *   step is the same:
 *     - the flip word comes before the growth: the decision `rand() <= eflip` depends on nothing the growth
 *       produces, and every test keeps its own iid draw;
 *     - no growth when the step does not flip: the reference grows the cluster and throws it away (alpha = 1,
 *       the trial is the single move), so the draws it spends have no effect on the chain;
 *     - the two ends are interleaved round by round: they test disjoint links with iid draws, so the law of
 *       (lower, upper) is that of the two loops run one after the other (the latitude oracle/eap_oracle.c took).
 */
#ifndef PLANAR_REF_H
#define PLANAR_REF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { PLANAR_DIELECTRIC = 0, PLANAR_POLAR = 1 };                            /* --chain-type  */
enum { PLANAR_NONINTERACTING = 0, PLANAR_INTERACTING = 1, PLANAR_ISING = 2 }; /* --energy-type */
enum { PLANAR_RNG_MWC64X = 0, PLANAR_RNG_XOSHIRO128PP = 1 };

/* the option table 2D/mcmc_clustering_eap_chain.jl:15-129, hot-path subset */
typedef struct planar_params {
  double E0, K1, K2, mu, kT, Fz, Fx, b;
  double phi_step;                      /* :64-67 */
  double adj_lb, adj_ub, adj_scale;     /* :75-86 */
  double cluster_prob;                  /* :71-74: probability OF flipping the cluster */
  int64_t n;                            /* --num-monomers */
  int64_t num_steps;                    /* --num-steps */
  int64_t steps_per_adjust;             /* :87-90 */
  uint64_t seed;                        /* ours: the reference never seeds */
  int32_t chain_type, energy_type, umbrella, rng;
  int32_t uniform_bits;                 /* 0 or 53: 53-bit eps; 23: u(w_eps) */
  int32_t pad_;
} planar_params;

enum { PLANAR_NOBS = 16 };   /* r1 r2 r3 r1sq r2sq r3sq rsq p1 p2 p3 p1sq p2sq p3sq psq U Usq; r2.. = 0 */

typedef struct planar_result {
  double sum[PLANAR_NOBS];   /* averager .value fields (2D/inc/average.jl:9) */
  double norm;               /* averager .normalizer: count, or sum of 1/e^w */
  int64_t nacc_total;
  int64_t words;             /* generator words drawn by this call (start included when the chain was drawn) */
  int64_t flips_proposed;    /* steps whose flip draw said flip */
  int64_t link_tests;        /* growth words drawn */
  double phi_step;           /* after the last adaptation */
  double r[2], p[2], U;      /* final microstate */
  uint32_t rng[4];           /* final generator state */
  int64_t nacc_window, natt_window;
} planar_result;

/* One call of mcmc(nsteps, pargs, chain), 2D/mcmc_clustering_eap_chain.jl:148-310: literal algorithm (trial = deep
 * copy, move!, full prefix sum, full energy recomputation, cluster_flip!, acceptor caching log pi + log alpha,
 * sum / count averagers, the adaptation rule).
 *   phi0 == NULL: the chain is drawn from the seeded generator (what the reference's mcmc() does on its first line,
 *                 :151, whatever chain it was handed);
 *   phi0 != NULL: starts from phi0[n] with generator state rng0[4] -- the carried chain of a burn-in rung, which the
 *                 reference's help text promises and this project's --carry-burn-in runs.
 * final_phi: [n] or NULL. */
int planar_run(const planar_params *P, uint64_t chain_id, const double *phi0, const uint32_t *rng0,
               planar_result *out, double *final_phi);

/* Building blocks for hand checks. */
void planar_dipole(const planar_params *P, double phi, double mu_out[2]);          /* 2D/inc/dipole_response.jl:7-27 */
/* U of the chain phi[n] (2D/inc/energy.jl) with r, p and sum(u) */
double planar_energy(const planar_params *P, const double *phi, double r_out[2], double p_out[2], double *usum_out);
/* cluster_flip! on phi[n] (in place) from monomer idx (0-based) with the uniforms u[0 .. nu) taken in contract order:
 * u[0] the flip draw, then the growth rounds.  Returns alpha; *lower, *upper the cluster grown (idx, idx when the step
 * does not flip), *flipped, *used the uniforms consumed. */
double planar_cluster_flip_u(const planar_params *P, double *phi, int64_t idx, const double *u, int nu, int64_t *lower,
                             int64_t *upper, int *flipped, int *used);
double planar_eps(int uniform_bits, uint32_t w_eps, uint32_t w_idx, uint32_t w_phi, uint32_t w_flip);
void planar_seed(const planar_params *P, uint64_t chain_id, uint32_t s[4]);
uint32_t planar_next(int rng, uint32_t s[4]);

#ifdef __cplusplus
}
#endif
#endif
