/*
 * pstat.h -- C ABI of libpstat.so: the MI355X (gfx950) implementation of the fixed-force-ensemble
 * MCMC hot path of grasingerm/polymer-stats.
 *
 * The reference exposes no FFI for this path: the whole of it lives inside one Julia function,
 * mcmc(nsteps, pargs) (mcmc_eap_chain.jl:171-376), reached only through the command line
 * (mcmc_eap_chain.jl:19-155) -- and, for the clustering main, mcmc(nsteps, pargs, chain)
 * (mcmc_clustering_eap_chain.jl:172-352) under its annealing driver (:354-387).  This header is
 * therefore the boundary a maintainer would bind with `ccall` when moving the step loop of those
 * functions onto the GPU; each entry point names the reference code it stands in for.
 * INTEGRATION.md shows the Julia-side binding.
 *
 * Conventions: plain C, caller-allocated output buffers, no callbacks, no exceptions across the ABI.
 * Every function returns PSTAT_OK (0) or a negative pstat_status; pstat_strerror() names it and
 * pstat_last_error() returns a thread-local detail string.  A handle is confined to one host thread
 * at a time; distinct handles may be used concurrently.  There is no CPU fallback: without a HIP
 * device pstat_create() fails with PSTAT_ERR_NO_DEVICE.
 *
 * One handle = `num_chains` independent Markov chains per case (chain-per-lane on the device), each
 * one statistically identical to one reference run with `--num-inits 1`; results are pooled.
 *
 * RESOLUTION OF THE UNIFORM DRAWS (ours; the reference draws Float64 uniforms with 52-53 random bits from an unseeded
 * generator, mcmc_eap_chain.jl:277-280,287).  Every uniform here is made from 32-bit generator words:
 *   * proposals  dphi = phi_step (2u - 1), dtheta = theta_step (2u - 1), u = (w >> 9) 2^-23: a lattice of step / 2^22
 *     (symmetric, so detailed balance holds on it; the adapted step sizes are incommensurate, so chains are not confined
 *     to one lattice), in every precision;
 *   * the Metropolis eps (mcmc_eap_chain.jl:287, inc/acceptance.jl:29-39): `uniform_bits` below.  With 23 bits eps = 0
 *     comes up once per 2^23 = 8.4e6 proposals and then ANY proposal of finite energy with exp(delta) > 0 is accepted, so
 *     acceptance probabilities have a floor of 2^-23 = 1.2e-7 (tests/test_gpu_parity.py pins this on a cold, strongly
 *     coupled chain).  With 53 bits -- the default of the f64 kernels -- the floor is 2^-53 = 1.1e-16, the reference's own;
 *   * the clustering main's link and skip draws (inc/eap_chain.jl:276,286,303) and the re-initialisation draw
 *     (mcmc_eap_chain.jl:357): 23 bits, `u <= p`.
 */
#ifndef PSTAT_H
#define PSTAT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSTAT_ABI_VERSION 6

typedef enum pstat_status {
  PSTAT_OK = 0,
  PSTAT_ERR_INVALID_ARG = -1,   /* bad parameter value (message in pstat_last_error)             */
  PSTAT_ERR_NO_DEVICE = -2,     /* no HIP device / device index out of range                     */
  PSTAT_ERR_HIP = -3,           /* a HIP runtime call failed                                     */
  PSTAT_ERR_UNSUPPORTED = -4,   /* valid reference option that has no device implementation      */
  PSTAT_ERR_NOMEM = -5,
  PSTAT_ERR_BAD_CHECKPOINT = -6,
  PSTAT_ERR_TOO_SMALL = -7      /* caller buffer too small; required size has been written back  */
} pstat_status;

/* --chain-type (mcmc_eap_chain.jl:25-28; inc/eap_chain.jl:81-87) */
enum { PSTAT_DIELECTRIC = 0, PSTAT_POLAR = 1 };
/* --energy-type (mcmc_eap_chain.jl:41-44; inc/eap_chain.jl:95-105) */
enum { PSTAT_NONINTERACTING = 0, PSTAT_INTERACTING = 1, PSTAT_ISING = 2,
       /* clustering main only (mcmc_clustering_eap_chain.jl:44-51; UCutoff, inc/eap_chain.jl:165-192):
        * dipole-dipole terms of pairs within cutoff_radius monomer lengths.  NB the reference's UCutoff
        * functor returns that sum ALONE -- with this energy neither the field nor the force enters U. */
       PSTAT_CUTOFF = 3 };
/* arithmetic of the device path:
 *   PSTAT_F64  f64 throughout: the reference's Float64 (inc/types.jl:1-4), and the default.  Reproduces the CPU oracle's
 *              (phi, theta) trajectory, generator state and counters bit for bit; observables to ~1e-15 relative.
 *   PSTAT_F32  opt-in fast path: f32 state and transcendentals, f64 running sums.  Bias of the pooled averages of the
 *              non-interacting energies <= 5e-6 relative.  NOT equivalent to f64 once chains
 *              have collapsed into 1/r^3 contacts (|U| >~ 1e4 kT; interacting/Ising/cutoff energies at strong coupling):
 *              kT-level fidelity there needs position differences good to ~1e-10 b (profiles/r02/config4_f32_vs_f64.json).
 *   PSTAT_Q16  opt-in: both angles live on a 2^16-point midpoint lattice (4 bytes of state per
 *              monomer, twice the chains resident per CU), f32 arithmetic, f64 running sums.
 *              Discretisation bias of ensemble averages: O(h^2) ~ 1e-10. */
enum { PSTAT_F32 = 0, PSTAT_F64 = 1, PSTAT_Q16 = 2 };
/* per-chain generator (the reference uses Julia's unseeded default RNG; ours are seeded):
 *   PSTAT_RNG_MWC64X        multiply-with-carry MWC64X, streams split by 2^40-output skip-ahead (default)
 *   PSTAT_RNG_XOSHIRO128PP  xoshiro128++ seeded per chain through Philox4x32-10 */
enum { PSTAT_RNG_MWC64X = 0, PSTAT_RNG_XOSHIRO128PP = 1 };
#define PSTAT_MWC64X_MAX_CHAINS (1ull << 22)   /* global chain ids with pairwise disjoint MWC64X streams */
/* which main's step is run:
 *   PSTAT_MOVES_SINGLE   mcmc_eap_chain.jl:276-291 -- one single-monomer trial move per step (default)
 *   PSTAT_MOVES_CLUSTER  mcmc_clustering_eap_chain.jl:268-279 -- the same move followed, on the trial
 *                        chain, by cluster_flip! (inc/eap_chain.jl:269-333); bending energy; two more
 *                        averagers (sum cos^2 theta, mean bond angle).  All four energies; the all-pairs
 *                        ones (interacting, cutoff) run one chain per wavefront, n <= 512.  Non-interacting and
 *                        Ising: one chain per lane, or -- f64 handles of up to 4 096 chains and sweeps of many cases
 *                        of <= 16 chains each, n <= 256, MWC64X -- one chain per wavefront as well (a phase scan of
 *                        the reference is 2 730 single-chain cases: 2.8 us per step instead of 29; pstat_launch_info.kernel
 *                        names the choice).  Trajectories do not depend on it. */
enum { PSTAT_MOVES_SINGLE = 0, PSTAT_MOVES_CLUSTER = 1 };

/* Flattened pargs::Dict (mcmc_eap_chain.jl:155) -- the keys the force-ensemble step loop reads. */
typedef struct pstat_params {
  /* physics: inc/eap_chain.jl:89-108 */
  double E0, K1, K2, mu, kT, Fz, Fx, b;
  /* proposal + adaptation: mcmc_eap_chain.jl:88-118,172-174,301-322 */
  double phi_step, theta_step;
  double adj_lb, adj_ub, adj_scale;
  int64_t steps_per_adjust;
  int64_t n;             /* --num-monomers                                                    */
  int64_t num_chains;    /* chains per case on this handle (ours)                             */
  uint64_t seed;         /* ours: the reference never seeds its RNG                           */
  uint64_t chain_id0;    /* global id of this handle's first chain: shards over GPUs.  With
                          * PSTAT_RNG_MWC64X chain_id0 + num_chains must stay <= 2^22 (PSTAT_MWC64X_MAX_CHAINS):
                          * chain k starts k * 2^40 outputs down ONE sequence of period ~2^63, so ids beyond
                          * 2^23 would wrap onto earlier streams (the bound keeps a factor 2 in hand); xoshiro128++ has no such bound */
  int32_t chain_type;    /* PSTAT_DIELECTRIC | PSTAT_POLAR                                    */
  int32_t energy_type;   /* PSTAT_NONINTERACTING | PSTAT_INTERACTING | PSTAT_ISING | PSTAT_CUTOFF */
  int32_t do_flips;      /* --do-flips                                                        */
  int32_t umbrella;      /* --umbrella-sampling                                               */
  int32_t precision;     /* PSTAT_F32 | PSTAT_F64 | PSTAT_Q16                                 */
  int32_t device;        /* HIP device ordinal                                                */
  int32_t rng;           /* PSTAT_RNG_MWC64X | PSTAT_RNG_XOSHIRO128PP                         */
  int32_t move_set;      /* PSTAT_MOVES_SINGLE | PSTAT_MOVES_CLUSTER                          */
  /* options of mcmc_clustering_eap_chain.jl (:36-43,87-90,142-148); all 0 in mcmc_eap_chain.jl */
  double bend_mod, bend_angle;   /* --bend-mod, --bend-angle (per case)                       */
  double cluster_prob;           /* --cluster-prob (per case)                                 */
  double x0_phi, x0_theta;       /* --x0 "[phi; theta]"                                       */
  double dx0_phi, dx0_theta;     /* --dx0                                                     */
  int32_t use_x0;                /* start from x0 + Uniform(0, dx0) instead of uniform angles */
  int32_t uniform_bits;          /* random bits of the Metropolis eps: 0 = the precision's default (53 for PSTAT_F64, 23
                                  * for PSTAT_F32 / PSTAT_Q16, whose comparison runs in a 24-bit mantissa), 23, or 53 (f64
                                  * only).  Under 53 eps = (w_eps 2^21 + lo) 2^-53, lo = the low 9 bits of the step's dtheta
                                  * word, the low 9 of its dphi word and the low 3 of its index word -- bits no proposal
                                  * uses; no extra draw, so the two settings consume the same stream and differ only in
                                  * decisions that fall inside [u, u + 2^-23).  23 reproduces ABI 5's trajectories.      */
  double cutoff_radius;          /* --cutoff-radius, monomer lengths (PSTAT_CUTOFF; per case)  */
} pstat_params;

/* Order of every 16-vector below = the columns of <prefix>_rolling.csv after "step"
 * (mcmc_eap_chain.jl:259). */
enum {
  PSTAT_R1, PSTAT_R2, PSTAT_R3, PSTAT_R1SQ, PSTAT_R2SQ, PSTAT_R3SQ, PSTAT_RSQ,
  PSTAT_P1, PSTAT_P2, PSTAT_P3, PSTAT_P1SQ, PSTAT_P2SQ, PSTAT_P3SQ, PSTAT_PSQ,
  PSTAT_U, PSTAT_USQ, PSTAT_NOBS
};

/* Length (in doubles) of the device-side reduction vector of pstat_reduce_device():
 *   [0]        number of chains reduced
 *   [1..19]    sum over chains of the per-chain running mean of: the 16 observables, the per-chain
 *              acceptance ratio, sum_i cos^2(theta_i), the mean bond angle (the last two are recorded
 *              by the clustering main only, mcmc_clustering_eap_chain.jl:243-244)
 *   [20..38]   sum over chains of the squares of those per-chain means
 *   [39]       proposals rejected because their trial energy was not finite (see pstat_summary.nan_rejects)
 *   [40]       chains whose current configuration has collapsed (see pstat_summary.chains_collapsed)
 * Every entry is additive across handles/GPUs, so one all-reduce(SUM) merges ensembles. */
#define PSTAT_NQ 19
#define PSTAT_NX 2
#define PSTAT_NRED (1 + 2 * PSTAT_NQ + PSTAT_NX)

/* The ten stdout quantities of mcmc_eap_chain.jl:386-395 plus bookkeeping. */
typedef struct pstat_summary {
  double avg[PSTAT_NOBS];      /* pooled running averages, rolling.csv order                    */
  double stderr_[PSTAT_NOBS];  /* across-chain standard error of each (0 if one chain)          */
  double acceptance_ratio;     /* "AR": accepted / attempted over all chains and steps          */
  double ar_stderr;
  int64_t num_chains;
  int64_t steps_per_chain;     /* steps recorded so far by every chain                          */
  double attempted_updates;    /* num_chains * steps_per_chain                                  */
  double extra_avg[2];         /* <sum cos^2 theta>, <psi> (clustering main: "<cos2(theta)>", "<psi>") */
  double extra_stderr[2];
  /* Failure surfacing.  The reference rejects a proposal whose energy is NaN silently
   * (inc/acceptance.jl:29-39: every comparison with NaN is false) and has no excluded volume, so with the
   * pair energies (inc/eap_chain.jl:200-207,215-228: 1/r^3) a chain can fall into r -> 0 and stay there.
   *   nan_rejects       proposals, over all chains and recorded steps, whose trial energy AS THE DEVICE EVALUATES IT was
   *                     NaN or +-Inf (identically 0 for the non-interacting energy, whose dU is always finite).  This is
   *                     the device's arithmetic, not a replay of the reference's: whether a contact is r = 0 exactly
   *                     (0 * inf = NaN) or r ~ 1e-17 (a finite 1e50) depends on the order positions are summed in.  The
   *                     reference's cumsum (inc/eap_chain.jl:49-51) absorbs the 1e-16 components of a pole-clamped
   *                     monomer into its running sum and lands two such monomers on exactly the same point; the kernels
   *                     (bond vector b/2 (n_i + n_j) for neighbours, prefix scan / incremental shifts for all pairs) keep
   *                     them 1e-17 apart.  Measured on one seeded case (23 monomers, --do-flips, 5 x 1500 steps): the
   *                     CPU restatement of the reference's arithmetic counts 17, the device 0 -- and every one of those
   *                     proposals is rejected on both sides anyway (the clamp gives sin(theta') = 0), which is why the
   *                     trajectories agree bit for bit.  Where the non-finite value does not hinge on rounding (every
   *                     pair at r = 0 with --mlen 0: tests/test_gpu_validation.py) the counts are equal.
   *   chains_collapsed  chains whose CURRENT energy has |U| > 1e3 * n * (kT + |E0| mu_max / 2 + b (|Fx| + |Fz|)),
   *                     mu_max = max(|K1|, |K2|) |E0| or |mu|: a thousand times what n separated monomers can hold
   *                     in field, force and thermal energy; only a 1/r^3 contact gets there (also counts NaN). */
  int64_t nan_rejects;
  int64_t chains_collapsed;
} pstat_summary;

typedef struct pstat_handle pstat_handle;

int pstat_abi_version(void);
const char *pstat_strerror(int status);
const char *pstat_last_error(void);
int pstat_device_count(void);

/* Fills *p with the reference's option defaults (mcmc_eap_chain.jl:19-153). */
void pstat_default_params(pstat_params *p);

/* Replaces `chain = EAPChain(pargs); chain.U = U(chain)` and the averager construction
 * (mcmc_eap_chain.jl:175-176,242-255; inc/eap_chain.jl:60-135): draws phi~U(0,2pi), theta~U(0,pi)
 * for every chain on the device, derives r, p, U, zeroes the running sums.
 * `cases`/`ncases`: ncases >= 1 parameter sets that differ only in the physics scalars
 * (E0,K1,K2,mu,kT,Fz,Fx,b; bend_mod, bend_angle, cluster_prob, cutoff_radius; seed, chain_id0) -- a sweep grid run in
 * one launch; every case gets num_chains chains.  Chains of several cases share a wavefront when a case has fewer
 * chains than a wave has lanes and that shortens the launch (pstat_launch_info.packed_cases); a chain's trajectory
 * depends on its (seed, chain id) and its case's options only, never on what else is in the handle.
 * `stream`: a hipStream_t to launch on (e.g. torch's current stream) or NULL for the handle's own. */
int pstat_create(const pstat_params *cases, int32_t ncases, void *stream, pstat_handle **out);
void pstat_destroy(pstat_handle *h);

/* The planar main, 2D/mcmc_clustering_eap_chain.jl: same pstat_params, same handle type.
 * A planar chain has ONE angle per monomer, n_i = (cos phi_i, sin phi_i); the field and Fz act on the second component,
 * Fx on the first (2D/inc/energy.jl:8, 2D/inc/eap_chain.jl:64); the target density has no sin(theta) Jacobian
 * (2D/inc/acceptance.jl:18-22).  One step = the single-monomer move phi_idx += dphi followed, on the trial chain, by
 * cluster_flip! (2D/inc/eap_chain.jl:194-257): with probability cluster_prob the cluster grown from the moved monomer is
 * inverted (phi_i += pi for every member), accepted by Metropolis-Hastings with the ratio alpha of its boundary links.
 * Replaces `chain = EAPChain(pargs)` (2D/mcmc_clustering_eap_chain.jl:151; phi ~ U(0, 2 pi)) and, through pstat_advance,
 * the step loop :238-278.  The reference's burn-in ladder (:323-336) has no effect on any of its outputs -- mcmc(nsteps,
 * pargs, chain) overwrites the chain it is handed on its first line -- so one run of that main is: pstat_create_planar,
 * pstat_advance(num-steps).  (A host that WANTS the ladder carries the chains through it with pstat_scale_kT,
 * pstat_reset_sampler and pstat_reset_averages, as the 3D clustering main does.)
 *
 * The planar observables are the 3D 16-vectors with component 1 in the x slots and component 2 in the z slots -- what the
 * reference's CSV headers call r1, r3 -- and every y entry (r2, r2sq, p2, p2sq) exactly 0; extra_avg (sum cos^2 theta,
 * <psi>) stays 0: the planar main has no such averagers.
 *
 * How pstat_params is read for a planar handle:
 *   read     E0, K1, K2, mu, kT, Fz, Fx, b, phi_step, adj_lb, adj_ub, adj_scale, steps_per_adjust, n, num_chains, seed,
 *            chain_id0, chain_type, energy_type, umbrella, precision, device, rng, uniform_bits, and cluster_prob -- here
 *            the probability OF flipping the cluster (2D/mcmc_clustering_eap_chain.jl:71-74), where the 3D clustering main
 *            reads it as the probability of not trying.  Under uniform_bits = 53 the low 21 bits of eps are the low 9 bits
 *            of the step's dphi word, the low 9 of its flip word and the low 3 of its index word.
 *   must be at their pstat_default_params values, else PSTAT_ERR_INVALID_ARG naming the field: do_flips, bend_mod,
 *            bend_angle, use_x0 (the planar main has no such options).
 *   ignored  theta_step, x0_*, dx0_*, cutoff_radius, move_set (a planar handle always runs the combined move).
 *   NB pstat_default_params keeps the 3D defaults: the planar main's --step-adjust-ub is 0.40, not 0.55; setting it is
 *   the caller's business.
 * PSTAT_ERR_UNSUPPORTED: precision other than PSTAT_F64; energy_type PSTAT_INTERACTING (planar all-pairs); n > 2 560 (8-byte
 * cells of eight chains must fit a CU's LDS).  PSTAT_CUTOFF is PSTAT_ERR_INVALID_ARG: the planar main has no such energy.
 * Every accessor works on a planar handle.  pstat_microstate: [r1, 0, r3, p1, 0, p3, U]; pstat_chain_state and series rows:
 * angles = n zeros, then phi[n]; steps = {phi_step, 0, normalizer}; pstat_chain_extras: zeros.  pstat_reinit and
 * pstat_restart_from_x0 return PSTAT_ERR_UNSUPPORTED (the planar main has neither --num-inits nor --x0).  A checkpoint
 * of a planar handle is refused by a handle of pstat_create and the reverse (PSTAT_ERR_BAD_CHECKPOINT).
 * Umbrella sampling uses the rising gauge of pstat_chain_state's normalizer: value / normalizer is what the reference's
 * a-priori gauge (2D/inc/average.jl:110-118) gives wherever that is finite. */
int pstat_create_planar(const pstat_params *cases, int32_t ncases, void *stream, pstat_handle **out);

/* Replaces `nsteps` iterations of the step loop, mcmc_eap_chain.jl:276-328, for every chain:
 * proposal draw (:277-280), move! (inc/eap_chain.jl:230-257), energy (inc/energy.jl:7-23),
 * Metropolis (inc/acceptance.jl:29-39), step-size adaptation (:301-322), record! x 8 (:327-328).
 * With move_set = PSTAT_MOVES_CLUSTER: the step loop of mcmc_clustering_eap_chain.jl:268-311 instead
 * (the same move, then cluster_flip! on the trial chain, Metropolis-Hastings with alpha, record! x 10).
 * Asynchronous on the handle's stream. */
int pstat_advance(pstat_handle *h, int64_t nsteps);
int pstat_sync(pstat_handle *h);

/* Replaces the re-initialisation between inits, mcmc_eap_chain.jl:352-361: every chain draws a
 * fresh random configuration and adopts it if `force_init` or by metropolis_acc
 * (inc/acceptance.jl:1-3); the within-init step counter restarts at 1. */
int pstat_reinit(pstat_handle *h, int32_t force_init);

/* Burn-in support (the reference's clustering main, mcmc_clustering_eap_chain.jl:134-141,365-386,
 * discards a burn-in run made on a temperature ladder; mcmc_eap_chain.jl itself records from step 1).
 * pstat_reset_averages: zero the running sums, the acceptance totals and the recorded-step count,
 * keep the chains, generators and adapted step sizes.  pstat_set_kT: change the temperature of case
 * `icase` (all cases if < 0) for subsequent launches; the microstate is unaffected (U does not
 * depend on kT). */
int pstat_reset_averages(pstat_handle *h);
int pstat_set_kT(pstat_handle *h, int32_t icase, double kT);
/* kT of every case <- (the kT it was created with) * mult: one rung of the burn-in ladder for a whole
 * sweep grid (mcmc_clustering_eap_chain.jl:368,379: burnargs["kT"] = kT_base * kT_mult). */
int pstat_scale_kT(pstat_handle *h, double mult);
/* What a fresh call of the reference's mcmc(nsteps, pargs, chain) resets besides the averagers
 * (mcmc_clustering_eap_chain.jl:172-181,263-266): step sizes back to --phi-step/--theta-step, the
 * adaptation counters, the acceptor's cache, the in-run step counter.  The chains are kept. */
int pstat_reset_sampler(pstat_handle *h);

/* Device-side reduction over the chains of case `icase` (or over all cases if icase < 0) into
 * `dev_out`, a DEVICE pointer to PSTAT_NRED doubles owned by the caller (e.g. a torch tensor that
 * is then all-reduced with RCCL).  Asynchronous on the handle's stream. */
int pstat_reduce_device(pstat_handle *h, int32_t icase, double *dev_out);
/* The same vector copied back to host memory (synchronises): shards held by several handles in one
 * process (one per device) are merged by adding their vectors. */
int pstat_reduce_host(pstat_handle *h, int32_t icase, double red_out[PSTAT_NRED]);

/* Replaces get_avg() over the 8 averagers as written to rolling.csv (mcmc_eap_chain.jl:334-346;
 * inc/average.jl:38): pooled running averages of case `icase`, plus across-chain standard errors.
 * Either output pointer may be NULL.  Synchronises. */
int pstat_rolling(pstat_handle *h, int32_t icase, double avg_out[PSTAT_NOBS],
                  double stderr_out[PSTAT_NOBS]);

/* Replaces the trajectory.csv row source, mcmc_eap_chain.jl:330-333: r(3), p(3), U of one chain
 * (`chain` counts over all cases: case = chain / num_chains).  Synchronises. */
int pstat_microstate(pstat_handle *h, int64_t chain, double out[7]);

/* The quantities printed at mcmc_eap_chain.jl:365,386-395.  Synchronises.  Like every accessor that
 * synchronises (pstat_sync, pstat_reduce_host, pstat_rolling, pstat_microstate, pstat_chain_state,
 * pstat_chain_extras, pstat_checkpoint, pstat_corr_read, pstat_corr_rows, pstat_shape_read, pstat_shape_rows, pstat_pdist_read, pstat_pdist_rows, pstat_energy_read, pstat_energy_rows, pstat_series_read, pstat_series_error_bars, pstat_hist_read) it fails with PSTAT_ERR_HIP if a launch since the last successful
 * call did not run to completion (a job of the persistent kernels timed out waiting for its predecessor):
 * the handle's averages are then not the averages of the steps it was asked for. */
int pstat_summary_get(pstat_handle *h, int32_t icase, pstat_summary *out);

/* Turns already-merged reduction vectors (host memory, PSTAT_NRED doubles, e.g. after an
 * all-reduce over GPUs) into a summary.  Pure host arithmetic. */
int pstat_summary_from_reduction(const double red[PSTAT_NRED], int64_t steps_per_chain,
                                 pstat_summary *out);

/* The stepout time series (the rows of <prefix>_trajectory.csv and <prefix>_rolling.csv, mcmc_eap_chain.jl:329-348,
 * mcmc_clustering_eap_chain.jl:312-335), recorded on the device for every case of the handle at once and read back in
 * bulk.  A series belongs to the handle it was opened on; it is not part of a checkpoint, and pstat_destroy closes the
 * ones still open.
 *   pstat_series_open     device memory for `capacity_rows` rows of ncases * (PSTAT_NRED + 7 [+ 2n]) doubles.
 *                         PSTAT_SERIES_ANGLES: rows also hold the angles of every case's first chain.  PSTAT_ERR_NOMEM if
 *                         the device allocation fails.
 *   pstat_advance_series  pstat_advance(h, nsteps) that appends a row after every `stepout`-th step counted from the start
 *                         of the call (one small launch per row for all cases; a remainder nsteps % stepout is advanced
 *                         and not recorded).  Asynchronous on the handle's stream.  The chains, generators, counters and
 *                         running sums end up exactly as after pstat_advance.  If the rows would not fit it fails with
 *                         PSTAT_ERR_TOO_SMALL before anything is enqueued.
 *   pstat_series_read     the first `nrows` rows recorded (at most those recorded so far), host memory; synchronises, and
 *                         fails like every accessor that does if a launch did not complete.  For row r and case k:
 *                         steps_recorded[r] the steps every chain had recorded; red[r][k] the vector pstat_reduce_host(h, k)
 *                         would have returned at that step; micro[r][k] what pstat_microstate(h, k * num_chains) would
 *                         have; angles[r][k] the theta[n] then phi[n] of pstat_chain_state for that chain -- equal as
 *                         doubles, each of them.  Any output pointer may be NULL (angles must be, without PSTAT_SERIES_ANGLES).
 *   pstat_series_clear    forgets the rows, keeps the memory. */
typedef struct pstat_series pstat_series;
enum { PSTAT_SERIES_ANGLES = 1 };
int pstat_series_open(pstat_handle *h, int64_t capacity_rows, int32_t flags, pstat_series **out);
int pstat_advance_series(pstat_handle *h, pstat_series *s, int64_t nsteps, int64_t stepout);
int pstat_series_read(pstat_handle *h, pstat_series *s, int64_t nrows, int64_t *steps_recorded /* [nrows] */,
                      double *red /* [nrows][ncases][PSTAT_NRED] */, double *micro /* [nrows][ncases][7] */,
                      double *angles /* [nrows][ncases][2n] */);
int pstat_series_clear(pstat_handle *h, pstat_series *s);
void pstat_series_close(pstat_handle *h, pstat_series *s);

/* Error bars from one run: blocked standard errors (Flyvbjerg & Petersen, J. Chem. Phys. 91, 461 (1989)) of the batch means
 * between the rows of a series, computed on the device; the series is not copied to the host.  The reference has no
 * equivalent: its author gets uncertainties by repeating runs (2D/run/Ising_2024-11-06.jl: run=1:10).
 * The estimator, for one column of N batch values (DESIGN.md 3.12 states it in full):
 *   level 0 is the column; level l+1 averages neighbours, x'[j] = (x[2j] + x[2j+1]) / 2, a trailing odd value dropped; levels
 *   exist while N_l >= 2, at most PSTAT_BLOCK_LEVELS.  se_l = sqrt(sum (x - m_l)^2 / (N_l - 1) / N_l) about the level's own
 *   mean m_l.  Among the levels with N_l >= min_blocks the one of largest se_l is picked (the lowest on ties);
 *   converged = 0 if that is the last such level AND se rose into it by more than its own uncertainty, se_l* - se_(l*-1) >
 *   se_l* / sqrt(2 (N_l* - 1)), or it is level 0: the curve is still rising, the run is too short for this observable.  (The
 *   last level alone would flag a third of the columns of an amply long series: on the plateau the largest se falls on the
 *   noisiest level.)
 *   A non-finite se_l among them: stderr, stderr_err, inefficiency = NaN, level = -1, converged = 0.  se_0 == 0 (a constant
 *   column, e.g. the y slots of a planar handle): stderr = 0, inefficiency = 1, level = 0, converged = 1.
 * Per column PSTAT_EB_FIELDS doubles: mean m_0, stderr se_l*, stderr_err se_l* / sqrt(2 (N_l* - 1)), inefficiency
 * (se_l* / se_0)^2, level l*, converged; `levels` (may be NULL): se_l of every level, 0 beyond the last.
 *
 *   pstat_series_error_bars  the columns are the PSTAT_NQ quantities of every case in the order of the reduction vector
 *       (16 observables, acceptance ratio, sum cos^2 theta, mean bond angle), the batches the differences of consecutive rows
 *       among [first_row, first_row + nrows): with S_r = red[r][k][1 + q] * steps[r] and d the rows' common spacing in steps,
 *       batch = (S_r - S_{r-1}) / (d * red[r][k][0]).  If steps[first_row] == d the series began at empty averages (creation,
 *       pstat_reset_averages): the baseline is zero and nrows rows give nrows batches; otherwise the first row is the
 *       baseline and they give nrows - 1.  *nbatches receives the count.  Synchronises, and fails like every accessor that
 *       does after an incomplete launch.  Every precision and every home, planar handles included.
 *       PSTAT_ERR_INVALID_ARG: a series of another handle; a row range outside the recorded rows; rows that are not equally
 *       spaced and increasing (two pstat_advance_series calls of different stepout, a pstat_reset_averages between rows: the
 *       message names the row); min_blocks < 2 other than 0.  PSTAT_ERR_TOO_SMALL: fewer batches than min_blocks (the
 *       count is written to *nbatches).  PSTAT_ERR_UNSUPPORTED: more than PSTAT_BLOCK_MAX_BATCHES batches (level 1 of a column
 *       must fit the LDS of a CU); an umbrella-sampling handle -- its recorded means are ratios value / normalizer with
 *       per-chain normalizers that the rows do not hold, so the rows' differences are not batch means.
 *   pstat_blocking_device    the same transform of any matrix x[nbatches][stride] in DEVICE memory of which the first `ncols`
 *       columns are taken (e.g. a torch tensor, or series merged over ranks), on `device` and on `stream` (NULL: the default
 *       stream); synchronises the stream and leaves the calling thread's current device as it found it.  The argument errors
 *       above plus stride < ncols, all raised before the device is touched.
 * NB the constant-column rule holds for se_0 == 0 exactly: a column of one value whose sums are exact (0, 2.5, ...).  A
 * constant that is not (0.1, say) leaves a rounding-noise stderr of ~1e-17 relative, and level / converged of that noise. */
#define PSTAT_BLOCK_LEVELS 24
#define PSTAT_BLOCK_MAX_BATCHES 40960
enum { PSTAT_EB_MEAN, PSTAT_EB_STDERR, PSTAT_EB_STDERR_ERR, PSTAT_EB_INEFFICIENCY, PSTAT_EB_LEVEL, PSTAT_EB_CONVERGED,
       PSTAT_EB_FIELDS };
int pstat_series_error_bars(pstat_handle *h, pstat_series *s, int64_t first_row, int64_t nrows /* < 0: to the last row */,
                            int32_t min_blocks /* 0: 32 */, int64_t *nbatches /* out, may be NULL */,
                            double *out /* host [ncases][PSTAT_NQ][PSTAT_EB_FIELDS] */,
                            double *levels /* host [ncases][PSTAT_NQ][PSTAT_BLOCK_LEVELS] or NULL */);
int pstat_blocking_device(const double *x /* DEVICE memory, [nbatches][stride] */, int64_t nbatches, int64_t ncols, int64_t stride,
                          int32_t min_blocks, int32_t device, void *stream, double *out /* host [ncols][PSTAT_EB_FIELDS] */,
                          double *levels /* host [ncols][PSTAT_BLOCK_LEVELS] or NULL */);

/* Replica exchange (parallel tempering) between the cases of one handle, on the device.  The reference has no equivalent:
 * it gets cold chains out of metastable states with an annealed burn-in ladder and by repeating runs (run=1:25).  A handle
 * already holds every rung of a temperature ladder side by side; one exchange round is two small launches on its stream.
 * The contract (DESIGN.md 3.13 states it in full; polymer_stats_amd/csrc/pstat_exchange.hip is the device's statement):
 *   ladder     cases that differ in nothing but kT, seed and chain_id0; rungs = its cases by kT ascending at open time, ties by
 *              case index.  ladder[i] >= 0 names case i's ladder, -1 keeps it out of every exchange.
 *   pairing    round t pairs rungs (2j + (t & 1), 2j + 1 + (t & 1)); a rung without a partner sits the round out; chain k of
 *              one case pairs with chain k of the other.  t starts at 0, advances by one per call and is 32-bit: the call
 *              that would overflow it fails with PSTAT_ERR_INVALID_ARG.
 *   criterion  f64, every operation rounded: d = (1 / kT_a - 1 / kT_b) (U_a - U_b); accept iff U_a, U_b are finite and
 *              (d >= 0 or u < exp(d)), with the cases' CURRENT kT (a burn-in rung set by pstat_scale_kT exchanges at its
 *              scaled temperatures).
 *   stream     o = Philox4x32-10(key = (seed_lo, seed_hi), ctr = (k, lower rung's case index, 0x7e3a9e0d, t)), `seed` the
 *              tempering object's own; u = ((o[0] << 21) | (o[1] >> 11)) 2^-53.  The chains' generators are not touched.
 *   an accepted exchange swaps the two chains' configurations (angles, r, p, U and the other cached observables) and resets
 *   the acceptor's cache offset of both; running sums, normalizers, generators, step sizes, adaptation windows and acceptance
 *   counts stay with the case (the temperature), so every case's averages remain averages at its own kT.
 *
 *   pstat_tempering_open      checks the ladders and uploads both parities' partner tables.  Before the device is touched,
 *                             PSTAT_ERR_INVALID_ARG: null arguments; a ladder id below -1; a ladder whose cases differ in a
 *                             physics field other than kT (the message names the field and the case).
 *                             PSTAT_ERR_UNSUPPORTED: umbrella-sampling handles (their weights and reference energy are per
 *                             chain, relative to the chain's first configuration).  A ladder of one case is allowed and
 *                             never exchanges.
 *   pstat_tempering_exchange  one round; asynchronous on the handle's stream, no host synchronisation.
 *   pstat_tempering_stats     per case, counted on the LOWER rung of a pair: exchanges attempted and accepted (one per pair
 *                             of chains and round); *rounds = exchange calls so far.  Any output may be NULL.  Synchronises.
 *   pstat_tempering_close     pstat_destroy closes the ones still open.
 * The round counter and the counts are not part of a checkpoint.  Results are Boltzmann-exact only where the step itself is:
 * the fixed-force main without re-initialisation, or the clustering mains with single moves only. */
typedef struct pstat_tempering pstat_tempering;
int pstat_tempering_open(pstat_handle *h, const int32_t *ladder /* [ncases]: ladder id >= 0, or -1: takes no part */,
                         uint64_t seed, pstat_tempering **out);
int pstat_tempering_exchange(pstat_handle *h, pstat_tempering *t);
int pstat_tempering_stats(pstat_handle *h, pstat_tempering *t, int64_t *attempted /* [ncases] */, int64_t *accepted /* [ncases] */,
                          int64_t *rounds);
void pstat_tempering_close(pstat_handle *h, pstat_tempering *t);

/* Distributions on the device: per-case histograms of the chains' current configurations.  The reference has no equivalent on
 * the device side of anything: its run/microstates-F*.jl studies write 10 000 trajectory rows per case only to histogram them
 * afterwards, and its run/phases_* studies look for a bimodal P(U), P(p).  A histogram object belongs to the handle it was
 * opened on; one record is one small launch on the handle's stream that reads DevState::obs of EVERY chain (the series keeps
 * each case's first chain only) and writes the histogram's own buffers only.
 * The contract (DESIGN.md 3.14 states it in full; polymer_stats_amd/csrc/pstat_hist.hip is the device's statement):
 *   channel    PSTAT_HC_R1 .. PSTAT_HC_U (0..6): the seven doubles of pstat_microstate.  PSTAT_HC_RMAG (7): sqrt(r1 r1 + r2 r2 +
 *              r3 r3), PSTAT_HC_PMAG (8) the same over p; products rounded singly, added left to right.
 *   binning    is the formula, not the real interval.  The host computes inv = (double)nbins / (hi - lo) once; the device
 *              t = (x - lo) * inv, two rounded operations.  x not finite: tails[2] += 1.  t < 0: tails[0] += 1.  t >= nbins:
 *              tails[1] += 1.  Otherwise bin (int)t (truncation) += 1.  So lo falls in bin 0 and hi in the upper tail.
 *   counts     64-bit integers: integer sums do not depend on order, so results are exact and reproducible.
 *
 *   pstat_hist_open     per_case = 0: specs[nspecs] is shared by all cases; per_case = 1: specs[ncases][nspecs], where a spec's
 *                       channel and nbins agree across cases and only lo, hi may differ (U's range follows E0).  Before the
 *                       device is touched, with a message naming the spec and case, PSTAT_ERR_INVALID_ARG: null arguments;
 *                       nspecs outside 1..PSTAT_HIST_MAX_SPECS; a channel outside 0..8; nbins < 1; lo or hi not finite;
 *                       hi <= lo, or inv not finite and positive (hi - lo overflows or is denormal).
 *                       PSTAT_ERR_UNSUPPORTED: more than PSTAT_HIST_MAX_BINS bins per case (a workgroup keeps a case's bins in
 *                       LDS); an umbrella-sampling handle (its samples carry
 *                       per-chain weights whose gauge the rows do not hold: the reason error bars and exchange refuse it).
 *                       PSTAT_ERR_NOMEM: the device allocation fails.
 *   pstat_hist_record   adds the current configuration of every chain, one sample per chain and spec; asynchronous on the
 *                       handle's stream, no host synchronisation: what a caller interleaves with pstat_tempering_exchange or
 *                       pstat_advance_series.
 *   pstat_advance_hist  pstat_advance(h, nsteps) with a record after every `stepout`-th step counted from the start of the call;
 *                       a remainder nsteps % stepout is advanced and not recorded.  The chains, generators, counters and running
 *                       sums end up exactly as after pstat_advance.
 *   pstat_hist_read     counts[ncases][total_bins] (the specs' bins concatenated in order), tails[ncases][nspecs][3] (below,
 *                       above, not finite) and *records; any of them may be NULL.  Per case and spec, bins + tails = records *
 *                       num_chains.  Synchronises, and fails like every accessor that does after an incomplete launch.
 *   pstat_hist_clear    zeroes the counts and the record count, on the stream.
 *   pstat_hist_close    pstat_destroy closes the ones still open.  A histogram is not part of a checkpoint.
 *   A histogram of another handle (or a closed one) is PSTAT_ERR_INVALID_ARG.  Every home, every precision and planar handles
 *   are accepted; for a planar handle the y channels put every sample in whichever bin holds 0.
 *   pstat_histogram_device  the same binning of the columns of any matrix x[nrows][stride] in DEVICE memory (a torch tensor, a
 *                       series merged over ranks): a spec's `channel` is a column index below `stride`.  counts[total_bins] and
 *                       tails[nspecs][3] are host memory (either may be NULL).  On `device` and `stream` (NULL: the default
 *                       stream); synchronises the stream and leaves the calling thread's current device as it found it.  The
 *                       argument errors above (a channel outside 0..stride-1 in place of 0..8) plus nrows < 0, all raised before
 *                       the device is touched. */
enum { PSTAT_HC_R1, PSTAT_HC_R2, PSTAT_HC_R3, PSTAT_HC_P1, PSTAT_HC_P2, PSTAT_HC_P3, PSTAT_HC_U, PSTAT_HC_RMAG, PSTAT_HC_PMAG,
       PSTAT_HC_COUNT };
#define PSTAT_HIST_MAX_BINS 8192
#define PSTAT_HIST_MAX_SPECS 16
typedef struct pstat_hist_spec { int32_t channel; int32_t nbins; double lo, hi; } pstat_hist_spec;
typedef struct pstat_hist pstat_hist;
int pstat_hist_open(pstat_handle *h, const pstat_hist_spec *specs /* [nspecs], or [ncases][nspecs] if per_case */, int32_t nspecs,
                    int32_t per_case, pstat_hist **out);
int pstat_hist_record(pstat_handle *h, pstat_hist *g);
int pstat_advance_hist(pstat_handle *h, pstat_hist *g, int64_t nsteps, int64_t stepout);
int pstat_hist_read(pstat_handle *h, pstat_hist *g, int64_t *counts /* [ncases][total_bins] */,
                    int64_t *tails /* [ncases][nspecs][3] */, int64_t *records);
int pstat_hist_clear(pstat_handle *h, pstat_hist *g);
void pstat_hist_close(pstat_handle *h, pstat_hist *g);
int pstat_histogram_device(const double *x /* DEVICE memory, [nrows][stride] */, int64_t nrows, int64_t stride,
                           const pstat_hist_spec *specs, int32_t nspecs, int32_t device, void *stream,
                           int64_t *counts /* host [total_bins] */, int64_t *tails /* host [nspecs][3] */);

/* Chain structure on the device: per-case lag correlations of the monomers' orientations and dipoles.  Everything above reads
 * the seven numbers r, p, U of a chain; this looks inside it.  The reference can only infer the tangent correlation of its
 * worm-like-chain check (run/wlc-test_2022-03-14.jl) from <r^2>, and its (E0, kT) phase scans record one-point and nearest-
 * neighbour order parameters only.  A correlation object belongs to the handle it was opened on; one record is a pair of
 * launches on the handle's stream that reads the stored angles of EVERY chain where they sit and writes the object's own
 * buffers only.
 * The contract (DESIGN.md 3.15 states it in full; polymer_stats_amd/csrc/pstat_corr.hip is the device's statement).  All in f64
 * from the doubles pstat_chain_state returns for the angles, whatever the handle's precision:
 *   3D handles      n_i = (cos phi_i sin theta_i, sin phi_i sin theta_i, cos theta_i); the field axis z is component 3.
 *                   dielectric mu_i = (K1 - K2) E0 cos theta_i n_i + K2 E0 z; polar mu_i = mu n_i; the case's own E0, K1, K2, mu.
 *   planar handles  n_i = (cos phi_i, sin phi_i); the field axis is component 2.
 *                   dielectric mu_i = (K1 - K2) E0 sin phi_i n_i + (0, K2 E0); polar mu_i = mu n_i.
 *   per chain c and lag k = 0 .. max_lag, (1 / (n - k)) sum_{i = 0}^{n - 1 - k} of
 *                   PSTAT_CORR_NN  n_i . n_{i+k}       (tangent correlation; k = 0 gives 1)
 *                   PSTAT_CORR_ZZ  n_{i,z} n_{i+k,z}   (along the field; with <r_z> / (n b) it gives the connected correlation)
 *                   PSTAT_CORR_MM  mu_i . mu_{i+k}     (dipole correlation)
 *   columns         the channels of the mask in the order NN, ZZ, MM, each max_lag + 1 wide: ncols = (max_lag + 1) * channels.
 *   totals          per case and column one record adds the sum over the case's chains of the per-chain value to `sum` and the
 *                   sum of its square to `sumsq`; both are additive across handles.  After ONE record the pooled mean
 *                   sum / num_chains has the across-chain standard error sqrt((sumsq / N - mean^2) / (N - 1)), N = num_chains,
 *                   which is rigorous because chains are independent.  Over many records the mean is sum / (records *
 *                   num_chains) and its error bar comes from the rows through pstat_blocking_device.
 *   reproducible    no floating-point atomics; the order of every addition depends on (ncases, num_chains, n, max_lag) only:
 *                   two identical runs give bit-identical totals.
 *
 *   pstat_corr_open     max_lag = -1 means n - 1.  capacity_rows = 0 keeps the totals only; > 0 also keeps one row per record.
 *                       Before the device is touched, with a message naming the argument, PSTAT_ERR_INVALID_ARG: null
 *                       arguments; channels outside 1 .. 7; max_lag < -1 or > n - 1; capacity_rows < 0.
 *                       PSTAT_ERR_UNSUPPORTED: an umbrella-sampling handle (its samples carry per-chain weights whose gauge the
 *                       sums do not hold: the reason error bars, exchange and histograms refuse it); a chain whose unit
 *                       vectors do not fit the 60 KiB of LDS a workgroup keeps them in: n > 2560 (planar handles: n > 3840).
 *                       PSTAT_ERR_NOMEM: the device allocation fails.
 *   pstat_corr_record   one record of the current configuration of every chain; asynchronous on the handle's stream, no host
 *                       synchronisation: what a caller interleaves with pstat_tempering_exchange or pstat_advance_series.
 *                       PSTAT_ERR_TOO_SMALL, with nothing enqueued, when capacity_rows > 0 and every row is taken.
 *   pstat_advance_corr  pstat_advance(h, nsteps) with a record after every `stepout`-th step counted from the start of the call;
 *                       a remainder nsteps % stepout is advanced and not recorded.  The chains, generators, counters and running
 *                       sums end up exactly as after pstat_advance.  PSTAT_ERR_TOO_SMALL before anything is enqueued when
 *                       capacity_rows > 0 and the call's nsteps / stepout rows would not fit; stepout < 1 or nsteps < 0 is
 *                       PSTAT_ERR_INVALID_ARG.
 *   pstat_corr_read     sum[ncases][ncols], sumsq[ncases][ncols] (host) and *records; any of them may be NULL.  Synchronises,
 *                       and fails like every accessor that does after an incomplete launch.
 *   pstat_corr_rows     *dev_rows = a matrix in DEVICE memory, [*nrows][*stride] with *stride = ncases * ncols: row r holds,
 *                       for every case and column, record r's sum over the case's chains / num_chains.  It is an input for
 *                       pstat_blocking_device (on the handle's device and stream).  NULL and 0 rows for an object opened with
 *                       capacity_rows = 0.  Synchronises like pstat_corr_read.  The pointer is good until the object is closed.
 *   pstat_corr_clear    zeroes the totals, the record and the row count, on the stream.
 *   pstat_corr_close    pstat_destroy closes the ones still open.  A correlation object is not part of a checkpoint.
 *   An object of another handle (or a closed one) is PSTAT_ERR_INVALID_ARG.  Every home, every precision and planar handles
 *   are accepted. */
enum { PSTAT_CORR_NN = 1, PSTAT_CORR_ZZ = 2, PSTAT_CORR_MM = 4 };
typedef struct pstat_corr pstat_corr;
int pstat_corr_open(pstat_handle *h, int32_t channels, int32_t max_lag, int64_t capacity_rows, pstat_corr **out);
int pstat_corr_record(pstat_handle *h, pstat_corr *g);
int pstat_advance_corr(pstat_handle *h, pstat_corr *g, int64_t nsteps, int64_t stepout);
int pstat_corr_read(pstat_handle *h, pstat_corr *g, double *sum /* [ncases][ncols] */, double *sumsq /* [ncases][ncols] */,
                    int64_t *records);
int pstat_corr_rows(pstat_handle *h, pstat_corr *g, const double **dev_rows /* DEVICE memory */, int64_t *nrows, int64_t *stride);
int pstat_corr_clear(pstat_handle *h, pstat_corr *g);
void pstat_corr_close(pstat_handle *h, pstat_corr *g);

/* Chain shape on the device: per-case gyration tensor and form factor S(q) of the monomers' positions.  The correlations above
 * read the bond directions; this reads where the monomers are: the size and shape of the coil and what it scatters.  The
 * reference keeps the positions (chain.xs, inc/eap_chain.jl:49-51) only to feed its pair energies.  A shape object is a sibling of
 * a correlation object: it belongs to the handle it was opened on, one record is a pair of launches on the handle's stream that
 * reads the stored angles of EVERY chain where they sit and writes the object's own buffers only.
 * The contract (DESIGN.md 3.16 states it in full; polymer_stats_amd/csrc/pstat_shape.hip is the device's statement).  All in f64
 * from the doubles pstat_chain_state returns for the angles, whatever the handle's precision:
 *   unit vectors    as for the correlations; a planar handle's n_i = (cos phi_i, sin phi_i) sits in the x and z slots, y = 0.
 *   positions       x_i = b (sum_{j <= i} n_j - n_i / 2), i = 0 .. n - 1: the monomers' centres, with the case's own b.
 *   gyration block  PSTAT_SHAPE_GYR = 8 columns per chain, in this order: gxx, gyy, gzz, gxy, gxz, gyz, rg2, trg2.
 *                   xbar = (1 / n) sum_i x_i;  G_ab = (1 / n) sum_i (x_i - xbar)_a (x_i - xbar)_b, centred first;
 *                   rg2 = G_xx + G_yy + G_zz;  trg2 = sum_ab G_ab^2, the off-diagonals counted twice.
 *                   A planar handle's gyy, gxy and gyz are exactly 0.
 *   form factor     nq >= 0 columns follow, one per wave-vector of the table q[nq][3] (absolute units; a planar handle
 *                   ignores q[.][1]):  S(c, q) = (1 / n) [(sum_i cos(q . x_i))^2 + (sum_i sin(q . x_i))^2]; q = 0 gives exactly n.
 *   columns         ncols = PSTAT_SHAPE_GYR + nq.
 *   totals          per case and column one record adds the sum over the case's chains of the per-chain value to `sum` and the
 *                   sum of its square to `sumsq`; both are additive across handles.  After ONE record the pooled mean
 *                   sum / num_chains has the across-chain standard error sqrt((sumsq / N - mean^2) / (N - 1)), N = num_chains.
 *                   Over many records the mean is sum / (records * num_chains) and its error bar comes from the rows through
 *                   pstat_blocking_device.
 *   reproducible    no floating-point atomics; the order of every addition, the prefix sum that makes the positions included,
 *                   depends on (ncases, num_chains, n, nq) only: two identical runs give bit-identical totals.
 *
 *   pstat_shape_open    q: host memory, copied.  capacity_rows = 0 keeps the totals only; > 0 also keeps one row per record.
 *                       Before the device is touched, with a message naming the argument, PSTAT_ERR_INVALID_ARG: null
 *                       arguments; nq < 0; a null q with nq > 0; a q component that is not finite; capacity_rows < 0; a
 *                       wave-vector and case with (|q_x| + |q_y| + |q_z|) b n >= 1e5 (below that the device's sincos is its
 *                       < 1 ulp routine; |q_y| does not count for a planar handle).  PSTAT_ERR_UNSUPPORTED: nq >
 *                       PSTAT_SHAPE_MAX_Q = 512; an umbrella-sampling handle (its samples carry per-chain weights whose gauge
 *                       the sums do not hold); a chain whose positions do not fit the 60 KiB of LDS a workgroup keeps them in:
 *                       n > 2560 (planar handles: n > 3840).  PSTAT_ERR_NOMEM: the device allocation fails.
 *   pstat_shape_record, pstat_advance_shape, pstat_shape_read, pstat_shape_rows, pstat_shape_clear, pstat_shape_close
 *                       what the pstat_corr_* call of the same name does for a correlation object: PSTAT_ERR_TOO_SMALL before
 *                       anything is enqueued when the rows would not fit; _read and _rows synchronise and fail like every
 *                       accessor that does after an incomplete launch; the rows are a DEVICE matrix [*nrows][*stride = ncases *
 *                       ncols] that pstat_blocking_device accepts; pstat_destroy closes the objects still open; a shape object
 *                       is not part of a checkpoint.
 *   An object of another handle (or a closed one) is PSTAT_ERR_INVALID_ARG.  Every home, every precision and planar handles
 *   are accepted. */
#define PSTAT_SHAPE_GYR 8
#define PSTAT_SHAPE_MAX_Q 512
typedef struct pstat_shape pstat_shape;
int pstat_shape_open(pstat_handle *h, const double *q /* host [nq][3] */, int32_t nq, int64_t capacity_rows, pstat_shape **out);
int pstat_shape_record(pstat_handle *h, pstat_shape *g);
int pstat_advance_shape(pstat_handle *h, pstat_shape *g, int64_t nsteps, int64_t stepout);
int pstat_shape_read(pstat_handle *h, pstat_shape *g, double *sum /* [ncases][ncols] */, double *sumsq /* [ncases][ncols] */,
                     int64_t *records);
int pstat_shape_rows(pstat_handle *h, pstat_shape *g, const double **dev_rows /* DEVICE memory */, int64_t *nrows, int64_t *stride);
int pstat_shape_clear(pstat_handle *h, pstat_shape *g);
void pstat_shape_close(pstat_handle *h, pstat_shape *g);

/* Pair distances on the device: per case the mean-square internal distance R^2(s), the closest approach of two monomers, the
 * distribution P(r) of the distances r_ij = |x_i - x_j| between two monomers of ONE chain, and the orientationally averaged
 * (Debye) structure factor.  The pair energies collapse into 1 / r^3 contacts; this is the recorder that shows how close the
 * closest pair is.  A pdist object is a sibling of a shape object: it belongs to the handle it was opened on, one record is a
 * pair of launches on the handle's stream that reads the stored angles of EVERY chain where they sit and writes the object's
 * own buffers only.
 * The contract (DESIGN.md 3.18 states it in full; polymer_stats_amd/csrc/pstat_pdist.hip is the device's statement).  All in f64
 * from the doubles pstat_chain_state returns for the angles, whatever the handle's precision:
 *   positions       exactly the shape recorder's: x_i = b (sum_{j <= i} n_j - n_i / 2); a planar handle's n_i sits in the x and z
 *                   slots, y = 0.
 *   pair distance   for i < j: d = x_j - x_i;  r2 = (d_x d_x + d_y d_y) + d_z d_z, every product rounded (a planar handle: without
 *                   the y term);  r = sqrt(r2), correctly rounded.
 *   options         fixed at open (pstat_pdist_spec): max_sep in 0 .. n - 1 (-1 means n - 1); min_sep in 1 .. n - 1; nbins >= 0;
 *                   rmax > 0 and finite, needed when nbins > 0, in absolute units, shared by all cases (spec.rmax) or one per
 *                   case (rmax_per_case, which then replaces spec.rmax); the device gets inv = nbins / rmax, computed once on the
 *                   host; q[nq], nq >= 0 magnitudes >= 0 in absolute units.
 *   columns         per chain, in this order; ncols = max_sep + 1 + (nbins ? nbins + 1 : 0) + nq:
 *     msd           max_sep columns, s = 1 .. max_sep:  R2(s) = (1 / (n - s)) sum_{i = 0}^{n - 1 - s} r2_{i,i+s}.
 *     rmin          one column: the minimum of r_ij over the pairs with j - i >= min_sep.
 *     histogram     nbins + 1 columns, absent when nbins = 0: per-chain COUNTS, as doubles, of the pairs with j - i >= min_sep.
 *                   t = r * inv; the pair goes to bin (int)t if t < nbins, otherwise to the last column, "above": r = 0 falls in
 *                   bin 0 and r = rmax in "above".  A chain's columns add up to (n - min_sep)(n - min_sep + 1) / 2 exactly.
 *     Debye         nq columns:  S(q) = 1 + (2 / n) sum_{i < j} sinc(q r_ij) over ALL pairs, whatever min_sep is;  x = q r is
 *                   rounded once, sinc(0) = 1 exactly and otherwise sin(x) / x with the device's < 1 ulp sine; q = 0 gives
 *                   exactly n.  A planar handle uses the same formula: the flat chain oriented at random in space.  The average
 *                   over in-plane orientations only would need the Bessel function J0, which the device math does not have.
 *   totals          as for a shape object: per case and column one record adds the sum over the case's chains of the per-chain
 *                   value to `sum` and the sum of its square to `sumsq`; both are additive across handles; a row is the record's
 *                   sum / num_chains.
 *   reproducible    no floating-point atomics; the order of every floating-point addition depends on (ncases, num_chains, n, the
 *                   object's options) only.  A chain's histogram is counted with integer adds, whose sum has no order.
 *
 *   pstat_pdist_open    q and rmax_per_case: host memory, copied; rmax_per_case may be NULL.  capacity_rows as for a shape object.
 *                       Before the device is touched, with a message naming the argument, PSTAT_ERR_INVALID_ARG: null
 *                       arguments (a null q with nq > 0 among them); n < 2 (there is no pair); max_sep or min_sep out of range;
 *                       nbins < 0; nq < 0; nbins > 0 with an rmax that is not finite or not positive or leaves no finite
 *                       nbins / rmax; a q that is negative or not finite; q b n >= 1e5 for any case (below that the device's
 *                       sine is its < 1 ulp routine); capacity_rows < 0.  PSTAT_ERR_UNSUPPORTED: nq > PSTAT_PDIST_MAX_Q = 64;
 *                       nbins > PSTAT_PDIST_MAX_BINS = 512; an umbrella-sampling handle (its samples carry per-chain weights
 *                       whose gauge the sums do not hold); a chain whose positions and one chain's nbins + 1 32-bit counters do
 *                       not fit the 60 KiB of LDS a workgroup keeps them in: n > (61440 - 8 ceil((nbins + 1) / 2)) / 24, that
 *                       is 2560 without a histogram and 2474 with 512 bins (planar handles: / 16, 3840 and 3711).
 *   pstat_pdist_record, pstat_advance_pdist, pstat_pdist_read, pstat_pdist_rows, pstat_pdist_clear, pstat_pdist_close
 *                       what the pstat_shape_* call of the same name does for a shape object, every rule included:
 *                       PSTAT_ERR_TOO_SMALL before anything is enqueued; _read and _rows synchronise and fail after an
 *                       incomplete launch; pstat_blocking_device accepts the rows; pstat_destroy closes the objects still open;
 *                       the object is not part of a checkpoint.
 *   An object of another handle (or a closed one) is PSTAT_ERR_INVALID_ARG.  Every home, every precision and planar handles
 *   are accepted. */
#define PSTAT_PDIST_MAX_Q 64
#define PSTAT_PDIST_MAX_BINS 512
typedef struct pstat_pdist_spec {
  int32_t max_sep, min_sep, nbins, nq;
  double rmax;
} pstat_pdist_spec;
typedef struct pstat_pdist pstat_pdist;
int pstat_pdist_open(pstat_handle *h, const pstat_pdist_spec *spec, const double *q /* host [nq] */,
                     const double *rmax_per_case /* host [ncases], or NULL */, int64_t capacity_rows, pstat_pdist **out);
int pstat_pdist_record(pstat_handle *h, pstat_pdist *g);
int pstat_advance_pdist(pstat_handle *h, pstat_pdist *g, int64_t nsteps, int64_t stepout);
int pstat_pdist_read(pstat_handle *h, pstat_pdist *g, double *sum /* [ncases][ncols] */, double *sumsq /* [ncases][ncols] */,
                     int64_t *records);
int pstat_pdist_rows(pstat_handle *h, pstat_pdist *g, const double **dev_rows /* DEVICE memory */, int64_t *nrows, int64_t *stride);
int pstat_pdist_clear(pstat_handle *h, pstat_pdist *g);
void pstat_pdist_close(pstat_handle *h, pstat_pdist *g);

/* The energy by term and separation on the device: per case what a chain's U is made of -- the field term, the work of the
 * force, the bending term, and the dipole-dipole sum split by the separation s = j - i along the chain, with the part beyond
 * max_sep and the part inside a radius.  An energy object is a sibling of a pdist object: it belongs to the handle it was opened
 * on, one record is a pair of launches on the handle's stream that reads the stored angles of EVERY chain where they sit and
 * writes the object's own buffers only.
 * The contract (DESIGN.md 3.19 states it in full; polymer_stats_amd/csrc/pstat_energy.hip is the device's statement).  All in f64
 * from the doubles pstat_chain_state returns for the angles, whatever the handle's precision:
 *   unit vectors,   exactly the correlation recorder's: 3D dielectric mu_i = (K1 - K2) E0 cos theta_i n_i + K2 E0 z, polar
 *   dipoles         mu_i = mu n_i, formed as f n_i + mb z with every product rounded; a planar handle has sin phi_i in place of
 *                   cos theta_i and keeps its vectors in the x and z slots, y = 0.
 *   positions       exactly the shape recorder's: x_i = b (sum_{j <= i} n_j - n_i / 2), the same scan.
 *   pair term       for i < j: d = x_j - x_i;  r2 = (d_x d_x + d_y d_y) + d_z d_z (planar: without the y term);  r = sqrt(r2),
 *                   correctly rounded;  mm = (mu_ix mu_jx + mu_iy mu_jy) + mu_iz mu_jz;  a = mu_i . d and c = mu_j . d added the
 *                   same way;  t_ij = (mm - 3 ((a c) / r2)) / (FOURPI (r2 r)) with FOURPI = 4.0 * 3.14159265358979323846 as a
 *                   double.  Every operation is rounded, the divisions are IEEE.  r = 0 gives a non-finite term, which reaches
 *                   the totals of the columns it belongs to and nothing else (the reference's own 0 * inf).
 *   options         fixed at open (pstat_energy_spec): max_sep in 0 .. n - 1 (-1 means n - 1); cutoff >= 0 in monomer lengths
 *                   as --cutoff-radius is, 0 for no `within` column, shared by all cases (spec.cutoff) or one per case
 *                   (cutoff_per_case, which then replaces spec.cutoff; a column exists when any of them is > 0).  On the
 *                   device crad = cutoff * b and crad2 = crad * crad, both rounded in f64, and a pair counts unless
 *                   r2 > crad2: the comparison and the products of the cutoff step kernel of an f64 handle.  n >= 1.
 *   columns         per chain, in this order; ncols = 3 + max_sep + 1 + (cutoff ? 1 : 0):
 *     field         sum_i (-E0 / 2) mu_{i,z} (planar: the second component).
 *     work          -(Fx R_x + Fz R_z) with R = x_{n-1} + (b / 2) n_{n-1}.
 *     bend          sum_{i < n-1} ((kappa / 2)(psi_i - psi0))(psi_i - psi0), psi_i = acos(clamp(n_i . n_{i+1}, -1, 1)) by the
 *                   device's 1.2 ulp acos.  Exactly 0 for every chain, with no acos evaluated, when the case's bend_mod is 0:
 *                   every handle of the fixed-force and of the planar main.
 *     pair[s]       max_sep columns, s = 1 .. max_sep:  sum_{i = 0}^{n-1-s} t_{i,i+s}.
 *     rest          sum_{s > max_sep} pair[s]; exactly 0 when max_sep = n - 1.
 *     within        sum_{i<j, r2 <= crad2} t_ij; only when a cutoff is set.
 *                   The pair columns hold the dipole-dipole sum WHATEVER the handle's energy type: on an Ising or a
 *                   non-interacting handle pair[2..] and rest are the energy the model leaves out.
 *   model total     the U the handle's own step carries (pstat_microstate's seventh value) is this combination of a chain's
 *                   columns, by the handle's energy_type:
 *                     PSTAT_NONINTERACTING  field + work + bend
 *                     PSTAT_ISING           field + work + bend + pair[1]
 *                     PSTAT_INTERACTING     field + work + bend + sum_s pair[s] + rest
 *                     PSTAT_CUTOFF          within alone, opened with the case's own cutoff_radius (UCutoff: no field, no force)
 *   totals          as for a pdist object: per case and column one record adds the sum over the case's chains of the per-chain
 *                   value to `sum` and the sum of its square to `sumsq`; both are additive across handles; a row is the record's
 *                   sum / num_chains.
 *   reproducible    no floating-point atomics; the order of every floating-point addition depends on (ncases, num_chains, n, the
 *                   object's options) only; two identical runs give identical bits.
 *
 *   pstat_energy_open   cutoff_per_case: host memory, copied; may be NULL.  capacity_rows as for a pdist object.  Before the
 *                       device is touched, with a message naming the argument, PSTAT_ERR_INVALID_ARG: null arguments; max_sep
 *                       outside -1 .. n - 1; reserved != 0; a cutoff that is negative or not finite, shared or per case;
 *                       capacity_rows < 0.  PSTAT_ERR_UNSUPPORTED: an umbrella-sampling handle (its samples carry per-chain
 *                       weights whose gauge the sums do not hold); a chain whose positions and dipoles do not fit the 60 KiB of
 *                       LDS a workgroup keeps them in: n > 61440 / 48 = 1280 (planar handles: / 32, 1920).
 *   pstat_energy_record, pstat_advance_energy, pstat_energy_read, pstat_energy_rows, pstat_energy_clear, pstat_energy_close
 *                       what the pstat_pdist_* call of the same name does for a pdist object, every rule included:
 *                       PSTAT_ERR_TOO_SMALL before anything is enqueued; _read and _rows synchronise and fail after an
 *                       incomplete launch; pstat_blocking_device accepts the rows; pstat_destroy closes the objects still open;
 *                       the object is not part of a checkpoint.
 *   An object of another handle (or a closed one) is PSTAT_ERR_INVALID_ARG.  Every home, every precision and planar handles
 *   are accepted. */
typedef struct pstat_energy_spec {
  int32_t max_sep, reserved;
  double cutoff;
} pstat_energy_spec;
typedef struct pstat_energy pstat_energy;
int pstat_energy_open(pstat_handle *h, const pstat_energy_spec *spec, const double *cutoff_per_case /* host [ncases], or NULL */,
                      int64_t capacity_rows, pstat_energy **out);
int pstat_energy_record(pstat_handle *h, pstat_energy *g);
int pstat_advance_energy(pstat_handle *h, pstat_energy *g, int64_t nsteps, int64_t stepout);
int pstat_energy_read(pstat_handle *h, pstat_energy *g, double *sum /* [ncases][ncols] */, double *sumsq /* [ncases][ncols] */,
                      int64_t *records);
int pstat_energy_rows(pstat_handle *h, pstat_energy *g, const double **dev_rows /* DEVICE memory */, int64_t *nrows, int64_t *stride);
int pstat_energy_clear(pstat_handle *h, pstat_energy *g);
void pstat_energy_close(pstat_handle *h, pstat_energy *g);

/* Per-chain accessors for tests and tooling (host buffers).  angles: theta[n] then phi[n] as
 * doubles, radians; sums: the 16 per-chain running sums in rolling.csv order;
 * counters: {accepted_total, steps_recorded, nacc_window, natt_window};
 * steps: {phi_step, theta_step, normalizer}, normalizer = the averagers' denominator for this chain
 * (steps recorded, or the sum of 1/e^w under umbrella sampling up to a per-chain factor that the sums share: the gauge
 * of w rises with the heaviest configuration a chain has visited, so that neither overflows -- DESIGN.md 3.5). */
int pstat_chain_state(pstat_handle *h, int64_t chain, double *angles /* [2n] */,
                      double sums[PSTAT_NOBS], int64_t counters[4], double steps[3],
                      uint32_t rng[4]);

/* Per-chain running means of case `icase` (all cases if < 0), host memory: out[q * nchains + k], q < PSTAT_NQ in the
 * order of the reduction vector (16 observables, acceptance ratio, the clustering main's two extras), k counting
 * the chains of that case.  This is what the device reduction folds; a host that honours --numeric-type
 * (mcmc_eap_chain.jl:186-197: Float128 / Dec128 / BigFloat averagers) merges these in its own wide type -- the
 * per-chain sums themselves are Float64 on the device, like the reference's default.  Synchronises. */
int pstat_chain_means(pstat_handle *h, int32_t icase, double *out /* [PSTAT_NQ][nchains] */);

/* Start every chain over from a given configuration, as EAPChain(pargs) does with --x0/--dx0
 * (inc/eap_chain.jl:61-79): x0 holds [phi; theta] (len 2: every monomer) or the interleaved
 * [phi1, theta1, phi2, theta2, ...] (len 2n); each angle gets + Uniform(0, dx0).  Generators are
 * re-seeded, so the result is what pstat_create would have produced with that start; averagers,
 * step sizes and counters are reset.  x0 is host memory, copied before the call returns. */
int pstat_restart_from_x0(pstat_handle *h, const double *x0, int64_t len, double dx0_phi, double dx0_theta);
/* The clustering main's two extra averagers for one chain: their running sums and their value in
 * the current configuration (sum cos^2 theta; mean bond angle). */
int pstat_chain_extras(pstat_handle *h, int64_t chain, double extra_sums[2], double extra_now[2]);

/* Checkpoint / resume of the full device state (angles, generators, step sizes, counters, running
 * sums) and of every case's CURRENT kT (a rung of the burn-in ladder set by pstat_scale_kT / pstat_set_kT is
 * restored with the image).  pstat_checkpoint: call with buf == NULL to get the size in *bytes; a buffer that is too
 * small fails with PSTAT_ERR_TOO_SMALL and the required size written back.  pstat_restore continues exactly the run
 * the image was taken from, on a handle created with the same options: the image's header (format 4) names the ABI
 * version, n, the chain and case counts, precision, chain / energy type, generator, move set, umbrella, do-flips,
 * uniform_bits, case 0's seed and first chain id, and a fingerprint of all cases' physics scalars (other than the
 * current kT), seeds, chain ids, num_chains and the proposal / adaptation options; any mismatch, a foreign or
 * truncated buffer fails with PSTAT_ERR_BAD_CHECKPOINT and leaves the handle untouched.  The reference has no
 * equivalent. */
int pstat_checkpoint(pstat_handle *h, void *buf, size_t *bytes);
int pstat_restore(pstat_handle *h, const void *buf, size_t bytes);

/* Introspection for benchmarks: kernel name, LDS bytes per workgroup, workgroups, resident
 * workgroups per CU as given by the occupancy API for the sweep kernel of this handle. */
typedef struct pstat_launch_info {
  char kernel[64];
  int32_t lds_bytes;
  int32_t threads_per_block;
  int32_t lanes_per_block;
  int64_t blocks;
  int32_t blocks_per_cu;
  int32_t num_cus;
  int32_t packed_cases;     /* 1: a workgroup holds `lanes_per_block` consecutive chains whichever cases they belong to (picked
                             * by pstat_create when cases have few chains each: the reference's sweeps run 1-25 per case,
                             * run/K1_E0-kT-phase.jl:19-45); 0: workgroups never straddle a case                          */
  int32_t reserved;
} pstat_launch_info;
int pstat_launch_info_get(pstat_handle *h, pstat_launch_info *out);

#ifdef __cplusplus
}
#endif
#endif
