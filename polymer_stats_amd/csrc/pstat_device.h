// pstat_device.h -- internal layout shared by the HIP kernels and the C-ABI host code.
// Not part of the public interface (that is include/pstat.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pstat {

// ---------------------------------------------------------------------------------------------
// Device-resident state of one handle.  Everything is struct-of-arrays over the chain index c
// (fastest-varying), so that the 64 lanes of a wave -- 64 consecutive chains -- touch 64
// consecutive elements: every spill/fill of chain state is a fully coalesced 256/512-byte access.
// C = ncases * chains_per_case.
// ---------------------------------------------------------------------------------------------
enum { OBS_R1 = 0, OBS_R2, OBS_R3, OBS_P1, OBS_P2, OBS_P3, OBS_U, OBS_USUM,
       OBS_C2,    // sum_i cos^2(theta_i)            (clustering main, mcmc_clustering_eap_chain.jl:243)
       OBS_PSI,   // sum of the n-1 bond angles psi   (:244)
       NOBS_STATE };
// per-chain running sums kept on the device; r.r and p.p are the sums of their components.  The
// first NSUMS_BASE are what mcmc_eap_chain.jl records; the clustering main adds two more.
enum { S_R1 = 0, S_R2, S_R3, S_R1SQ, S_R2SQ, S_R3SQ, S_P1, S_P2, S_P3, S_P1SQ, S_P2SQ, S_P3SQ,
       S_U, S_USQ, NSUMS_BASE, S_C2 = NSUMS_BASE, S_PSI, NSUMS };

struct DevState {
  void *ang;            // R  [2][n][C]   plane 0 = theta, plane 1 = phi (radians); planar handles: plane 0 is zero
  void *ang_tmp;        // R  [2][n][C]   scratch for re-initialisation
  uint32_t *rng;        // u32[4][C]      xoshiro128++ state
  double *stepsz;       // f64[2][C]      phi_step, theta_step (mcmc_eap_chain.jl:172)
  int64_t *win;         // i64[2][C]      nacc, natt since the last adaptation (:263,265; Int in the reference:
                        //                a window is never reset while the ratio stays inside the band)
  int64_t *nacc_total;  // i64[C]         (:264)
  double *obs;          // f64[NOBS_STATE][C]  r, p, U, sum(u) of the current microstate
  double *sums;         // f64[NSUMS][C]  averager .value fields (inc/average.jl:9)
  double *wnorm;        // f64[C]         averager .normalizer under umbrella sampling
  double *lag;          // f64[C]         acceptor's cached log-pi minus the chain's own (re-init)
  double *uref;         // f64[C]         sum(u) of the chain's first configuration: the umbrella weights
                        //                are taken relative to it (a per-chain constant factor cancels
                        //                in value/normalizer, inc/average.jl:38,63-67)
  void *work;           // homes SweepMem and ClusterMem only: the waves' working copy of their chains while a segment
                        //                runs (filled from / spilled to `ang` like LDS is); not checkpointed.  Sweep:
                        //                [chain block][n][64] double2 (theta, phi), chain-contiguous for the Ising energy.
                        //                Clustering main: [chain block][lane][n] 40-byte (f32: 20-byte) cells (pstat_cluster_gm.hip)
  int64_t *nanrej;      // i64[C]         proposals whose trial energy was NaN or +-Inf (1/r^3 singularities of the
                        //                pair energies; the reference rejects them silently, inc/acceptance.jl:29-39)
  int64_t C;
};

struct CaseConst {      // physics scalars of one case (inc/eap_chain.jl:89-108)
  double E0, K1, K2, mu, kT, Fz, Fx, b;
  uint64_t seed, chain_id0;
  double kappa, psi0;     // --bend-mod, --bend-angle (clustering main; 0 in mcmc_eap_chain.jl)
  double cluster_prob;    // --cluster-prob: probability of NOT attempting a cluster flip (planar main: OF flipping)
  double cutoff_radius;   // --cutoff-radius in monomer lengths (energy-type cutoff)
};
// AntiDipoleWeightFunction's scale (inc/average.jl:104-124): the umbrella weight of a configuration is sum(u) times this
__host__ __device__ inline double umbrella_wscale(const CaseConst &cc) {
  return (0.2 + 0.8 * exp(-(cc.Fx * cc.Fx + cc.Fz * cc.Fz) / cc.kT)) / cc.kT;
}

struct InitOpts {       // how EAPChain(pargs) draws the first configuration (inc/eap_chain.jl:61-79)
  int use_x0;           // 0: uniform angles; 1: (x0_phi, x0_theta) for every monomer; 2: per monomer from x0_vec
  double x0_phi, x0_theta, dx0_phi, dx0_theta;
  const double *x0_vec; // device, [phi1, theta1, phi2, theta2, ...] (use_x0 == 2)
};

struct SweepArgs {
  int64_t n;
  int64_t chains_per_case;
  int64_t blocks_per_case;
  int64_t nsteps;            // steps to run in this launch
  int64_t step0;             // steps already done in the current init
  int64_t steps_per_adjust;
  double adj_lb, adj_ub, adj_scale;
  int32_t lanes;             // chains per workgroup (64, or fewer when n is too long for LDS)
  int32_t adaptive;          // adj_scale != 1 && steps_per_adjust > 0
  int64_t ncases;
  int64_t seg_len;           // steps per time segment (job) of this launch
  int32_t nseg;              // segments per chain block in this launch
  int32_t max_spins;         // bound on the predecessor wait (each spin sleeps ~2 us)
  int32_t lds_rows;          // f64 state-in-memory sweep: monomers [0, lds_rows) keep their cells in LDS
  int32_t wide_eps;          // f64 kernels: the Metropolis eps carries 53 random bits (pstat_params.uniform_bits; eps_uniform, pstat_math.h)
  int64_t nblocks;           // chain blocks (workgroup-sized groups of `lanes` chains) of the whole handle
  int32_t packed;            // 1: a block holds `lanes` CONSECUTIVE GLOBAL chains, i.e. several cases when a case has fewer
                             // chains than a wave has lanes (run_job_queue<true>); 0: blocks never straddle a case
  int32_t pad_;
};

template <typename R> struct K;  // constants of the adaptation logic (f64, like the reference)
template <> struct K<double> {
  static constexpr double pi = 3.14159265358979323846;
  static constexpr double half_pi = 1.57079632679489661923;
};
// The step-size adaptation of mcmc_eap_chain.jl:301-322 and mcmc_clustering_eap_chain.jl:287-308, per chain and in f64 like
// the reference, at the end of an adaptation window.  The acceptance window is kept as its value when the segment began
// (nacc_off, natt_off) plus the segment's own counts; a window that restarts becomes minus those counts.  The steps are in
// radians.  Returns the new steps and the new window.  THETA = false is the planar main's form
// (2D/mcmc_clustering_eap_chain.jl:257-275): phi_step alone, thstep passed through.  Every step kernel calls this; run_segment
// of pstat_kernels.hip keeps a copy of its own.  Everything goes in and out by value and the function is always
// inlined: that compiles to what the rule written in place compiles to (profiles/cluster_step/ab_stated_once.txt).
struct Adapted { double phistep, thstep; int64_t nacc_off, natt_off; };
template <bool THETA = true>
__host__ __device__ __forceinline__ Adapted adapt_steps(int64_t nacc_off, int64_t natt_off, const int nacc_seg, const int steps_seg,
                                                        const double lb, const double ub, const double scale, double phistep,
                                                        double thstep) {
  const int64_t nacc = nacc_off + nacc_seg, natt = natt_off + steps_seg;
  const double ratio = (double)nacc / (double)natt;
  if (ratio > ub && phistep != K<double>::pi && (!THETA || thstep != K<double>::half_pi)) {
    nacc_off = -nacc_seg; natt_off = -steps_seg;
    phistep = fmin(K<double>::pi, phistep * scale);
    if (THETA) thstep = fmin(K<double>::half_pi, thstep * scale);
  } else if (ratio < lb) {
    nacc_off = -nacc_seg; natt_off = -steps_seg;
    phistep /= scale;
    if (THETA) thstep /= scale;
  }
  return Adapted{phistep, thstep, nacc_off, natt_off};
}

// ---------------------------------------------------------------------------------------------
// Random stream contract (restated, not shared, in oracle/eap_oracle.c).  Two generators:
//
//  PSTAT_RNG_MWC64X (default): D. Thomas' MWC64X multiply-with-carry, state (x, c) 32+32 bits,
//      out = x ^ c;  (c:x) <- A * x + c,  A = 4294883355,  period ~2^63, passes TestU01 BigCrush.
//      One v_mad_u64_u32 + one v_xor per output: measured 125 cycles per MC step (4 outputs) for a
//      lone wave against 226 for xoshiro128++ (tools/ubench).  As an LCG it is s <- A*s mod M with
//      s = c*2^32 + x, M = A*2^32 - 1, so streams are split by SKIP-AHEAD: all chains of a run walk
//      ONE sequence, chain id k starting k * 2^40 outputs after the seed-selected base state
//      (s_k = s_base * G^k mod M, G = A^(2^40) mod M): disjoint by construction for 2^40 outputs
//      (~2.7e11 MC steps) per chain.  The base state comes from Philox4x32-10(key = seed).
//  PSTAT_RNG_XOSHIRO128PP: xoshiro128++ seeded per chain by Philox4x32-10(key = seed,
//      ctr = (chain_lo, chain_hi, 0x5eed, 0)).
//
//  u(w) = (w >> 9) * 2^-23;  idx = mulhi32(w, n).  The f64 kernels' Metropolis eps has 53 bits by default, made of its own
//  word and the unused low bits of the step's other draws (eps_uniform, pstat_math.h; pstat_params.uniform_bits).
// ---------------------------------------------------------------------------------------------
__host__ __device__ inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                              uint32_t k0, uint32_t k1, uint32_t out[4]) {
  for (int round = 0; round < 10; ++round) {
    uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    uint32_t n1 = (uint32_t)p1;
    uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    uint32_t n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

struct Xoshiro128pp {
  uint32_t s0, s1, s2, s3;
  __host__ __device__ inline void seed(uint64_t seed, uint64_t chain_id) {
    uint32_t o[4];
    philox4x32_10((uint32_t)chain_id, (uint32_t)(chain_id >> 32), 0x5eedu, 0u,
                  (uint32_t)seed, (uint32_t)(seed >> 32), o);
    if ((o[0] | o[1] | o[2] | o[3]) == 0u) o[0] = 1u;
    s0 = o[0]; s1 = o[1]; s2 = o[2]; s3 = o[3];
  }
  __host__ __device__ inline uint32_t next() {
    uint32_t a = s0 + s3;
    uint32_t result = ((a << 7) | (a >> 25)) + s0;
    uint32_t t = s1 << 9;
    s2 ^= s0; s3 ^= s1; s1 ^= s2; s0 ^= s3;
    s2 ^= t;
    s3 = (s3 << 11) | (s3 >> 21);
    return result;
  }
  // adopt the advanced copy `o` where `take` holds (branch-free conditional draw)
  __host__ __device__ inline void pick(bool take, const Xoshiro128pp &o) {
    s0 = take ? o.s0 : s0; s1 = take ? o.s1 : s1; s2 = take ? o.s2 : s2; s3 = take ? o.s3 : s3;
  }
  __host__ __device__ inline void load(const uint32_t *p, int64_t stride) {
    s0 = p[0]; s1 = p[stride]; s2 = p[2 * stride]; s3 = p[3 * stride];
  }
  __host__ __device__ inline void store(uint32_t *p, int64_t stride) const {
    p[0] = s0; p[stride] = s1; p[2 * stride] = s2; p[3 * stride] = s3;
  }
};

struct Mwc64x {
  static constexpr uint32_t A = 4294883355u;
  static constexpr uint64_t M = 0xFFFEB81AFFFFFFFFull;   // A * 2^32 - 1
  static constexpr uint64_t G40 = 0x82A211110E454078ull; // A^(2^40) mod M
  uint32_t x, c;
  __host__ __device__ static inline uint64_t addmod(uint64_t a, uint64_t b) {
    uint64_t s = a + b;                       // a, b < M < 2^64
    if (s < a || s >= M) s -= M;              // on wrap-around the true sum is s + 2^64
    return s;
  }
  __host__ __device__ static inline uint64_t mulmod(uint64_t a, uint64_t b) {
    uint64_t r = 0;
    while (b) {
      if (b & 1) r = addmod(r, a);
      a = addmod(a, a);
      b >>= 1;
    }
    return r;
  }
  __host__ __device__ static inline uint64_t powmod(uint64_t g, uint64_t e) {
    uint64_t r = 1;
    while (e) {
      if (e & 1) r = mulmod(r, g);
      g = mulmod(g, g);
      e >>= 1;
    }
    return r;
  }
  __host__ __device__ inline void seed(uint64_t seed, uint64_t chain_id) {
    uint32_t o[4];
    philox4x32_10(0u, 0u, 0x5eedu, 1u, (uint32_t)seed, (uint32_t)(seed >> 32), o);
    const uint64_t v = (uint64_t)o[0] | ((uint64_t)o[1] << 32);
    const uint64_t base = 1 + v % (M - 2);                 // in [1, M-2]
    const uint64_t s = mulmod(base, powmod(G40, chain_id));
    x = (uint32_t)s; c = (uint32_t)(s >> 32);
  }
  __host__ __device__ inline uint32_t next() {
    const uint32_t r = x ^ c;
    const uint64_t t = (uint64_t)x * A + c;
    x = (uint32_t)t; c = (uint32_t)(t >> 32);
    return r;
  }
  __host__ __device__ inline void pick(bool take, const Mwc64x &o) { x = take ? o.x : x; c = take ? o.c : c; }
  __host__ __device__ inline void load(const uint32_t *p, int64_t stride) { x = p[0]; c = p[stride]; }
  __host__ __device__ inline void store(uint32_t *p, int64_t stride) const {
    p[0] = x; p[stride] = c; p[2 * stride] = 0u; p[3 * stride] = 0u;
  }
};


#if defined(__HIPCC__)
// Persistent job loop of the chain-per-lane kernels (sweep_kernel, cluster_kernel).  A job = (chain
// block, time segment); jobs are handed out in segment-major order from one atomic counter, so all
// LDS-limited workgroup slots of the chip stay busy even when the number of chain blocks is not a
// multiple of the slots (e.g. 1286 blocks on 1024 slots at n = 100).  Segment s of a block may start
// only after segment s-1 of the same block has been spilled: a per-block counter, published with an
// agent-scope release and awaited with a relaxed poll + one agent-scope acquire
// (placement-independent; cdna_hip_programming.md Guideline 16).  Deadlock-free for any residency: a
// job's predecessor was handed out earlier, to a workgroup that is running and that itself only ever
// waits on still earlier jobs; the wait is bounded (max_spins) and a timeout is reported through the
// queue's error word.  `body(case constants, global chain, first step, number of steps, chain block)` runs one
// segment of one lane's chain.
//
// Which chains a block holds.  PACKED = false: blocks never straddle a case -- block (case, j) holds chains j * lanes ... of
// that case, so the case's physics scalars are wave-uniform and live in SGPRs; a case of 16 chains lights 16 lanes.
// PACKED = true (pstat_create picks it when it shortens the launch: the reference's own sweeps run 1-25 chains per case,
// run/K1_E0-kT-phase.jl:19-45): block b holds the `lanes` consecutive GLOBAL chains b * lanes ..., whichever cases they
// belong to; lane -> (case, chain) by one division per job, and `cases[icase]` is then a per-lane load, so the same body
// compiles with the case's scalars in VGPRs.  A chain's trajectory does not depend on which lanes share its wave.
template <bool PACKED = false, typename Body>
__device__ __forceinline__ void run_job_queue(const SweepArgs &A, int *__restrict__ queue, const int lane, Body &&body,
                                              const CaseConst *__restrict__ cases) {
  const int nblocks = (int)A.nblocks;
  const int njobs = nblocks * A.nseg;
  int *error = queue, *head = queue + 1, *done = queue + 2;   // the error word is sticky: launches clear queue[1..]
  bool failed = false;
  while (!failed) {
    int job = 0;
    if (lane == 0) job = atomicAdd(head, 1);
    job = __builtin_amdgcn_readfirstlane(job);
    if (job >= njobs) break;
    const int blk = job % nblocks, seg = job / nblocks;
    if (seg > 0) {
      int spins = 0;
      for (;;) {
        const int have = __builtin_amdgcn_readfirstlane(
            __hip_atomic_load(&done[blk], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        if (have >= seg) break;
        if (++spins > A.max_spins) { failed = true; break; }
        __builtin_amdgcn_s_sleep(64);
      }
      if (failed) {  // a predecessor never finished: flag it and stop taking jobs
        if (lane == 0) atomicExch(error, 1 + job);
        break;
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    const int64_t first = (int64_t)seg * A.seg_len;
    const int64_t left = A.nsteps - first;
    const int64_t len = left < A.seg_len ? left : A.seg_len;
    // lanes own disjoint LDS columns and never exchange data: idle lanes just skip the body
    if constexpr (PACKED) {
      const int64_t chain = (int64_t)blk * A.lanes + lane;
      if (len > 0 && lane < A.lanes && chain < A.ncases * A.chains_per_case)
        body(cases[chain / A.chains_per_case], chain, A.step0 + first, len, blk);
    } else {
      const int64_t icase = blk / A.blocks_per_case;
      const int64_t local = (int64_t)(blk % A.blocks_per_case) * A.lanes + lane;
      if (len > 0 && lane < A.lanes && local < A.chains_per_case)
        body(cases[icase], icase * A.chains_per_case + local, A.step0 + first, len, blk);
    }
    if (A.nseg > 1) {
      // publish: this wave's spill stores are complete and written back before the counter moves
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (lane == 0) __hip_atomic_store(&done[blk], seg + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}
#endif  // __HIPCC__

// The kernel family that runs a handle's steps, chosen once by choose_home() (pstat_api.hip).  The first four and the last
// run one chain per lane in chain blocks from the job queue (run_job_queue), the others one chain per wavefront.
enum Home {
  SweepLds,          // fixed-force main, cells in LDS (pstat_kernels.hip)
  SweepMem,          // fixed-force main, f64, cells in the global working buffer DevState::work (run_segment, ST = 2)
  ClusterLds,        // clustering main, cells in LDS (pstat_cluster.hip)
  ClusterMem,        // clustering main, chains in DevState::work (pstat_cluster_gm.hip: f64, and f32 for large ensembles)
  ClusterChainWave,  // clustering main, small f64 ensembles: one chain per wavefront (pstat_cluster_cw.hip)
  ClusterAllPairs,   // clustering main with the all-pairs energies (pstat_cluster_wave.hip)
  Interacting,       // fixed-force main with the all-pairs energy (pstat_interacting.hip)
  Planar,            // planar (2D) clustering main, one chain per lane, 8-byte phi cells in LDS (pstat_planar.hip)
};

// What pstat_api.hip chooses and reads once per handle; the host entry points below are asynchronous on `stream`.
struct LaunchCfg {
  int precision, chain_type, energy_type, do_flips, umbrella, has_fx;
  int lag;  // a re-init has happened on this handle
  int rng;  // PSTAT_RNG_MWC64X | PSTAT_RNG_XOSHIRO128PP
  int move_set;  // PSTAT_MOVES_SINGLE (mcmc_eap_chain.jl) | PSTAT_MOVES_CLUSTER (mcmc_clustering_eap_chain.jl)
  Home home;     // the kernel family
  int packed;    // chain blocks straddle cases (SweepArgs::packed): the kernel instantiation with per-lane case scalars
  int planar;    // a handle of pstat_create_planar (2D/mcmc_clustering_eap_chain.jl): one angle per monomer, home Planar
};

struct SweepRare {  // wave-uniform switches of the sweep's rarely used options (RARE instantiations only)
  int flips;        // --do-flips
  int lag;          // a re-init happened: the acceptor's cached log-pi may be offset (see reinit_kernel)
  int umb;          // --umbrella-sampling: AntiDipoleWeightFunction + UmbrellaAverager
};

// The instantiation that runs a handle's steps.  Each family file exports one function that resolves it for (cfg, n): the
// only place its template tree is walked and its display name (pstat_launch_info.kernel) stated.  The handle keeps the
// result; pstat_api.hip probes its occupancy and launches it.  Every step kernel takes (SweepArgs, DevState,
// const CaseConst *) and then its family's scalars, listed with each function (launch_steps passes them).
struct StepKernel {
  const void *fn;
  const char *name;
};
// the chain-per-lane kernels' name: the packed-cases instantiation says so
#define PSTAT_KERNEL_NAME(cfg, s) ((cfg).packed ? s " [packed cases]" : s)
StepKernel sweep_step_kernel(const LaunchCfg &cfg, int64_t n);         // homes SweepLds, SweepMem: SweepRare, int *queue
StepKernel cluster_step_kernel(const LaunchCfg &cfg, int64_t n);       // ClusterLds: int umbrella, int *queue
StepKernel cluster_gm_step_kernel(const LaunchCfg &cfg, int64_t n);    // ClusterMem: int umbrella, int *queue
StepKernel cluster_cw_step_kernel(const LaunchCfg &cfg, int64_t n);    // ClusterChainWave (n <= 256): int umbrella
StepKernel cluster_wave_step_kernel(const LaunchCfg &cfg, int64_t n);  // ClusterAllPairs (n <= 512): int umbrella, int cutoff
StepKernel interacting_step_kernel(const LaunchCfg &cfg, int64_t n);   // Interacting (n <= 512): int do_flips, int lag, int reinit_mode
StepKernel planar_step_kernel(const LaunchCfg &cfg, int64_t n);        // Planar: int umbrella, int *queue
// bytes of DevState::work for home ClusterMem
size_t cluster_gm_work_bytes(const LaunchCfg &cfg, const SweepArgs &a);

// initialisation and re-initialisation (pstat_kernels.hip)
hipError_t launch_init(const LaunchCfg &cfg, const SweepArgs &a, const DevState &s,
                       const CaseConst *cases, double phi_step, double theta_step,
                       const InitOpts &io, hipStream_t stream);
// the planar handle's initialisation (pstat_planar.hip; launch_init hands over to it): n words per chain, phi plane only
hipError_t launch_planar_init(const LaunchCfg &cfg, const SweepArgs &a, const DevState &s, const CaseConst *cases,
                              double phi_step, hipStream_t stream);
hipError_t launch_reset_sampler(const DevState &s, double phi_step, double theta_step, hipStream_t stream);
hipError_t launch_reinit(const LaunchCfg &cfg, const SweepArgs &a, const DevState &s,
                         const CaseConst *cases, int force_init, hipStream_t stream);
// true iff x is NaN or +-Inf (one v_cmp_class)
template <typename R> __host__ __device__ inline bool not_finite(R x) { return !__builtin_isfinite(x); }
// sum over the 64 lanes of a wavefront, valid in lane 0: the shfl_down tree whose order is part of every reduced result
// (pstat_reduce.hip, pstat_blocking.hip)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
// The ensemble reduction (pstat_reduce.hip), kernels and host statements of the same arithmetic.
// reduction of chains [c0, c1) into out[PSTAT_NRED]; partial = scratch of reduce_scratch_doubles()
hipError_t launch_reduce(const DevState &s, int64_t c0, int64_t c1, int64_t steps_recorded,
                         int umbrella, const CaseConst *cases, int64_t chains_per_case, int64_t n,
                         double *partial, double *out, hipStream_t stream);
size_t reduce_scratch_doubles();
// one row of a series: for every case k of the handle, red[k][PSTAT_NRED] = what launch_reduce gives for
// the case's chains, micro[k][7] = obs of the case's first chain, and, unless angles is null, angles[k][2n] = that chain's
// theta then phi in radians
hipError_t launch_record(const LaunchCfg &cfg, const SweepArgs &a, const DevState &s, const CaseConst *cases,
                         int64_t steps_recorded, double *red, double *micro, double *angles, hipStream_t stream);
// host: out[PSTAT_NOBS] = the sums in include/pstat.h order from the S_* rows of a [NSUMS][stride] array
void sums_in_abi_order(const double *sums, int64_t stride, double *out);
// host: out[PSTAT_NQ][m] = the mean vectors the reduction folds, of m chains gathered as sums[NSUMS][m], nacc[m] and, under
// umbrella sampling, wnorm[m] (null otherwise: the normaliser is `steps`)
void chain_means_host(const double *sums, const double *wnorm, const int64_t *nacc, int64_t steps, int64_t m, double *out);

// Blocked standard errors (pstat_blocking.hip; the estimator: DESIGN.md 3.12).
// x[nbatches][ncases * PSTAT_NQ] = the batch means between consecutive rows of a series' red[row][ncases][PSTAT_NRED], batch b
// ending at row row0 + b, where every chain had recorded steps0 + b d steps; zero_base: batch 0 starts from empty averages
hipError_t launch_series_batches(const double *red, int64_t row0, int64_t nbatches, int64_t ncases, int64_t steps0, int64_t d,
                                 int zero_base, double *x, hipStream_t stream);
// the blocking transform of every column of x[nbatches][stride]: out[ncols][PSTAT_EB_FIELDS] and, unless null,
// levels[ncols][PSTAT_BLOCK_LEVELS]; 2 <= nbatches <= blocking_max_batches(), stride >= ncols
hipError_t launch_blocking(const double *x, int64_t nbatches, int64_t ncols, int64_t stride, int min_blocks, double *out,
                           double *levels, hipStream_t stream);
int64_t blocking_max_batches();

// Replica exchange between cases (pstat_exchange.hip states the contract).
struct ExchangeArgs {
  int64_t per, C, n;           // chains per case, chains of the handle, monomers
  int64_t npairs;              // pairs of this round's parity
  uint32_t round;              // t
  uint32_t seed_lo, seed_hi;   // the tempering object's seed
  uint32_t pad_;
};
// one round: decisions for every (pair, chain) into flags[npairs * per], counted on the lower rung's case in attempted / accepted
// [ncases]; then the accepted pairs' ang and obs rows swapped and their lag zeroed.  pairs[npairs][2] = (lower, upper) case.
hipError_t launch_exchange(const ExchangeArgs &a, const DevState &s, const CaseConst *cases, const int32_t *pairs,
                           unsigned char *flags, int64_t *attempted, int64_t *accepted, size_t elem, hipStream_t stream);

// Per-case histograms of the chains' current configurations (pstat_hist.hip states the binning contract).
struct HistSpec {              // one spec as the device reads it
  int32_t channel;             // PSTAT_HC_* of a handle's histogram; a column of the matrix for pstat_histogram_device
  int32_t nbins;
  int32_t offset;              // of the spec's first bin among the case's total_bins
  int32_t pad_;
  double lo, inv;              // inv = (double)nbins / (hi - lo), computed once on the host
};
struct HistArgs {
  int64_t per;                 // samples per case: chains per case, or the rows of the matrix
  int64_t ncases;
  int64_t stride;              // between the channels of one sample's source: C for DevState::obs, 1 for a matrix
  int64_t pitch;               // between consecutive samples: 1 for DevState::obs, the matrix's stride
  int32_t nspecs, total_bins;
  int32_t per_case;            // specs[ncases][nspecs] instead of specs[nspecs]
  int32_t matrix;              // channels are plain columns (no magnitude channels)
};
// one record: for every case k and spec i, counts[k][offset_i + bin] or tails[k][i][0..2] += 1 per sample; src = DevState::obs,
// or the matrix
hipError_t launch_hist(const HistArgs &a, const double *src, const HistSpec *specs, int64_t *counts, int64_t *tails,
                       hipStream_t stream);

// The tile frame the correlation, the shape and the pair-distance recorder share (pstat_tile.h): a workgroup takes a tile of consecutive chains of
// one case, and its 256 threads are `groups` groups of `lpc` threads over the columns of the kind's hot loop.
struct TileArgs {
  int64_t per, ncases, n;      // chains per case, cases, monomers
  int64_t tiles;               // workgroups per case: ceil(per / tile_chains)
  int32_t ncols;               // columns of a case's record
  int32_t elem;                // bytes per stored angle of DevState::ang
  int32_t planar;
  int32_t tile_chains;         // chains per workgroup
  int32_t lpc, groups, nslots; // threads per group, groups per workgroup (lpc * groups = 256), columns per thread
};
// fills tiles, tile_chains, lpc, groups, nslots from the other fields and the `width` of the hot loop (lags, wave-vectors): 16
// chains per tile, fewer where a case has fewer or LDS is short; lpc = min(256, 2^ceil(log2 width)).  The shape of the
// reduction, which is part of the result
void tile_layout(TileArgs &a, int width);
// the longest chain whose unit vectors fit a workgroup's LDS
int64_t tile_max_n(int planar);
size_t tile_partial_doubles(const TileArgs &a);

// Per-case lag correlations of the chains' current orientations and dipoles (pstat_corr.hip states the contract).
struct CorrArgs : TileArgs {   // ncols = (max_lag + 1) * channels set; tile_layout's width = max_lag + 1
  int32_t channels;            // PSTAT_CORR_* mask
  int32_t max_lag;
  int32_t polar;
};
// one record: totals[2][ncases][ncols] (sum, then sumsq) += this record's, row[ncases][ncols] (unless null) = the cases' means
hipError_t launch_corr(const CorrArgs &a, const void *ang, const CaseConst *cases, double *partial, double *totals, double *row,
                       hipStream_t stream);

// Per-case gyration tensor and form factor of the chains' current positions (pstat_shape.hip states the contract).
struct ShapeArgs : TileArgs {  // ncols = PSTAT_SHAPE_GYR + nq; tile_layout's width = nq
  int32_t nq;                  // wave-vectors
};
// one record: totals[2][ncases][ncols] (sum, then sumsq) += this record's, row[ncases][ncols] (unless null) = the cases' means;
// q = the wave-vectors [nq][3] in device memory (may be null when nq = 0)
hipError_t launch_shape(const ShapeArgs &a, const void *ang, const CaseConst *cases, const double *q, double *partial,
                        double *totals, double *row, hipStream_t stream);

// Per-case pair distances of the chains' current positions (pstat_pdist.hip states the contract).
struct PdistArgs : TileArgs {  // ncols = max_sep + 1 + (nbins ? nbins + 1 : 0) + nq
  int32_t max_sep, min_sep;    // R2(s) for s = 1 .. max_sep; rmin and the histogram over the pairs with j - i >= min_sep
  int32_t nbins, nq;           // bins below rmax (0: no histogram); Debye magnitudes
};
// fills the tile fields of `a` from the others: tile_layout's, with fewer chains per tile where one chain's bin counters would
// not fit LDS behind the positions
void pdist_layout(PdistArgs &a);
// the longest chain whose positions and one chain's nbins + 1 counters fit a workgroup's LDS beside the scratch
int64_t pdist_max_n(int planar, int nbins);
// one record, as launch_shape; q = the magnitudes [nq], inv = nbins / rmax per case [ncases] in device memory (null when there
// are none)
hipError_t launch_pdist(const PdistArgs &a, const void *ang, const CaseConst *cases, const double *q, const double *inv,
                        double *partial, double *totals, double *row, hipStream_t stream);

// Per-case energy breakdown of the chains' current configurations (pstat_energy.hip states the contract).
struct EnergyArgs : TileArgs {  // ncols = 3 + max_sep + 1 + (cut ? 1 : 0)
  int32_t max_sep;              // pair[s] for s = 1 .. max_sep, the separations beyond it in `rest`
  int32_t cut;                  // a `within` column, its radius per case in the launch's table
  int32_t polar;
  int32_t paired;               // the pair mapping: separations u and n - u share a wavefront pass (1, the default), or one each
};
// fills the tile fields of `a` from the others: tile_layout's, with fewer chains per tile where the dipoles would not fit LDS
// behind the positions
void energy_layout(EnergyArgs &a);
// the longest chain whose positions and dipoles fit a workgroup's LDS beside the scratch
int64_t energy_max_n(int planar);
// one record, as launch_pdist; cutoff = the radius per case [ncases] in monomer lengths, device memory (null without the column)
hipError_t launch_energy(const EnergyArgs &a, const void *ang, const CaseConst *cases, const double *cutoff, double *partial,
                         double *totals, double *row, hipStream_t stream);

}  // namespace pstat
