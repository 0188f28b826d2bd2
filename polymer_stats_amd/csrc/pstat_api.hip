// pstat_api.hip -- the C ABI of include/pstat.h on top of the kernels in pstat_kernels.hip.
// Host-side only: owns device memory, validates options the way the reference's constructors do
// (inc/eap_chain.jl:81-105 error() branches), sequences launches on one HIP stream.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <utility>
#include <vector>

#include "../../include/pstat.h"
#include "pstat_cluster_common.h"
#include "pstat_device.h"
#include "pstat_math.h"

using namespace pstat;

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}

#define HIP_TRY(expr)                                                                     \
  do {                                                                                    \
    hipError_t _e = (expr);                                                               \
    if (_e != hipSuccess)                                                                 \
      return fail(PSTAT_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e));          \
  } while (0)

// an int-returning step of an entry point: PSTAT_OK or the status to hand back
#define PSTAT_TRY(expr)             \
  do {                              \
    int _rc = (expr);               \
    if (_rc) return _rc;            \
  } while (0)

constexpr uint64_t CKPT_MAGIC = 0x5053544154434b34ull;  // "PSTATCK4" (v4: the header identifies the handle it was taken from)
constexpr size_t kStateBuffers = 11;   // a checkpoint image holds the handle's first kStateBuffers allocations (pstat_create)
constexpr int kLdsBudget = 160 * 1024;   // LDS of a CU: the most a workgroup's dynamic LDS can be

struct Buffer {
  void *ptr = nullptr;
  size_t bytes = 0;
};

// Knobs for tests and experiments that force a choice the handle would otherwise make by its own measured rules.  Read once,
// when the handle is created; unset or out of range, each leaves that rule in charge.
//   PSTAT_F64_STATE=w...    the chain-per-wavefront kernel, for a configuration it covers (choose_home)
//   PSTAT_F64_STATE=l|g...  rules that kernel out; the f64 chain-per-lane kernels keep their cells in LDS | in memory
//   PSTAT_F32_STATE=l|g...  the f32 clustering main keeps its chains in LDS | in memory
//   PSTAT_PACK=0|1          set at all, rules out the chain-per-wavefront kernel; forces packed cases off | on for a
//                           chain-per-lane home with ncases > 1, and 1 prices the packed layout as a deep launch (shape)
//   PSTAT_LANES=k           lanes per workgroup: 1..64 for ClusterMem, 1..the LDS lane cap for the LDS homes (not SweepMem)
//   PSTAT_F64_LDS_ROWS=k    SweepMem: monomers whose cells stay in LDS, 0..the rows of a quarter of the LDS
//   PSTAT_SEGMENTS=k        time segments per chain-per-lane launch (below 1: 1), with no f32 bound on a segment's steps
//   PSTAT_MAX_SPINS=k       bound on the job queue's predecessor wait, if k > 0
//   PSTAT_ENERGY_MAP=s|p    the energy recorder's pair mapping: a separation per wavefront pass | s and n - s paired (the default)
struct Overrides {
  char f64_state = 0, f32_state = 0;   // first letter of the value (0: unset)
  int pack = -1;                       // -1: unset
  int lanes = 0, f64_lds_rows = -1;    // as atoi() reads them (0 / -1: unset)
  int segments = 0, max_spins = 0;     // 0: unset
  char energy_map = 0;                 // first letter of the value (0: unset)
};

Overrides read_overrides() {
  Overrides o;
  if (const char *e = getenv("PSTAT_F64_STATE")) o.f64_state = e[0];
  if (const char *e = getenv("PSTAT_F32_STATE")) o.f32_state = e[0];
  if (const char *e = getenv("PSTAT_PACK")) o.pack = atoi(e) != 0 ? 1 : 0;
  if (const char *e = getenv("PSTAT_LANES")) o.lanes = atoi(e);
  if (const char *e = getenv("PSTAT_F64_LDS_ROWS")) o.f64_lds_rows = atoi(e);
  if (const char *e = getenv("PSTAT_SEGMENTS")) o.segments = atoi(e) > 1 ? atoi(e) : 1;
  if (const char *e = getenv("PSTAT_ENERGY_MAP")) o.energy_map = e[0];
  if (const char *e = getenv("PSTAT_MAX_SPINS")) o.max_spins = atoi(e) > 0 ? atoi(e) : 0;
  return o;
}

// Device memory that goes with its owner: the scratch of one call, or a member of a recorder object.
template <class T>
struct DeviceMem {
  T *p = nullptr;
  DeviceMem() = default;
  DeviceMem(const DeviceMem &) = delete;
  DeviceMem &operator=(const DeviceMem &) = delete;
  ~DeviceMem() { (void)hipFree(p); }
  hipError_t malloc(size_t count) { return hipMalloc((void **)&p, count * sizeof(T)); }
  int alloc(size_t count) {
    hipError_t e = malloc(count);
    if (e != hipSuccess) return fail(PSTAT_ERR_NOMEM, "hipMalloc(%zu) failed: %s", count * sizeof(T), hipGetErrorString(e));
    return PSTAT_OK;
  }
};
using DeviceDoubles = DeviceMem<double>;

}  // namespace

template <class T>
using OpenList = std::vector<std::unique_ptr<T>>;   // deleting the handle, or erasing an entry, frees the object

struct pstat_handle {
  pstat_params base{};              // case 0's parameters (shared, non-physics fields)
  std::vector<CaseConst> cases;     // host copy
  std::vector<double> kT0;          // kT each case was created with (pstat_scale_kT)
  CaseConst *d_cases = nullptr;
  int ncases = 0;
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  LaunchCfg cfg{};
  StepKernel kernel{};              // the step kernel of cfg, resolved whenever cfg changes (resolve_kernel)
  Overrides ov;                     // test knobs, read at creation
  SweepArgs args{};
  DevState S{};
  std::vector<Buffer> bufs;         // every device allocation, in checkpoint order
  int *d_queue = nullptr;           // sweep job queue: counter, error flag, per-block progress
  int slots = 0;                    // resident sweep workgroups on the whole device
  double *d_partial = nullptr;      // reduction scratch
  double *d_red = nullptr;          // PSTAT_NRED doubles
  int64_t steps_recorded = 0;       // steps every chain has recorded so far (all inits)
  int64_t step_in_init = 0;         // the reference's loop variable `step` (mcmc_eap_chain.jl:276)
  size_t elem = 4;                  // sizeof(R)
  int failed_job = 0;               // sticky: 1 + the job of a persistent launch that timed out (0 = none)
  OpenList<pstat_series> series;        // the recorder objects still open
  OpenList<pstat_tempering> tempering;
  OpenList<pstat_hist> hists;
  OpenList<pstat_corr> corrs;
  OpenList<pstat_shape> shapes;
  OpenList<pstat_pdist> pdists;
  OpenList<pstat_energy> energies;
};

// ---- the recorder objects of a handle.  Each owns its device memory; the handle owns those that are open.

// The stepout time series of one handle: rows recorded on the device by launch_record, read back in bulk.
struct pstat_series {
  int64_t capacity = 0, rows = 0;
  DeviceDoubles d_red;              // [capacity][ncases][PSTAT_NRED]
  DeviceDoubles d_micro;            // [capacity][ncases][7]
  DeviceDoubles d_angles;           // [capacity][ncases][2n], PSTAT_SERIES_ANGLES only
  std::vector<int64_t> steps;       // [capacity]: the handle's steps_recorded at each row (known when the row is enqueued)
};

// Replica exchange between the cases of one handle (pstat_exchange.hip).
struct pstat_tempering {
  uint64_t seed = 0;
  uint64_t round = 0;               // the next round's t; 32 bits on the device
  int64_t npairs[2] = {0, 0};       // pairs of the even and of the odd rounds
  DeviceMem<int32_t> d_pairs[2];    // [npairs][2] = (lower, upper rung's case)
  DeviceMem<unsigned char> d_flags; // [max npairs * chains per case]
  DeviceMem<int64_t> d_counts;      // [2][ncases]: attempted, accepted, on the lower rung's case
};

// Per-case histograms of one handle (pstat_hist.hip).
struct pstat_hist {
  int32_t nspecs = 0, total_bins = 0, per_case = 0;
  int64_t records = 0;              // records enqueued since open / the last clear (known when a record is enqueued)
  DeviceMem<HistSpec> d_specs;      // [ncases][nspecs] if per_case, else [nspecs]
  DeviceMem<int64_t> d_counts;      // [ncases][total_bins], then tails [ncases][nspecs][3]
  size_t slots = 0;                 // int64 words of d_counts
};

// What the correlation, the shape and the pair-distance recorder share: per-case column totals, summed over the chains of every record.
struct ColumnTotals {
  size_t stride = 0;                // ncases * ncols: doubles of one row
  int64_t records = 0;              // records enqueued since open / the last clear (known when a record is enqueued)
  int64_t capacity = 0, rows = 0;   // rows kept (0: totals only) and taken
  DeviceDoubles d_totals;           // [2][ncases][ncols]: sum, sumsq
  DeviceDoubles d_partial;          // the tiles' partial sums of one record
  DeviceDoubles d_rows;             // [capacity][ncases][ncols]
  double *next_row() const { return capacity > 0 ? d_rows.p + (size_t)rows * stride : nullptr; }
};

// Per-case lag correlations of one handle (pstat_corr.hip).
struct pstat_corr : ColumnTotals {
  CorrArgs args{};
};

// Per-case gyration tensor and form factor of one handle (pstat_shape.hip).
struct pstat_shape : ColumnTotals {
  ShapeArgs args{};
  DeviceDoubles d_q;                // [nq][3]: the wave-vectors
};

// Per-case pair distances of one handle (pstat_pdist.hip).
struct pstat_pdist : ColumnTotals {
  PdistArgs args{};
  DeviceDoubles d_tab;              // [nq] the magnitudes, then [ncases] nbins / rmax (the latter only with nbins > 0)
};

// Per-case energy breakdown of one handle (pstat_energy.hip).
struct pstat_energy : ColumnTotals {
  EnergyArgs args{};
  DeviceDoubles d_cut;              // [ncases] the radius in monomer lengths (only with a `within` column)
};

namespace {

// energies whose every step needs all n(n-1)/2 pairs: one chain per wavefront
bool all_pairs(int energy_type) { return energy_type == PSTAT_INTERACTING || energy_type == PSTAT_CUTOFF; }
// homes that run one chain per lane in chain blocks from the job queue; the others run one chain per wavefront
bool chain_per_lane(Home home) {
  return home == SweepLds || home == SweepMem || home == ClusterLds || home == ClusterMem || home == Planar;
}

// The kernel family that runs the steps of a handle of `ncases` x `chains_per_case` chains of n monomers.
Home choose_home(const LaunchCfg &cfg, int64_t n, int64_t chains_per_case, int64_t ncases, const Overrides &ov) {
  if (cfg.planar) return Planar;   // the planar main has one kernel family (pstat_planar.hip)
  const bool cluster = cfg.move_set == PSTAT_MOVES_CLUSTER;
  if (all_pairs(cfg.energy_type)) return cluster ? ClusterAllPairs : Interacting;
  const int64_t total = chains_per_case * ncases;
  // The chain-per-wavefront kernel covers the f64 / MWC64X clustering main up to n = 256.  It is chosen for (measured at
  // n = 100 on the (E0, kT) grid of run/K1_E0-kT-phase.jl, tools/time_cluster_cw.py -> profiles/r04/experiments/time_cluster_cw.txt):
  // one wave per chain costs the chip ~0.85 ns per chain-step whatever the clusters do (2 730 chains: 3.1 us per step, 43 680:
  // 36 us).  The chain-per-lane kernel steps a whole ensemble in 4.5-5.5 us while its waves fit the chip once and every chain
  // is disordered, but a wave runs at the pace of its longest cluster (25-33 us per step on an aligned chain) and a launch at
  // the pace of its slowest wave: the same grids take it 29-45 us per step at 1 to 16 chains per case.  So: every ensemble of
  // up to 4 096 chains, and sweeps of many small cases (<= 16 chains each) up to 49 152 chains; large ensembles of few cases
  // keep the chain-per-lane kernels, whose full waves are 10 x cheaper per chain-step there.  (PSTAT_PACK: a test or
  // experiment about the block layout is about the chain-per-lane kernels.)
  if (cluster && cfg.precision == PSTAT_F64 && cfg.rng == PSTAT_RNG_MWC64X && n >= 1 && n <= 256) {
    if (ov.f64_state == 'w') return ClusterChainWave;
    if (ov.f64_state != 'l' && ov.f64_state != 'g' && ov.pack < 0 &&
        (total <= 4096 || (ncases >= 8 && chains_per_case <= 16 && total <= (n <= 128 ? 49152 : 24576))))
      return ClusterChainWave;
  }
  bool mem = false;   // the chain-per-lane kernel keeps its state in DevState::work instead of LDS
  if (cluster && cfg.precision == PSTAT_F32) {
    // The f32 clustering main has the in-memory kernel too (20-byte cells, pstat_cluster_gm.hip).  Its LDS kernel is the
    // faster one while the ensemble is resident or nearly so (measured, 65 536 chains: n <= 80 2.2-2.5e10 proposals/s
    // against 1.8-2.4e10; n = 100 a tie; the 546 x 64-chain n = 200 phase scan 1.88 s against 2.18 s); an ensemble of more
    // than twice what LDS seats (160 KiB / 8 n chains per CU) runs in memory (n = 200, 65 536 chains: 1.5e10 against 7.7e9).
    const int64_t seats = (160 * 1024 / (8 * (n > 0 ? n : 1))) * 256;
    mem = ov.f32_state != 'l' && (ov.f32_state == 'g' || total > 2 * seats);
  } else if (cfg.precision == PSTAT_F64) {
    // f64 cells are 16 bytes: LDS seats 160 KiB / (16 n) chains per CU.  Once that is fewer than four full waves (n > 40)
    // the non-interacting f64 sweep keeps its cells in global memory instead and runs 64 lanes on every SIMD (run_segment,
    // ST = 2).  The clustering main's kernel in memory carries the trigonometric cache and is faster at every chain length
    // (measured n = 10 / 20 / 40: 1.5e10 / 1.4e10 / 1.3e10 proposals/s against 1.0e10 with the cells in LDS).
    mem = ov.f64_state != 'l' && (ov.f64_state == 'g' || cluster || n * 16 * 256 > 160 * 1024);
  }
  if (cluster) return mem ? ClusterMem : ClusterLds;
  return mem ? SweepMem : SweepLds;
}

int alloc(pstat_handle *h, void **p, size_t bytes) {
  hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess) return fail(PSTAT_ERR_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
  h->bufs.push_back({*p, bytes});
  return PSTAT_OK;
}

int validate(const pstat_params *c, int ncases) {
  if (ncases < 1) return fail(PSTAT_ERR_INVALID_ARG, "ncases must be >= 1");
  const pstat_params &b = c[0];
  if (b.n < 1) return fail(PSTAT_ERR_INVALID_ARG, "num-monomers must be >= 1");
  if (b.n > 0x7fffffff / 64) return fail(PSTAT_ERR_INVALID_ARG, "num-monomers too large");
  if (b.num_chains < 1) return fail(PSTAT_ERR_INVALID_ARG, "num-chains must be >= 1");
  if (b.chain_type != PSTAT_DIELECTRIC && b.chain_type != PSTAT_POLAR)
    return fail(PSTAT_ERR_INVALID_ARG, "chain-type is not understood.");       // eap_chain.jl:86
  if (b.energy_type < PSTAT_NONINTERACTING || b.energy_type > PSTAT_CUTOFF)
    return fail(PSTAT_ERR_INVALID_ARG, "energy-type is not understood.");      // eap_chain.jl:104
  if (b.energy_type == PSTAT_CUTOFF && b.move_set != PSTAT_MOVES_CLUSTER)
    return fail(PSTAT_ERR_INVALID_ARG, "energy-type 'cutoff' belongs to the clustering main (mcmc_eap_chain.jl has "
                "no --cutoff-radius)");
  if (all_pairs(b.energy_type) && b.n > 512)
    return fail(PSTAT_ERR_UNSUPPORTED, "the all-pairs energies run one chain per 64-lane wavefront with up to 8 "
                "monomers per lane: num-monomers must be <= 512, got %lld", (long long)b.n);
  if (b.precision != PSTAT_F32 && b.precision != PSTAT_F64 && b.precision != PSTAT_Q16)
    return fail(PSTAT_ERR_INVALID_ARG, "precision must be PSTAT_F32, PSTAT_F64 or PSTAT_Q16");
  if (b.precision == PSTAT_Q16 && all_pairs(b.energy_type))
    return fail(PSTAT_ERR_UNSUPPORTED, "the lattice state (PSTAT_Q16) is not implemented for energy-type 'interacting'");
  if (b.rng != PSTAT_RNG_MWC64X && b.rng != PSTAT_RNG_XOSHIRO128PP)
    return fail(PSTAT_ERR_INVALID_ARG, "rng must be PSTAT_RNG_MWC64X or PSTAT_RNG_XOSHIRO128PP");
  if (b.uniform_bits != 0 && b.uniform_bits != 23 && b.uniform_bits != 53)
    return fail(PSTAT_ERR_INVALID_ARG, "uniform_bits must be 0 (the precision's default), 23 or 53");
  if (b.uniform_bits == 53 && b.precision != PSTAT_F64)
    return fail(PSTAT_ERR_INVALID_ARG, "uniform_bits = 53 needs PSTAT_F64: the f32 / q16 arithmetic compares eps in a 24-bit mantissa");
  if (b.rng == PSTAT_RNG_MWC64X)
    for (int i = 0; i < ncases; ++i)
      if (c[i].chain_id0 > PSTAT_MWC64X_MAX_CHAINS || (uint64_t)b.num_chains > PSTAT_MWC64X_MAX_CHAINS - c[i].chain_id0)
        return fail(PSTAT_ERR_INVALID_ARG, "MWC64X streams are disjoint only for global chain ids < 2^22 (chain k starts "
                    "k * 2^40 outputs down one sequence of period ~2^63): chain_id0 + num_chains = %llu + %lld exceeds "
                    "that (case %d); use PSTAT_RNG_XOSHIRO128PP for larger ids",
                    (unsigned long long)c[i].chain_id0, (long long)b.num_chains, i);
  if (b.move_set != PSTAT_MOVES_SINGLE && b.move_set != PSTAT_MOVES_CLUSTER)
    return fail(PSTAT_ERR_INVALID_ARG, "move_set must be PSTAT_MOVES_SINGLE or PSTAT_MOVES_CLUSTER");
  if (b.move_set == PSTAT_MOVES_CLUSTER) {
    if (b.do_flips) return fail(PSTAT_ERR_INVALID_ARG, "mcmc_clustering_eap_chain.jl has no --do-flips");
    if (b.n < 2) return fail(PSTAT_ERR_INVALID_ARG, "cluster moves need num-monomers >= 2 (the mean bond angle)");
  }
  if (b.use_x0 != 0 && b.use_x0 != 1) return fail(PSTAT_ERR_INVALID_ARG, "use_x0 must be 0 or 1");
  if (b.use_x0 && (!std::isfinite(b.x0_phi) || !std::isfinite(b.x0_theta) || !std::isfinite(b.dx0_phi) ||
                   !std::isfinite(b.dx0_theta)))
    return fail(PSTAT_ERR_INVALID_ARG, "non-finite x0 / dx0");
  if (!(b.phi_step > 0) || !(b.theta_step > 0))
    return fail(PSTAT_ERR_INVALID_ARG, "phi-step and theta-step must be > 0");
  if (!(b.adj_scale > 0)) return fail(PSTAT_ERR_INVALID_ARG, "step-adjust-scale must be > 0");
  for (int i = 0; i < ncases; ++i) {
    const pstat_params &p = c[i];
    if (!(p.kT > 0)) return fail(PSTAT_ERR_INVALID_ARG, "kT must be > 0 (case %d)", i);
    if (!std::isfinite(p.E0) || !std::isfinite(p.K1) || !std::isfinite(p.K2) || !std::isfinite(p.mu) ||
        !std::isfinite(p.Fz) || !std::isfinite(p.Fx) || !std::isfinite(p.b) || !std::isfinite(p.bend_mod) ||
        !std::isfinite(p.bend_angle))
      return fail(PSTAT_ERR_INVALID_ARG, "non-finite physics parameter (case %d)", i);
    if (b.energy_type == PSTAT_CUTOFF && !(p.cutoff_radius > 0.0))
      return fail(PSTAT_ERR_INVALID_ARG, "cutoff-radius must be > 0 (case %d)", i);
    if (!(p.cluster_prob >= 0.0 && p.cluster_prob <= 1.0) && b.move_set == PSTAT_MOVES_CLUSTER)
      return fail(PSTAT_ERR_INVALID_ARG, "cluster-prob must be in [0, 1] (case %d)", i);
    if (b.move_set == PSTAT_MOVES_SINGLE && p.bend_mod != 0.0)
      return fail(PSTAT_ERR_INVALID_ARG, "bend-mod belongs to the clustering main (move_set = PSTAT_MOVES_CLUSTER)");
    if (p.n != b.n || p.num_chains != b.num_chains || p.chain_type != b.chain_type ||
        p.energy_type != b.energy_type || p.do_flips != b.do_flips || p.umbrella != b.umbrella ||
        p.precision != b.precision || p.device != b.device || p.rng != b.rng || p.phi_step != b.phi_step ||
        p.theta_step != b.theta_step || p.adj_lb != b.adj_lb || p.adj_ub != b.adj_ub ||
        p.adj_scale != b.adj_scale || p.steps_per_adjust != b.steps_per_adjust || p.move_set != b.move_set ||
        p.use_x0 != b.use_x0 || p.x0_phi != b.x0_phi || p.x0_theta != b.x0_theta || p.dx0_phi != b.dx0_phi ||
        p.dx0_theta != b.dx0_theta || p.uniform_bits != b.uniform_bits)
      return fail(PSTAT_ERR_INVALID_ARG, "case %d differs from case 0 in a non-physics field", i);
  }
  return PSTAT_OK;
}

// ---- the handle's step kernel: resolved once, probed and launched here
// bytes of one monomer's cell in LDS: (theta, phi), or phi alone for the planar main (f64 only)
int cell_bytes(Home home, int precision) {
  if (home == Planar) return 8;
  return precision == PSTAT_F64 ? 16 : (precision == PSTAT_Q16 ? 4 : 8);
}

// the most lanes (64, 32, 16, 8) whose chains of n cells fit a CU's LDS; 0: not even 8
int choose_lanes(Home home, int precision, int64_t n) {
  for (int lanes = 64; lanes >= 8; lanes >>= 1)
    if (n * cell_bytes(home, precision) * lanes <= kLdsBudget) return lanes;
  return 0;
}

// dynamic LDS of a workgroup of a.lanes chains
int lds_bytes(Home home, int precision, const SweepArgs &a) {
  if (home == SweepMem) return (a.lds_rows + 1) * 64 * 16;   // + the trash row
  if (home == SweepLds || home == ClusterLds || home == Planar) return (int)(a.n * a.lanes * cell_bytes(home, precision));
  return 0;
}

// pstat_create_planar's reading of pstat_params (include/pstat.h, next to its declaration)
int validate_planar(const pstat_params *c, int ncases) {
  if (ncases < 1) return fail(PSTAT_ERR_INVALID_ARG, "ncases must be >= 1");
  const pstat_params &b = c[0];
  pstat_params d;
  pstat_default_params(&d);
  if (b.n < 1) return fail(PSTAT_ERR_INVALID_ARG, "num-monomers must be >= 1");
  if (b.n > 0x7fffffff / 64) return fail(PSTAT_ERR_INVALID_ARG, "num-monomers too large");
  if (b.num_chains < 1) return fail(PSTAT_ERR_INVALID_ARG, "num-chains must be >= 1");
  if (b.chain_type != PSTAT_DIELECTRIC && b.chain_type != PSTAT_POLAR)
    return fail(PSTAT_ERR_INVALID_ARG, "chain-type is not understood.");       // 2D/inc/eap_chain.jl:74
  if (b.energy_type == PSTAT_CUTOFF)
    return fail(PSTAT_ERR_INVALID_ARG, "energy_type: the planar main has no energy-type 'cutoff' (2D/inc/eap_chain.jl:81-89)");
  if (b.energy_type < PSTAT_NONINTERACTING || b.energy_type > PSTAT_CUTOFF)
    return fail(PSTAT_ERR_INVALID_ARG, "energy-type is not understood.");      // 2D/inc/eap_chain.jl:88
  if (b.precision != PSTAT_F32 && b.precision != PSTAT_F64 && b.precision != PSTAT_Q16)
    return fail(PSTAT_ERR_INVALID_ARG, "precision must be PSTAT_F32, PSTAT_F64 or PSTAT_Q16");
  // options the planar main does not have: anything but the default is a mistake of the caller's
  if (b.do_flips != d.do_flips) return fail(PSTAT_ERR_INVALID_ARG, "do_flips: 2D/mcmc_clustering_eap_chain.jl has no --do-flips");
  if (b.bend_mod != d.bend_mod) return fail(PSTAT_ERR_INVALID_ARG, "bend_mod: 2D/mcmc_clustering_eap_chain.jl has no --bend-mod");
  if (b.bend_angle != d.bend_angle)
    return fail(PSTAT_ERR_INVALID_ARG, "bend_angle: 2D/mcmc_clustering_eap_chain.jl has no --bend-angle");
  if (b.use_x0 != d.use_x0) return fail(PSTAT_ERR_INVALID_ARG, "use_x0: 2D/mcmc_clustering_eap_chain.jl has no --x0");
  if (b.rng != PSTAT_RNG_MWC64X && b.rng != PSTAT_RNG_XOSHIRO128PP)
    return fail(PSTAT_ERR_INVALID_ARG, "rng must be PSTAT_RNG_MWC64X or PSTAT_RNG_XOSHIRO128PP");
  if (b.uniform_bits != 0 && b.uniform_bits != 23 && b.uniform_bits != 53)
    return fail(PSTAT_ERR_INVALID_ARG, "uniform_bits must be 0 (the precision's default), 23 or 53");
  if (b.rng == PSTAT_RNG_MWC64X)
    for (int i = 0; i < ncases; ++i)
      if (c[i].chain_id0 > PSTAT_MWC64X_MAX_CHAINS || (uint64_t)b.num_chains > PSTAT_MWC64X_MAX_CHAINS - c[i].chain_id0)
        return fail(PSTAT_ERR_INVALID_ARG, "MWC64X streams are disjoint only for global chain ids < 2^22: chain_id0 + "
                    "num_chains = %llu + %lld exceeds that (case %d); use PSTAT_RNG_XOSHIRO128PP for larger ids",
                    (unsigned long long)c[i].chain_id0, (long long)b.num_chains, i);
  if (!(b.phi_step > 0)) return fail(PSTAT_ERR_INVALID_ARG, "phi-step must be > 0");
  if (!(b.adj_scale > 0)) return fail(PSTAT_ERR_INVALID_ARG, "step-adjust-scale must be > 0");
  for (int i = 0; i < ncases; ++i) {
    const pstat_params &p = c[i];
    if (!(p.kT > 0)) return fail(PSTAT_ERR_INVALID_ARG, "kT must be > 0 (case %d)", i);
    if (!std::isfinite(p.E0) || !std::isfinite(p.K1) || !std::isfinite(p.K2) || !std::isfinite(p.mu) ||
        !std::isfinite(p.Fz) || !std::isfinite(p.Fx) || !std::isfinite(p.b))
      return fail(PSTAT_ERR_INVALID_ARG, "non-finite physics parameter (case %d)", i);
    if (!(p.cluster_prob >= 0.0 && p.cluster_prob <= 1.0))
      return fail(PSTAT_ERR_INVALID_ARG, "cluster-prob must be in [0, 1] (case %d)", i);
    if (p.n != b.n || p.num_chains != b.num_chains || p.chain_type != b.chain_type || p.energy_type != b.energy_type ||
        p.do_flips != b.do_flips || p.umbrella != b.umbrella || p.precision != b.precision || p.device != b.device ||
        p.rng != b.rng || p.phi_step != b.phi_step || p.adj_lb != b.adj_lb || p.adj_ub != b.adj_ub ||
        p.adj_scale != b.adj_scale || p.steps_per_adjust != b.steps_per_adjust || p.use_x0 != b.use_x0 ||
        p.bend_mod != b.bend_mod || p.bend_angle != b.bend_angle || p.uniform_bits != b.uniform_bits)
      return fail(PSTAT_ERR_INVALID_ARG, "case %d differs from case 0 in a non-physics field", i);
  }
  // valid options of the reference that the device path lacks
  if (b.precision != PSTAT_F64)
    return fail(PSTAT_ERR_UNSUPPORTED, "the planar main runs in PSTAT_F64 only (no f32 / q16 planar state)");
  if (b.energy_type == PSTAT_INTERACTING)
    return fail(PSTAT_ERR_UNSUPPORTED, "energy-type 'interacting' (all pairs) is not implemented for the planar main");
  if (choose_lanes(Planar, b.precision, b.n) == 0)
    return fail(PSTAT_ERR_UNSUPPORTED, "num-monomers = %lld: a planar chain's 8-byte cells must fit the 160 KiB LDS of a CU "
                "eight chains at a time, num-monomers <= %d", (long long)b.n, kLdsBudget / (8 * 8));
  return PSTAT_OK;
}

// queue layout: [0] error flag (sticky: never cleared by a launch), [1] job counter, [2 ..] per-block "segments done"
size_t queue_ints(const SweepArgs &a) { return 2 + (size_t)a.nblocks; }

// The kernel that runs cfg's steps, ready to launch with any LDS size the handle can ask for.
int resolve_kernel(const LaunchCfg &cfg, int64_t n, StepKernel *out) {
  static StepKernel (*const of_home[])(const LaunchCfg &, int64_t) = {   // indexed by Home
      sweep_step_kernel, sweep_step_kernel, cluster_step_kernel, cluster_gm_step_kernel,
      cluster_cw_step_kernel, cluster_wave_step_kernel, interacting_step_kernel, planar_step_kernel};
  static_assert(sizeof of_home / sizeof *of_home == Planar + 1, "one resolver per Home");
  *out = of_home[cfg.home](cfg, n);
  if (cfg.home == SweepLds || cfg.home == SweepMem || cfg.home == ClusterLds || cfg.home == Planar)
    HIP_TRY(hipFuncSetAttribute(out->fn, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBudget));
  return PSTAT_OK;
}

// The sweep's instantiation depends on cfg.lag: whoever changes a handle's lag does it here.
int set_lag(pstat_handle *h, int lag) {
  h->cfg.lag = lag;
  return resolve_kernel(h->cfg, h->base.n, &h->kernel);
}

// resident workgroups per CU of kernel k with `lds` bytes of dynamic LDS
hipError_t occupancy(const StepKernel &k, int lds, int *blocks_per_cu) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, k.fn, 64, lds);
}

// ---- launch shape of the chain-per-lane kernels: active lanes per workgroup (one wave) and what a workgroup holds.
// `shape` prices the best lane count (at most a.lanes) of one block layout with the makespan model of the home's kernel
// family; packed blocks (run_job_queue<true>: a block holds `lanes` consecutive global chains, whichever cases they belong
// to) are taken when they shorten the launch by more than 5 % -- an ensemble of 2 730 cases x 16 chains is 683 full
// waves instead of 2 730 quarter-filled ones: measured 2.3 x (non-interacting) and 2.5 x (Ising) on the f64 sweep.
// Otherwise blocks stay inside a case and its scalars in SGPRs.
// The clustering main packs into waves no larger than a case's own chains would fill (16 lanes for cases of up to 16
// chains) unless the unpacked launch is at least four rounds of the resident slots deep.  Its step time is not
// uniform: a wave runs at the pace of its longest cluster, and across a phase grid that is 4.5 us per step for a
// disordered chain against 25-33 us for an aligned one (n = 100, tools/phase_latency.py).  A sweep that mixes them is
// paced by the sequential step time of its cold cases, not by throughput, and there a 64-lane wave of four cases is a
// little slower than four 16-lane waves (run/K1_E0-kT-phase.jl's grid, 2 730 x 16 chains, 3e5 steps: 11.5 s unpacked,
// 13.0 s packed four to a wave), while filling the idle lanes of a 16-lane wave with further cases is a gain throughout
// (2 730 x 5 chains: 1 012 -> 865 ms per 2e4 steps on the whole grid, 747 -> 353 on its cold part; 5 760 x 1 chain:
// 1.6-2.4 x); only when workgroups queue several deep does the throughput of full waves win (all-cold 2 730 x 16:
// 676 -> 366 ms per 1e4 steps).  profiles/r04/experiments/time_packed*.txt, twin.txt.
struct Shape { int lanes; int64_t nblocks; double cost; };

// (k: the kernel of cfg, whose `packed` names the layout)
Shape shape(const StepKernel &k, const LaunchCfg &cfg, const SweepArgs &a, const bool deep, const int cus, const int force_lanes) {
  const bool packed = cfg.packed != 0;
  const int lanes = a.lanes;
  const int64_t per_case = a.chains_per_case, total = per_case * a.ncases;
  auto wgs_of = [&](const int cand) -> int64_t {
    return packed ? (total + cand - 1) / cand : a.ncases * ((per_case + cand - 1) / cand);
  };
  Shape best{lanes, wgs_of(lanes), 1e300};
  if (cfg.home == SweepMem) {   // f64 sweep with its cells in memory: 64 lanes on every SIMD
    int bpc = 0;
    if (occupancy(k, lds_bytes(cfg.home, cfg.precision, a), &bpc) != hipSuccess || bpc < 1) bpc = 4;
    double cost = (double)best.nblocks / ((double)bpc * cus);
    best.cost = cost < 1.0 ? 1.0 : cost;
    return best;
  }
  if (cfg.home == ClusterMem) {
    // Chains in device memory: nothing limits a wave to fewer than 64 lanes, but an ensemble of fewer waves than the
    // chip has SIMDs (a phase scan: 546 grid points x 64 chains) runs faster as more, emptier waves -- they fill the
    // idle SIMDs, and a wave's step lasts as long as its LONGEST cluster, which grows like the logarithm of its lanes.
    int bpc = 0;
    if (occupancy(k, 0, &bpc) != hipSuccess || bpc < 1) bpc = 1;
    const double slots = (double)bpc * cus;
    // (packed, and the unpacked launch not many rounds deep: no wave larger than a case's chains rounded up to 16 / 32 / 64
    // -- the clustering main's packing rule, above)
    int cmax = 64;
    if (packed && !deep) cmax = per_case <= 16 ? 16 : (per_case <= 32 ? 32 : 64);
    for (int cand = cmax; cand >= 16; cand >>= 1) {
      if (force_lanes >= 1 && force_lanes <= 64 && cand != force_lanes) continue;
      double cost = (double)wgs_of(cand) / slots;
      if (cost < 1.0) cost = 1.0;
      cost *= 1.0 + 0.1 * std::log2(cand / 16.0);
      if (cost < best.cost) best = Shape{cand, wgs_of(cand), cost};
    }
    return best;
  }
  // State in LDS: a CU holds at most 160 KiB / (bytes per chain) chains; pick the lane count that minimises the
  // makespan max(1, workgroups / resident slots) of one launch -- e.g. f32, n = 100: 51 lanes x 4 workgroups per CU
  // (204 chains, all four SIMDs) instead of 64 x 3 (192 chains, three SIMDs).
  int bpc0 = 0;
  const bool lds_starved =      // full waves: fewer than one per SIMD fit a CU's LDS
      occupancy(k, lds_bytes(cfg.home, cfg.precision, a), &bpc0) == hipSuccess && bpc0 < 4;
  for (int cand = lanes; cand >= 8; --cand) {
    if (force_lanes >= 1 && force_lanes <= lanes && cand != force_lanes) continue;
    SweepArgs probe = a;
    probe.lanes = cand;
    int bpc = 0;
    if (occupancy(k, lds_bytes(cfg.home, cfg.precision, probe), &bpc) != hipSuccess || bpc < 1) continue;
    const double slots = (double)bpc * cus;
    double cost = (double)wgs_of(cand) / slots;
    if (cost < 1.0) cost = 1.0;
    cost *= 1.0 + 1e-4 * (64 - cand);   // ties: prefer fuller waves
    if (cfg.home == ClusterLds && lds_starved) {
      // (only when LDS seats fewer than four FULL waves per CU.)  The cluster step runs a wave for as long as its
      // LONGEST cluster, so a wave of fewer lanes finishes its steps sooner (~ log of the lane count), and more,
      // emptier waves also put the idle SIMDs to work.  Measured, n = 100, f64 (LDS seats 102 chains per CU): 4 x 25 lanes
      // 4.08e9 proposals/s against 2 x 51 lanes 3.61e9 (non-interacting; Ising 5.70e9 / 5.57e9).  Sharing a SIMD
      // between waves costs more than it gains here (f32: 4 x 51 lanes 1.77e10, 8 x 25 lanes 1.52e10).
      const double waves_per_simd = bpc / 4.0;
      cost *= 1.0 + 0.1 * std::log2(cand / 16.0);
      if (waves_per_simd > 1.0) cost *= 1.0 + 0.25 * (waves_per_simd - 1.0);
    }
    if (cost < best.cost) best = Shape{cand, wgs_of(cand), cost};
  }
  return best;
}

// Splits a launch of `nsteps` steps into time segments so that blocks*segments fills the resident
// workgroup slots evenly (see sweep_kernel).  Returns segments per block.
int choose_segments(int64_t blocks, int64_t slots, int64_t nsteps, int64_t min_seg) {
  if (blocks <= slots || nsteps < 2 * min_seg) return 1;
  int best = 1;
  double best_eff = 0;
  for (int s = 1; s <= 12; ++s) {
    if (nsteps / s < min_seg) break;              // keep fill/spill amortised
    const double jobs = (double)blocks * s;
    const double eff = jobs / (std::ceil(jobs / slots) * slots);   // busy fraction of the slots
    if (eff > best_eff + 0.02) { best_eff = eff; best = s; }
  }
  return best;
}

// Launches the handle's step kernel for `nsteps` steps from step `step0` of the current init (nsteps = 0: the all-pairs
// kernels derive r, p, U from fresh angles; reinit_mode 1 | 2: home Interacting re-initialises, 2 = forced).  A chain-per-lane
// launch is split into time segments of its job queue.
hipError_t launch_steps(pstat_handle *h, int64_t step0, int64_t nsteps, int reinit_mode = 0) {
  SweepArgs &A = h->args;
  A.nsteps = nsteps;
  A.step0 = step0;
  unsigned grid = 0;
  if (chain_per_lane(h->cfg.home)) {
    const int64_t blocks = A.nblocks;
    // (a fill + spill of the f64 cluster kernel's working buffer costs about ten of its steps, the LDS kernels' a few
    // hundred of theirs)
    int nseg = h->ov.segments ? h->ov.segments : choose_segments(blocks, h->slots, nsteps, h->cfg.home == ClusterMem ? 400 : 2000);
    // f32/q16 running totals are re-derived from the angles at every segment start: bound the stretch
    // over which their rounding errors can random-walk
    if (h->base.precision != PSTAT_F64 && !h->ov.segments) {
      const int64_t need = (nsteps + 32767) / 32768;
      if (need > nseg) nseg = (int)(need < 0x3fffffffLL ? need : 0x3fffffffLL);
    }
    if (nseg > nsteps) nseg = nsteps > 1 ? (int)nsteps : 1;
    if (blocks * nseg > 0x3fffffffLL) nseg = 1;
    A.nseg = nseg;
    A.seg_len = (nsteps + nseg - 1) / nseg;
    // A job waits at most for one segment of its predecessor.  Bound the wait by a generous multiple of the
    // longest plausible segment (a spin sleeps ~2 us; a step of the cluster kernel on a long, aligned chain
    // can take tens of us), so that a long launch is never mistaken for a lost predecessor.
    const int64_t want = (1ll << 22) + A.seg_len * 256;
    A.max_spins = h->ov.max_spins ? h->ov.max_spins : (int32_t)(want < 0x7fffffffLL ? want : 0x7fffffffLL);
    // Segments of one block run one after the other, so at most `blocks` jobs are runnable at any time:
    // more workgroups than that would only sit in the predecessor wait -- and, worse, leave the working
    // ones unevenly spread over the SIMDs.
    grid = (unsigned)(blocks < h->slots ? blocks : h->slots);
    hipError_t e = hipMemsetAsync(h->d_queue + 1, 0, sizeof(int) * (queue_ints(A) - 1), h->stream);   // [0]: the sticky error word
    if (e != hipSuccess) return e;
  } else {
    grid = (unsigned)h->S.C;
  }
  // the kernel's arguments: (SweepArgs, DevState, cases) and the family's scalars (StepKernel, pstat_device.h)
  const LaunchCfg &cfg = h->cfg;
  SweepRare rare{cfg.do_flips, cfg.lag, cfg.umbrella};
  int umbrella = cfg.umbrella, cutoff = cfg.energy_type == PSTAT_CUTOFF ? 1 : 0;
  int do_flips = cfg.do_flips, lag = (cfg.lag || reinit_mode) ? 1 : 0;
  void *argv[6] = {&A, &h->S, &h->d_cases};
  switch (cfg.home) {
    case SweepLds: case SweepMem: argv[3] = &rare; argv[4] = &h->d_queue; break;
    case ClusterLds: case ClusterMem: case Planar: argv[3] = &umbrella; argv[4] = &h->d_queue; break;
    case ClusterChainWave: argv[3] = &umbrella; break;
    case ClusterAllPairs: argv[3] = &umbrella; argv[4] = &cutoff; break;
    case Interacting: argv[3] = &do_flips; argv[4] = &lag; argv[5] = &reinit_mode; break;
  }
  return hipLaunchKernel(h->kernel.fn, dim3(grid), dim3(64), argv, lds_bytes(cfg.home, cfg.precision, A), h->stream);
}

int set_device(pstat_handle *h) {
  HIP_TRY(hipSetDevice(h->device));
  return PSTAT_OK;
}

int report_failed_job(pstat_handle *h) {
  int q[10] = {0};
  (void)hipMemcpy(q, h->d_queue, sizeof q, hipMemcpyDeviceToHost);
  return fail(PSTAT_ERR_HIP, "a persistent launch did not complete: job %d waited too long for its predecessor "
              "(queue head %d, done[0..7] = %d %d %d %d %d %d %d %d); the handle's averages are not those of the "
              "steps asked for", h->failed_job - 1, q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], q[9]);
}

// Waits for the handle's stream and then looks at the error word of the persistent kernels' job queue
// (run_job_queue, pstat_device.h).  The word is never cleared by a launch and the failure is sticky on
// the handle: every entry point that hands results to the caller goes through here.
int sync_checked(pstat_handle *h) {
  if (h->failed_job) return report_failed_job(h);
  int flag = 0;
  HIP_TRY(hipMemcpyAsync(&flag, h->d_queue, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (flag) {
    h->failed_job = flag;
    return report_failed_job(h);
  }
  return PSTAT_OK;
}

// `nsteps` steps of every chain, in launches of at most 2^30 (per-launch step counters are 32-bit)
int enqueue_steps(pstat_handle *h, int64_t nsteps) {
  const int64_t max_launch = 1ll << 30;
  while (nsteps > 0) {
    const int64_t len = nsteps < max_launch ? nsteps : max_launch;
    HIP_TRY(launch_steps(h, h->step_in_init, len));
    h->step_in_init += len;
    h->steps_recorded += len;
    nsteps -= len;
  }
  return PSTAT_OK;
}

// ---- the recorder lifecycle: the rules every kind of recorder object follows, each stated here once

template <class T>
bool owns(const OpenList<T> &list, const T *p) {
  for (const auto &mine : list)
    if (mine.get() == p) return true;
  return false;
}

// What every entry point that takes an object tests first: the arguments (`others`: its further pointers that must not be
// null), then that `p` is one of the handle's open objects; `not_open` is the kind's message.  Touches no device.
template <class T>
int check_open(pstat_handle *h, OpenList<T> pstat_handle::*list, const T *p, bool others, const char *not_open) {
  if (!h || !p || !others) return fail(PSTAT_ERR_INVALID_ARG, "null argument");
  if (!owns(h->*list, p)) return fail(PSTAT_ERR_INVALID_ARG, "%s", not_open);
  return PSTAT_OK;
}

int open_series(pstat_handle *h, const pstat_series *s, bool others = true) {
  return check_open(h, &pstat_handle::series, s, others, "the series is not an open series of this handle");
}
int open_tempering(pstat_handle *h, const pstat_tempering *t) {
  return check_open(h, &pstat_handle::tempering, t, true, "the tempering object is not an open one of this handle");
}
int open_hist(pstat_handle *h, const pstat_hist *g) {
  return check_open(h, &pstat_handle::hists, g, true, "the histogram is not an open histogram of this handle");
}
int open_corr(pstat_handle *h, const pstat_corr *g, bool others = true) {
  return check_open(h, &pstat_handle::corrs, g, others, "the correlation object is not an open one of this handle");
}
int open_shape(pstat_handle *h, const pstat_shape *g, bool others = true) {
  return check_open(h, &pstat_handle::shapes, g, others, "the shape object is not an open one of this handle");
}
int open_pdist(pstat_handle *h, const pstat_pdist *g, bool others = true) {
  return check_open(h, &pstat_handle::pdists, g, others, "the pdist object is not an open one of this handle");
}
int open_energy(pstat_handle *h, const pstat_energy *g, bool others = true) {
  return check_open(h, &pstat_handle::energies, g, others, "the energy object is not an open one of this handle");
}

// The end of every pstat_X_open: the handle takes the finished object and the caller gets its address.
template <class T>
int adopt(OpenList<T> &list, std::unique_ptr<T> &p, T **out) {
  T *const raw = p.get();
  try {
    list.push_back(std::move(p));   // (a push_back that throws leaves p alone, and the caller's return frees the object)
  } catch (const std::bad_alloc &) {
    return fail(PSTAT_ERR_NOMEM, "host allocation failed");
  }
  *out = raw;
  return PSTAT_OK;
}

// Every pstat_X_close: an object that is not one of the handle's open ones is left alone.
template <class T>
void close_object(pstat_handle *h, OpenList<T> pstat_handle::*list, const T *p) {
  if (!h || !p || !owns(h->*list, p)) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);   // a record (row, round) may still be in flight
  OpenList<T> &open = h->*list;
  for (size_t i = 0; i < open.size(); ++i)
    if (open[i].get() == p) { open.erase(open.begin() + (long)i); break; }
}

// Every pstat_advance_X: advance(nsteps) with one record after every `stepout`-th step; the remainder is advanced without
// one.  `capacity` > 0: the object keeps a row per record and has `rows` of them taken; a call that would overflow is refused
// before anything is enqueued.  `record` enqueues one record and returns a status.
template <class Record>
int advance_recording(pstat_handle *h, int64_t nsteps, int64_t stepout, int64_t capacity, int64_t rows, const char *noun,
                      Record record) {
  if (nsteps < 0) return fail(PSTAT_ERR_INVALID_ARG, "nsteps must be >= 0");
  if (stepout < 1) return fail(PSTAT_ERR_INVALID_ARG, "stepout must be >= 1");
  const int64_t nrec = nsteps / stepout;
  if (capacity > 0 && nrec > capacity - rows)
    return fail(PSTAT_ERR_TOO_SMALL, "the %s has %lld of %lld rows free, this call would record %lld", noun,
                (long long)(capacity - rows), (long long)capacity, (long long)nrec);
  PSTAT_TRY(set_device(h));
  if (h->failed_job) return report_failed_job(h);
  for (int64_t i = 0; i < nrec; ++i) {
    PSTAT_TRY(enqueue_steps(h, stepout));
    PSTAT_TRY(record());
  }
  return enqueue_steps(h, nsteps - nrec * stepout);
}

// Checks specs[rows][nspecs] (rows = 1, or the cases of a per-case table) and states them as the device reads them; touches no
// device.  nchannels: channels are 0 .. nchannels - 1 (`what` names that range's owner in the message).
int hist_specs(const pstat_hist_spec *specs, int32_t nspecs, int64_t rows, int64_t nchannels, const char *what,
               std::vector<HistSpec> &dev, int32_t *total_bins) {
  if (nspecs < 1 || nspecs > PSTAT_HIST_MAX_SPECS)
    return fail(PSTAT_ERR_INVALID_ARG, "nspecs must be in 1 .. %d, not %d", PSTAT_HIST_MAX_SPECS, nspecs);
  int64_t total = 0;
  for (int64_t k = 0; k < rows; ++k)
    for (int32_t i = 0; i < nspecs; ++i) {
      const pstat_hist_spec &sp = specs[k * nspecs + i];
      if (sp.channel < 0 || sp.channel >= nchannels)
        return fail(PSTAT_ERR_INVALID_ARG, "spec %d, case %lld: channel %d is outside 0 .. %lld (%s)", i, (long long)k, sp.channel,
                    (long long)nchannels - 1, what);
      if (sp.nbins < 1) return fail(PSTAT_ERR_INVALID_ARG, "spec %d, case %lld: nbins must be >= 1, not %d", i, (long long)k, sp.nbins);
      if (!std::isfinite(sp.lo) || !std::isfinite(sp.hi))
        return fail(PSTAT_ERR_INVALID_ARG, "spec %d, case %lld: lo = %g, hi = %g must be finite", i, (long long)k, sp.lo, sp.hi);
      if (!(sp.hi > sp.lo))
        return fail(PSTAT_ERR_INVALID_ARG, "spec %d, case %lld: hi = %.17g must be above lo = %.17g", i, (long long)k, sp.hi, sp.lo);
      const double inv = (double)sp.nbins / (sp.hi - sp.lo);
      if (!std::isfinite(inv) || !(inv > 0.0))   // t = (x - lo) * inv is then never NaN for a finite x
        return fail(PSTAT_ERR_INVALID_ARG, "spec %d, case %lld: hi - lo = %g leaves no finite positive nbins / (hi - lo) for %d bins",
                    i, (long long)k, sp.hi - sp.lo, sp.nbins);
      if (k > 0 && (sp.channel != specs[i].channel || sp.nbins != specs[i].nbins))
        return fail(PSTAT_ERR_INVALID_ARG, "spec %d, case %lld: channel %d, nbins %d differ from case 0's %d, %d; only lo and hi "
                    "may differ between cases", i, (long long)k, sp.channel, sp.nbins, specs[i].channel, specs[i].nbins);
      if (k == 0) total += sp.nbins;
    }
  if (total > PSTAT_HIST_MAX_BINS)
    return fail(PSTAT_ERR_UNSUPPORTED, "%lld bins per case: at most %d (a workgroup keeps a case's bins in LDS)", (long long)total,
                PSTAT_HIST_MAX_BINS);
  dev.resize((size_t)(rows * nspecs));
  for (int64_t k = 0; k < rows; ++k) {
    int32_t offset = 0;
    for (int32_t i = 0; i < nspecs; ++i) {
      const pstat_hist_spec &sp = specs[k * nspecs + i];
      dev[(size_t)(k * nspecs + i)] = HistSpec{sp.channel, sp.nbins, offset, 0, sp.lo, (double)sp.nbins / (sp.hi - sp.lo)};
      offset += sp.nbins;
    }
  }
  *total_bins = (int32_t)total;
  return PSTAT_OK;
}

// one histogram record, enqueued
int enqueue_hist(pstat_handle *h, pstat_hist *g) {
  const HistArgs a{h->base.num_chains, h->ncases, h->S.C, 1, g->nspecs, g->total_bins, g->per_case, 0};
  HIP_TRY(launch_hist(a, h->S.obs, g->d_specs.p, g->d_counts.p, g->d_counts.p + (size_t)h->ncases * (size_t)g->total_bins, h->stream));
  g->records += 1;
  return PSTAT_OK;
}

// ---- the correlation and the shape recorder: what they do with their ColumnTotals, given the kind's words
struct TotalsText {
  const char *object;     // "the <object> has ... rows free"
  const char *no_room;    // capacity_rows overflows the address space (%lld rows)
  const char *nomem;      // a hipMalloc failed (%zu columns, %lld rows, %s)
  const char *hip;        // another HIP call of the open failed (%s)
};
constexpr TotalsText kCorrText{"correlation object", "%lld rows of correlations do not fit the address space",
                               "correlations of %zu columns, %lld rows: %s", "correlation totals: %s"};
constexpr TotalsText kShapeText{"shape object", "%lld rows of shape columns do not fit the address space",
                                "shape object of %zu columns, %lld rows: %s", "shape totals: %s"};
constexpr TotalsText kPdistText{"pdist object", "%lld rows of pair-distance columns do not fit the address space",
                                "pdist object of %zu columns, %lld rows: %s", "pdist totals: %s"};
constexpr TotalsText kEnergyText{"energy object", "%lld rows of energy columns do not fit the address space",
                                 "energy object of %zu columns, %lld rows: %s", "energy totals: %s"};

// The allocation tail of pstat_corr_open / pstat_shape_open / pstat_pdist_open / pstat_energy_open, after the kind's own argument checks: a new object g with zeroed
// totals of ncols columns per case, `partial` doubles of scratch and capacity_rows kept rows.
template <class T>
int new_totals(pstat_handle *h, int32_t ncols, int64_t capacity_rows, size_t partial, const TotalsText &text, std::unique_ptr<T> &g) {
  const size_t stride = (size_t)h->ncases * (size_t)ncols;
  if (capacity_rows > 0 && (uint64_t)capacity_rows > (SIZE_MAX / sizeof(double)) / stride)
    return fail(PSTAT_ERR_NOMEM, text.no_room, (long long)capacity_rows);
  PSTAT_TRY(set_device(h));
  g.reset(new (std::nothrow) T);
  if (!g) return fail(PSTAT_ERR_NOMEM, "host allocation failed");
  g->stride = stride;
  g->capacity = capacity_rows;
  hipError_t e = g->d_totals.malloc(2 * stride);
  if (e == hipSuccess) e = g->d_partial.malloc(partial);
  if (e == hipSuccess && capacity_rows > 0) e = g->d_rows.malloc((size_t)capacity_rows * stride);
  if (e != hipSuccess) return fail(PSTAT_ERR_NOMEM, text.nomem, stride, (long long)capacity_rows, hipGetErrorString(e));
  e = hipMemsetAsync(g->d_totals.p, 0, 2 * stride * sizeof(double), h->stream);   // ahead of the first record
  if (e != hipSuccess) return fail(PSTAT_ERR_HIP, text.hip, hipGetErrorString(e));
  return PSTAT_OK;
}

// pstat_X_record: one record outside an advance; `enqueue` launches it
template <class Enqueue>
int totals_record(pstat_handle *h, const ColumnTotals *g, const TotalsText &text, Enqueue enqueue) {
  if (g->capacity > 0 && g->rows >= g->capacity)
    return fail(PSTAT_ERR_TOO_SMALL, "the %s has 0 of %lld rows free", text.object, (long long)g->capacity);
  PSTAT_TRY(set_device(h));
  if (h->failed_job) return report_failed_job(h);
  return enqueue();
}

// what a record leaves on the host side once its launch is enqueued; the caller has checked that a row is free
int recorded(ColumnTotals *g) {
  g->records += 1;
  if (g->capacity > 0) g->rows += 1;
  return PSTAT_OK;
}

int totals_read(pstat_handle *h, const ColumnTotals *g, double *sum, double *sumsq, int64_t *records) {
  PSTAT_TRY(set_device(h));
  PSTAT_TRY(sync_checked(h));
  if (sum) HIP_TRY(hipMemcpy(sum, g->d_totals.p, g->stride * sizeof(double), hipMemcpyDeviceToHost));
  if (sumsq) HIP_TRY(hipMemcpy(sumsq, g->d_totals.p + g->stride, g->stride * sizeof(double), hipMemcpyDeviceToHost));
  if (records) *records = g->records;
  return PSTAT_OK;
}

int totals_rows(pstat_handle *h, const ColumnTotals *g, const double **dev_rows, int64_t *nrows, int64_t *stride) {
  PSTAT_TRY(set_device(h));
  PSTAT_TRY(sync_checked(h));
  *dev_rows = g->d_rows.p;
  *nrows = g->rows;
  *stride = (int64_t)g->stride;
  return PSTAT_OK;
}

int totals_clear(pstat_handle *h, ColumnTotals *g) {
  PSTAT_TRY(set_device(h));
  HIP_TRY(hipMemsetAsync(g->d_totals.p, 0, 2 * g->stride * sizeof(double), h->stream));   // behind the records already enqueued
  g->records = 0;
  g->rows = 0;
  return PSTAT_OK;
}

int enqueue_corr(pstat_handle *h, pstat_corr *g) {
  HIP_TRY(launch_corr(g->args, h->S.ang, h->d_cases, g->d_partial.p, g->d_totals.p, g->next_row(), h->stream));
  return recorded(g);
}

int enqueue_shape(pstat_handle *h, pstat_shape *g) {
  HIP_TRY(launch_shape(g->args, h->S.ang, h->d_cases, g->d_q.p, g->d_partial.p, g->d_totals.p, g->next_row(), h->stream));
  return recorded(g);
}

int enqueue_pdist(pstat_handle *h, pstat_pdist *g) {
  const double *q = g->args.nq > 0 ? g->d_tab.p : nullptr;
  const double *inv = g->args.nbins > 0 ? g->d_tab.p + g->args.nq : nullptr;
  HIP_TRY(launch_pdist(g->args, h->S.ang, h->d_cases, q, inv, g->d_partial.p, g->d_totals.p, g->next_row(), h->stream));
  return recorded(g);
}

int enqueue_energy(pstat_handle *h, pstat_energy *g) {
  HIP_TRY(launch_energy(g->args, h->S.ang, h->d_cases, g->d_cut.p, g->d_partial.p, g->d_totals.p, g->next_row(), h->stream));
  return recorded(g);
}

// the blocking transform of x[nbatches][stride] (device) on `stream`, results to host memory; waits for the stream
int blocking_to_host(const double *x, int64_t nbatches, int64_t ncols, int64_t stride, int min_blocks, hipStream_t stream,
                     double *out, double *levels) {
  DeviceDoubles d_out, d_levels;
  PSTAT_TRY(d_out.alloc((size_t)ncols * PSTAT_EB_FIELDS));
  if (levels) PSTAT_TRY(d_levels.alloc((size_t)ncols * PSTAT_BLOCK_LEVELS));
  HIP_TRY(launch_blocking(x, nbatches, ncols, stride, min_blocks, d_out.p, d_levels.p, stream));
  HIP_TRY(hipMemcpyAsync(out, d_out.p, (size_t)ncols * PSTAT_EB_FIELDS * sizeof(double), hipMemcpyDeviceToHost, stream));
  if (levels)
    HIP_TRY(hipMemcpyAsync(levels, d_levels.p, (size_t)ncols * PSTAT_BLOCK_LEVELS * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return PSTAT_OK;
}

int reduce_to_host(pstat_handle *h, int icase, double red[PSTAT_NRED]) {
  int rc = pstat_reduce_device(h, icase, h->d_red);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(red, h->d_red, sizeof(double) * PSTAT_NRED, hipMemcpyDeviceToHost, h->stream));
  return sync_checked(h);
}

}  // namespace

extern "C" {

int pstat_abi_version(void) { return PSTAT_ABI_VERSION; }

const char *pstat_strerror(int status) {
  switch (status) {
    case PSTAT_OK: return "ok";
    case PSTAT_ERR_INVALID_ARG: return "invalid argument";
    case PSTAT_ERR_NO_DEVICE: return "no HIP device";
    case PSTAT_ERR_HIP: return "HIP runtime error";
    case PSTAT_ERR_UNSUPPORTED: return "option not supported on the device path";
    case PSTAT_ERR_NOMEM: return "out of device memory";
    case PSTAT_ERR_BAD_CHECKPOINT: return "checkpoint does not match this handle";
    case PSTAT_ERR_TOO_SMALL: return "buffer too small";
    default: return "unknown status";
  }
}

const char *pstat_last_error(void) { return g_err; }

int pstat_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

void pstat_default_params(pstat_params *p) {
  // mcmc_eap_chain.jl:19-153
  std::memset(p, 0, sizeof *p);
  p->E0 = 0.0; p->K1 = 1.0; p->K2 = 0.0; p->mu = 1e-2; p->kT = 1.0;
  p->Fz = 0.0; p->Fx = 0.0; p->b = 1.0;
  p->phi_step = 3 * M_PI / 8; p->theta_step = 3 * M_PI / 16;
  p->adj_lb = 0.15; p->adj_ub = 0.55; p->adj_scale = 1.1;
  p->steps_per_adjust = 2500;
  p->n = 100;
  p->num_chains = 1;
  p->seed = 0; p->chain_id0 = 0;
  p->chain_type = PSTAT_DIELECTRIC; p->energy_type = PSTAT_NONINTERACTING;
  p->do_flips = 0; p->umbrella = 0;
  p->precision = PSTAT_F64; p->device = 0;   // the reference's Float64 (inc/types.jl); PSTAT_F32 is the opt-in fast path
  p->rng = PSTAT_RNG_MWC64X; p->uniform_bits = 0;   // 0 = the precision's default: 53 random bits in eps for f64, 23 for f32 / q16
  // mcmc_clustering_eap_chain.jl:36-43,87-90,142-148 (only read when move_set = PSTAT_MOVES_CLUSTER / use_x0)
  p->move_set = PSTAT_MOVES_SINGLE;
  p->bend_mod = 0.0; p->bend_angle = 0.0; p->cluster_prob = 0.5;
  p->use_x0 = 0; p->x0_phi = 0.0; p->x0_theta = 0.0; p->dx0_phi = 2 * M_PI; p->dx0_theta = 1e-1;
  p->cutoff_radius = 7.5;
}

// pstat_create and pstat_create_planar: the same handle, allocations and launch shape; `planar` picks the validation,
// the one-angle state and home Planar
static int create_handle(const pstat_params *cases, int32_t ncases, void *stream, pstat_handle **out, const bool planar) {
  if (!cases || !out) return fail(PSTAT_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  int rc = planar ? validate_planar(cases, ncases) : validate(cases, ncases);
  if (rc) return rc;
  int ndev = pstat_device_count();
  if (ndev < 1) return fail(PSTAT_ERR_NO_DEVICE, "no HIP device is visible (this library has no CPU path)");
  if (cases[0].device < 0 || cases[0].device >= ndev)
    return fail(PSTAT_ERR_NO_DEVICE, "device %d out of range (have %d)", cases[0].device, ndev);

  struct Destroy { void operator()(pstat_handle *p) const { pstat_destroy(p); } };
  std::unique_ptr<pstat_handle, Destroy> owner(new (std::nothrow) pstat_handle);   // every early return below destroys it
  pstat_handle *const h = owner.get();
  if (!h) return fail(PSTAT_ERR_NOMEM, "host allocation failed");
  try {   // std::vector growth may throw: nothing propagates through the C ABI
  h->base = cases[0];
  if (planar) {   // what a planar handle ignores is normalised, so that checkpoints of equal runs match
    h->base.theta_step = 0.0;
    h->base.move_set = PSTAT_MOVES_CLUSTER;
  }
  h->ncases = ncases;
  h->device = cases[0].device;
  h->elem = cases[0].precision == PSTAT_F64 ? 8 : (cases[0].precision == PSTAT_Q16 ? 2 : 4);
  for (int i = 0; i < ncases; ++i) {
    const pstat_params &p = cases[i];
    h->cases.push_back({p.E0, p.K1, p.K2, p.mu, p.kT, p.Fz, p.Fx, p.b, p.seed, p.chain_id0,
                        p.bend_mod, p.bend_angle, p.cluster_prob, p.cutoff_radius});
    h->kT0.push_back(p.kT);
  }
  bool any_fx = false;
  for (auto &c : h->cases) any_fx = any_fx || c.Fx != 0.0;
  h->ov = read_overrides();
  h->cfg = {h->base.precision, h->base.chain_type, h->base.energy_type, h->base.do_flips ? 1 : 0,
            h->base.umbrella ? 1 : 0, any_fx ? 1 : 0, 0, h->base.rng, h->base.move_set};
  h->cfg.planar = planar ? 1 : 0;
  const Home home = h->cfg.home = choose_home(h->cfg, h->base.n, h->base.num_chains, ncases, h->ov);

  const int lanes = (home == SweepLds || home == ClusterLds || home == Planar) ? choose_lanes(home, h->base.precision, h->base.n) : 64;
  if (lanes == 0)
    return fail(PSTAT_ERR_UNSUPPORTED, "num-monomers = %lld does not fit the 160 KiB LDS of a CU",
                (long long)cases[0].n);
  SweepArgs &A = h->args;
  A.n = h->base.n;
  A.chains_per_case = h->base.num_chains;
  A.blocks_per_case = (h->base.num_chains + lanes - 1) / lanes;
  A.nblocks = A.blocks_per_case * ncases;
  A.nsteps = 0; A.step0 = 0;
  A.steps_per_adjust = h->base.steps_per_adjust;
  A.adj_lb = h->base.adj_lb; A.adj_ub = h->base.adj_ub; A.adj_scale = h->base.adj_scale;
  A.lanes = lanes;
  A.adaptive = (h->base.adj_scale != 1.0 && h->base.steps_per_adjust > 0) ? 1 : 0;  // mcmc_eap_chain.jl:302
  A.ncases = ncases; A.seg_len = 0; A.nseg = 1; A.max_spins = 1 << 22;
  A.lds_rows = 0; A.packed = 0; A.pad_ = 0;
  A.wide_eps = (h->base.precision == PSTAT_F64 && h->base.uniform_bits != 23) ? 1 : 0;
  if (home == SweepMem) {   // a quarter of a CU's LDS per wave: four resident waves, 64 lanes x 16 B per row
    int rows = 160 * 1024 / 4 / (64 * 16) - 1;   // one row of the quarter is the trash row of run_segment
    if (h->ov.f64_lds_rows >= 0 && h->ov.f64_lds_rows <= rows) rows = h->ov.f64_lds_rows;
    A.lds_rows = (int32_t)(h->base.n < rows ? h->base.n : rows);
  }

  HIP_TRY(hipSetDevice(h->device));
  PSTAT_TRY(resolve_kernel(h->cfg, A.n, &h->kernel));
  hipDeviceProp_t prop;
  if (chain_per_lane(home)) {
    HIP_TRY(hipGetDeviceProperties(&prop, h->device));
    Shape pick = shape(h->kernel, h->cfg, A, false, prop.multiProcessorCount, h->ov.lanes);
    if (ncases > 1) {   // (every chain-per-lane kernel has a packed-cases instantiation)
      LaunchCfg packed = h->cfg;
      packed.packed = 1;
      StepKernel kp;
      PSTAT_TRY(resolve_kernel(packed, A.n, &kp));
      const Shape pk = shape(kp, packed, A, pick.cost >= 4.0 || h->ov.pack == 1, prop.multiProcessorCount, h->ov.lanes);
      if (h->ov.pack >= 0 ? h->ov.pack == 1 : pk.cost < 0.95 * pick.cost) {
        pick = pk;
        h->cfg = packed;
        h->kernel = kp;
        A.packed = 1;
      }
    }
    A.lanes = pick.lanes;
    A.blocks_per_case = (h->base.num_chains + pick.lanes - 1) / pick.lanes;
    A.nblocks = pick.nblocks;
    if (home == ClusterMem && (uint64_t)pick.lanes * (uint64_t)h->base.n * (h->base.precision == PSTAT_F64 ? PSTAT_CLUSTER_GM_CELL : 20u) >= 0x80000000ull)
      return fail(PSTAT_ERR_UNSUPPORTED, "num-monomers = %lld: a wave's working buffer must stay below 2 GiB",
                  (long long)cases[0].n);
  }
  // (checked on the FINAL lane count: the job queue counts blocks and (block, segment) jobs in 32 bits)
  if (A.nblocks > 0x3fffffffLL)
    return fail(PSTAT_ERR_INVALID_ARG, "too many chains for one handle: %lld chain blocks", (long long)A.nblocks);
  if (stream) {
    h->stream = (hipStream_t)stream;
  } else {
    HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->own_stream = true;
  }
  DevState &S = h->S;
  const int64_t C = (int64_t)ncases * h->base.num_chains;
  S.C = C;
  const size_t n = (size_t)h->base.n, Cz = (size_t)C;
  // checkpoint order = allocation order: the image is these buffers
  const struct { void **p; size_t bytes; } state[] = {
      {&S.ang, 2 * n * Cz * h->elem},
      {(void **)&S.rng, 4 * Cz * sizeof(uint32_t)},
      {(void **)&S.stepsz, 2 * Cz * sizeof(double)},
      {(void **)&S.win, 2 * Cz * sizeof(int64_t)},
      {(void **)&S.nacc_total, Cz * sizeof(int64_t)},
      {(void **)&S.obs, NOBS_STATE * Cz * sizeof(double)},
      {(void **)&S.sums, NSUMS * Cz * sizeof(double)},
      {(void **)&S.wnorm, Cz * sizeof(double)},
      {(void **)&S.lag, Cz * sizeof(double)},
      {(void **)&S.uref, Cz * sizeof(double)},
      {(void **)&S.nanrej, Cz * sizeof(int64_t)},
  };
  static_assert(sizeof state / sizeof *state == kStateBuffers, "the checkpoint image is the first kStateBuffers allocations");
  for (const auto &b : state) PSTAT_TRY(alloc(h, b.p, b.bytes));
  PSTAT_TRY(alloc(h, &S.ang_tmp, 2 * n * Cz * h->elem));
  if (home == ClusterMem)    // working copy of the chains, [chain block][lane][n] cells of 40 (f64) / 20 (f32) bytes (pstat_cluster_gm.hip)
    PSTAT_TRY(alloc(h, &S.work, cluster_gm_work_bytes(h->cfg, A)));
  else if (home == SweepMem)   // working copy of the cells, [chain block][n][64] double2 (run_segment, ST = 2)
    PSTAT_TRY(alloc(h, &S.work, (size_t)A.nblocks * n * 64 * 16));
  PSTAT_TRY(alloc(h, (void **)&h->d_cases, sizeof(CaseConst) * (size_t)ncases));
  PSTAT_TRY(alloc(h, (void **)&h->d_queue, sizeof(int) * queue_ints(h->args)));
  PSTAT_TRY(alloc(h, (void **)&h->d_partial, sizeof(double) * reduce_scratch_doubles()));
  PSTAT_TRY(alloc(h, (void **)&h->d_red, sizeof(double) * PSTAT_NRED));
  HIP_TRY(hipMemsetAsync(h->d_queue, 0, sizeof(int) * queue_ints(h->args), h->stream));
  HIP_TRY(hipMemcpyAsync(h->d_cases, h->cases.data(), sizeof(CaseConst) * (size_t)ncases,
                         hipMemcpyHostToDevice, h->stream));
  const InitOpts io{h->base.use_x0, h->base.x0_phi, h->base.x0_theta, h->base.dx0_phi, h->base.dx0_theta, nullptr};
  HIP_TRY(launch_init(h->cfg, h->args, h->S, h->d_cases, h->base.phi_step, h->base.theta_step, io, h->stream));
  if (all_pairs(h->base.energy_type))  // a zero-step launch derives r, p, U (with the pair energy) from the fresh angles
    HIP_TRY(launch_steps(h, 0, 0));
  HIP_TRY(hipStreamSynchronize(h->stream));  // h->cases must outlive the copy; also surfaces faults here
  if (chain_per_lane(home)) {
    int bpc = 0;
    HIP_TRY(occupancy(h->kernel, lds_bytes(home, h->cfg.precision, h->args), &bpc));
    h->slots = (bpc > 0 ? bpc : 1) * prop.multiProcessorCount;
  }
  } catch (const std::bad_alloc &) {
    return fail(PSTAT_ERR_NOMEM, "host allocation failed");
  }
  *out = owner.release();
  return PSTAT_OK;
}

int pstat_create(const pstat_params *cases, int32_t ncases, void *stream, pstat_handle **out) {
  return create_handle(cases, ncases, stream, out, false);
}

int pstat_create_planar(const pstat_params *cases, int32_t ncases, void *stream, pstat_handle **out) {
  return create_handle(cases, ncases, stream, out, true);
}

void pstat_destroy(pstat_handle *h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (auto &b : h->bufs) (void)hipFree(b.ptr);
  if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
  delete h;   // with the recorder objects still open: nothing of theirs is in flight behind the synchronise above
}

int pstat_advance(pstat_handle *h, int64_t nsteps) {
  if (!h) return fail(PSTAT_ERR_INVALID_ARG, "null handle");
  if (nsteps < 0) return fail(PSTAT_ERR_INVALID_ARG, "nsteps must be >= 0");
  if (nsteps == 0) return PSTAT_OK;
  int rc = set_device(h);
  if (rc) return rc;
  if (h->failed_job) return report_failed_job(h);
  return enqueue_steps(h, nsteps);
}

int pstat_series_open(pstat_handle *h, int64_t capacity_rows, int32_t flags, pstat_series **out) {
  if (!h || !out) return fail(PSTAT_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  if (capacity_rows < 1) return fail(PSTAT_ERR_INVALID_ARG, "capacity_rows must be >= 1");
  if (flags & ~PSTAT_SERIES_ANGLES) return fail(PSTAT_ERR_INVALID_ARG, "unknown series flags %d", flags);
  const size_t cases = (size_t)h->ncases, n2 = 2 * (size_t)h->base.n;
  const size_t row_doubles = cases * (PSTAT_NRED + 7 + ((flags & PSTAT_SERIES_ANGLES) ? n2 : 0));
  if ((uint64_t)capacity_rows > (SIZE_MAX / sizeof(double)) / row_doubles)
    return fail(PSTAT_ERR_NOMEM, "a series of %lld rows does not fit the address space", (long long)capacity_rows);
  PSTAT_TRY(set_device(h));
  std::unique_ptr<pstat_series> s(new (std::nothrow) pstat_series);
  if (!s) return fail(PSTAT_ERR_NOMEM, "host allocation failed");
  const size_t rows = (size_t)capacity_rows;
  PSTAT_TRY(s->d_red.alloc(rows * cases * PSTAT_NRED));
  PSTAT_TRY(s->d_micro.alloc(rows * cases * 7));
  if (flags & PSTAT_SERIES_ANGLES) PSTAT_TRY(s->d_angles.alloc(rows * cases * n2));
  try {
    s->steps.resize(rows);
  } catch (const std::bad_alloc &) {
    return fail(PSTAT_ERR_NOMEM, "host allocation failed");
  }
  s->capacity = capacity_rows;
  return adopt(h->series, s, out);
}

int pstat_advance_series(pstat_handle *h, pstat_series *s, int64_t nsteps, int64_t stepout) {
  PSTAT_TRY(open_series(h, s));
  const size_t cases = (size_t)h->ncases, n2 = 2 * (size_t)h->base.n;
  return advance_recording(h, nsteps, stepout, s->capacity, s->rows, "series", [&]() -> int {
    const size_t row = (size_t)s->rows;
    HIP_TRY(launch_record(h->cfg, h->args, h->S, h->d_cases, h->steps_recorded, s->d_red.p + row * cases * PSTAT_NRED,
                          s->d_micro.p + row * cases * 7, s->d_angles.p ? s->d_angles.p + row * cases * n2 : nullptr, h->stream));
    s->steps[row] = h->steps_recorded;
    s->rows += 1;
    return PSTAT_OK;
  });
}

int pstat_series_read(pstat_handle *h, pstat_series *s, int64_t nrows, int64_t *steps_recorded, double *red, double *micro,
                      double *angles) {
  PSTAT_TRY(open_series(h, s));
  if (nrows < 0 || nrows > s->rows)
    return fail(PSTAT_ERR_INVALID_ARG, "%lld rows asked for, %lld recorded", (long long)nrows, (long long)s->rows);
  if (angles && !s->d_angles.p) return fail(PSTAT_ERR_INVALID_ARG, "the series was opened without PSTAT_SERIES_ANGLES");
  PSTAT_TRY(set_device(h));
  PSTAT_TRY(sync_checked(h));
  const size_t rows = (size_t)nrows, cases = (size_t)h->ncases, n2 = 2 * (size_t)h->base.n;
  if (!rows) return PSTAT_OK;
  if (steps_recorded) std::memcpy(steps_recorded, s->steps.data(), rows * sizeof(int64_t));
  if (red) HIP_TRY(hipMemcpy(red, s->d_red.p, rows * cases * PSTAT_NRED * sizeof(double), hipMemcpyDeviceToHost));
  if (micro) HIP_TRY(hipMemcpy(micro, s->d_micro.p, rows * cases * 7 * sizeof(double), hipMemcpyDeviceToHost));
  if (angles) HIP_TRY(hipMemcpy(angles, s->d_angles.p, rows * cases * n2 * sizeof(double), hipMemcpyDeviceToHost));
  return PSTAT_OK;
}

int pstat_series_clear(pstat_handle *h, pstat_series *s) {
  PSTAT_TRY(open_series(h, s));
  s->rows = 0;   // later rows are enqueued behind whatever still writes the old ones
  return PSTAT_OK;
}

void pstat_series_close(pstat_handle *h, pstat_series *s) { close_object(h, &pstat_handle::series, s); }

int pstat_series_error_bars(pstat_handle *h, pstat_series *s, int64_t first_row, int64_t nrows, int32_t min_blocks,
                            int64_t *nbatches, double *out, double *levels) {
  PSTAT_TRY(open_series(h, s, out != nullptr));
  if (h->cfg.umbrella)
    return fail(PSTAT_ERR_UNSUPPORTED, "error bars under --umbrella-sampling: the recorded means are ratios with per-chain "
                "normalizers that the rows do not hold");
  if (min_blocks == 0) min_blocks = 32;
  if (min_blocks < 2) return fail(PSTAT_ERR_INVALID_ARG, "min_blocks must be >= 2 (or 0 for the default 32), not %d", min_blocks);
  if (nrows < 0) nrows = s->rows - first_row;
  if (first_row < 0 || nrows < 0 || first_row > s->rows || nrows > s->rows - first_row)
    return fail(PSTAT_ERR_INVALID_ARG, "rows [%lld, %lld) asked for, %lld recorded", (long long)first_row,
                (long long)(first_row + nrows), (long long)s->rows);
  // the rows' common spacing; a row that breaks it was recorded with another stepout or after a pstat_reset_averages
  const int64_t *steps = s->steps.data() + first_row;
  const int64_t d = nrows >= 2 ? steps[1] - steps[0] : (nrows == 1 ? steps[0] : 1);
  for (int64_t r = 1; r < nrows; ++r)
    if (d < 1 || steps[r] - steps[r - 1] != d)
      return fail(PSTAT_ERR_INVALID_ARG, "row %lld was recorded at step %lld, row %lld at step %lld: the rows are not "
                  "equally spaced%s", (long long)(first_row + r), (long long)steps[r], (long long)(first_row + r - 1),
                  (long long)steps[r - 1], d < 1 ? " and increasing" : "");
  const bool zero_base = nrows >= 1 && steps[0] == d;   // the series began at empty averages
  const int64_t nb = zero_base ? nrows : (nrows > 0 ? nrows - 1 : 0);
  if (nbatches) *nbatches = nb;
  if (nb < min_blocks)
    return fail(PSTAT_ERR_TOO_SMALL, "%lld batches, min_blocks = %d", (long long)nb, min_blocks);
  if (nb > blocking_max_batches())
    return fail(PSTAT_ERR_UNSUPPORTED, "%lld batches: the blocking kernel takes at most %lld (level 1 of a column must fit "
                "the LDS of a CU)", (long long)nb, (long long)blocking_max_batches());
  PSTAT_TRY(set_device(h));
  PSTAT_TRY(sync_checked(h));
  const int64_t ncols = (int64_t)h->ncases * PSTAT_NQ;
  DeviceDoubles x;
  PSTAT_TRY(x.alloc((size_t)nb * (size_t)ncols));
  const int64_t row0 = first_row + (zero_base ? 0 : 1);
  HIP_TRY(launch_series_batches(s->d_red.p, row0, nb, h->ncases, s->steps[(size_t)row0], d, zero_base ? 1 : 0, x.p, h->stream));
  return blocking_to_host(x.p, nb, ncols, ncols, min_blocks, h->stream, out, levels);
}

int pstat_blocking_device(const double *x, int64_t nbatches, int64_t ncols, int64_t stride, int32_t min_blocks, int32_t device,
                          void *stream, double *out, double *levels) {
  if (!x || !out) return fail(PSTAT_ERR_INVALID_ARG, "null argument");
  if (min_blocks == 0) min_blocks = 32;
  if (min_blocks < 2) return fail(PSTAT_ERR_INVALID_ARG, "min_blocks must be >= 2 (or 0 for the default 32), not %d", min_blocks);
  if (ncols < 1 || ncols > 0x7fffffff) return fail(PSTAT_ERR_INVALID_ARG, "ncols must be in 1 .. 2^31 - 1");
  if (stride < ncols) return fail(PSTAT_ERR_INVALID_ARG, "stride %lld < ncols %lld", (long long)stride, (long long)ncols);
  if (nbatches < min_blocks)
    return fail(PSTAT_ERR_TOO_SMALL, "%lld batches, min_blocks = %d", (long long)nbatches, min_blocks);
  if (nbatches > blocking_max_batches())
    return fail(PSTAT_ERR_UNSUPPORTED, "%lld batches: the blocking kernel takes at most %lld (level 1 of a column must fit "
                "the LDS of a CU)", (long long)nbatches, (long long)blocking_max_batches());
  int before = -1;      // the caller's current device is put back: the callers are programs with a device of their own (torch)
  if (hipGetDevice(&before) != hipSuccess) before = -1;
  if (hipSetDevice(device) != hipSuccess) return fail(PSTAT_ERR_NO_DEVICE, "device %d is not available", device);
  const int rc = blocking_to_host(x, nbatches, ncols, stride, min_blocks, (hipStream_t)stream, out, levels);
  if (before >= 0 && before != device) (void)hipSetDevice(before);
  return rc;
}

int pstat_tempering_open(pstat_handle *h, const int32_t *ladder, uint64_t seed, pstat_tempering **out) {
  if (!h || !ladder || !out) return fail(PSTAT_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  const int nc = h->ncases;
  for (int i = 0; i < nc; ++i)
    if (ladder[i] < -1) return fail(PSTAT_ERR_INVALID_ARG, "ladder[%d] = %d: a ladder id is >= 0, or -1 for a case that takes no part", i, ladder[i]);
  if (h->cfg.umbrella)
    return fail(PSTAT_ERR_UNSUPPORTED, "replica exchange under --umbrella-sampling: the weights and their reference energy are "
                "per chain, relative to the chain's first configuration");
  try {
    // a ladder's cases agree with its first one in every physics scalar but kT
    std::vector<int> first((size_t)nc, -1), order;
    for (int i = 0; i < nc; ++i) {
      if (ladder[i] < 0) continue;
      int f = -1;
      for (int j = 0; j < i && f < 0; ++j)
        if (ladder[j] == ladder[i]) f = j;
      first[(size_t)i] = f < 0 ? i : first[(size_t)f];
      if (f < 0) continue;
      const CaseConst &a = h->cases[(size_t)first[(size_t)i]], &b = h->cases[(size_t)i];
      const struct { const char *name; double x, y; } fields[] = {
          {"E0", a.E0, b.E0}, {"K1", a.K1, b.K1}, {"K2", a.K2, b.K2}, {"mu", a.mu, b.mu}, {"Fz", a.Fz, b.Fz}, {"Fx", a.Fx, b.Fx},
          {"b", a.b, b.b}, {"bend_mod", a.kappa, b.kappa}, {"bend_angle", a.psi0, b.psi0},
          {"cluster_prob", a.cluster_prob, b.cluster_prob}, {"cutoff_radius", a.cutoff_radius, b.cutoff_radius}};
      for (const auto &fd : fields)
        if (fd.x != fd.y)
          return fail(PSTAT_ERR_INVALID_ARG, "ladder %d: case %d differs from case %d in %s (%.17g against %.17g); the cases of "
                      "a ladder differ in kT, seed and chain_id0 only", ladder[i], i, first[(size_t)i], fd.name, fd.y, fd.x);
    }
    // rungs: each ladder's cases by (kT, case index) ascending; pairs of both parities
    std::vector<int32_t> pairs[2];
    for (int i = 0; i < nc; ++i) {
      if (first[(size_t)i] != i) continue;
      order.clear();
      for (int j = i; j < nc; ++j)
        if (ladder[j] == ladder[i]) order.push_back(j);
      for (size_t x = 1; x < order.size(); ++x)   // insertion sort: stable, so ties keep the case order
        for (size_t y = x; y > 0 && h->cases[(size_t)order[y]].kT < h->cases[(size_t)order[y - 1]].kT; --y)
          std::swap(order[y], order[y - 1]);
      for (int parity = 0; parity < 2; ++parity)
        for (size_t r = (size_t)parity; r + 1 < order.size(); r += 2) {
          pairs[parity].push_back(order[r]);
          pairs[parity].push_back(order[r + 1]);
        }
    }
    PSTAT_TRY(set_device(h));
    std::unique_ptr<pstat_tempering> t(new (std::nothrow) pstat_tempering);
    if (!t) return fail(PSTAT_ERR_NOMEM, "host allocation failed");
    t->seed = seed;
    const size_t per = (size_t)h->base.num_chains;
    size_t most = 0;
    hipError_t e = hipSuccess;
    for (int parity = 0; parity < 2 && e == hipSuccess; ++parity) {
      t->npairs[parity] = (int64_t)(pairs[parity].size() / 2);
      most = pairs[parity].size() / 2 > most ? pairs[parity].size() / 2 : most;
      if (pairs[parity].empty()) continue;
      e = t->d_pairs[parity].malloc(pairs[parity].size());
      if (e == hipSuccess)
        e = hipMemcpy(t->d_pairs[parity].p, pairs[parity].data(), pairs[parity].size() * sizeof(int32_t), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess && most) e = t->d_flags.malloc(most * per);
    if (e == hipSuccess) e = t->d_counts.malloc(2 * (size_t)nc);
    if (e == hipSuccess) e = hipMemsetAsync(t->d_counts.p, 0, 2 * (size_t)nc * sizeof(int64_t), h->stream);   // ahead of the first round
    if (e != hipSuccess)
      return fail(e == hipErrorOutOfMemory ? PSTAT_ERR_NOMEM : PSTAT_ERR_HIP, "tempering tables: %s", hipGetErrorString(e));
    return adopt(h->tempering, t, out);
  } catch (const std::bad_alloc &) {
    return fail(PSTAT_ERR_NOMEM, "host allocation failed");
  }
}

int pstat_tempering_exchange(pstat_handle *h, pstat_tempering *t) {
  PSTAT_TRY(open_tempering(h, t));
  if (t->round > 0xffffffffull)
    return fail(PSTAT_ERR_INVALID_ARG, "the 32-bit round counter of this tempering object is used up (2^32 rounds)");
  PSTAT_TRY(set_device(h));
  if (h->failed_job) return report_failed_job(h);
  const int parity = (int)(t->round & 1);
  const ExchangeArgs a{h->base.num_chains, h->S.C, h->base.n, t->npairs[parity], (uint32_t)t->round,
                       (uint32_t)t->seed, (uint32_t)(t->seed >> 32), 0u};
  HIP_TRY(launch_exchange(a, h->S, h->d_cases, t->d_pairs[parity].p, t->d_flags.p, t->d_counts.p, t->d_counts.p + h->ncases,
                          h->elem, h->stream));
  t->round += 1;
  return PSTAT_OK;
}

int pstat_tempering_stats(pstat_handle *h, pstat_tempering *t, int64_t *attempted, int64_t *accepted, int64_t *rounds) {
  PSTAT_TRY(open_tempering(h, t));
  PSTAT_TRY(set_device(h));
  PSTAT_TRY(sync_checked(h));
  const size_t bytes = (size_t)h->ncases * sizeof(int64_t);
  if (attempted) HIP_TRY(hipMemcpy(attempted, t->d_counts.p, bytes, hipMemcpyDeviceToHost));
  if (accepted) HIP_TRY(hipMemcpy(accepted, t->d_counts.p + h->ncases, bytes, hipMemcpyDeviceToHost));
  if (rounds) *rounds = (int64_t)t->round;
  return PSTAT_OK;
}

void pstat_tempering_close(pstat_handle *h, pstat_tempering *t) { close_object(h, &pstat_handle::tempering, t); }

int pstat_hist_open(pstat_handle *h, const pstat_hist_spec *specs, int32_t nspecs, int32_t per_case, pstat_hist **out) {
  if (!h || !specs || !out) return fail(PSTAT_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  try {
    std::vector<HistSpec> dev;
    int32_t total_bins = 0;
    PSTAT_TRY(hist_specs(specs, nspecs, per_case ? h->ncases : 1, PSTAT_HC_COUNT, "the PSTAT_HC_* channels", dev, &total_bins));
    if (h->cfg.umbrella)
      return fail(PSTAT_ERR_UNSUPPORTED, "histograms under --umbrella-sampling: the samples carry per-chain weights whose gauge "
                  "the counts do not hold");
    PSTAT_TRY(set_device(h));
    std::unique_ptr<pstat_hist> g(new (std::nothrow) pstat_hist);
    if (!g) return fail(PSTAT_ERR_NOMEM, "host allocation failed");
    g->nspecs = nspecs;
    g->total_bins = total_bins;
    g->per_case = per_case ? 1 : 0;
    g->slots = (size_t)h->ncases * ((size_t)total_bins + 3 * (size_t)nspecs);
    hipError_t e = g->d_specs.malloc(dev.size());
    if (e == hipSuccess) e = g->d_counts.malloc(g->slots);
    if (e != hipSuccess) return fail(PSTAT_ERR_NOMEM, "histogram of %zu counters: %s", g->slots, hipGetErrorString(e));
    e = hipMemcpy(g->d_specs.p, dev.data(), dev.size() * sizeof(HistSpec), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemsetAsync(g->d_counts.p, 0, g->slots * sizeof(int64_t), h->stream);   // ahead of the first record
    if (e != hipSuccess) return fail(PSTAT_ERR_HIP, "histogram tables: %s", hipGetErrorString(e));
    return adopt(h->hists, g, out);
  } catch (const std::bad_alloc &) {
    return fail(PSTAT_ERR_NOMEM, "host allocation failed");
  }
}

int pstat_hist_record(pstat_handle *h, pstat_hist *g) {
  PSTAT_TRY(open_hist(h, g));
  PSTAT_TRY(set_device(h));
  if (h->failed_job) return report_failed_job(h);
  return enqueue_hist(h, g);
}

int pstat_advance_hist(pstat_handle *h, pstat_hist *g, int64_t nsteps, int64_t stepout) {
  PSTAT_TRY(open_hist(h, g));
  return advance_recording(h, nsteps, stepout, 0, 0, "histogram", [&] { return enqueue_hist(h, g); });
}

int pstat_hist_read(pstat_handle *h, pstat_hist *g, int64_t *counts, int64_t *tails, int64_t *records) {
  PSTAT_TRY(open_hist(h, g));
  PSTAT_TRY(set_device(h));
  PSTAT_TRY(sync_checked(h));
  const size_t nbins = (size_t)h->ncases * (size_t)g->total_bins;
  if (counts) HIP_TRY(hipMemcpy(counts, g->d_counts.p, nbins * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (tails) HIP_TRY(hipMemcpy(tails, g->d_counts.p + nbins, (g->slots - nbins) * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (records) *records = g->records;
  return PSTAT_OK;
}

int pstat_hist_clear(pstat_handle *h, pstat_hist *g) {
  PSTAT_TRY(open_hist(h, g));
  PSTAT_TRY(set_device(h));
  HIP_TRY(hipMemsetAsync(g->d_counts.p, 0, g->slots * sizeof(int64_t), h->stream));   // behind the records already enqueued
  g->records = 0;
  return PSTAT_OK;
}

void pstat_hist_close(pstat_handle *h, pstat_hist *g) { close_object(h, &pstat_handle::hists, g); }

int pstat_histogram_device(const double *x, int64_t nrows, int64_t stride, const pstat_hist_spec *specs, int32_t nspecs,
                           int32_t device, void *stream, int64_t *counts, int64_t *tails) {
  if (!x || !specs) return fail(PSTAT_ERR_INVALID_ARG, "null argument");
  if (nrows < 0) return fail(PSTAT_ERR_INVALID_ARG, "nrows must be >= 0, not %lld", (long long)nrows);
  if (stride < 1) return fail(PSTAT_ERR_INVALID_ARG, "stride must be >= 1, not %lld", (long long)stride);
  std::vector<HistSpec> dev;
  std::vector<int64_t> host;
  int32_t total_bins = 0;
  try {
    PSTAT_TRY(hist_specs(specs, nspecs, 1, stride, "the columns below stride", dev, &total_bins));
    host.resize((size_t)total_bins + 3 * (size_t)nspecs);
  } catch (const std::bad_alloc &) {
    return fail(PSTAT_ERR_NOMEM, "host allocation failed");
  }
  int before = -1;      // the caller's current device is put back, as pstat_blocking_device does
  if (hipGetDevice(&before) != hipSuccess) before = -1;
  if (hipSetDevice(device) != hipSuccess) return fail(PSTAT_ERR_NO_DEVICE, "device %d is not available", device);
  const hipStream_t st = (hipStream_t)stream;
  const size_t bytes = host.size() * sizeof(int64_t);
  HistSpec *d_specs = nullptr;
  int64_t *d_counts = nullptr;
  int rc = PSTAT_OK;
  hipError_t e = hipMalloc((void **)&d_specs, dev.size() * sizeof(HistSpec));
  if (e == hipSuccess) e = hipMalloc((void **)&d_counts, bytes);
  if (e != hipSuccess) rc = fail(PSTAT_ERR_NOMEM, "hipMalloc failed: %s", hipGetErrorString(e));
  if (e == hipSuccess) e = hipMemcpyAsync(d_specs, dev.data(), dev.size() * sizeof(HistSpec), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync(d_counts, 0, bytes, st);
  if (e == hipSuccess)
    e = launch_hist(HistArgs{nrows, 1, 1, stride, nspecs, total_bins, 0, 1}, x, d_specs, d_counts, d_counts + total_bins, st);
  if (e == hipSuccess) e = hipMemcpyAsync(host.data(), d_counts, bytes, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess && rc == PSTAT_OK) rc = fail(PSTAT_ERR_HIP, "pstat_histogram_device: %s", hipGetErrorString(e));
  (void)hipFree(d_specs);
  (void)hipFree(d_counts);
  if (before >= 0 && before != device) (void)hipSetDevice(before);
  if (rc) return rc;
  if (counts) std::memcpy(counts, host.data(), (size_t)total_bins * sizeof(int64_t));
  if (tails) std::memcpy(tails, host.data() + total_bins, 3 * (size_t)nspecs * sizeof(int64_t));
  return PSTAT_OK;
}

int pstat_corr_open(pstat_handle *h, int32_t channels, int32_t max_lag, int64_t capacity_rows, pstat_corr **out) {
  if (!h || !out) return fail(PSTAT_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  const int64_t n = h->base.n;
  if (channels < 1 || channels > (PSTAT_CORR_NN | PSTAT_CORR_ZZ | PSTAT_CORR_MM))
    return fail(PSTAT_ERR_INVALID_ARG, "channels must be a mask of PSTAT_CORR_NN | _ZZ | _MM in 1 .. 7, not %d", channels);
  if (max_lag < -1 || max_lag > n - 1)
    return fail(PSTAT_ERR_INVALID_ARG, "max_lag must be in 0 .. n - 1 = %lld (or -1 for n - 1), not %d", (long long)n - 1, max_lag);
  if (capacity_rows < 0) return fail(PSTAT_ERR_INVALID_ARG, "capacity_rows must be >= 0, not %lld", (long long)capacity_rows);
  if (h->cfg.umbrella)
    return fail(PSTAT_ERR_UNSUPPORTED, "correlations under --umbrella-sampling: the samples carry per-chain weights whose gauge "
                "the sums do not hold");
  if (n > tile_max_n(h->cfg.planar))
    return fail(PSTAT_ERR_UNSUPPORTED, "n = %lld: a chain's unit vectors must fit the LDS of a workgroup, n <= %lld for a %s handle",
                (long long)n, (long long)tile_max_n(h->cfg.planar), h->cfg.planar ? "planar" : "3D");
  if (max_lag < 0) max_lag = (int32_t)(n - 1);
  const int nch = (channels & 1) + ((channels >> 1) & 1) + ((channels >> 2) & 1);
  CorrArgs a{};
  a.per = h->base.num_chains; a.ncases = h->ncases; a.n = n;
  a.channels = channels; a.max_lag = max_lag; a.ncols = nch * (max_lag + 1);
  a.elem = (int32_t)h->elem; a.planar = h->cfg.planar ? 1 : 0; a.polar = h->cfg.chain_type == PSTAT_POLAR ? 1 : 0;
  tile_layout(a, max_lag + 1);
  std::unique_ptr<pstat_corr> g;
  PSTAT_TRY(new_totals(h, a.ncols, capacity_rows, tile_partial_doubles(a), kCorrText, g));
  g->args = a;
  return adopt(h->corrs, g, out);
}

int pstat_corr_record(pstat_handle *h, pstat_corr *g) {
  PSTAT_TRY(open_corr(h, g));
  return totals_record(h, g, kCorrText, [&] { return enqueue_corr(h, g); });
}

int pstat_advance_corr(pstat_handle *h, pstat_corr *g, int64_t nsteps, int64_t stepout) {
  PSTAT_TRY(open_corr(h, g));
  return advance_recording(h, nsteps, stepout, g->capacity, g->rows, kCorrText.object, [&] { return enqueue_corr(h, g); });
}

int pstat_corr_read(pstat_handle *h, pstat_corr *g, double *sum, double *sumsq, int64_t *records) {
  PSTAT_TRY(open_corr(h, g));
  return totals_read(h, g, sum, sumsq, records);
}

int pstat_corr_rows(pstat_handle *h, pstat_corr *g, const double **dev_rows, int64_t *nrows, int64_t *stride) {
  PSTAT_TRY(open_corr(h, g, dev_rows && nrows && stride));
  return totals_rows(h, g, dev_rows, nrows, stride);
}

int pstat_corr_clear(pstat_handle *h, pstat_corr *g) {
  PSTAT_TRY(open_corr(h, g));
  return totals_clear(h, g);
}

void pstat_corr_close(pstat_handle *h, pstat_corr *g) { close_object(h, &pstat_handle::corrs, g); }

int pstat_shape_open(pstat_handle *h, const double *q, int32_t nq, int64_t capacity_rows, pstat_shape **out) {
  if (!h || !out) return fail(PSTAT_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  const int64_t n = h->base.n;
  const bool planar = h->cfg.planar;
  if (nq < 0) return fail(PSTAT_ERR_INVALID_ARG, "nq must be >= 0, not %d", nq);
  if (nq > PSTAT_SHAPE_MAX_Q)
    return fail(PSTAT_ERR_UNSUPPORTED, "nq = %d: at most PSTAT_SHAPE_MAX_Q = %d wave-vectors per shape object", nq, PSTAT_SHAPE_MAX_Q);
  if (nq > 0 && !q) return fail(PSTAT_ERR_INVALID_ARG, "q is null with nq = %d", nq);
  for (int32_t k = 0; k < 3 * nq; ++k)
    if (!std::isfinite(q[k])) return fail(PSTAT_ERR_INVALID_ARG, "q[%d][%d] is not finite", k / 3, k % 3);
  if (capacity_rows < 0) return fail(PSTAT_ERR_INVALID_ARG, "capacity_rows must be >= 0, not %lld", (long long)capacity_rows);
  for (int32_t k = 0; k < nq; ++k) {
    const double q1 = std::fabs(q[3 * k]) + (planar ? 0.0 : std::fabs(q[3 * k + 1])) + std::fabs(q[3 * k + 2]);
    for (int c = 0; c < h->ncases; ++c)
      if (!(q1 * std::fabs(h->cases[(size_t)c].b) * (double)n < 1.0e5))
        return fail(PSTAT_ERR_INVALID_ARG, "q[%d] = (%g, %g, %g) with case %d (b = %g, n = %lld): (|q_x| + |q_y| + |q_z|) b n must stay "
                    "below 1e5, where the device's sincos is its < 1 ulp routine", k, q[3 * k], q[3 * k + 1], q[3 * k + 2], c,
                    h->cases[(size_t)c].b, (long long)n);
  }
  if (h->cfg.umbrella)
    return fail(PSTAT_ERR_UNSUPPORTED, "chain shape under --umbrella-sampling: the samples carry per-chain weights whose gauge "
                "the sums do not hold");
  if (n > tile_max_n(h->cfg.planar))
    return fail(PSTAT_ERR_UNSUPPORTED, "n = %lld: a chain's positions must fit the LDS of a workgroup, n <= %lld for a %s handle",
                (long long)n, (long long)tile_max_n(h->cfg.planar), planar ? "planar" : "3D");
  ShapeArgs a{};
  a.per = h->base.num_chains; a.ncases = h->ncases; a.n = n;
  a.nq = nq; a.ncols = PSTAT_SHAPE_GYR + nq;
  a.elem = (int32_t)h->elem; a.planar = planar ? 1 : 0;
  tile_layout(a, nq);
  std::unique_ptr<pstat_shape> g;
  PSTAT_TRY(new_totals(h, a.ncols, capacity_rows, tile_partial_doubles(a), kShapeText, g));
  g->args = a;
  if (nq > 0) {   // the wave-vectors: a copy, the caller's table may go
    hipError_t e = g->d_q.malloc(3 * (size_t)nq);
    if (e != hipSuccess) return fail(PSTAT_ERR_NOMEM, kShapeText.nomem, g->stride, (long long)capacity_rows, hipGetErrorString(e));
    e = hipMemcpy(g->d_q.p, q, 3 * (size_t)nq * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(PSTAT_ERR_HIP, kShapeText.hip, hipGetErrorString(e));
  }
  return adopt(h->shapes, g, out);
}

int pstat_shape_record(pstat_handle *h, pstat_shape *g) {
  PSTAT_TRY(open_shape(h, g));
  return totals_record(h, g, kShapeText, [&] { return enqueue_shape(h, g); });
}

int pstat_advance_shape(pstat_handle *h, pstat_shape *g, int64_t nsteps, int64_t stepout) {
  PSTAT_TRY(open_shape(h, g));
  return advance_recording(h, nsteps, stepout, g->capacity, g->rows, kShapeText.object, [&] { return enqueue_shape(h, g); });
}

int pstat_shape_read(pstat_handle *h, pstat_shape *g, double *sum, double *sumsq, int64_t *records) {
  PSTAT_TRY(open_shape(h, g));
  return totals_read(h, g, sum, sumsq, records);
}

int pstat_shape_rows(pstat_handle *h, pstat_shape *g, const double **dev_rows, int64_t *nrows, int64_t *stride) {
  PSTAT_TRY(open_shape(h, g, dev_rows && nrows && stride));
  return totals_rows(h, g, dev_rows, nrows, stride);
}

int pstat_shape_clear(pstat_handle *h, pstat_shape *g) {
  PSTAT_TRY(open_shape(h, g));
  return totals_clear(h, g);
}

void pstat_shape_close(pstat_handle *h, pstat_shape *g) { close_object(h, &pstat_handle::shapes, g); }

int pstat_pdist_open(pstat_handle *h, const pstat_pdist_spec *spec, const double *q, const double *rmax_per_case,
                     int64_t capacity_rows, pstat_pdist **out) {
  if (!h || !spec || !out) return fail(PSTAT_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  const int64_t n = h->base.n;
  const bool planar = h->cfg.planar;
  const int32_t nbins = spec->nbins, nq = spec->nq, min_sep = spec->min_sep;
  int32_t max_sep = spec->max_sep;
  if (n < 2) return fail(PSTAT_ERR_INVALID_ARG, "n = %lld: a chain of fewer than two monomers has no pair", (long long)n);
  if (max_sep < -1 || max_sep > n - 1)
    return fail(PSTAT_ERR_INVALID_ARG, "max_sep must be in 0 .. n - 1 = %lld (or -1 for n - 1), not %d", (long long)n - 1, max_sep);
  if (min_sep < 1 || min_sep > n - 1)
    return fail(PSTAT_ERR_INVALID_ARG, "min_sep must be in 1 .. n - 1 = %lld, not %d", (long long)n - 1, min_sep);
  if (nbins < 0) return fail(PSTAT_ERR_INVALID_ARG, "nbins must be >= 0, not %d", nbins);
  if (nq < 0) return fail(PSTAT_ERR_INVALID_ARG, "nq must be >= 0, not %d", nq);
  if (nbins > PSTAT_PDIST_MAX_BINS)
    return fail(PSTAT_ERR_UNSUPPORTED, "nbins = %d: at most PSTAT_PDIST_MAX_BINS = %d bins per pdist object (a workgroup keeps a "
                "chain's counters in LDS)", nbins, PSTAT_PDIST_MAX_BINS);
  if (nq > PSTAT_PDIST_MAX_Q)
    return fail(PSTAT_ERR_UNSUPPORTED, "nq = %d: at most PSTAT_PDIST_MAX_Q = %d magnitudes per pdist object", nq, PSTAT_PDIST_MAX_Q);
  std::vector<double> tab;
  try {
    tab.resize((size_t)nq + (nbins > 0 ? (size_t)h->ncases : 0));
  } catch (const std::bad_alloc &) {
    return fail(PSTAT_ERR_NOMEM, "host allocation failed");
  }
  for (int c = 0; nbins > 0 && c < h->ncases; ++c) {
    const double rmax = rmax_per_case ? rmax_per_case[c] : spec->rmax;
    const char *which = rmax_per_case ? "rmax_per_case" : "rmax";
    if (!std::isfinite(rmax) || !(rmax > 0.0))
      return fail(PSTAT_ERR_INVALID_ARG, "%s = %g (case %d) must be finite and > 0 when nbins = %d", which, rmax, c, nbins);
    const double inv = (double)nbins / rmax;
    if (!std::isfinite(inv) || !(inv > 0.0))   // t = r * inv is then never NaN for a finite r
      return fail(PSTAT_ERR_INVALID_ARG, "%s = %g (case %d) leaves no finite positive nbins / rmax for %d bins", which, rmax, c, nbins);
    tab[(size_t)nq + (size_t)c] = inv;
  }
  if (nq > 0 && !q) return fail(PSTAT_ERR_INVALID_ARG, "q is null with nq = %d", nq);
  for (int32_t k = 0; k < nq; ++k) {
    if (!std::isfinite(q[k]) || q[k] < 0.0) return fail(PSTAT_ERR_INVALID_ARG, "q[%d] = %g must be finite and >= 0", k, q[k]);
    for (int c = 0; c < h->ncases; ++c)
      if (!(q[k] * std::fabs(h->cases[(size_t)c].b) * (double)n < 1.0e5))
        return fail(PSTAT_ERR_INVALID_ARG, "q[%d] = %g with case %d (b = %g, n = %lld): q b n must stay below 1e5, where the device's "
                    "sincos is its < 1 ulp routine", k, q[k], c, h->cases[(size_t)c].b, (long long)n);
    tab[(size_t)k] = q[k];
  }
  if (capacity_rows < 0) return fail(PSTAT_ERR_INVALID_ARG, "capacity_rows must be >= 0, not %lld", (long long)capacity_rows);
  if (h->cfg.umbrella)
    return fail(PSTAT_ERR_UNSUPPORTED, "pair distances under --umbrella-sampling: the samples carry per-chain weights whose gauge "
                "the sums do not hold");
  if (n > pdist_max_n(planar, nbins))
    return fail(PSTAT_ERR_UNSUPPORTED, "n = %lld: a chain's positions and its %d bin counters must fit the LDS of a workgroup, "
                "n <= %lld for a %s handle", (long long)n, nbins > 0 ? nbins + 1 : 0, (long long)pdist_max_n(planar, nbins),
                planar ? "planar" : "3D");
  if (max_sep < 0) max_sep = (int32_t)(n - 1);
  PdistArgs a{};
  a.per = h->base.num_chains; a.ncases = h->ncases; a.n = n;
  a.max_sep = max_sep; a.min_sep = min_sep; a.nbins = nbins; a.nq = nq;
  a.ncols = max_sep + 1 + (nbins > 0 ? nbins + 1 : 0) + nq;
  a.elem = (int32_t)h->elem; a.planar = planar ? 1 : 0;
  pdist_layout(a);
  std::unique_ptr<pstat_pdist> g;
  PSTAT_TRY(new_totals(h, a.ncols, capacity_rows, tile_partial_doubles(a), kPdistText, g));
  g->args = a;
  if (!tab.empty()) {   // the magnitudes and the cases' nbins / rmax: a copy, the caller's tables may go
    hipError_t e = g->d_tab.malloc(tab.size());
    if (e != hipSuccess) return fail(PSTAT_ERR_NOMEM, kPdistText.nomem, g->stride, (long long)capacity_rows, hipGetErrorString(e));
    e = hipMemcpy(g->d_tab.p, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(PSTAT_ERR_HIP, kPdistText.hip, hipGetErrorString(e));
  }
  return adopt(h->pdists, g, out);
}

int pstat_pdist_record(pstat_handle *h, pstat_pdist *g) {
  PSTAT_TRY(open_pdist(h, g));
  return totals_record(h, g, kPdistText, [&] { return enqueue_pdist(h, g); });
}

int pstat_advance_pdist(pstat_handle *h, pstat_pdist *g, int64_t nsteps, int64_t stepout) {
  PSTAT_TRY(open_pdist(h, g));
  return advance_recording(h, nsteps, stepout, g->capacity, g->rows, kPdistText.object, [&] { return enqueue_pdist(h, g); });
}

int pstat_pdist_read(pstat_handle *h, pstat_pdist *g, double *sum, double *sumsq, int64_t *records) {
  PSTAT_TRY(open_pdist(h, g));
  return totals_read(h, g, sum, sumsq, records);
}

int pstat_pdist_rows(pstat_handle *h, pstat_pdist *g, const double **dev_rows, int64_t *nrows, int64_t *stride) {
  PSTAT_TRY(open_pdist(h, g, dev_rows && nrows && stride));
  return totals_rows(h, g, dev_rows, nrows, stride);
}

int pstat_pdist_clear(pstat_handle *h, pstat_pdist *g) {
  PSTAT_TRY(open_pdist(h, g));
  return totals_clear(h, g);
}

void pstat_pdist_close(pstat_handle *h, pstat_pdist *g) { close_object(h, &pstat_handle::pdists, g); }

int pstat_energy_open(pstat_handle *h, const pstat_energy_spec *spec, const double *cutoff_per_case, int64_t capacity_rows,
                      pstat_energy **out) {
  if (!h || !spec || !out) return fail(PSTAT_ERR_INVALID_ARG, "null argument");
  *out = nullptr;
  const int64_t n = h->base.n;
  const bool planar = h->cfg.planar;
  int32_t max_sep = spec->max_sep;
  if (max_sep < -1 || max_sep > n - 1)
    return fail(PSTAT_ERR_INVALID_ARG, "max_sep must be in 0 .. n - 1 = %lld (or -1 for n - 1), not %d", (long long)n - 1, max_sep);
  if (spec->reserved != 0) return fail(PSTAT_ERR_INVALID_ARG, "reserved must be 0, not %d", spec->reserved);
  std::vector<double> tab;
  try {
    tab.resize((size_t)h->ncases);
  } catch (const std::bad_alloc &) {
    return fail(PSTAT_ERR_NOMEM, "host allocation failed");
  }
  bool cut = false;
  for (int c = 0; c < h->ncases; ++c) {
    const double v = cutoff_per_case ? cutoff_per_case[c] : spec->cutoff;
    if (!std::isfinite(v) || v < 0.0)
      return fail(PSTAT_ERR_INVALID_ARG, "%s = %g (case %d) must be finite and >= 0 (0: no `within` column)",
                  cutoff_per_case ? "cutoff_per_case" : "cutoff", v, c);
    tab[(size_t)c] = v;
    cut = cut || v > 0.0;
  }
  if (capacity_rows < 0) return fail(PSTAT_ERR_INVALID_ARG, "capacity_rows must be >= 0, not %lld", (long long)capacity_rows);
  if (h->cfg.umbrella)
    return fail(PSTAT_ERR_UNSUPPORTED, "the energy by term under --umbrella-sampling: the samples carry per-chain weights whose gauge "
                "the sums do not hold");
  if (n > energy_max_n(planar))
    return fail(PSTAT_ERR_UNSUPPORTED, "n = %lld: a chain's positions and dipoles must fit the LDS of a workgroup, n <= %lld for a %s "
                "handle", (long long)n, (long long)energy_max_n(planar), planar ? "planar" : "3D");
  if (max_sep < 0) max_sep = (int32_t)(n - 1);
  EnergyArgs a{};
  a.per = h->base.num_chains; a.ncases = h->ncases; a.n = n;
  a.max_sep = max_sep; a.cut = cut ? 1 : 0; a.paired = h->ov.energy_map == 's' ? 0 : 1;
  a.ncols = 3 + max_sep + 1 + (cut ? 1 : 0);
  a.elem = (int32_t)h->elem; a.planar = planar ? 1 : 0; a.polar = h->cfg.chain_type == PSTAT_POLAR ? 1 : 0;
  energy_layout(a);
  std::unique_ptr<pstat_energy> g;
  PSTAT_TRY(new_totals(h, a.ncols, capacity_rows, tile_partial_doubles(a), kEnergyText, g));
  g->args = a;
  if (cut) {   // the cases' radii: a copy, the caller's table may go
    hipError_t e = g->d_cut.malloc(tab.size());
    if (e != hipSuccess) return fail(PSTAT_ERR_NOMEM, kEnergyText.nomem, g->stride, (long long)capacity_rows, hipGetErrorString(e));
    e = hipMemcpy(g->d_cut.p, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(PSTAT_ERR_HIP, kEnergyText.hip, hipGetErrorString(e));
  }
  return adopt(h->energies, g, out);
}

int pstat_energy_record(pstat_handle *h, pstat_energy *g) {
  PSTAT_TRY(open_energy(h, g));
  return totals_record(h, g, kEnergyText, [&] { return enqueue_energy(h, g); });
}

int pstat_advance_energy(pstat_handle *h, pstat_energy *g, int64_t nsteps, int64_t stepout) {
  PSTAT_TRY(open_energy(h, g));
  return advance_recording(h, nsteps, stepout, g->capacity, g->rows, kEnergyText.object, [&] { return enqueue_energy(h, g); });
}

int pstat_energy_read(pstat_handle *h, pstat_energy *g, double *sum, double *sumsq, int64_t *records) {
  PSTAT_TRY(open_energy(h, g));
  return totals_read(h, g, sum, sumsq, records);
}

int pstat_energy_rows(pstat_handle *h, pstat_energy *g, const double **dev_rows, int64_t *nrows, int64_t *stride) {
  PSTAT_TRY(open_energy(h, g, dev_rows && nrows && stride));
  return totals_rows(h, g, dev_rows, nrows, stride);
}

int pstat_energy_clear(pstat_handle *h, pstat_energy *g) {
  PSTAT_TRY(open_energy(h, g));
  return totals_clear(h, g);
}

void pstat_energy_close(pstat_handle *h, pstat_energy *g) { close_object(h, &pstat_handle::energies, g); }

int pstat_sync(pstat_handle *h) {
  if (!h) return fail(PSTAT_ERR_INVALID_ARG, "null handle");
  int rc = set_device(h);
  if (rc) return rc;
  return sync_checked(h);
}

int pstat_reinit(pstat_handle *h, int32_t force_init) {
  if (!h) return fail(PSTAT_ERR_INVALID_ARG, "null handle");
  if (h->cfg.planar)
    return fail(PSTAT_ERR_UNSUPPORTED, "2D/mcmc_clustering_eap_chain.jl has no --num-inits: nothing to re-initialise");
  if (h->cfg.move_set == PSTAT_MOVES_CLUSTER)
    return fail(PSTAT_ERR_UNSUPPORTED, "mcmc_clustering_eap_chain.jl has no --num-inits: nothing to re-initialise");
  int rc = set_device(h);
  if (rc) return rc;
  if (h->cfg.home == Interacting)   // done inside the one-chain-per-wave kernel
    HIP_TRY(launch_steps(h, 0, 0, force_init ? 2 : 1));
  else
    HIP_TRY(launch_reinit(h->cfg, h->args, h->S, h->d_cases, force_init, h->stream));
  h->step_in_init = 0;
  return set_lag(h, 1);  // from now on the sweep tracks the acceptor's stale-cache offset
}

int pstat_reset_averages(pstat_handle *h) {
  if (!h) return fail(PSTAT_ERR_INVALID_ARG, "null handle");
  int rc = set_device(h);
  if (rc) return rc;
  const size_t C = (size_t)h->S.C;
  HIP_TRY(hipMemsetAsync(h->S.sums, 0, NSUMS * C * sizeof(double), h->stream));
  HIP_TRY(hipMemsetAsync(h->S.wnorm, 0, C * sizeof(double), h->stream));
  HIP_TRY(hipMemsetAsync(h->S.nacc_total, 0, C * sizeof(int64_t), h->stream));
  HIP_TRY(hipMemsetAsync(h->S.nanrej, 0, C * sizeof(int64_t), h->stream));
  h->steps_recorded = 0;
  return PSTAT_OK;
}

int pstat_reset_sampler(pstat_handle *h) {
  if (!h) return fail(PSTAT_ERR_INVALID_ARG, "null handle");
  int rc = set_device(h);
  if (rc) return rc;
  HIP_TRY(launch_reset_sampler(h->S, h->base.phi_step, h->base.theta_step, h->stream));
  h->step_in_init = 0;
  return PSTAT_OK;
}

int pstat_set_kT(pstat_handle *h, int32_t icase, double kT) {
  if (!h) return fail(PSTAT_ERR_INVALID_ARG, "null handle");
  if (!(kT > 0) || !std::isfinite(kT)) return fail(PSTAT_ERR_INVALID_ARG, "kT must be > 0");
  if (icase >= h->ncases) return fail(PSTAT_ERR_INVALID_ARG, "case %d out of range", icase);
  int rc = set_device(h);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));   // the host copy of the constants is re-uploaded
  for (int i = 0; i < h->ncases; ++i)
    if (icase < 0 || icase == i) h->cases[(size_t)i].kT = kT;
  HIP_TRY(hipMemcpy(h->d_cases, h->cases.data(), sizeof(CaseConst) * (size_t)h->ncases, hipMemcpyHostToDevice));
  return PSTAT_OK;
}

int pstat_restart_from_x0(pstat_handle *h, const double *x0, int64_t len, double dx0_phi, double dx0_theta) {
  if (!h || !x0) return fail(PSTAT_ERR_INVALID_ARG, "null argument");
  if (h->cfg.planar) return fail(PSTAT_ERR_UNSUPPORTED, "2D/mcmc_clustering_eap_chain.jl has no --x0: a planar chain starts uniform");
  if (len != 2 && len != 2 * h->base.n)
    return fail(PSTAT_ERR_INVALID_ARG, "Invalid input for 'x0': length %lld is neither 2 nor 2 * num-monomers",
                (long long)len);                                                      // inc/eap_chain.jl:77
  for (int64_t i = 0; i < len; ++i)
    if (!std::isfinite(x0[i])) return fail(PSTAT_ERR_INVALID_ARG, "non-finite x0[%lld]", (long long)i);
  if (!std::isfinite(dx0_phi) || !std::isfinite(dx0_theta)) return fail(PSTAT_ERR_INVALID_ARG, "non-finite dx0");
  int rc = set_device(h);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  double *d_x0 = nullptr;
  InitOpts io{1, x0[0], x0[1], dx0_phi, dx0_theta, nullptr};
  if (len != 2) {
    HIP_TRY(hipMalloc((void **)&d_x0, sizeof(double) * (size_t)len));
    hipError_t e = hipMemcpy(d_x0, x0, sizeof(double) * (size_t)len, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(d_x0); return fail(PSTAT_ERR_HIP, "copy of x0 failed: %s", hipGetErrorString(e)); }
    io.use_x0 = 2;
    io.x0_vec = d_x0;
  }
  hipError_t e = launch_init(h->cfg, h->args, h->S, h->d_cases, h->base.phi_step, h->base.theta_step, io, h->stream);
  if (e == hipSuccess && all_pairs(h->base.energy_type)) e = launch_steps(h, 0, 0);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (d_x0) (void)hipFree(d_x0);
  if (e != hipSuccess) return fail(PSTAT_ERR_HIP, "re-initialisation from x0 failed: %s", hipGetErrorString(e));
  h->steps_recorded = 0;
  h->step_in_init = 0;
  return set_lag(h, 0);
}

int pstat_scale_kT(pstat_handle *h, double mult) {
  if (!h) return fail(PSTAT_ERR_INVALID_ARG, "null handle");
  if (!(mult > 0) || !std::isfinite(mult)) return fail(PSTAT_ERR_INVALID_ARG, "kT multiplier must be > 0");
  int rc = set_device(h);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  for (int i = 0; i < h->ncases; ++i) h->cases[(size_t)i].kT = h->kT0[(size_t)i] * mult;
  HIP_TRY(hipMemcpy(h->d_cases, h->cases.data(), sizeof(CaseConst) * (size_t)h->ncases, hipMemcpyHostToDevice));
  return PSTAT_OK;
}

int pstat_reduce_device(pstat_handle *h, int32_t icase, double *dev_out) {
  if (!h || !dev_out) return fail(PSTAT_ERR_INVALID_ARG, "null argument");
  if (icase >= h->ncases) return fail(PSTAT_ERR_INVALID_ARG, "case %d out of range", icase);
  int rc = set_device(h);
  if (rc) return rc;
  const int64_t per = h->base.num_chains;
  const int64_t c0 = icase < 0 ? 0 : icase * per;
  const int64_t c1 = icase < 0 ? h->S.C : c0 + per;
  HIP_TRY(launch_reduce(h->S, c0, c1, h->steps_recorded, h->cfg.umbrella, h->d_cases, h->base.num_chains, h->base.n,
                        h->d_partial, dev_out, h->stream));
  return PSTAT_OK;
}

int pstat_reduce_host(pstat_handle *h, int32_t icase, double red_out[PSTAT_NRED]) {
  if (!h || !red_out) return fail(PSTAT_ERR_INVALID_ARG, "null argument");
  return reduce_to_host(h, icase, red_out);
}

int pstat_summary_from_reduction(const double red[PSTAT_NRED], int64_t steps_per_chain,
                                 pstat_summary *out) {
  if (!red || !out) return fail(PSTAT_ERR_INVALID_ARG, "null argument");
  std::memset(out, 0, sizeof *out);
  const double C = red[0];
  out->num_chains = (int64_t)std::llround(C);
  out->steps_per_chain = steps_per_chain;
  out->attempted_updates = C * (double)steps_per_chain;
  if (C < 1) return PSTAT_OK;
  for (int q = 0; q < PSTAT_NQ; ++q) {
    const double mean = red[1 + q] / C;
    double se = 0.0;
    if (C > 1) {
      double var = (red[1 + PSTAT_NQ + q] / C - mean * mean) * C / (C - 1);  // unbiased across-chain variance
      se = var > 0 ? std::sqrt(var / C) : 0.0;
    }
    if (q < PSTAT_NOBS) { out->avg[q] = mean; out->stderr_[q] = se; }
    else if (q == PSTAT_NOBS) { out->acceptance_ratio = mean; out->ar_stderr = se; }
    else { out->extra_avg[q - PSTAT_NOBS - 1] = mean; out->extra_stderr[q - PSTAT_NOBS - 1] = se; }
  }
  out->nan_rejects = (int64_t)std::llround(red[1 + 2 * PSTAT_NQ]);
  out->chains_collapsed = (int64_t)std::llround(red[2 + 2 * PSTAT_NQ]);
  return PSTAT_OK;
}

int pstat_summary_get(pstat_handle *h, int32_t icase, pstat_summary *out) {
  if (!h || !out) return fail(PSTAT_ERR_INVALID_ARG, "null argument");
  double red[PSTAT_NRED];
  int rc = reduce_to_host(h, icase, red);
  if (rc) return rc;
  return pstat_summary_from_reduction(red, h->steps_recorded, out);
}

int pstat_rolling(pstat_handle *h, int32_t icase, double avg_out[PSTAT_NOBS],
                  double stderr_out[PSTAT_NOBS]) {
  pstat_summary s;
  int rc = pstat_summary_get(h, icase, &s);
  if (rc) return rc;
  if (avg_out) std::memcpy(avg_out, s.avg, sizeof s.avg);
  if (stderr_out) std::memcpy(stderr_out, s.stderr_, sizeof s.stderr_);
  return PSTAT_OK;
}

int pstat_microstate(pstat_handle *h, int64_t chain, double out[7]) {
  if (!h || !out) return fail(PSTAT_ERR_INVALID_ARG, "null argument");
  if (chain < 0 || chain >= h->S.C) return fail(PSTAT_ERR_INVALID_ARG, "chain out of range");
  int rc = set_device(h);
  if (rc) return rc;
  // obs is [NOBS_STATE][C]: a strided gather of 7 doubles
  HIP_TRY(hipMemcpy2DAsync(out, sizeof(double), h->S.obs + chain, sizeof(double) * (size_t)h->S.C,
                           sizeof(double), 7, hipMemcpyDeviceToHost, h->stream));
  return sync_checked(h);
}

int pstat_chain_state(pstat_handle *h, int64_t chain, double *angles, double sums[PSTAT_NOBS],
                      int64_t counters[4], double steps[3], uint32_t rng[4]) {
  if (!h) return fail(PSTAT_ERR_INVALID_ARG, "null handle");
  if (chain < 0 || chain >= h->S.C) return fail(PSTAT_ERR_INVALID_ARG, "chain out of range");
  int rc = set_device(h);
  if (rc) return rc;
  const size_t C = (size_t)h->S.C, n = (size_t)h->base.n;
  rc = sync_checked(h);
  if (rc) return rc;
  if (angles) {
    std::unique_ptr<unsigned char[]> tmp(new (std::nothrow) unsigned char[2 * n * h->elem]);
    if (!tmp) return fail(PSTAT_ERR_NOMEM, "host allocation failed");
    HIP_TRY(hipMemcpy2D(tmp.get(), h->elem, (char *)h->S.ang + (size_t)chain * h->elem, C * h->elem,
                        h->elem, 2 * n, hipMemcpyDeviceToHost));
    // storage formats: pstat_math.h (radians | turns | lattice index); the ABI speaks radians
    for (size_t i = 0; i < 2 * n; ++i) angles[i] = load_angle(tmp.get(), (int64_t)i, h->elem, i < n);
  }
  if (sums) {
    double s[NSUMS];
    HIP_TRY(hipMemcpy2D(s, sizeof(double), h->S.sums + chain, C * sizeof(double), sizeof(double), NSUMS,
                        hipMemcpyDeviceToHost));
    sums_in_abi_order(s, 1, sums);
  }
  if (counters) {
    int64_t w[2];
    int64_t tot;
    HIP_TRY(hipMemcpy2D(w, sizeof(int64_t), h->S.win + chain, C * sizeof(int64_t), sizeof(int64_t), 2,
                        hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&tot, h->S.nacc_total + chain, sizeof tot, hipMemcpyDeviceToHost));
    counters[0] = tot; counters[1] = h->steps_recorded; counters[2] = w[0]; counters[3] = w[1];
  }
  if (steps) {
    HIP_TRY(hipMemcpy2D(steps, sizeof(double), h->S.stepsz + chain, C * sizeof(double), sizeof(double), 2,
                        hipMemcpyDeviceToHost));
    if (h->cfg.umbrella) HIP_TRY(hipMemcpy(&steps[2], h->S.wnorm + chain, sizeof(double), hipMemcpyDeviceToHost));
    else steps[2] = (double)h->steps_recorded;
  }
  if (rng)
    HIP_TRY(hipMemcpy2D(rng, sizeof(uint32_t), h->S.rng + chain, C * sizeof(uint32_t), sizeof(uint32_t), 4,
                        hipMemcpyDeviceToHost));
  return PSTAT_OK;
}

int pstat_chain_means(pstat_handle *h, int32_t icase, double *out) {
  if (!h || !out) return fail(PSTAT_ERR_INVALID_ARG, "null argument");
  if (icase >= h->ncases) return fail(PSTAT_ERR_INVALID_ARG, "case %d out of range", icase);
  int rc = set_device(h);
  if (rc) return rc;
  rc = sync_checked(h);
  if (rc) return rc;
  const size_t C = (size_t)h->S.C, per = (size_t)h->base.num_chains;
  const size_t c0 = icase < 0 ? 0 : (size_t)icase * per, m = icase < 0 ? C : per;
  try {
    std::vector<double> sums((size_t)NSUMS * m), wn(m);
    std::vector<int64_t> nacc(m);
    HIP_TRY(hipMemcpy2D(sums.data(), m * sizeof(double), h->S.sums + c0, C * sizeof(double), m * sizeof(double), NSUMS,
                        hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(nacc.data(), h->S.nacc_total + c0, m * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (h->cfg.umbrella) HIP_TRY(hipMemcpy(wn.data(), h->S.wnorm + c0, m * sizeof(double), hipMemcpyDeviceToHost));
    chain_means_host(sums.data(), h->cfg.umbrella ? wn.data() : nullptr, nacc.data(), h->steps_recorded, (int64_t)m, out);
  } catch (const std::bad_alloc &) {
    return fail(PSTAT_ERR_NOMEM, "host allocation failed");
  }
  return PSTAT_OK;
}

int pstat_chain_extras(pstat_handle *h, int64_t chain, double extra_sums[2], double extra_now[2]) {
  if (!h) return fail(PSTAT_ERR_INVALID_ARG, "null handle");
  if (chain < 0 || chain >= h->S.C) return fail(PSTAT_ERR_INVALID_ARG, "chain out of range");
  int rc = set_device(h);
  if (rc) return rc;
  const size_t C = (size_t)h->S.C;
  rc = sync_checked(h);
  if (rc) return rc;
  if (extra_sums)
    HIP_TRY(hipMemcpy2D(extra_sums, sizeof(double), h->S.sums + (size_t)S_C2 * C + chain, C * sizeof(double),
                        sizeof(double), 2, hipMemcpyDeviceToHost));
  if (extra_now) {
    HIP_TRY(hipMemcpy2D(extra_now, sizeof(double), h->S.obs + (size_t)OBS_C2 * C + chain, C * sizeof(double),
                        sizeof(double), 2, hipMemcpyDeviceToHost));
    extra_now[1] /= (double)(h->base.n > 1 ? h->base.n - 1 : 1);
  }
  return PSTAT_OK;
}

// checkpoint image: header, the cases' current kT, then the eleven state buffers in allocation order
struct CkptHeader {
  uint64_t magic;
  int32_t abi_version, header_bytes;
  int64_t n, C, ncases, steps_recorded, step_in_init;
  int32_t precision, chain_type, energy_type, rng, move_set, umbrella, do_flips, uniform_bits, lag;
  int32_t planar;               // 1: the image of a planar handle (pstat_create_planar); 0 in every other image
  uint64_t seed, chain_id0;     // case 0's
  uint64_t params_fnv;          // fingerprint of everything else a chain's continuation depends on (params_fingerprint)
};

// FNV-1a over the options that are not spelled out in the header: every case's physics scalars except its current kT
// (which the image carries and restore re-instates), its seed and first chain id, the kT it was created with, and the
// proposal / adaptation options.  A checkpoint continues exactly the run it was taken from, on a handle created with
// the same options -- anything else would silently be a different Markov chain wearing this one's averages.
static uint64_t params_fingerprint(const pstat_handle *h) {
  uint64_t f = 0xcbf29ce484222325ull;
  auto mix = [&](const void *p, size_t nbytes) {
    const unsigned char *q = (const unsigned char *)p;
    for (size_t i = 0; i < nbytes; ++i) { f ^= q[i]; f *= 0x100000001b3ull; }
  };
  for (size_t i = 0; i < h->cases.size(); ++i) {
    const CaseConst &c = h->cases[i];
    const double v[12] = {c.E0, c.K1, c.K2, c.mu, c.Fz, c.Fx, c.b, c.kappa, c.psi0, c.cluster_prob, c.cutoff_radius, h->kT0[i]};
    mix(v, sizeof v);
    mix(&c.seed, sizeof c.seed);
    mix(&c.chain_id0, sizeof c.chain_id0);
  }
  const double a[5] = {h->base.phi_step, h->base.theta_step, h->base.adj_lb, h->base.adj_ub, h->base.adj_scale};
  mix(a, sizeof a);
  mix(&h->base.steps_per_adjust, sizeof h->base.steps_per_adjust);
  mix(&h->base.num_chains, sizeof h->base.num_chains);
  return f;
}

static size_t checkpoint_bytes(const pstat_handle *h) {
  size_t need = sizeof(CkptHeader) + sizeof(double) * (size_t)h->ncases;
  for (size_t i = 0; i < kStateBuffers; ++i) need += h->bufs[i].bytes;
  return need;
}

int pstat_checkpoint(pstat_handle *h, void *buf, size_t *bytes) {
  if (!h || !bytes) return fail(PSTAT_ERR_INVALID_ARG, "null argument");
  const size_t need = checkpoint_bytes(h);
  if (!buf) { *bytes = need; return PSTAT_OK; }
  if (*bytes < need) { *bytes = need; return fail(PSTAT_ERR_TOO_SMALL, "checkpoint needs %zu bytes", need); }
  int rc = set_device(h);
  if (rc) return rc;
  rc = sync_checked(h);
  if (rc) return rc;
  CkptHeader hd{};
  hd.magic = CKPT_MAGIC; hd.abi_version = PSTAT_ABI_VERSION; hd.header_bytes = (int32_t)sizeof(CkptHeader);
  hd.n = h->base.n; hd.C = h->S.C; hd.ncases = h->ncases;
  hd.steps_recorded = h->steps_recorded; hd.step_in_init = h->step_in_init;
  hd.precision = h->base.precision; hd.chain_type = h->base.chain_type; hd.energy_type = h->base.energy_type;
  hd.rng = h->base.rng; hd.move_set = h->base.move_set; hd.umbrella = h->base.umbrella ? 1 : 0;
  hd.do_flips = h->base.do_flips ? 1 : 0; hd.uniform_bits = h->args.wide_eps ? 53 : 23; hd.lag = h->cfg.lag;
  hd.planar = h->cfg.planar;
  hd.seed = h->cases[0].seed; hd.chain_id0 = h->cases[0].chain_id0;
  hd.params_fnv = params_fingerprint(h);
  char *q = (char *)buf;
  std::memcpy(q, &hd, sizeof hd);
  q += sizeof hd;
  for (int i = 0; i < h->ncases; ++i, q += sizeof(double)) std::memcpy(q, &h->cases[(size_t)i].kT, sizeof(double));
  for (size_t i = 0; i < kStateBuffers; ++i) {
    HIP_TRY(hipMemcpy(q, h->bufs[i].ptr, h->bufs[i].bytes, hipMemcpyDeviceToHost));
    q += h->bufs[i].bytes;
  }
  *bytes = need;
  return PSTAT_OK;
}

int pstat_restore(pstat_handle *h, const void *buf, size_t bytes) {
  if (!h || !buf) return fail(PSTAT_ERR_INVALID_ARG, "null argument");
  if (bytes < sizeof(CkptHeader)) return fail(PSTAT_ERR_BAD_CHECKPOINT, "checkpoint is %zu bytes: not even a header", bytes);
  CkptHeader hd;
  std::memcpy(&hd, buf, sizeof hd);
  if (hd.magic != CKPT_MAGIC)
    return fail(PSTAT_ERR_BAD_CHECKPOINT, "not a checkpoint of this library version (magic %016llx)", (unsigned long long)hd.magic);
  if (hd.abi_version != PSTAT_ABI_VERSION || hd.header_bytes != (int32_t)sizeof(CkptHeader))
    return fail(PSTAT_ERR_BAD_CHECKPOINT, "checkpoint written under ABI version %d, this library is version %d", hd.abi_version,
                PSTAT_ABI_VERSION);
#define CKPT_SAME(field, mine, what)                                                                              \
  if ((long long)(hd.field) != (long long)(mine))                                                                 \
    return fail(PSTAT_ERR_BAD_CHECKPOINT, "checkpoint does not match this handle: %s is %lld in the checkpoint, " \
                "%lld here", what, (long long)(hd.field), (long long)(mine))
  CKPT_SAME(n, h->base.n, "num-monomers");
  CKPT_SAME(C, h->S.C, "the number of chains");
  CKPT_SAME(ncases, h->ncases, "the number of cases");
  CKPT_SAME(precision, h->base.precision, "precision");
  CKPT_SAME(chain_type, h->base.chain_type, "chain-type");
  CKPT_SAME(energy_type, h->base.energy_type, "energy-type");
  CKPT_SAME(rng, h->base.rng, "the generator (0 MWC64X, 1 xoshiro128++: the state words mean different things)");
  CKPT_SAME(move_set, h->base.move_set, "move_set (0 mcmc_eap_chain.jl, 1 mcmc_clustering_eap_chain.jl)");
  CKPT_SAME(umbrella, h->base.umbrella ? 1 : 0, "umbrella-sampling");
  CKPT_SAME(do_flips, h->base.do_flips ? 1 : 0, "do-flips");
  CKPT_SAME(uniform_bits, h->args.wide_eps ? 53 : 23, "uniform_bits");
  CKPT_SAME(planar, h->cfg.planar, "planar (1: a handle of pstat_create_planar, 0: of pstat_create)");
#undef CKPT_SAME
  if (hd.seed != h->cases[0].seed || hd.chain_id0 != h->cases[0].chain_id0)
    return fail(PSTAT_ERR_BAD_CHECKPOINT, "checkpoint does not match this handle: seed / chain_id0 %llu / %llu in the "
                "checkpoint, %llu / %llu here", (unsigned long long)hd.seed, (unsigned long long)hd.chain_id0,
                (unsigned long long)h->cases[0].seed, (unsigned long long)h->cases[0].chain_id0);
  if (hd.params_fnv != params_fingerprint(h))
    return fail(PSTAT_ERR_BAD_CHECKPOINT, "checkpoint does not match this handle: a physics scalar, a case's seed or chain "
                "ids, num-chains, or a proposal / adaptation option differs from the run it was taken from");
  const size_t need = checkpoint_bytes(h);
  if (bytes < need) return fail(PSTAT_ERR_BAD_CHECKPOINT, "checkpoint is truncated: %zu bytes, this handle's image has %zu", bytes, need);
  const char *q = (const char *)buf + sizeof hd;
  std::unique_ptr<double[]> kT(new (std::nothrow) double[(size_t)h->ncases]);
  if (!kT) return fail(PSTAT_ERR_NOMEM, "host allocation failed");
  for (int i = 0; i < h->ncases; ++i, q += sizeof(double)) {
    std::memcpy(&kT[(size_t)i], q, sizeof(double));
    if (!(kT[(size_t)i] > 0) || !std::isfinite(kT[(size_t)i]))
      return fail(PSTAT_ERR_BAD_CHECKPOINT, "checkpoint holds kT = %g for case %d", kT[(size_t)i], i);
  }
  int rc = set_device(h);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(h->stream));
  // the temperature of every case as it was when the image was taken (a rung of the burn-in ladder: pstat_scale_kT / pstat_set_kT)
  for (int i = 0; i < h->ncases; ++i) h->cases[(size_t)i].kT = kT[(size_t)i];
  HIP_TRY(hipMemcpy(h->d_cases, h->cases.data(), sizeof(CaseConst) * (size_t)h->ncases, hipMemcpyHostToDevice));
  for (size_t i = 0; i < kStateBuffers; ++i) {
    HIP_TRY(hipMemcpy(h->bufs[i].ptr, q, h->bufs[i].bytes, hipMemcpyHostToDevice));
    q += h->bufs[i].bytes;
  }
  h->steps_recorded = hd.steps_recorded;
  h->step_in_init = hd.step_in_init;
  return set_lag(h, hd.lag);
}

int pstat_launch_info_get(pstat_handle *h, pstat_launch_info *out) {
  if (!h || !out) return fail(PSTAT_ERR_INVALID_ARG, "null argument");
  int rc = set_device(h);
  if (rc) return rc;
  std::memset(out, 0, sizeof *out);
  const int lds = lds_bytes(h->cfg.home, h->cfg.precision, h->args);
  int bpc = 0;
  HIP_TRY(occupancy(h->kernel, lds, &bpc));
  std::snprintf(out->kernel, sizeof out->kernel, "%s", h->kernel.name);
  out->lds_bytes = lds;
  out->threads_per_block = 64;
  out->lanes_per_block = h->args.lanes;
  out->blocks = chain_per_lane(h->cfg.home) ? h->args.nblocks : h->S.C;
  out->packed_cases = h->args.packed;
  out->blocks_per_cu = bpc;
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, h->device));
  out->num_cus = prop.multiProcessorCount;
  return PSTAT_OK;
}

}  // extern "C"
