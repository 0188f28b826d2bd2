"""ctypes binding of libpstat.so (include/pstat.h).  No CPU fallback: if the HIP library is missing
or no GPU is visible, calls fail loudly."""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# PSTAT_LIB: another build of the same library (kernel experiments: tools/build_variant.sh); never needed in production
LIB_PATH = os.environ.get("PSTAT_LIB") or os.path.join(HERE, "libpstat.so")

DIELECTRIC, POLAR = 0, 1
NONINTERACTING, INTERACTING, ISING, CUTOFF = 0, 1, 2, 3
F32, F64, Q16 = 0, 1, 2
RNG_MWC64X, RNG_XOSHIRO128PP = 0, 1
NOBS = 16
NQ = 19
NX = 2
NRED = 1 + 2 * NQ + NX
MWC64X_MAX_CHAINS = 1 << 22
MOVES_SINGLE, MOVES_CLUSTER = 0, 1
SERIES_ANGLES = 1
OBS_NAMES = ["r1", "r2", "r3", "r1sq", "r2sq", "r3sq", "rsq",
             "p1", "p2", "p3", "p1sq", "p2sq", "p3sq", "psq", "U", "Usq"]
# the planar main's rolling.csv columns after "step" (2D/mcmc_clustering_eap_chain.jl:230) and where each sits in the
# 16-vector: component 1 in the x slots, component 2 in the z slots, the y slots exactly 0
PLANAR_OBS_NAMES = ["r1", "r3", "r1sq", "r3sq", "rsq", "p1", "p3", "p1sq", "p3sq", "psq", "U", "Usq"]
PLANAR_OBS_INDEX = [OBS_NAMES.index(k) for k in PLANAR_OBS_NAMES]
# blocked standard errors (pstat_series_error_bars, pstat_blocking_device): the columns of a series' error bars, the six
# doubles per column in the order of the PSTAT_EB_* enum, and the kernel's bounds
EB_NAMES = OBS_NAMES + ["AR", "cos2", "psi"]
EB_FIELDS = ["mean", "stderr", "stderr_err", "inefficiency", "level", "converged"]
BLOCK_LEVELS = 24
BLOCK_MAX_BATCHES = 40960
# histogram channels (pstat_hist_*, the PSTAT_HC_* enum): the seven doubles of a microstate, then |r| and |p|
HC_NAMES = ["r1", "r2", "r3", "p1", "p2", "p3", "U", "rmag", "pmag"]
HIST_MAX_BINS = 8192
HIST_MAX_SPECS = 16
# correlation channels (pstat_corr_*): bit i of the PSTAT_CORR_* mask is CORR_NAMES[i]; columns come in this order
CORR_NAMES = ("nn", "zz", "mm")
# the gyration block of a shape object (pstat_shape_*): its first PSTAT_SHAPE_GYR columns, in this order; S(q) columns follow
SHAPE_NAMES = ("gxx", "gyy", "gzz", "gxy", "gxz", "gyz", "rg2", "trg2")
SHAPE_MAX_Q = 512
# a pair-distance object (pstat_pdist_*): its column families in column order, and the library's limits
PDIST_NAMES = ("msd", "rmin", "hist", "sq")
PDIST_MAX_Q = 64
PDIST_MAX_BINS = 512
# an energy object (pstat_energy_*): its first three columns, in this order; pair[1 .. max_sep], rest and (with a cutoff) within follow
ENERGY_NAMES = ("field", "work", "bend")

# every symbol include/pstat.h declares (tests check the built library exports all of them)
SYMBOLS = [
    "pstat_abi_version", "pstat_strerror", "pstat_last_error", "pstat_device_count",
    "pstat_default_params", "pstat_create", "pstat_destroy", "pstat_advance", "pstat_sync",
    "pstat_reinit", "pstat_reset_averages", "pstat_set_kT", "pstat_scale_kT", "pstat_reset_sampler", "pstat_reduce_device", "pstat_reduce_host", "pstat_rolling", "pstat_microstate",
    "pstat_summary_get", "pstat_summary_from_reduction", "pstat_chain_state", "pstat_chain_extras", "pstat_restart_from_x0",
    "pstat_checkpoint", "pstat_restore", "pstat_launch_info_get", "pstat_chain_means",
    "pstat_series_open", "pstat_advance_series", "pstat_series_read", "pstat_series_clear", "pstat_series_close",
    "pstat_create_planar", "pstat_series_error_bars", "pstat_blocking_device",
    "pstat_tempering_open", "pstat_tempering_exchange", "pstat_tempering_stats", "pstat_tempering_close",
    "pstat_hist_open", "pstat_hist_record", "pstat_advance_hist", "pstat_hist_read", "pstat_hist_clear", "pstat_hist_close",
    "pstat_histogram_device",
    "pstat_corr_open", "pstat_corr_record", "pstat_advance_corr", "pstat_corr_read", "pstat_corr_rows", "pstat_corr_clear",
    "pstat_corr_close",
    "pstat_shape_open", "pstat_shape_record", "pstat_advance_shape", "pstat_shape_read", "pstat_shape_rows", "pstat_shape_clear",
    "pstat_shape_close",
    "pstat_pdist_open", "pstat_pdist_record", "pstat_advance_pdist", "pstat_pdist_read", "pstat_pdist_rows", "pstat_pdist_clear",
    "pstat_pdist_close",
    "pstat_energy_open", "pstat_energy_record", "pstat_advance_energy", "pstat_energy_read", "pstat_energy_rows", "pstat_energy_clear",
    "pstat_energy_close",
]
ABI_VERSION = 6


class PstatError(RuntimeError):
    def __init__(self, code: int, what: str, detail: str):
        super().__init__(f"libpstat: {what} ({code}): {detail}")
        self.code = code


class Params(C.Structure):
    _fields_ = [(k, C.c_double) for k in
                ("E0", "K1", "K2", "mu", "kT", "Fz", "Fx", "b",
                 "phi_step", "theta_step", "adj_lb", "adj_ub", "adj_scale")] + \
               [("steps_per_adjust", C.c_int64), ("n", C.c_int64), ("num_chains", C.c_int64),
                ("seed", C.c_uint64), ("chain_id0", C.c_uint64)] + \
               [(k, C.c_int32) for k in
                ("chain_type", "energy_type", "do_flips", "umbrella", "precision", "device", "rng", "move_set")] + \
               [(k, C.c_double) for k in
                ("bend_mod", "bend_angle", "cluster_prob", "x0_phi", "x0_theta", "dx0_phi", "dx0_theta")] + \
               [("use_x0", C.c_int32), ("uniform_bits", C.c_int32), ("cutoff_radius", C.c_double)]


class Summary(C.Structure):
    _fields_ = [("avg", C.c_double * NOBS), ("stderr", C.c_double * NOBS),
                ("acceptance_ratio", C.c_double), ("ar_stderr", C.c_double),
                ("num_chains", C.c_int64), ("steps_per_chain", C.c_int64),
                ("attempted_updates", C.c_double),
                ("extra_avg", C.c_double * 2), ("extra_stderr", C.c_double * 2),
                ("nan_rejects", C.c_int64), ("chains_collapsed", C.c_int64)]


class HistSpec(C.Structure):
    _fields_ = [("channel", C.c_int32), ("nbins", C.c_int32), ("lo", C.c_double), ("hi", C.c_double)]


class PdistSpec(C.Structure):
    _fields_ = [("max_sep", C.c_int32), ("min_sep", C.c_int32), ("nbins", C.c_int32), ("nq", C.c_int32), ("rmax", C.c_double)]


class EnergySpec(C.Structure):
    _fields_ = [("max_sep", C.c_int32), ("reserved", C.c_int32), ("cutoff", C.c_double)]


def hist_spec(channel, nbins: int, lo: float, hi: float) -> HistSpec:
    """One histogram spec: `channel` a name of HC_NAMES or an index (a column index for histogram_device), `nbins` bins of
    the formula bin = int((x - lo) * (nbins / (hi - lo)))."""
    if isinstance(channel, str):
        if channel not in HC_NAMES:
            raise ValueError(f"unknown histogram channel {channel!r}: one of {', '.join(HC_NAMES)}")
        channel = HC_NAMES.index(channel)
    return HistSpec(int(channel), int(nbins), float(lo), float(hi))


class LaunchInfo(C.Structure):
    _fields_ = [("kernel", C.c_char * 64), ("lds_bytes", C.c_int32), ("threads_per_block", C.c_int32),
                ("lanes_per_block", C.c_int32), ("blocks", C.c_int64), ("blocks_per_cu", C.c_int32),
                ("num_cus", C.c_int32), ("packed_cases", C.c_int32), ("reserved", C.c_int32)]


_lib = None


def load():
    """Loads libpstat.so (built by `make -C polymer_stats_amd/csrc` / __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `make -C polymer_stats_amd/csrc` "
                          "(there is no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, dp = C.c_void_p, C.c_int32, C.c_int64, C.POINTER(C.c_double)
    L.pstat_abi_version.restype = C.c_int
    L.pstat_strerror.argtypes = [C.c_int]
    L.pstat_strerror.restype = C.c_char_p
    L.pstat_last_error.restype = C.c_char_p
    L.pstat_device_count.restype = C.c_int
    L.pstat_default_params.argtypes = [C.POINTER(Params)]
    L.pstat_default_params.restype = None
    L.pstat_create.argtypes = [C.POINTER(Params), i32, vp, C.POINTER(vp)]
    L.pstat_create_planar.argtypes = [C.POINTER(Params), i32, vp, C.POINTER(vp)]
    L.pstat_destroy.argtypes = [vp]
    L.pstat_destroy.restype = None
    L.pstat_advance.argtypes = [vp, i64]
    L.pstat_sync.argtypes = [vp]
    L.pstat_reinit.argtypes = [vp, i32]
    L.pstat_reset_averages.argtypes = [vp]
    L.pstat_set_kT.argtypes = [vp, i32, C.c_double]
    L.pstat_reset_sampler.argtypes = [vp]
    L.pstat_scale_kT.argtypes = [vp, C.c_double]
    L.pstat_restart_from_x0.argtypes = [vp, dp, i64, C.c_double, C.c_double]
    L.pstat_chain_extras.argtypes = [vp, i64, dp, dp]
    L.pstat_reduce_device.argtypes = [vp, i32, vp]
    L.pstat_reduce_host.argtypes = [vp, i32, dp]
    L.pstat_rolling.argtypes = [vp, i32, dp, dp]
    L.pstat_microstate.argtypes = [vp, i64, dp]
    L.pstat_summary_get.argtypes = [vp, i32, C.POINTER(Summary)]
    L.pstat_summary_from_reduction.argtypes = [dp, i64, C.POINTER(Summary)]
    L.pstat_chain_state.argtypes = [vp, i64, dp, dp, C.POINTER(C.c_int64), dp, C.POINTER(C.c_uint32)]
    L.pstat_checkpoint.argtypes = [vp, vp, C.POINTER(C.c_size_t)]
    L.pstat_restore.argtypes = [vp, vp, C.c_size_t]
    L.pstat_launch_info_get.argtypes = [vp, C.POINTER(LaunchInfo)]
    L.pstat_chain_means.argtypes = [vp, i32, dp]
    L.pstat_series_open.argtypes = [vp, i64, i32, C.POINTER(vp)]
    L.pstat_advance_series.argtypes = [vp, vp, i64, i64]
    L.pstat_series_read.argtypes = [vp, vp, i64, C.POINTER(C.c_int64), dp, dp, dp]
    L.pstat_series_clear.argtypes = [vp, vp]
    L.pstat_series_close.argtypes = [vp, vp]
    L.pstat_series_close.restype = None
    L.pstat_series_error_bars.argtypes = [vp, vp, i64, i64, i32, C.POINTER(C.c_int64), dp, dp]
    L.pstat_blocking_device.argtypes = [vp, i64, i64, i64, i32, i32, vp, dp, dp]
    L.pstat_tempering_open.argtypes = [vp, C.POINTER(C.c_int32), C.c_uint64, C.POINTER(vp)]
    L.pstat_tempering_exchange.argtypes = [vp, vp]
    L.pstat_tempering_stats.argtypes = [vp, vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.pstat_tempering_close.argtypes = [vp, vp]
    L.pstat_tempering_close.restype = None
    ip = C.POINTER(C.c_int64)
    L.pstat_hist_open.argtypes = [vp, C.POINTER(HistSpec), i32, i32, C.POINTER(vp)]
    L.pstat_hist_record.argtypes = [vp, vp]
    L.pstat_advance_hist.argtypes = [vp, vp, i64, i64]
    L.pstat_hist_read.argtypes = [vp, vp, ip, ip, ip]
    L.pstat_hist_clear.argtypes = [vp, vp]
    L.pstat_hist_close.argtypes = [vp, vp]
    L.pstat_hist_close.restype = None
    L.pstat_histogram_device.argtypes = [vp, i64, i64, C.POINTER(HistSpec), i32, i32, vp, ip, ip]
    dp = C.POINTER(C.c_double)
    L.pstat_corr_open.argtypes = [vp, i32, i32, i64, C.POINTER(vp)]
    L.pstat_corr_record.argtypes = [vp, vp]
    L.pstat_advance_corr.argtypes = [vp, vp, i64, i64]
    L.pstat_corr_read.argtypes = [vp, vp, dp, dp, ip]
    L.pstat_corr_rows.argtypes = [vp, vp, C.POINTER(vp), ip, ip]
    L.pstat_corr_clear.argtypes = [vp, vp]
    L.pstat_corr_close.argtypes = [vp, vp]
    L.pstat_corr_close.restype = None
    L.pstat_shape_open.argtypes = [vp, dp, i32, i64, C.POINTER(vp)]
    L.pstat_shape_record.argtypes = [vp, vp]
    L.pstat_advance_shape.argtypes = [vp, vp, i64, i64]
    L.pstat_shape_read.argtypes = [vp, vp, dp, dp, ip]
    L.pstat_shape_rows.argtypes = [vp, vp, C.POINTER(vp), ip, ip]
    L.pstat_shape_clear.argtypes = [vp, vp]
    L.pstat_shape_close.argtypes = [vp, vp]
    L.pstat_shape_close.restype = None
    L.pstat_pdist_open.argtypes = [vp, C.POINTER(PdistSpec), dp, dp, i64, C.POINTER(vp)]
    L.pstat_pdist_record.argtypes = [vp, vp]
    L.pstat_advance_pdist.argtypes = [vp, vp, i64, i64]
    L.pstat_pdist_read.argtypes = [vp, vp, dp, dp, ip]
    L.pstat_pdist_rows.argtypes = [vp, vp, C.POINTER(vp), ip, ip]
    L.pstat_pdist_clear.argtypes = [vp, vp]
    L.pstat_pdist_close.argtypes = [vp, vp]
    L.pstat_pdist_close.restype = None
    L.pstat_energy_open.argtypes = [vp, C.POINTER(EnergySpec), dp, i64, C.POINTER(vp)]
    L.pstat_energy_record.argtypes = [vp, vp]
    L.pstat_advance_energy.argtypes = [vp, vp, i64, i64]
    L.pstat_energy_read.argtypes = [vp, vp, dp, dp, ip]
    L.pstat_energy_rows.argtypes = [vp, vp, C.POINTER(vp), ip, ip]
    L.pstat_energy_clear.argtypes = [vp, vp]
    L.pstat_energy_close.argtypes = [vp, vp]
    L.pstat_energy_close.restype = None
    if L.pstat_abi_version() != ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has ABI version {L.pstat_abi_version()}, this binding needs {ABI_VERSION}: "
                          "rebuild it with `make -C polymer_stats_amd/csrc`")
    _lib = L
    return L


def check(rc: int):
    if rc != 0:
        L = load()
        raise PstatError(rc, L.pstat_strerror(rc).decode(), L.pstat_last_error().decode())


def default_params(**kw) -> Params:
    p = Params()
    load().pstat_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def default_planar_params(**kw) -> Params:
    """Option defaults of the planar main (2D/mcmc_clustering_eap_chain.jl:15-129) for Ensemble(..., planar=True): those of
    default_params except --step-adjust-ub 0.40."""
    return default_params(**{"adj_ub": 0.40, **kw})
