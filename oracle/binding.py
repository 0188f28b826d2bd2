"""ctypes binding for the CPU oracle (oracle/liboracle.so).

TEST INFRASTRUCTURE ONLY: import this from tests/, from __graft_entry__.smoke() and from
bench.py's cpu_baseline leg -- never from polymer_stats_amd/ (the product).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from dataclasses import dataclass, field

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "liboracle.so")

DIELECTRIC, POLAR = 0, 1
NONINTERACTING, INTERACTING, ISING, CUTOFF = 0, 1, 2, 3
RNG_MWC64X, RNG_XOSHIRO128PP = 0, 1
NOBS = 16
OBS_NAMES = ["r1", "r2", "r3", "r1sq", "r2sq", "r3sq", "rsq",
             "p1", "p2", "p3", "p1sq", "p2sq", "p3sq", "psq", "U", "Usq"]


class EapParams(C.Structure):
    _fields_ = [(k, C.c_double) for k in
                ("E0", "K1", "K2", "mu", "kT", "Fz", "Fx", "b",
                 "phi_step", "theta_step", "adj_lb", "adj_ub", "adj_scale")] + \
               [(k, C.c_int64) for k in
                ("n", "num_steps", "num_inits", "steps_per_adjust", "stepout")] + \
               [("seed", C.c_uint64)] + \
               [(k, C.c_int32) for k in
                ("chain_type", "energy_type", "do_flips", "force_init", "umbrella", "rng")] + \
               [(k, C.c_double) for k in
                ("bend_mod", "bend_angle", "cluster_prob", "x0_phi", "x0_theta", "dx0_phi", "dx0_theta")] + \
               [("burn_sched", C.c_double * 8), ("burn_in", C.c_int64),
                ("burn_nsched", C.c_int32), ("use_x0", C.c_int32), ("cutoff_radius", C.c_double),
                ("x0_vec", C.POINTER(C.c_double)), ("x0_len", C.c_int64),
                ("uniform_bits", C.c_int32), ("pad_", C.c_int32)]


class EapResult(C.Structure):
    _fields_ = [("sum", C.c_double * NOBS), ("norm", C.c_double),
                ("nacc_total", C.c_int64), ("nsteps_total", C.c_int64),
                ("phi_step", C.c_double), ("theta_step", C.c_double),
                ("r", C.c_double * 3), ("p", C.c_double * 3), ("U", C.c_double),
                ("rng", C.c_uint32 * 4), ("extra_sum", C.c_double * 2), ("nan_rejects", C.c_int64)]


class EapTrace(C.Structure):
    _fields_ = [("final_phi", C.POINTER(C.c_double)), ("final_theta", C.POINTER(C.c_double)),
                ("accepted", C.POINTER(C.c_uint8)),
                ("rolling_rows", C.POINTER(C.c_double)), ("traj_rows", C.POINTER(C.c_double)),
                ("max_rows", C.c_int64), ("rows_written", C.c_int64)]


class EapStepOut(C.Structure):
    _fields_ = [("rng", C.c_uint32 * 4), ("idx", C.c_int64), ("lower", C.c_int64), ("upper", C.c_int64),
                ("flipped", C.c_int32), ("flip_bit", C.c_int32), ("accept", C.c_int32), ("pad_", C.c_int32),
                ("ngrow", C.c_int64), ("phi_trial", C.c_double), ("theta_trial", C.c_double),
                ("d", C.c_double), ("eps", C.c_double), ("mag", C.c_double), ("log_alpha", C.c_double),
                ("U_cur", C.c_double), ("U_trial", C.c_double), ("usum_cur", C.c_double), ("usum_trial", C.c_double)]


class EapReinitOut(C.Structure):
    _fields_ = [("rng", C.c_uint32 * 4), ("adopt", C.c_int32), ("pad_", C.c_int32), ("eps", C.c_double), ("d", C.c_double),
                ("lag_out", C.c_double), ("U_cur", C.c_double), ("U_fresh", C.c_double), ("usum_cur", C.c_double),
                ("usum_fresh", C.c_double), ("mag", C.c_double)]


def build(force: bool = False) -> str:
    src = os.path.join(HERE, "eap_oracle.c")
    if force or not os.path.exists(LIB_PATH) or \
            (os.path.exists(src) and os.path.getmtime(src) > os.path.getmtime(LIB_PATH)):
        subprocess.check_call(["make", "-C", HERE, "-s"])
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(LIB_PATH)
        L.eap_philox4x32_10.argtypes = [C.POINTER(C.c_uint32)] * 3
        L.eap_rng_seed.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32)]
        L.eap_xoshiro128pp_next.argtypes = [C.POINTER(C.c_uint32)]
        L.eap_xoshiro128pp_next.restype = C.c_uint32
        L.eap_mwc64x_seed.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32)]
        L.eap_mwc64x_next.argtypes = [C.POINTER(C.c_uint32)]
        L.eap_mwc64x_next.restype = C.c_uint32
        L.eap_mwc64x_skip.argtypes = [C.c_uint64, C.c_uint64]
        L.eap_mwc64x_skip.restype = C.c_uint64
        L.eap_u01.argtypes = [C.c_uint32]
        L.eap_u01.restype = C.c_double
        L.eap_eps.argtypes = [C.c_int] + [C.c_uint32] * 4
        L.eap_eps.restype = C.c_double
        L.eap_find_eps23_zero.argtypes = [C.POINTER(EapParams), C.c_uint64, C.c_int64, C.POINTER(C.c_int64), C.c_int64]
        L.eap_find_eps23_zero.restype = C.c_int64
        for f in (L.eap_run_faithful, L.eap_run_fast, L.eap_run_cluster):
            f.argtypes = [C.POINTER(EapParams), C.c_uint64, C.POINTER(EapResult), C.POINTER(EapTrace)]
            f.restype = C.c_int
        L.eap_run_many.argtypes = [C.POINTER(EapParams), C.c_uint64, C.c_int64, C.c_int, C.c_int,
                                   C.POINTER(EapResult)]
        L.eap_run_many.restype = C.c_int
        L.eap_dipole.argtypes = [C.POINTER(EapParams)] + [C.c_double] * 4 + [C.POINTER(C.c_double)]
        L.eap_pair_energy.argtypes = [C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int]
        L.eap_pair_energy.restype = C.c_double
        L.eap_chain_energy.argtypes = [C.POINTER(EapParams)] + [C.POINTER(C.c_double)] * 4
        L.eap_chain_energy.restype = C.c_double
        dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint32)
        L.eap_step_judge.argtypes = [C.POINTER(EapParams), dp, dp, up, C.c_double, C.c_double, dp, C.POINTER(EapStepOut), dp, dp]
        L.eap_step_judge.restype = C.c_int
        L.eap_step_judge_cluster.argtypes = L.eap_step_judge.argtypes + [dp, C.c_int64]
        L.eap_step_judge_cluster.restype = C.c_int
        L.eap_reinit_judge.argtypes = [C.POINTER(EapParams), dp, dp, up, C.c_double, C.c_int, dp, dp, C.POINTER(EapReinitOut), dp, dp]
        L.eap_reinit_judge.restype = C.c_int
        L.eap_seed_state.argtypes = [C.POINTER(EapParams), C.c_uint64, up, dp, dp]
        L.eap_seed_state.restype = None
        L.eap_adapt.argtypes = [C.POINTER(EapParams), C.c_int64, dp, dp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.eap_adapt.restype = None
        _lib = L
    return _lib


def make_params(**kw) -> EapParams:
    """Defaults are the reference's option defaults (mcmc_eap_chain.jl:19-153)."""
    d = dict(E0=0.0, K1=1.0, K2=0.0, mu=1e-2, kT=1.0, Fz=0.0, Fx=0.0, b=1.0,
             phi_step=3 * np.pi / 8, theta_step=3 * np.pi / 16,
             adj_lb=0.15, adj_ub=0.55, adj_scale=1.1,
             n=100, num_steps=100000, num_inits=1, steps_per_adjust=2500, stepout=500,
             seed=0, chain_type=DIELECTRIC, energy_type=NONINTERACTING,
             do_flips=0, force_init=0, umbrella=0, rng=RNG_MWC64X,
             bend_mod=0.0, bend_angle=0.0, cluster_prob=1.0, x0_phi=0.0, x0_theta=0.0,
             dx0_phi=2 * np.pi, dx0_theta=0.1, burn_in=0, burn_nsched=0, use_x0=0, cutoff_radius=7.5,
             uniform_bits=0)      # 0 | 53: the Metropolis eps has 53 random bits (the f64 kernels' default); 23: the f32 one
    sched = list(kw.pop("burn_sched", []))
    x0_vec = kw.pop("x0_vec", None)
    unknown = set(kw) - set(d)
    if unknown:
        raise KeyError(f"unknown oracle parameter(s): {sorted(unknown)}")
    d.update(kw)
    if sched:
        d["burn_nsched"] = len(sched)
    p = EapParams(**d)
    for i, v in enumerate(sched):
        p.burn_sched[i] = v
    if x0_vec is not None:       # per-monomer start [phi1, theta1, phi2, theta2, ...]; keep the buffer alive on p
        p._x0_keep = np.ascontiguousarray(x0_vec, dtype=np.float64)
        p.x0_vec = p._x0_keep.ctypes.data_as(C.POINTER(C.c_double))
        p.x0_len = len(p._x0_keep)
        p.use_x0 = 1
    return p


@dataclass
class Run:
    sums: np.ndarray
    norm: float
    nacc_total: int
    nsteps_total: int
    phi_step: float
    theta_step: float
    r: np.ndarray
    p: np.ndarray
    U: float
    rng: np.ndarray
    final_phi: np.ndarray | None = None
    final_theta: np.ndarray | None = None
    accepted: np.ndarray | None = None
    rolling: np.ndarray | None = None
    traj: np.ndarray | None = None
    extra_sums: np.ndarray | None = None      # clustering main: sum cos^2(theta), mean psi
    nan_rejects: int = 0                      # proposals with a non-finite trial energy
    extra: dict = field(default_factory=dict)

    @property
    def avg(self) -> np.ndarray:
        return self.sums / self.norm

    @property
    def ar(self) -> float:
        return self.nacc_total / self.nsteps_total


def _unpack(res: EapResult) -> Run:
    return Run(sums=np.array(res.sum[:]), norm=res.norm, nacc_total=res.nacc_total,
               nsteps_total=res.nsteps_total, phi_step=res.phi_step, theta_step=res.theta_step,
               r=np.array(res.r[:]), p=np.array(res.p[:]), U=res.U, rng=np.array(res.rng[:], dtype=np.uint32),
               extra_sums=np.array(res.extra_sum[:]), nan_rejects=int(res.nan_rejects))


def run(params: EapParams, chain_id: int = 0, mode: str = "faithful", trace: bool = False,
        rows: bool = False) -> Run:
    L = lib()
    res = EapResult()
    tr = EapTrace()
    keep = {}
    if trace:
        keep["phi"] = np.zeros(params.n)
        keep["th"] = np.zeros(params.n)
        keep["acc"] = np.zeros(max(1, params.num_inits * params.num_steps + params.burn_nsched * params.burn_in),
                               dtype=np.uint8)
        tr.final_phi = keep["phi"].ctypes.data_as(C.POINTER(C.c_double))
        tr.final_theta = keep["th"].ctypes.data_as(C.POINTER(C.c_double))
        tr.accepted = keep["acc"].ctypes.data_as(C.POINTER(C.c_uint8))
    if rows and params.stepout > 0:
        nrows = params.num_inits * (params.num_steps // params.stepout)
        keep["roll"] = np.zeros((max(1, nrows), 17))
        keep["traj"] = np.zeros((max(1, nrows), 8))
        tr.rolling_rows = keep["roll"].ctypes.data_as(C.POINTER(C.c_double))
        tr.traj_rows = keep["traj"].ctypes.data_as(C.POINTER(C.c_double))
        tr.max_rows = nrows
    fn = {"faithful": L.eap_run_faithful, "fast": L.eap_run_fast, "cluster": L.eap_run_cluster}[mode]
    rc = fn(C.byref(params), chain_id, C.byref(res), C.byref(tr))
    if rc != 0:
        raise RuntimeError(f"oracle returned {rc}")
    out = _unpack(res)
    if trace:
        out.final_phi, out.final_theta, out.accepted = keep["phi"], keep["th"], keep["acc"]
    if rows and params.stepout > 0:
        out.rolling = keep["roll"][:tr.rows_written]
        out.traj = keep["traj"][:tr.rows_written]
    return out


def run_many(params: EapParams, id0: int, nchains: int, nthreads: int = 1, mode: str = "fast", extras: bool = False):
    """Returns (sums[nchains,16], norm[nchains], nacc[nchains]) for chain ids id0..id0+nchains-1
    (+ extra_sums[nchains,2], the clustering main's two more averagers, if `extras`)."""
    L = lib()
    arr = (EapResult * nchains)()
    rc = L.eap_run_many(C.byref(params), id0, nchains, nthreads, {"faithful": 0, "fast": 1, "cluster": 2}[mode], arr)
    if rc != 0:
        raise RuntimeError(f"oracle returned {rc}")
    sums = np.array([a.sum[:] for a in arr])
    norm = np.array([a.norm for a in arr])
    nacc = np.array([a.nacc_total for a in arr])
    if extras:
        return sums, norm, nacc, np.array([a.extra_sum[:] for a in arr])
    return sums, norm, nacc


def find_eps23_zero(params: EapParams, chain_id: int, nsteps: int, max_hits: int = 64):
    """0-based steps of the chain (fixed-force main, no flips, first init) whose Metropolis word has 23 leading zero bits."""
    hits = (C.c_int64 * max_hits)()
    k = lib().eap_find_eps23_zero(C.byref(params), chain_id, nsteps, hits, max_hits)
    return [int(hits[i]) for i in range(min(k, max_hits))]


def philox(ctr, key):
    c = (C.c_uint32 * 4)(*ctr)
    k = (C.c_uint32 * 2)(*key)
    o = (C.c_uint32 * 4)()
    lib().eap_philox4x32_10(c, k, o)
    return list(o)


def xoshiro_stream(seed: int, chain_id: int, count: int):
    s = (C.c_uint32 * 4)()
    lib().eap_rng_seed(seed, chain_id, s)
    init = list(s)
    return init, [lib().eap_xoshiro128pp_next(s) for _ in range(count)]


def mwc64x_stream(seed: int, chain_id: int, count: int):
    s = (C.c_uint32 * 4)()
    lib().eap_mwc64x_seed(seed, chain_id, s)
    init = (s[0], s[1])
    return init, [lib().eap_mwc64x_next(s) for _ in range(count)]


def pair_energy(xs: np.ndarray, mus: np.ndarray, ising: bool = False) -> float:
    """xs, mus: arrays of shape (n, 3)."""
    xs = np.ascontiguousarray(xs, dtype=np.float64)
    mus = np.ascontiguousarray(mus, dtype=np.float64)
    return lib().eap_pair_energy(xs.shape[0], xs.ctypes.data_as(C.POINTER(C.c_double)),
                                 mus.ctypes.data_as(C.POINTER(C.c_double)), int(ising))


def chain_energy(params: EapParams, phi: np.ndarray, theta: np.ndarray):
    phi = np.ascontiguousarray(phi, dtype=np.float64)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    r = np.zeros(3)
    p = np.zeros(3)
    dp = C.POINTER(C.c_double)
    U = lib().eap_chain_energy(C.byref(params), phi.ctypes.data_as(dp), theta.ctypes.data_as(dp),
                               r.ctypes.data_as(dp), p.ctypes.data_as(dp))
    return U, r, p


@dataclass
class Step:
    """One judged step (eap_step_out): see oracle/eap_oracle.h for the meaning of every field."""
    rng: np.ndarray            # generator words after the step
    idx: int
    lower: int
    upper: int
    flipped: bool
    flip_bit: bool
    accept: bool
    phi_trial: float
    theta_trial: float
    d: float
    eps: float
    mag: float
    log_alpha: float
    U_cur: float
    U_trial: float
    usum_cur: float            # sum(us) of both chains
    usum_trial: float
    trial_phi: np.ndarray      # [n] every angle of the trial chain
    trial_theta: np.ndarray
    grow: np.ndarray           # [ngrow, 3]: draw, link probability, draw - probability


def step_judge(params: EapParams, phi, theta, rng, phi_step: float, theta_step: float, cluster: bool = False,
               moved_to=None) -> Step:
    """One step of the fixed-force main (or of the clustering main) from an explicit state, judged in f64.
    moved_to = (phi', theta'): where the single move puts its monomer, in place of the step's own displacement."""
    L = lib()
    n = params.n
    phi = np.ascontiguousarray(phi, dtype=np.float64)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    assert phi.shape == (n,) and theta.shape == (n,)
    words = (C.c_uint32 * 4)(*[int(w) for w in rng])
    out = EapStepOut()
    tphi, tth = np.empty(n), np.empty(n)
    dp = C.POINTER(C.c_double)
    to = None if moved_to is None else (C.c_double * 2)(float(moved_to[0]), float(moved_to[1]))
    args = [C.byref(params), phi.ctypes.data_as(dp), theta.ctypes.data_as(dp), words, float(phi_step), float(theta_step),
            to, C.byref(out), tphi.ctypes.data_as(dp), tth.ctypes.data_as(dp)]
    if cluster:
        grow = np.zeros((n + 2, 3))
        rc = L.eap_step_judge_cluster(*args, grow.ctypes.data_as(dp), grow.shape[0])
    else:
        grow = np.zeros((0, 3))
        rc = L.eap_step_judge(*args)
    if rc != 0:
        raise RuntimeError(f"oracle returned {rc}")
    return Step(rng=np.array(out.rng[:], dtype=np.uint32), idx=out.idx, lower=out.lower, upper=out.upper,
                flipped=bool(out.flipped), flip_bit=bool(out.flip_bit), accept=bool(out.accept),
                phi_trial=out.phi_trial, theta_trial=out.theta_trial, d=out.d, eps=out.eps, mag=out.mag,
                log_alpha=out.log_alpha, U_cur=out.U_cur, U_trial=out.U_trial, usum_cur=out.usum_cur,
                usum_trial=out.usum_trial, trial_phi=tphi, trial_theta=tth,
                grow=grow[:out.ngrow])


@dataclass
class Reinit:
    """One judged re-init (eap_reinit_out): see oracle/eap_oracle.h for the meaning of every field."""
    rng: np.ndarray            # generator words after the draws
    adopt: bool
    forced: bool
    eps: float
    d: float
    lag_in: float
    lag_out: float
    U_cur: float
    U_fresh: float
    usum_cur: float
    usum_fresh: float
    mag: float
    fresh_phi: np.ndarray      # [n] the fresh configuration
    fresh_theta: np.ndarray


def reinit_judge(params: EapParams, phi, theta, rng, lag_in: float = 0.0, force: bool = False, fresh_to=None) -> Reinit:
    """One re-init of the fixed-force main (mcmc_eap_chain.jl:352-361) from an explicit state, judged in f64.
    fresh_to = (phi[n], theta[n]): angles that stand in for the fresh draw's (every word is still drawn)."""
    n = params.n
    phi = np.ascontiguousarray(phi, dtype=np.float64)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    assert phi.shape == (n,) and theta.shape == (n,)
    words = (C.c_uint32 * 4)(*[int(w) for w in rng])
    out = EapReinitOut()
    fphi, fth = np.empty(n), np.empty(n)
    dp = C.POINTER(C.c_double)
    tp = tt = None
    if fresh_to is not None:
        keep = [np.ascontiguousarray(a, dtype=np.float64) for a in fresh_to]
        assert keep[0].shape == (n,) and keep[1].shape == (n,)
        tp, tt = keep[0].ctypes.data_as(dp), keep[1].ctypes.data_as(dp)
    rc = lib().eap_reinit_judge(C.byref(params), phi.ctypes.data_as(dp), theta.ctypes.data_as(dp), words, float(lag_in),
                                int(bool(force)), tp, tt, C.byref(out), fphi.ctypes.data_as(dp), fth.ctypes.data_as(dp))
    if rc != 0:
        raise RuntimeError(f"oracle returned {rc}")
    return Reinit(rng=np.array(out.rng[:], dtype=np.uint32), adopt=bool(out.adopt), forced=bool(force), eps=out.eps, d=out.d,
                  lag_in=float(lag_in), lag_out=out.lag_out, U_cur=out.U_cur, U_fresh=out.U_fresh, usum_cur=out.usum_cur,
                  usum_fresh=out.usum_fresh, mag=out.mag, fresh_phi=fphi, fresh_theta=fth)


def seed_state(params: EapParams, chain_id: int = 0):
    """(phi[n], theta[n], rng[4]) of the seeded start of a chain: what every run of the oracle begins from."""
    n = params.n
    phi, th = np.empty(n), np.empty(n)
    words = (C.c_uint32 * 4)()
    dp = C.POINTER(C.c_double)
    lib().eap_seed_state(C.byref(params), chain_id, words, phi.ctypes.data_as(dp), th.ctypes.data_as(dp))
    return phi, th, np.array(words[:], dtype=np.uint32)


def adapt(params: EapParams, step: int, phi_step: float, theta_step: float, nacc: int, natt: int):
    """The step-size adaptation after in-run step `step` (1-based): returns (phi_step, theta_step, nacc, natt)."""
    a, b = C.c_double(phi_step), C.c_double(theta_step)
    k, m = C.c_int64(nacc), C.c_int64(natt)
    lib().eap_adapt(C.byref(params), step, C.byref(a), C.byref(b), C.byref(k), C.byref(m))
    return a.value, b.value, k.value, m.value
