"""ctypes binding of the planar restatement (tests/planar/planar_ref.c).

TEST INFRASTRUCTURE ONLY: import this from tests/ and from measuring tools -- never from polymer_stats_amd/.
The library is built with `gcc -O2` into a temporary directory on first use.
"""
from __future__ import annotations

import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile
from dataclasses import dataclass

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

DIELECTRIC, POLAR = 0, 1
NONINTERACTING, INTERACTING, ISING = 0, 1, 2
RNG_MWC64X, RNG_XOSHIRO128PP = 0, 1
NOBS = 16


class PlanarParams(C.Structure):
    _fields_ = [(k, C.c_double) for k in
                ("E0", "K1", "K2", "mu", "kT", "Fz", "Fx", "b", "phi_step", "adj_lb", "adj_ub", "adj_scale",
                 "cluster_prob")] + \
               [("n", C.c_int64), ("num_steps", C.c_int64), ("steps_per_adjust", C.c_int64), ("seed", C.c_uint64)] + \
               [(k, C.c_int32) for k in ("chain_type", "energy_type", "umbrella", "rng", "uniform_bits", "pad_")]


class PlanarResult(C.Structure):
    _fields_ = [("sum", C.c_double * NOBS), ("norm", C.c_double), ("nacc_total", C.c_int64), ("words", C.c_int64),
                ("flips_proposed", C.c_int64), ("link_tests", C.c_int64), ("phi_step", C.c_double),
                ("r", C.c_double * 2), ("p", C.c_double * 2), ("U", C.c_double), ("rng", C.c_uint32 * 4),
                ("nacc_window", C.c_int64), ("natt_window", C.c_int64)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        tmp = tempfile.mkdtemp(prefix="planar_ref_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        so = os.path.join(tmp, "libplanar_ref.so")
        subprocess.check_call(["gcc", "-O2", "-std=c11", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Werror",
                               os.path.join(HERE, "planar_ref.c"), "-o", so, "-lm"])
        L = C.CDLL(so)
        dp, u32p = C.POINTER(C.c_double), C.POINTER(C.c_uint32)
        L.planar_run.argtypes = [C.POINTER(PlanarParams), C.c_uint64, dp, u32p, C.POINTER(PlanarResult), dp]
        L.planar_run.restype = C.c_int
        L.planar_dipole.argtypes = [C.POINTER(PlanarParams), C.c_double, dp]
        L.planar_dipole.restype = None
        L.planar_energy.argtypes = [C.POINTER(PlanarParams), dp, dp, dp, dp]
        L.planar_energy.restype = C.c_double
        L.planar_cluster_flip_u.argtypes = [C.POINTER(PlanarParams), dp, C.c_int64, dp, C.c_int, C.POINTER(C.c_int64),
                                            C.POINTER(C.c_int64), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.planar_cluster_flip_u.restype = C.c_double
        L.planar_eps.argtypes = [C.c_int] + [C.c_uint32] * 4
        L.planar_eps.restype = C.c_double
        L.planar_seed.argtypes = [C.POINTER(PlanarParams), C.c_uint64, u32p]
        L.planar_seed.restype = None
        L.planar_next.argtypes = [C.c_int, u32p]
        L.planar_next.restype = C.c_uint32
        _lib = L
    return _lib


def make_params(**kw) -> PlanarParams:
    """Defaults are the option defaults of 2D/mcmc_clustering_eap_chain.jl:15-129."""
    d = dict(E0=0.0, K1=1.0, K2=0.0, mu=1e-2, kT=1.0, Fz=0.0, Fx=0.0, b=1.0, phi_step=3 * np.pi / 8,
             adj_lb=0.15, adj_ub=0.40, adj_scale=1.1, cluster_prob=0.5, n=100, num_steps=1000000,
             steps_per_adjust=2500, seed=0, chain_type=DIELECTRIC, energy_type=NONINTERACTING, umbrella=0,
             rng=RNG_MWC64X, uniform_bits=0)
    unknown = set(kw) - set(d)
    if unknown:
        raise KeyError(f"unknown planar parameter(s): {sorted(unknown)}")
    d.update(kw)
    return PlanarParams(**d)


@dataclass
class Run:
    sums: np.ndarray
    norm: float
    nacc_total: int
    words: int
    flips_proposed: int
    link_tests: int
    phi_step: float
    r: np.ndarray
    p: np.ndarray
    U: float
    rng: np.ndarray
    nacc_window: int
    natt_window: int
    final_phi: np.ndarray

    @property
    def avg(self) -> np.ndarray:
        return self.sums / self.norm

    @property
    def microstate(self) -> np.ndarray:
        """[r1, 0, r3, p1, 0, p3, U]: what pstat_microstate returns for a planar handle."""
        return np.array([self.r[0], 0.0, self.r[1], self.p[0], 0.0, self.p[1], self.U])


def run(params: PlanarParams, chain_id: int = 0, phi0=None, rng0=None) -> Run:
    """One mcmc() call of the planar main; `phi0`, `rng0`: start from a carried chain instead of drawing one."""
    res = PlanarResult()
    fin = np.zeros(params.n)
    dp, u32p = C.POINTER(C.c_double), C.POINTER(C.c_uint32)
    a = r = None
    if phi0 is not None:
        a = np.ascontiguousarray(phi0, dtype=np.float64)
        r = np.ascontiguousarray(rng0, dtype=np.uint32)
        assert a.shape == (params.n,) and r.shape == (4,)
    rc = lib().planar_run(C.byref(params), chain_id, a.ctypes.data_as(dp) if a is not None else None,
                          r.ctypes.data_as(u32p) if r is not None else None, C.byref(res), fin.ctypes.data_as(dp))
    if rc != 0:
        raise RuntimeError(f"planar_run returned {rc}")
    return Run(sums=np.array(res.sum[:]), norm=res.norm, nacc_total=res.nacc_total, words=res.words,
               flips_proposed=res.flips_proposed, link_tests=res.link_tests, phi_step=res.phi_step,
               r=np.array(res.r[:]), p=np.array(res.p[:]), U=res.U, rng=np.array(res.rng[:], dtype=np.uint32),
               nacc_window=res.nacc_window, natt_window=res.natt_window, final_phi=fin)


def dipole(params: PlanarParams, phi: float) -> np.ndarray:
    mu = np.zeros(2)
    lib().planar_dipole(C.byref(params), float(phi), mu.ctypes.data_as(C.POINTER(C.c_double)))
    return mu


def energy(params: PlanarParams, phi):
    """(U, r[2], p[2], sum(u)) of the chain phi[n]."""
    a = np.ascontiguousarray(phi, dtype=np.float64)
    assert a.shape == (params.n,)
    r, p, us = np.zeros(2), np.zeros(2), C.c_double(0)
    dp = C.POINTER(C.c_double)
    U = lib().planar_energy(C.byref(params), a.ctypes.data_as(dp), r.ctypes.data_as(dp), p.ctypes.data_as(dp), C.byref(us))
    return U, r, p, us.value


def cluster_flip(params: PlanarParams, phi, idx: int, uniforms):
    """cluster_flip! from monomer idx (0-based) with the given uniforms in contract order (flip draw first).
    Returns (alpha, phi_after, lower, upper, flipped, uniforms_used)."""
    a = np.array(phi, dtype=np.float64)
    u = np.ascontiguousarray(uniforms, dtype=np.float64)
    lo, up, fl, used = C.c_int64(0), C.c_int64(0), C.c_int(0), C.c_int(0)
    dp = C.POINTER(C.c_double)
    alpha = lib().planar_cluster_flip_u(C.byref(params), a.ctypes.data_as(dp), idx, u.ctypes.data_as(dp), len(u),
                                        C.byref(lo), C.byref(up), C.byref(fl), C.byref(used))
    return alpha, a, lo.value, up.value, bool(fl.value), used.value


def stream(params: PlanarParams, chain_id: int, count: int):
    s = (C.c_uint32 * 4)()
    lib().planar_seed(C.byref(params), chain_id, s)
    return [lib().planar_next(params.rng, s) for _ in range(count)]
