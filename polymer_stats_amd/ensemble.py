"""Ensemble: Python handle on a libpstat ensemble of chains (thin wrapper, no arithmetic of its own)."""
from __future__ import annotations

import ctypes as C
from typing import Iterable, Sequence

import numpy as np

from . import _lib
from ._lib import NOBS, NRED, Params, Summary, LaunchInfo, check


class Ensemble:
    """`cases`: one Params or a list of Params that differ only in physics scalars (a sweep grid).
    `stream`: raw hipStream_t (int) to launch on, e.g. torch.cuda.current_stream().cuda_stream.
    `planar`: the planar main (2D/mcmc_clustering_eap_chain.jl, pstat_create_planar): one angle per monomer; observables
    are the 16-vectors with the y slots 0 (PLANAR_OBS_NAMES / PLANAR_OBS_INDEX), chain_state()["theta"] is zeros."""

    def __init__(self, cases: Params | Sequence[Params], stream: int | None = None, planar: bool = False):
        self._L = _lib.load()
        if isinstance(cases, Params):
            cases = [cases]
        self.cases = list(cases)
        self.ncases = len(self.cases)
        arr = (Params * self.ncases)(*self.cases)
        self._h = C.c_void_p()
        self.planar = bool(planar)
        create = self._L.pstat_create_planar if self.planar else self._L.pstat_create
        check(create(arr, self.ncases, C.c_void_p(stream) if stream else None, C.byref(self._h)))
        self.n = int(self.cases[0].n)
        self.num_chains = int(self.cases[0].num_chains)

    def close(self):
        if getattr(self, "_h", None):
            self._L.pstat_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # --- the step loop
    def advance(self, nsteps: int):
        check(self._L.pstat_advance(self._h, int(nsteps)))

    def sync(self):
        check(self._L.pstat_sync(self._h))

    def reinit(self, force_init: bool):
        check(self._L.pstat_reinit(self._h, 1 if force_init else 0))

    def reset_averages(self):
        """Discard what has been recorded so far (burn-in); chains, generators, step sizes stay."""
        check(self._L.pstat_reset_averages(self._h))

    def reset_sampler(self):
        """What a fresh mcmc(nsteps, pargs, chain) call of the reference resets besides the averagers:
        step sizes, adaptation window, the acceptor's cache, the in-run step counter."""
        check(self._L.pstat_reset_sampler(self._h))

    def set_kT(self, kT: float, icase: int = -1):
        check(self._L.pstat_set_kT(self._h, icase, float(kT)))

    def restart_from_x0(self, x0, dx0_phi: float, dx0_theta: float):
        """Start every chain over from x0 ([phi, theta] or interleaved per-monomer angles) + Uniform(0, dx0)."""
        a = np.ascontiguousarray(x0, dtype=np.float64)
        check(self._L.pstat_restart_from_x0(self._h, a.ctypes.data_as(C.POINTER(C.c_double)), len(a),
                                            float(dx0_phi), float(dx0_theta)))

    def scale_kT(self, mult: float):
        """kT of every case <- its creation-time kT * mult (one rung of the burn-in ladder for a grid)."""
        check(self._L.pstat_scale_kT(self._h, float(mult)))

    # --- the stepout time series, recorded on the device
    def open_series(self, capacity_rows: int, angles: bool = False) -> "Series":
        """Device memory for `capacity_rows` rows; `angles`: rows also hold every case's first chain's angles."""
        s = C.c_void_p()
        check(self._L.pstat_series_open(self._h, int(capacity_rows), _lib.SERIES_ANGLES if angles else 0, C.byref(s)))
        return Series(self, s, bool(angles))

    def advance_series(self, series: "Series", nsteps: int, stepout: int):
        """advance(nsteps) that appends a row to `series` after every `stepout`-th step (asynchronous)."""
        check(self._L.pstat_advance_series(self._h, series._s, int(nsteps), int(stepout)))
        series.rows += int(nsteps) // int(stepout)

    # --- replica exchange between the cases (pstat_tempering_*)
    def open_tempering(self, ladder, seed: int = 0) -> "Tempering":
        """`ladder[i]`: the ladder case i belongs to (>= 0; ladders_by builds it), or -1 for a case that takes no part.  The
        cases of a ladder differ in kT, seed and chain_id0 only; its rungs are ordered by kT."""
        a = np.ascontiguousarray(ladder, dtype=np.int32)
        if a.shape != (self.ncases,):
            raise ValueError(f"ladder must name a ladder for each of the {self.ncases} cases")
        t = C.c_void_p()
        check(self._L.pstat_tempering_open(self._h, a.ctypes.data_as(C.POINTER(C.c_int32)), int(seed), C.byref(t)))
        return Tempering(self, t)

    def advance_tempered(self, t: "Tempering", nsteps: int, every: int):
        """advance(every) followed by one exchange round, repeated; the remainder nsteps % every is advanced without an
        exchange (asynchronous)."""
        nsteps, every = int(nsteps), int(every)
        if every < 1:
            raise ValueError("every must be >= 1")
        for _ in range(nsteps // every):
            self.advance(every)
            t.exchange()
        self.advance(nsteps % every)

    # --- per-case histograms of the chains' current configurations (pstat_hist_*)
    def open_hist(self, specs, per_case: bool = False) -> "Hist":
        """`specs`: a list of hist_spec(...) shared by all cases, or with `per_case` one such list per case (same channels and
        bin counts, lo and hi free).  Every record adds one sample per chain and spec."""
        rows = [list(r) for r in specs] if per_case else [list(specs)]
        if per_case and (len(rows) != self.ncases or any(len(r) != len(rows[0]) for r in rows)):
            raise ValueError(f"per-case specs must be {self.ncases} lists of equal length")
        nspecs = len(rows[0])
        flat = [s for r in rows for s in r]
        arr = (_lib.HistSpec * max(len(flat), 1))(*flat)
        g = C.c_void_p()
        check(self._L.pstat_hist_open(self._h, arr, nspecs, 1 if per_case else 0, C.byref(g)))
        return Hist(self, g, rows)

    def advance_hist(self, hist: "Hist", nsteps: int, stepout: int):
        """advance(nsteps) with a record into `hist` after every `stepout`-th step (asynchronous)."""
        check(self._L.pstat_advance_hist(self._h, hist._g, int(nsteps), int(stepout)))

    # --- per-case lag correlations of the monomers' orientations and dipoles (pstat_corr_*)
    def open_corr(self, channels=("nn",), max_lag: int | None = None, capacity_rows: int = 0) -> "Corr":
        """`channels`: names of CORR_NAMES ("nn" tangent, "zz" along the field, "mm" dipole); `max_lag`: lags 0 .. max_lag
        (default n - 1); `capacity_rows` > 0 also keeps one row of case means per record, for Corr.error_bars."""
        if isinstance(channels, str):
            channels = (channels,)
        unknown = [c for c in channels if c not in _lib.CORR_NAMES]
        if unknown:
            raise ValueError(f"unknown correlation channel {unknown[0]!r}: one of {', '.join(_lib.CORR_NAMES)}")
        names = tuple(c for c in _lib.CORR_NAMES if c in channels)
        mask = sum(1 << _lib.CORR_NAMES.index(c) for c in names)
        g = C.c_void_p()
        check(self._L.pstat_corr_open(self._h, mask, -1 if max_lag is None else int(max_lag), int(capacity_rows), C.byref(g)))
        return Corr(self, g, names, self.n - 1 if max_lag is None else int(max_lag))

    def advance_corr(self, corr: "Corr", nsteps: int, stepout: int):
        """advance(nsteps) with a record into `corr` after every `stepout`-th step (asynchronous)."""
        check(self._L.pstat_advance_corr(self._h, corr._g, int(nsteps), int(stepout)))

    # --- per-case gyration tensor and form factor of the monomers' positions (pstat_shape_*)
    def open_shape(self, q=None, capacity_rows: int = 0) -> "Shape":
        """`q`: wave-vectors in absolute units, array-like [nq, 3] (a planar handle also takes [nq, 2], mapped to the x and z
        slots); None or empty: the gyration block only.  `capacity_rows` > 0 also keeps one row of case means per record, for
        Shape.error_bars."""
        qa = _shape_q(q, self.planar)
        g = C.c_void_p()
        check(self._L.pstat_shape_open(self._h, qa.ctypes.data_as(C.POINTER(C.c_double)) if len(qa) else None, len(qa),
                                       int(capacity_rows), C.byref(g)))
        return Shape(self, g, qa)

    def advance_shape(self, shape: "Shape", nsteps: int, stepout: int):
        """advance(nsteps) with a record into `shape` after every `stepout`-th step (asynchronous)."""
        check(self._L.pstat_advance_shape(self._h, shape._g, int(nsteps), int(stepout)))

    # --- per-case pair distances of the monomers' positions (pstat_pdist_*)
    def open_pdist(self, max_sep: int = -1, min_sep: int = 1, bins=None, q=None, capacity_rows: int = 0) -> "Pdist":
        """`max_sep`: R2(s) for s = 1 .. max_sep (-1: n - 1; 0: none); `min_sep`: the closest approach and the histogram count
        the pairs with j - i >= min_sep; `bins`: None, or (nbins, rmax) with rmax in absolute units, or (nbins, [rmax per case]);
        `q`: the Debye magnitudes, array-like [nq] >= 0 in absolute units (None: none).  `capacity_rows` > 0 also keeps one row
        of case means per record, for Pdist.error_bars."""
        nbins, rmax = _pdist_bins(bins, self.ncases)
        qa = _pdist_q(q)
        spec = _lib.PdistSpec(int(max_sep), int(min_sep), nbins, len(qa), float(rmax[0]) if len(rmax) == 1 else 0.0)
        dp = C.POINTER(C.c_double)
        g = C.c_void_p()
        check(self._L.pstat_pdist_open(self._h, C.byref(spec), qa.ctypes.data_as(dp) if len(qa) else None,
                                       rmax.ctypes.data_as(dp) if len(rmax) > 1 else None, int(capacity_rows), C.byref(g)))
        per_case = np.broadcast_to(rmax, (self.ncases,)).copy() if nbins else np.zeros(self.ncases)
        return Pdist(self, g, self.n - 1 if int(max_sep) < 0 else int(max_sep), int(min_sep), nbins, per_case, qa)

    def advance_pdist(self, pdist: "Pdist", nsteps: int, stepout: int):
        """advance(nsteps) with a record into `pdist` after every `stepout`-th step (asynchronous)."""
        check(self._L.pstat_advance_pdist(self._h, pdist._g, int(nsteps), int(stepout)))

    # --- per-case energy by term and separation (pstat_energy_*)
    def open_energy(self, max_sep: int = -1, cutoff=None, capacity_rows: int = 0) -> "Energy":
        """`max_sep`: pair[s] for s = 1 .. max_sep (-1: n - 1; 0: none), the separations beyond it in `rest`; `cutoff`: the
        radius of the `within` column in monomer lengths, a number or one per case; None: the cases' own cutoff_radius on a
        CUTOFF handle, no column otherwise.  `capacity_rows` > 0 also keeps one row of case means per record, for
        Energy.error_bars."""
        types = [int(p.energy_type) for p in self.cases]
        if cutoff is None:
            cut = np.array([float(p.cutoff_radius) for p in self.cases]) if types[0] == _lib.CUTOFF else np.zeros(1)
        else:
            cut = np.atleast_1d(np.asarray(cutoff, dtype=np.float64))
            if cut.ndim != 1 or len(cut) not in (1, self.ncases):
                raise ValueError(f"cutoff must be one number or one per case ({self.ncases}), not {cut.shape}")
        cut = np.ascontiguousarray(cut)
        spec = _lib.EnergySpec(int(max_sep), 0, float(cut[0]) if len(cut) == 1 else 0.0)
        g = C.c_void_p()
        check(self._L.pstat_energy_open(self._h, C.byref(spec), cut.ctypes.data_as(C.POINTER(C.c_double)) if len(cut) > 1 else None,
                                        int(capacity_rows), C.byref(g)))
        per_case = np.broadcast_to(cut, (self.ncases,)).copy()
        return Energy(self, g, self.n - 1 if int(max_sep) < 0 else int(max_sep), per_case, types)

    def advance_energy(self, energy: "Energy", nsteps: int, stepout: int):
        """advance(nsteps) with a record into `energy` after every `stepout`-th step (asynchronous)."""
        check(self._L.pstat_advance_energy(self._h, energy._g, int(nsteps), int(stepout)))

    # --- read-outs
    def reduce_into(self, dev_ptr: int, icase: int = -1):
        """Device-side reduction into a caller-owned device buffer of NRED doubles (async)."""
        check(self._L.pstat_reduce_device(self._h, icase, C.c_void_p(dev_ptr)))

    def reduce_host(self, icase: int = -1) -> np.ndarray:
        red = np.zeros(NRED)
        check(self._L.pstat_reduce_host(self._h, icase, red.ctypes.data_as(C.POINTER(C.c_double))))
        return red

    def summary(self, icase: int = -1) -> Summary:
        s = Summary()
        check(self._L.pstat_summary_get(self._h, icase, C.byref(s)))
        return s

    def rolling(self, icase: int = -1):
        avg = np.zeros(NOBS)
        se = np.zeros(NOBS)
        dp = C.POINTER(C.c_double)
        check(self._L.pstat_rolling(self._h, icase, avg.ctypes.data_as(dp), se.ctypes.data_as(dp)))
        return avg, se

    def chain_means(self, icase: int = -1) -> np.ndarray:
        """Per-chain running means, shape [NQ, chains]: what the device reduction folds (pstat_chain_means)."""
        m = self.num_chains * (self.ncases if icase < 0 else 1)
        out = np.zeros((_lib.NQ, m))
        check(self._L.pstat_chain_means(self._h, icase, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def microstate(self, chain: int = 0) -> np.ndarray:
        out = np.zeros(7)
        check(self._L.pstat_microstate(self._h, chain, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def chain_state(self, chain: int) -> dict:
        ang = np.zeros(2 * self.n)
        sums = np.zeros(NOBS)
        cnt = np.zeros(4, dtype=np.int64)
        steps = np.zeros(3)
        rng = np.zeros(4, dtype=np.uint32)
        dp = C.POINTER(C.c_double)
        check(self._L.pstat_chain_state(self._h, chain, ang.ctypes.data_as(dp), sums.ctypes.data_as(dp),
                                        cnt.ctypes.data_as(C.POINTER(C.c_int64)), steps.ctypes.data_as(dp),
                                        rng.ctypes.data_as(C.POINTER(C.c_uint32))))
        return dict(theta=ang[:self.n], phi=ang[self.n:], sums=sums, nacc_total=int(cnt[0]),
                    steps_recorded=int(cnt[1]), nacc_window=int(cnt[2]), natt_window=int(cnt[3]),
                    phi_step=steps[0], theta_step=steps[1], normalizer=steps[2], rng=rng)

    def chain_extras(self, chain: int) -> dict:
        """Clustering main only: running sums and current values of sum cos^2(theta) and <psi>."""
        sums = np.zeros(2)
        now = np.zeros(2)
        dp = C.POINTER(C.c_double)
        check(self._L.pstat_chain_extras(self._h, chain, sums.ctypes.data_as(dp), now.ctypes.data_as(dp)))
        return dict(sums=sums, now=now)

    def checkpoint(self) -> bytes:
        size = C.c_size_t(0)
        check(self._L.pstat_checkpoint(self._h, None, C.byref(size)))
        buf = C.create_string_buffer(size.value)
        check(self._L.pstat_checkpoint(self._h, buf, C.byref(size)))
        return buf.raw[:size.value]

    def restore(self, blob: bytes):
        buf = C.create_string_buffer(blob, len(blob))
        check(self._L.pstat_restore(self._h, buf, len(blob)))

    def launch_info(self) -> LaunchInfo:
        info = LaunchInfo()
        check(self._L.pstat_launch_info_get(self._h, C.byref(info)))
        return info


class _Recorder:
    """An object that a handle keeps open for its Ensemble (pstat_<_kind>_*): `_g` is its address, None once closed."""

    _kind = ""

    def __init__(self, ensemble: Ensemble, g):
        self._e, self._g = ensemble, g

    def _fn(self, name: str):
        return getattr(self._e._L, f"pstat_{self._kind}_{name}")

    def close(self):
        if self._g and self._e._h:      # (closing the ensemble closes its objects)
            self._fn("close")(self._e._h, self._g)
        self._g = None


class Series(_Recorder):
    """Rows recorded by Ensemble.advance_series (pstat_series_*); `rows` counts them."""

    _kind = "series"
    _s = property(lambda self: self._g)

    def __init__(self, ensemble: Ensemble, s, angles: bool):
        super().__init__(ensemble, s)
        self.angles, self.rows = angles, 0

    def read(self, nrows: int | None = None):
        """(steps[rows], red[rows, ncases, NRED], micro[rows, ncases, 7], angles[rows, ncases, 2n] or None) of the first
        `nrows` rows (default: all recorded).  Synchronises."""
        e = self._e
        r = self.rows if nrows is None else int(nrows)
        steps = np.zeros(r, dtype=np.int64)
        red = np.zeros((r, e.ncases, NRED))
        micro = np.zeros((r, e.ncases, 7))
        ang = np.zeros((r, e.ncases, 2 * e.n)) if self.angles else None
        dp = C.POINTER(C.c_double)
        check(e._L.pstat_series_read(e._h, self._s, r, steps.ctypes.data_as(C.POINTER(C.c_int64)), red.ctypes.data_as(dp),
                                     micro.ctypes.data_as(dp), ang.ctypes.data_as(dp) if self.angles else None))
        return steps, red, micro, ang

    def error_bars(self, first_row: int = 0, nrows: int | None = None, min_blocks: int = 32, levels: bool = False) -> "ErrorBars":
        """Blocked standard errors of the batch means between the rows [first_row, first_row + nrows) (default: to the
        last row), computed on the device (pstat_series_error_bars): arrays of shape [ncases, NQ], columns EB_NAMES.
        Synchronises."""
        e = self._e
        out = np.zeros((e.ncases, _lib.NQ, len(_lib.EB_FIELDS)))
        lev = np.zeros((e.ncases, _lib.NQ, _lib.BLOCK_LEVELS)) if levels else None
        nb = C.c_int64(0)
        dp = C.POINTER(C.c_double)
        check(e._L.pstat_series_error_bars(e._h, self._s, int(first_row), -1 if nrows is None else int(nrows), int(min_blocks),
                                           C.byref(nb), out.ctypes.data_as(dp), lev.ctypes.data_as(dp) if levels else None))
        return ErrorBars(out, int(nb.value), lev)

    def clear(self):
        check(self._e._L.pstat_series_clear(self._e._h, self._s))
        self.rows = 0


class Tempering(_Recorder):
    """Replica exchange between the cases of an Ensemble (Ensemble.open_tempering)."""

    _kind = "tempering"
    _t = property(lambda self: self._g)

    def exchange(self):
        """One round: even rounds pair rungs (0, 1), (2, 3), ..., odd rounds (1, 2), (3, 4), ... (asynchronous)."""
        check(self._e._L.pstat_tempering_exchange(self._e._h, self._t))

    def stats(self):
        """(attempted[ncases], accepted[ncases], rounds): exchanges of pairs of chains, counted on the lower rung of a pair,
        and the exchange calls so far.  Synchronises."""
        e = self._e
        att = np.zeros(e.ncases, dtype=np.int64)
        acc = np.zeros(e.ncases, dtype=np.int64)
        rounds = C.c_int64(0)
        ip = C.POINTER(C.c_int64)
        check(e._L.pstat_tempering_stats(e._h, self._t, att.ctypes.data_as(ip), acc.ctypes.data_as(ip), C.byref(rounds)))
        return att, acc, int(rounds.value)


def _edges(spec) -> np.ndarray:
    return spec.lo + (spec.hi - spec.lo) * np.arange(spec.nbins + 1) / spec.nbins


class HistResult:
    """What Hist.read returns.  `counts[i]`: int64 [ncases, nbins_i] of spec i; `tails`: int64 [ncases, nspecs, 3] (below lo,
    at or above hi, not finite); `records`; `samples`: records * chains per case, which bins + tails add up to for every case
    and spec."""

    def __init__(self, specs, counts, tails, records: int, samples: int):
        self.specs, self.counts, self.tails, self.records, self.samples = specs, counts, tails, records, samples

    def _spec(self, i: int, case: int):
        return self.specs[case if len(self.specs) > 1 else 0][i]

    def edges(self, i: int, case: int = 0) -> np.ndarray:
        """The nbins + 1 nominal bin edges of spec i (the binning itself is the formula of include/pstat.h)."""
        return _edges(self._spec(i, case))

    def centers(self, i: int, case: int = 0) -> np.ndarray:
        e = self.edges(i, case)
        return 0.5 * (e[:-1] + e[1:])

    def density(self, i: int, case: int = 0) -> np.ndarray:
        """counts / (samples * bin width): integrates to the fraction of the samples that fell inside [lo, hi)."""
        sp = self._spec(i, case)
        return self.counts[i][case] / (max(self.samples, 1) * (sp.hi - sp.lo) / sp.nbins)


class Hist(_Recorder):
    """Histograms recorded on the device (Ensemble.open_hist, pstat_hist_*)."""

    _kind = "hist"

    def __init__(self, ensemble: Ensemble, g, specs):
        super().__init__(ensemble, g)
        self.specs = specs

    def record(self):
        """Adds the current configuration of every chain (asynchronous)."""
        check(self._e._L.pstat_hist_record(self._e._h, self._g))

    def read(self) -> HistResult:
        """Synchronises."""
        e = self._e
        nb = [int(s.nbins) for s in self.specs[0]]
        counts = np.zeros((e.ncases, sum(nb)), dtype=np.int64)
        tails = np.zeros((e.ncases, len(nb), 3), dtype=np.int64)
        records = C.c_int64(0)
        ip = C.POINTER(C.c_int64)
        check(e._L.pstat_hist_read(e._h, self._g, counts.ctypes.data_as(ip), tails.ctypes.data_as(ip), C.byref(records)))
        off = np.concatenate([[0], np.cumsum(nb)])
        per = [np.ascontiguousarray(counts[:, off[i]:off[i + 1]]) for i in range(len(nb))]
        return HistResult(self.specs, per, tails, int(records.value), int(records.value) * e.num_chains)

    def clear(self):
        check(self._e._L.pstat_hist_clear(self._e._h, self._g))


def _mean_and_chain_stderr(sum_: np.ndarray, sumsq: np.ndarray, records: int, N: int):
    """Of column totals over `records` records of N chains: sum / (records * N), and the across-chain standard error of that
    mean, defined after exactly one record (chains are independent, records of one chain are not) and NaN otherwise."""
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = sum_ / (records * N) if records > 0 else np.full(sum_.shape, np.nan)
        if records == 1 and N > 1:
            return mean, np.sqrt(np.maximum(sumsq / N - (sum_ / N) ** 2, 0.0) / (N - 1))
        return mean, np.full(sum_.shape, np.nan)


class CorrResult:
    """What Corr.read returns.  `sum`, `sumsq`: the raw totals, float64 [ncases, ncols] with the channels' columns side by side
    in the order of `channels`, each max_lag + 1 wide; `records`; `mean[channel]`: sum / (records * chains per case), shape
    [ncases, max_lag + 1]; `chain_stderr[channel]`: the across-chain standard error of that mean, defined after exactly one
    record (chains are independent, records of one chain are not) and NaN otherwise."""

    def __init__(self, channels, max_lag: int, num_chains: int, sum_: np.ndarray, sumsq: np.ndarray, records: int):
        self.channels, self.max_lag, self.records, self.sum, self.sumsq = channels, max_lag, records, sum_, sumsq
        w = max_lag + 1
        mean, stderr = _mean_and_chain_stderr(sum_, sumsq, records, num_chains)
        self.mean = {ch: mean[:, i * w:(i + 1) * w] for i, ch in enumerate(channels)}
        self.chain_stderr = {ch: stderr[:, i * w:(i + 1) * w] for i, ch in enumerate(channels)}


class _Totals(_Recorder):
    """What Corr, Shape, Pdist and Energy share: per-case totals of `ncols` columns and, with capacity_rows > 0 at the open, one row of case
    means per record."""

    def __init__(self, ensemble: Ensemble, g, ncols: int):
        super().__init__(ensemble, g)
        self.ncols = ncols
        self._record = self._fn("record")

    def record(self):
        """One record of the current configuration of every chain (asynchronous)."""
        check(self._record(self._e._h, self._g))

    def _read(self):
        """(sum, sumsq, records) as the library keeps them.  Synchronises."""
        e = self._e
        s = np.zeros((e.ncases, self.ncols))
        q = np.zeros((e.ncases, self.ncols))
        records = C.c_int64(0)
        dp = C.POINTER(C.c_double)
        check(self._fn("read")(e._h, self._g, s.ctypes.data_as(dp), q.ctypes.data_as(dp), C.byref(records)))
        return s, q, int(records.value)

    def rows(self):
        """(device pointer, rows, stride) of the per-record case means, a float64 matrix [rows][ncases * ncols] in device
        memory (pstat_corr_rows, pstat_shape_rows, pstat_pdist_rows, pstat_energy_rows).  Synchronises."""
        e = self._e
        ptr, nrows, stride = C.c_void_p(), C.c_int64(0), C.c_int64(0)
        check(self._fn("rows")(e._h, self._g, C.byref(ptr), C.byref(nrows), C.byref(stride)))
        return ptr.value or 0, int(nrows.value), int(stride.value)

    def error_bars(self, min_blocks: int = 32, levels: bool = False, device: int | None = None) -> "ErrorBars":
        """Blocked standard errors of the recorded rows' columns (pstat_blocking_device on rows()): arrays of shape
        [ncases, ncols].  Needs capacity_rows > 0 at open_corr / open_shape / open_pdist / open_energy and at least `min_blocks` records.  Synchronises."""
        e = self._e
        ptr, nrows, stride = self.rows()
        dev = int(e.cases[0].device) if device is None else int(device)
        eb = blocking_device(ptr, nrows, stride, stride, min_blocks=min_blocks, levels=levels, device=dev)
        out = np.stack([eb.mean, eb.stderr, eb.stderr_err, eb.inefficiency, eb.level.astype(float), eb.converged.astype(float)], axis=-1)
        lev = eb.levels.reshape(e.ncases, self.ncols, -1) if levels else None
        return ErrorBars(out.reshape(e.ncases, self.ncols, -1), nrows, lev)

    def clear(self):
        check(self._fn("clear")(self._e._h, self._g))


class Corr(_Totals):
    """Lag correlations recorded on the device (Ensemble.open_corr, pstat_corr_*)."""

    _kind = "corr"

    def __init__(self, ensemble: Ensemble, g, channels, max_lag: int):
        super().__init__(ensemble, g, len(channels) * (max_lag + 1))
        self.channels, self.max_lag = channels, max_lag

    def read(self) -> CorrResult:
        """Synchronises."""
        return CorrResult(self.channels, self.max_lag, self._e.num_chains, *self._read())


def _shape_q(q, planar: bool) -> np.ndarray:
    """The wave-vector table as the library takes it: float64 [nq, 3], C order."""
    if q is None:
        return np.zeros((0, 3))
    a = np.asarray(q, dtype=np.float64)
    if a.size == 0:
        return np.zeros((0, 3))
    if a.ndim != 2 or a.shape[1] not in ((2, 3) if planar else (3,)):
        raise ValueError(f"q must be [nq, 3]{' or [nq, 2]' if planar else ''}, not {a.shape}")
    if a.shape[1] == 2:                 # a planar handle's (x, z)
        a = np.stack([a[:, 0], np.zeros(len(a)), a[:, 1]], axis=1)
    return np.ascontiguousarray(a)


class ShapeResult:
    """What Shape.read returns.  `sum`, `sumsq`: the raw totals, float64 [ncases, 8 + nq], the columns SHAPE_NAMES and then one
    per wave-vector of `q` ([nq, 3]); `records`; `mean`: sum / (records * chains per case); `chain_stderr`: the across-chain
    standard error of that mean, defined after exactly one record (chains are independent, records of one chain are not) and
    NaN otherwise; `gyration`: the mean tensor [ncases, 3, 3]; `rg2`: [ncases]; `sq`: the mean form factor [ncases, nq]."""

    def __init__(self, q: np.ndarray, num_chains: int, planar: bool, sum_: np.ndarray, sumsq: np.ndarray, records: int):
        self.q, self.num_chains, self.planar, self.records, self.sum, self.sumsq = q, num_chains, planar, records, sum_, sumsq
        m, self.chain_stderr = _mean_and_chain_stderr(sum_, sumsq, records, num_chains)
        self.mean = m
        self.gyration = np.stack([np.stack([m[:, 0], m[:, 3], m[:, 4]], axis=-1), np.stack([m[:, 3], m[:, 1], m[:, 5]], axis=-1),
                                  np.stack([m[:, 4], m[:, 5], m[:, 2]], axis=-1)], axis=1)
        self.rg2 = m[:, 6]
        self.sq = m[:, len(_lib.SHAPE_NAMES):]


def shape_anisotropy(result: ShapeResult) -> np.ndarray:
    """The relative shape anisotropy of every case as a ratio of averages, [ncases]: (3 <trg2> - <rg2^2>) / (2 <rg2^2>) for a 3D
    handle, (2 <trg2> - <rg2^2>) / <rg2^2> for a planar one, with <rg2^2> = sumsq / (records * chains per case) of the rg2
    column.  0 for a sphere (disc), 1 for a rod."""
    i_rg2, i_trg2 = _lib.SHAPE_NAMES.index("rg2"), _lib.SHAPE_NAMES.index("trg2")
    with np.errstate(invalid="ignore", divide="ignore"):
        rg4 = result.sumsq[:, i_rg2] / (result.records * result.num_chains)
        trg2 = result.mean[:, i_trg2]
        return (2.0 * trg2 - rg4) / rg4 if result.planar else (3.0 * trg2 - rg4) / (2.0 * rg4)


class Shape(_Totals):
    """Gyration tensor and form factor recorded on the device (Ensemble.open_shape, pstat_shape_*)."""

    _kind = "shape"

    def __init__(self, ensemble: Ensemble, g, q: np.ndarray):
        super().__init__(ensemble, g, len(_lib.SHAPE_NAMES) + len(q))
        self.q = q

    def read(self) -> ShapeResult:
        """Synchronises."""
        return ShapeResult(self.q, self._e.num_chains, self._e.planar, *self._read())


def _pdist_bins(bins, ncases: int):
    """(nbins, rmax as float64 [1] or [ncases]) from None | (nbins, rmax) | (nbins, [rmax per case])."""
    if bins is None:
        return 0, np.ones(1)
    try:
        nbins, rmax = bins
        nbins = int(nbins)
        rmax = np.atleast_1d(np.asarray(rmax, dtype=np.float64))
    except (TypeError, ValueError):
        raise ValueError("bins must be None, (nbins, rmax) or (nbins, [rmax per case])")
    if rmax.ndim != 1 or len(rmax) not in (1, ncases):
        raise ValueError(f"bins: rmax must be one number or one per case ({ncases}), not {rmax.shape}")
    if nbins == 0:
        return 0, np.ones(1)
    return nbins, np.ascontiguousarray(rmax)


def _pdist_q(q) -> np.ndarray:
    """The Debye magnitudes as the library takes them: float64 [nq]."""
    if q is None:
        return np.zeros(0)
    a = np.asarray(q, dtype=np.float64)
    if a.size == 0:
        return np.zeros(0)
    if a.ndim != 1:
        raise ValueError(f"q must be [nq] magnitudes, not {a.shape}")
    return np.ascontiguousarray(a)


class PdistResult:
    """What Pdist.read returns.  `sum`, `sumsq`: the raw totals, float64 [ncases, ncols], the columns msd (s = 1 .. max_sep),
    rmin, the nbins + 1 histogram columns (none without bins) and one per magnitude of `q`; `records`; `mean`: sum / (records *
    chains per case); `chain_stderr`: the across-chain standard error of that mean, defined after exactly one record and NaN
    otherwise.  Views of `mean`: `msd` [ncases, max_sep], `rmin` [ncases], `sq` [ncases, nq]; of `sum`: `counts` [ncases, nbins]
    and `above` [ncases], the pairs counted over all records and chains (exact integers kept as doubles).  `pairs`: how many pairs
    of one chain the histogram and rmin look at, (n - min_sep)(n - min_sep + 1) / 2."""

    def __init__(self, n: int, max_sep: int, min_sep: int, nbins: int, rmax: np.ndarray, q: np.ndarray, num_chains: int,
                 sum_: np.ndarray, sumsq: np.ndarray, records: int):
        self.n, self.max_sep, self.min_sep, self.nbins, self.rmax, self.q = n, max_sep, min_sep, nbins, rmax, q
        self.num_chains, self.records, self.sum, self.sumsq = num_chains, records, sum_, sumsq
        self.mean, self.chain_stderr = _mean_and_chain_stderr(sum_, sumsq, records, num_chains)
        self.pairs = (n - min_sep) * (n - min_sep + 1) // 2
        h0 = max_sep + 1
        h1 = h0 + (nbins + 1 if nbins else 0)
        self.msd, self.rmin, self.sq = self.mean[:, :max_sep], self.mean[:, max_sep], self.mean[:, h1:]
        self.counts = sum_[:, h0:h0 + nbins]
        self.above = sum_[:, h1 - 1] if nbins else np.zeros(len(sum_))

    def edges(self, k: int = 0) -> np.ndarray:
        """The nbins + 1 bin edges of case k: rmax (0 .. nbins) / nbins."""
        return float(self.rmax[k]) * np.arange(self.nbins + 1) / max(self.nbins, 1)

    def centers(self, k: int = 0) -> np.ndarray:
        e = self.edges(k)
        return 0.5 * (e[:-1] + e[1:])

    def density(self, k: int = 0) -> np.ndarray:
        """P(r) of case k: counts / (pairs counted * bin width), so it integrates to the share of pairs below rmax."""
        counted = self.records * self.num_chains * self.pairs
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.counts[k] / (counted * (float(self.rmax[k]) / max(self.nbins, 1)))


class Pdist(_Totals):
    """Pair distances recorded on the device (Ensemble.open_pdist, pstat_pdist_*)."""

    _kind = "pdist"

    def __init__(self, ensemble: Ensemble, g, max_sep: int, min_sep: int, nbins: int, rmax: np.ndarray, q: np.ndarray):
        super().__init__(ensemble, g, max_sep + 1 + (nbins + 1 if nbins else 0) + len(q))
        self.max_sep, self.min_sep, self.nbins, self.rmax, self.q = max_sep, min_sep, nbins, rmax, q

    def read(self) -> PdistResult:
        """Synchronises."""
        e = self._e
        return PdistResult(e.n, self.max_sep, self.min_sep, self.nbins, self.rmax, self.q, e.num_chains, *self._read())


class EnergyResult:
    """What Energy.read returns.  `sum`, `sumsq`: the raw totals, float64 [ncases, ncols], the columns field, work, bend,
    pair[1 .. max_sep], rest and, with a cutoff, within; `records`; `mean`: sum / (records * chains per case); `chain_stderr`: the
    across-chain standard error of that mean, defined after exactly one record and NaN otherwise.  Views of `mean`: `field`,
    `work`, `bend`, `rest`, `within` [ncases] (`within`: None without the column) and `pair` [ncases, max_sep].  `model_sum`,
    `model` [ncases]: the energy the handle's own step carries, from `sum` and `mean`, by each case's energy type
    (`model_columns`); on a CUTOFF handle opened without its `within` column they raise ValueError."""

    def __init__(self, max_sep: int, cutoff: np.ndarray, energy_types, num_chains: int, sum_: np.ndarray, sumsq: np.ndarray,
                 records: int):
        self.max_sep, self.cutoff, self.energy_types = max_sep, cutoff, list(energy_types)
        self.num_chains, self.records, self.sum, self.sumsq = num_chains, records, sum_, sumsq
        self.mean, self.chain_stderr = _mean_and_chain_stderr(sum_, sumsq, records, num_chains)
        self.has_within = sum_.shape[1] == 3 + max_sep + 2
        m = self.mean
        self.field, self.work, self.bend = m[:, 0], m[:, 1], m[:, 2]
        self.pair, self.rest = m[:, 3:3 + max_sep], m[:, 3 + max_sep]
        self.within = m[:, 4 + max_sep] if self.has_within else None

    def model_columns(self, k: int) -> list[int]:
        """The columns whose sum is the energy case k's own step carries (include/pstat.h, "model total")."""
        return energy_model_columns(self.energy_types[k], self.max_sep, self.has_within)

    def _model(self, a: np.ndarray) -> np.ndarray:
        return np.array([a[k, self.model_columns(k)].sum() for k in range(len(a))])

    @property
    def model_sum(self) -> np.ndarray:
        return self._model(self.sum)

    @property
    def model(self) -> np.ndarray:
        return self._model(self.mean)


def energy_model_columns(energy_type: int, max_sep: int, has_within: bool) -> list[int]:
    """Columns of an energy object whose sum is the U a handle of `energy_type` carries: field + work + bend, with pair[1]
    (Ising) or every pair column and rest (interacting); `within` alone for the cutoff energy."""
    if energy_type == _lib.CUTOFF:
        if not has_within:
            raise ValueError("the model total of a cutoff handle is its `within` column: open the energy object with a cutoff")
        return [4 + max_sep]
    cols = [0, 1, 2]
    if energy_type == _lib.ISING:
        if max_sep < 1:
            raise ValueError("the model total of an Ising handle needs pair[1]: open the energy object with max_sep >= 1")
        cols.append(3)
    elif energy_type == _lib.INTERACTING:
        cols += list(range(3, 4 + max_sep))
    return cols


class Energy(_Totals):
    """The energy by term and separation recorded on the device (Ensemble.open_energy, pstat_energy_*)."""

    _kind = "energy"

    def __init__(self, ensemble: Ensemble, g, max_sep: int, cutoff: np.ndarray, energy_types):
        self.has_within = bool(np.any(cutoff > 0.0))
        super().__init__(ensemble, g, 3 + max_sep + 1 + (1 if self.has_within else 0))
        self.max_sep, self.cutoff, self.energy_types = max_sep, cutoff, energy_types

    def read(self) -> EnergyResult:
        """Synchronises."""
        return EnergyResult(self.max_sep, self.cutoff, self.energy_types, self._e.num_chains, *self._read())

    def model_error_bars(self, min_blocks: int = 32) -> "ErrorBars":
        """Blocked standard errors of the model total, arrays of shape [ncases]: the blocking transform of the rows' COMBINED
        column (the parts of one record are correlated, so their errors do not add).  The rows come to the host, the combined
        column goes back as a matrix [rows][ncases] of its own.  Needs capacity_rows > 0 at open_energy.  Synchronises."""
        e = self._e
        ptr, nrows, stride = self.rows()
        hip = _hip_runtime()
        rows = np.zeros((nrows, e.ncases, self.ncols))
        if nrows and hip.hipMemcpy(rows.ctypes.data, ptr, rows.nbytes, 2):          # 2: device to host
            raise RuntimeError("copying the energy rows to the host failed")
        cols = [energy_model_columns(t, self.max_sep, self.has_within) for t in self.energy_types]
        model = np.ascontiguousarray(np.stack([rows[:, k, cols[k]].sum(axis=1) for k in range(e.ncases)], axis=1))
        dev = C.c_void_p()
        if hip.hipMalloc(C.byref(dev), max(model.nbytes, 8)):
            raise MemoryError("no device memory for the combined column")
        try:
            if nrows and hip.hipMemcpy(dev, model.ctypes.data, model.nbytes, 1):    # 1: host to device
                raise RuntimeError("copying the combined column to the device failed")
            return blocking_device(dev.value, nrows, e.ncases, min_blocks=min_blocks, device=int(e.cases[0].device))
        finally:
            hip.hipFree(dev)


def _hip_runtime():
    """The HIP runtime libpstat has loaded into this process, for the few copies this module makes itself."""
    with open("/proc/self/maps") as f:
        path = next(line.split()[-1] for line in f if "libamdhip64" in line)
    hip = C.CDLL(path)
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    return hip


def histogram_device(ptr: int, nrows: int, stride: int, specs, device: int = 0, stream: int | None = None):
    """Histograms of columns of a float64 matrix x[nrows][stride] in DEVICE memory at `ptr` (e.g. tensor.data_ptr() of a
    contiguous torch tensor); a spec's channel is its column.  Returns (counts: one int64 [nbins] array per spec,
    tails int64 [nspecs, 3]) (pstat_histogram_device).  Synchronises `stream`."""
    specs = list(specs)
    arr = (_lib.HistSpec * max(len(specs), 1))(*specs)
    nb = [max(int(s.nbins), 0) for s in specs]
    counts = np.zeros(max(sum(nb), 1), dtype=np.int64)
    tails = np.zeros((max(len(specs), 1), 3), dtype=np.int64)
    ip = C.POINTER(C.c_int64)
    check(_lib.load().pstat_histogram_device(C.c_void_p(ptr), int(nrows), int(stride), arr, len(specs), int(device),
                                             C.c_void_p(stream) if stream else None, counts.ctypes.data_as(ip),
                                             tails.ctypes.data_as(ip)))
    off = np.concatenate([[0], np.cumsum(nb)])
    return [counts[off[i]:off[i + 1]].copy() for i in range(len(nb))], tails[:len(specs)]


def ladders_by(cases, key=None) -> np.ndarray:
    """The `ladder` array of Ensemble.open_tempering: cases that agree in everything but kT (and seed, chain_id0) share a
    ladder; ids count the ladders in order of their first case.  `key`: a function of a Params whose equal values mean
    "same ladder" (default: every field but kT, seed and chain_id0)."""
    if key is None:
        names = [f for f, _ in Params._fields_ if f not in ("kT", "seed", "chain_id0")]
        key = lambda p: tuple(getattr(p, f) for f in names)
    ids: dict = {}
    return np.array([ids.setdefault(key(p), len(ids)) for p in cases], dtype=np.int32)


class ErrorBars:
    """What the blocking transform gives per column (include/pstat.h, PSTAT_EB_*): `mean`, `stderr` (the blocked standard
    error), `stderr_err` (its own uncertainty), `inefficiency` ((stderr / naive stderr)^2), `level` (blocking level picked),
    `converged` (False: the curve was still rising at the last level, the run is too short for this column); `nbatches`;
    `levels`: se_l of every level, 0 beyond the last, or None."""

    def __init__(self, out: np.ndarray, nbatches: int, levels: np.ndarray | None):
        self.mean, self.stderr, self.stderr_err, self.inefficiency = (out[..., i] for i in range(4))
        self.level = out[..., 4].astype(np.int64)
        self.converged = out[..., 5] != 0
        self.nbatches, self.levels = nbatches, levels


def blocking_device(ptr: int, nbatches: int, ncols: int, stride: int | None = None, min_blocks: int = 32, levels: bool = False,
                    device: int = 0, stream: int | None = None) -> ErrorBars:
    """The blocking transform of a float64 matrix x[nbatches][stride] in DEVICE memory at `ptr` (e.g. tensor.data_ptr() of a
    contiguous torch tensor, or a series merged over ranks), first `ncols` columns: arrays of shape [ncols]
    (pstat_blocking_device).  `stream`: raw hipStream_t the matrix was produced on.  Synchronises that stream."""
    stride = int(ncols) if stride is None else int(stride)
    out = np.zeros((max(int(ncols), 0), len(_lib.EB_FIELDS)))
    lev = np.zeros((max(int(ncols), 0), _lib.BLOCK_LEVELS)) if levels else None
    dp = C.POINTER(C.c_double)
    check(_lib.load().pstat_blocking_device(C.c_void_p(ptr), int(nbatches), int(ncols), stride, int(min_blocks), int(device),
                                            C.c_void_p(stream) if stream else None, out.ctypes.data_as(dp),
                                            lev.ctypes.data_as(dp) if levels else None))
    return ErrorBars(out, int(nbatches), lev)


def summary_from_reduction(red: Iterable[float], steps_per_chain: int) -> Summary:
    """Host arithmetic on an (all-reduced) NRED vector -> pooled averages and standard errors."""
    a = np.ascontiguousarray(np.asarray(list(red), dtype=np.float64))
    assert a.shape == (NRED,)
    s = Summary()
    check(_lib.load().pstat_summary_from_reduction(a.ctypes.data_as(C.POINTER(C.c_double)),
                                                   int(steps_per_chain), C.byref(s)))
    return s
