"""GPU tests of the recorder lifecycle: the rules that the six kinds of object a handle keeps open -- series,
tempering, hist, corr, shape, pdist -- share, asserted for every kind alike through the raw entry points of the library: whose
object it is, the order of the refusals of an advance, a full row buffer, the count of records, clearing, reading with no
output, totals kept without rows, use after close, a checkpoint restored under open objects, and a handle destroyed with objects
open.  What a record holds is the business of each kind's own tests."""
import ctypes as C

import numpy as np
import pytest

from recorder_cases import ps  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu

NSTEPS, STEPOUT = 10, 3          # three records and a remainder of one step
NOT_OPEN = {"series": b"not an open series", "tempering": b"the tempering object is not an open one",
            "hist": b"not an open histogram", "corr": b"the correlation object is not an open one",
            "shape": b"the shape object is not an open one", "pdist": b"the pdist object is not an open one"}
KINDS = tuple(NOT_OPEN)
TOTALS = ("corr", "shape", "pdist")                  # the kinds that keep column totals (a _Totals)
RECORDING = ("series", "hist") + TOTALS              # the kinds with a pstat_advance_X and a pstat_X_clear
WITH_ROWS = ("series",) + TOTALS                     # the kinds with a row capacity
NOUN = {"series": b"the series has", "corr": b"the correlation object has", "shape": b"the shape object has",
        "pdist": b"the pdist object has"}


def ensemble(ps, planar):
    """3 cases x 20 chains of n = 5 that differ in kT (20 is no multiple of the recorders' 16-chain tile); planar: one case."""
    if planar:
        return ps.Ensemble(ps.default_planar_params(n=5, num_chains=20, Fz=0.3, seed=3), planar=True)
    return ps.Ensemble([ps.default_params(n=5, num_chains=20, kT=kT, Fz=0.3, seed=3) for kT in (1.0, 1.5, 2.5)])


def open_kind(ps, e, kind, capacity=8):
    if kind == "series":
        return e.open_series(capacity)
    if kind == "tempering":
        return e.open_tempering(np.zeros(e.ncases, dtype=np.int32), seed=5)
    if kind == "hist":
        return e.open_hist([ps._lib.hist_spec("r3", 8, -5.0, 5.0)])
    if kind == "corr":
        return e.open_corr(("nn",), capacity_rows=capacity)
    if kind == "shape":
        return e.open_shape([[0.0, 0.0, 0.5]], capacity_rows=capacity)
    return e.open_pdist(q=[1.0], capacity_rows=capacity)


def entry_points(lib, kind):
    """{name: f(handle, object) -> status} for every entry point of the kind that takes an object and returns a status, each
    with arguments that an open object of the handle accepts as far as the ownership test."""
    out = (C.c_double * 4096)()
    ptr, a, b = C.c_void_p(), C.c_int64(), C.c_int64()
    if kind == "series":
        return {"advance_series": lambda h, p: lib.pstat_advance_series(h, p, 0, 1),
                "series_read": lambda h, p: lib.pstat_series_read(h, p, 0, None, None, None, None),
                "series_clear": lib.pstat_series_clear,
                "series_error_bars": lambda h, p: lib.pstat_series_error_bars(h, p, 0, -1, 0, None, out, None)}
    if kind == "tempering":
        return {"tempering_exchange": lib.pstat_tempering_exchange,
                "tempering_stats": lambda h, p: lib.pstat_tempering_stats(h, p, None, None, None)}
    fns = {f"{kind}_record": getattr(lib, f"pstat_{kind}_record"),
           f"advance_{kind}": lambda h, p: getattr(lib, f"pstat_advance_{kind}")(h, p, 0, 1),
           f"{kind}_read": lambda h, p: getattr(lib, f"pstat_{kind}_read")(h, p, None, None, None),
           f"{kind}_clear": getattr(lib, f"pstat_{kind}_clear")}
    if kind != "hist":
        fns[f"{kind}_rows"] = lambda h, p: getattr(lib, f"pstat_{kind}_rows")(h, p, C.byref(ptr), C.byref(a), C.byref(b))
    return fns


def advance_raw(lib, kind, h, p, nsteps, stepout):
    return getattr(lib, f"pstat_advance_{kind}")(h, p, nsteps, stepout)


def advance(e, kind, obj, nsteps, stepout):
    if kind == "tempering":
        e.advance_tempered(obj, nsteps, stepout)
    else:
        getattr(e, f"advance_{kind}")(obj, nsteps, stepout)


def count(lib, e, kind, obj):
    """Records (rows, rounds) the object holds, as the library counts them.  Synchronises."""
    if kind == "series":       # the most rows that a read is not refused
        return max(n for n in range(10) if lib.pstat_series_read(e._h, obj._g, n, None, None, None, None) == 0)
    if kind == "tempering":
        return obj.stats()[2]
    return obj.read().records


def steps_recorded(e):
    return [e.chain_state(c)["steps_recorded"] for c in (0, e.ncases * e.num_chains - 1)]


@pytest.mark.parametrize("planar", [False, True], ids=["3d", "planar"])
@pytest.mark.parametrize("kind", KINDS)
def test_an_object_belongs_to_its_handle(ps, kind, planar):
    lib = ps._lib.load()
    with ensemble(ps, planar) as e, ensemble(ps, planar) as other:
        obj = open_kind(ps, e, kind)
        for name, f in entry_points(lib, kind).items():
            assert f(other._h, obj._g) == -1 and NOT_OPEN[kind] in lib.pstat_last_error(), name
        if kind in RECORDING:      # whose object it is comes before what the arguments are
            assert advance_raw(lib, kind, other._h, obj._g, NSTEPS, 0) == -1 and NOT_OPEN[kind] in lib.pstat_last_error()
        getattr(lib, f"pstat_{kind}_close")(other._h, obj._g)      # ignored: it is not the other handle's to close
        assert steps_recorded(other) == [0, 0]
        advance(e, kind, obj, NSTEPS, STEPOUT)                     # the object still works
        assert count(lib, e, kind, obj) == 3 and steps_recorded(e) == [NSTEPS, NSTEPS]
        for name, f in entry_points(lib, kind).items():
            if name != "series_error_bars":                        # (three rows are too few batches: -7 from the owner)
                assert f(e._h, obj._g) == 0, (name, lib.pstat_last_error())


@pytest.mark.parametrize("planar", [False, True], ids=["3d", "planar"])
@pytest.mark.parametrize("kind", RECORDING)
def test_advance_refuses_before_it_enqueues(ps, kind, planar):
    lib = ps._lib.load()
    with ensemble(ps, planar) as e:
        obj = open_kind(ps, e, kind, capacity=3)
        assert advance_raw(lib, kind, e._h, obj._g, NSTEPS, 0) == -1 and b"stepout" in lib.pstat_last_error()
        assert advance_raw(lib, kind, e._h, obj._g, -1, STEPOUT) == -1 and b"nsteps" in lib.pstat_last_error()
        assert advance_raw(lib, kind, e._h, obj._g, -1, 0) == -1 and b"nsteps" in lib.pstat_last_error()
        assert steps_recorded(e) == [0, 0] and count(lib, e, kind, obj) == 0
        assert advance_raw(lib, kind, e._h, obj._g, NSTEPS, STEPOUT) == 0, lib.pstat_last_error()
        assert steps_recorded(e) == [NSTEPS, NSTEPS] and count(lib, e, kind, obj) == 3
        if kind in WITH_ROWS:      # the row buffer is full: refused with nothing enqueued
            assert advance_raw(lib, kind, e._h, obj._g, STEPOUT, STEPOUT) == -7
            assert NOUN[kind] + b" 0 of 3 rows free, this call would record 1" in lib.pstat_last_error()
            assert advance_raw(lib, kind, e._h, obj._g, -1, STEPOUT) == -1      # an argument error comes before the full buffer
            if kind != "series":
                assert getattr(lib, f"pstat_{kind}_record")(e._h, obj._g) == -7
            assert steps_recorded(e) == [NSTEPS, NSTEPS] and count(lib, e, kind, obj) == 3
        assert advance_raw(lib, kind, e._h, obj._g, STEPOUT - 1, STEPOUT) == 0      # a call that records nothing always fits
        assert steps_recorded(e) == [NSTEPS + STEPOUT - 1] * 2 and count(lib, e, kind, obj) == 3
        obj.clear()                                                # no records, and every row free again
        assert count(lib, e, kind, obj) == 0 and (kind not in TOTALS or obj.rows()[1] == 0)
        assert advance_raw(lib, kind, e._h, obj._g, NSTEPS, STEPOUT) == 0, lib.pstat_last_error()
        assert count(lib, e, kind, obj) == 3
        if kind != "series":       # every output may be NULL
            records = C.c_int64(-1)
            assert getattr(lib, f"pstat_{kind}_read")(e._h, obj._g, None, None, C.byref(records)) == 0 and records.value == 3


@pytest.mark.parametrize("planar", [False, True], ids=["3d", "planar"])
@pytest.mark.parametrize("kind", TOTALS)
def test_totals_without_rows_have_no_limit(ps, kind, planar):
    with ensemble(ps, planar) as e:
        obj = open_kind(ps, e, kind, capacity=0)                   # no rows kept: no limit, and no rows to hand out
        advance(e, kind, obj, 50, 1)
        assert obj.read().records == 50 and obj.rows() == (0, 0, e.ncases * obj.ncols)
        with pytest.raises(ps.PstatError):
            obj.error_bars()


@pytest.mark.parametrize("planar", [False, True], ids=["3d", "planar"])
@pytest.mark.parametrize("kind", KINDS)
def test_a_closed_object_is_refused(ps, kind, planar):
    lib = ps._lib.load()
    with ensemble(ps, planar) as e:
        keep, obj = open_kind(ps, e, kind), open_kind(ps, e, kind)
        advance(e, kind, obj, NSTEPS, STEPOUT)
        raw = obj._g
        obj.close()                                                # with its last record still in flight
        assert obj._g is None
        for name, f in entry_points(lib, kind).items():
            assert f(e._h, raw) == -1 and NOT_OPEN[kind] in lib.pstat_last_error(), name
        getattr(lib, f"pstat_{kind}_close")(e._h, raw)             # a second close is harmless
        obj.close()
        advance(e, kind, keep, NSTEPS, STEPOUT)                    # the handle and its other objects go on
        assert count(lib, e, kind, keep) == 3 and steps_recorded(e) == [2 * NSTEPS, 2 * NSTEPS]
        e.restore(e.checkpoint())                                  # no object is part of a checkpoint
        assert count(lib, e, kind, keep) == 3 and steps_recorded(e) == [2 * NSTEPS, 2 * NSTEPS]


@pytest.mark.parametrize("planar", [False, True], ids=["3d", "planar"])
def test_destroy_with_every_kind_open(ps, planar):
    lib = ps._lib.load()
    e = ensemble(ps, planar)
    objs = {kind: open_kind(ps, e, kind) for kind in KINDS}
    for kind, obj in objs.items():
        advance(e, kind, obj, NSTEPS, STEPOUT)                     # no synchronise: the last records are in flight
    e.close()
    for obj in objs.values():
        obj.close()                                                # the ensemble has closed them: nothing left to do
    with ensemble(ps, planar) as e:                                # the next handle of the process works
        objs = {kind: open_kind(ps, e, kind) for kind in KINDS}
        for kind, obj in objs.items():
            advance(e, kind, obj, NSTEPS, STEPOUT)
        assert steps_recorded(e) == [len(KINDS) * NSTEPS] * 2
        assert all(count(lib, e, kind, obj) == 3 for kind, obj in objs.items())
