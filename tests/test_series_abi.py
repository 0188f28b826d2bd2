"""CPU tests of the stepout time series' entry points (pstat_series_*, pstat_advance_series): declared in include/pstat.h,
exported by the library, bound by the ctypes mirror, and refusing null arguments before they touch a device."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pstat_series_open", "pstat_advance_series", "pstat_series_read", "pstat_series_clear", "pstat_series_close"]


@pytest.fixture(scope="module")
def lib():
    import polymer_stats_amd as ps
    return ps._lib.load()


def test_series_symbols_are_declared_exported_and_bound(lib):
    import polymer_stats_amd as ps
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pstat.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pstat_[A-Za-z_0-9]+)\s*\(", text))
    for name in NEW:
        assert name in declared, f"include/pstat.h does not declare {name}"
        assert name in ps._lib.SYMBOLS, f"the binding does not list {name}"
        fn = getattr(lib, name)
        assert fn.argtypes is not None, f"the binding gives {name} no argtypes"
    assert re.search(r"PSTAT_SERIES_ANGLES\s*=\s*1\b", text) and ps._lib.SERIES_ANGLES == 1
    assert lib.pstat_abi_version() == 6          # additive: the ABI version does not move
    assert lib.pstat_series_close.restype is None


def test_series_entry_points_refuse_null_arguments(lib):
    """Null handle, and null series behind a handle that is never looked at: PSTAT_ERR_INVALID_ARG with a message, on a
    machine with or without a device."""
    room = C.create_string_buffer(64)            # stands in for a handle: the null check on the series comes first
    fake = C.cast(room, C.c_void_p)
    out = C.c_void_p()
    calls = [
        ("open, null handle", lambda: lib.pstat_series_open(None, 4, 0, C.byref(out))),
        ("open, null out", lambda: lib.pstat_series_open(fake, 4, 0, None)),
        ("advance, null handle", lambda: lib.pstat_advance_series(None, fake, 10, 5)),
        ("advance, null series", lambda: lib.pstat_advance_series(fake, None, 10, 5)),
        ("read, null handle", lambda: lib.pstat_series_read(None, fake, 0, None, None, None, None)),
        ("read, null series", lambda: lib.pstat_series_read(fake, None, 0, None, None, None, None)),
        ("clear, null handle", lambda: lib.pstat_series_clear(None, fake)),
        ("clear, null series", lambda: lib.pstat_series_clear(fake, None)),
    ]
    import polymer_stats_amd as ps
    bad = ps.default_params(n=0)
    for what, call in calls:
        assert lib.pstat_create(C.byref(bad), 1, None, C.byref(out)) == -1 and b"null" not in lib.pstat_last_error()
        assert call() == -1, what
        assert b"null" in lib.pstat_last_error(), what
    assert out.value is None
    lib.pstat_series_close(None, None)           # void: nothing to close, nothing happens
    lib.pstat_series_close(fake, None)
    lib.pstat_series_close(None, fake)
