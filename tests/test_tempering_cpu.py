"""CPU tests of replica exchange between the cases of a handle (pstat_tempering_*): the entry points are
declared, exported and bound; they refuse null arguments before they touch a device; ladders_by groups a grid; the twin's
pairing schedule; the phase scan refuses --exchange together with --error-bars.  (The refusals that need a handle -- a
ladder id below -1, a ladder whose cases differ in more than kT, umbrella sampling -- are in tests/test_gpu_tempering.py: a
handle exists only on a device.)"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import tempering_ref as tw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["pstat_tempering_open", "pstat_tempering_exchange", "pstat_tempering_stats", "pstat_tempering_close"]


@pytest.fixture(scope="module")
def ps():
    import polymer_stats_amd as ps
    ps._lib.load()
    return ps


def test_tempering_symbols_are_declared_exported_and_bound(ps):
    lib = ps._lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pstat.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pstat_[A-Za-z_0-9]+)\s*\(", text))
    for name in NEW:
        assert name in declared, f"include/pstat.h does not declare {name}"
        assert name in ps._lib.SYMBOLS, f"the binding does not list {name}"
        assert getattr(lib, name).argtypes is not None, f"the binding gives {name} no argtypes"
    assert re.search(r"typedef\s+struct\s+pstat_tempering\s+pstat_tempering\s*;", text)
    assert lib.pstat_abi_version() == 6 and "#define PSTAT_ABI_VERSION 6" in text      # additive
    assert lib.pstat_tempering_close.restype is None
    for name in ("Tempering", "ladders_by"):
        assert name in ps.__all__ and hasattr(ps, name)
    assert all(hasattr(ps.Ensemble, m) for m in ("open_tempering", "advance_tempered"))


def test_tempering_entry_points_refuse_null_arguments(ps):
    """PSTAT_ERR_INVALID_ARG with a message, on a machine with or without a device: the handle is never looked at."""
    lib = ps._lib.load()
    room = C.create_string_buffer(64)
    fake = C.cast(room, C.c_void_p)
    out = C.c_void_p()
    ladder = (C.c_int32 * 1)(0)
    n = C.c_int64(0)
    calls = [
        ("open, null handle", lambda: lib.pstat_tempering_open(None, ladder, 0, C.byref(out))),
        ("open, null ladder", lambda: lib.pstat_tempering_open(fake, None, 0, C.byref(out))),
        ("open, null out", lambda: lib.pstat_tempering_open(fake, ladder, 0, None)),
        ("exchange, null handle", lambda: lib.pstat_tempering_exchange(None, fake)),
        ("exchange, null object", lambda: lib.pstat_tempering_exchange(fake, None)),
        ("stats, null handle", lambda: lib.pstat_tempering_stats(None, fake, None, None, C.byref(n))),
        ("stats, null object", lambda: lib.pstat_tempering_stats(fake, None, None, None, C.byref(n))),
    ]
    bad = ps.default_params(n=0)
    for what, call in calls:
        assert lib.pstat_create(C.byref(bad), 1, None, C.byref(out)) == -1 and b"null" not in lib.pstat_last_error()
        assert call() == -1, what
        assert b"null" in lib.pstat_last_error(), what
    assert out.value is None
    lib.pstat_tempering_close(None, None)        # void: nothing to close, nothing happens
    lib.pstat_tempering_close(fake, None)
    lib.pstat_tempering_close(None, fake)


def test_ladders_by_groups_a_grid(ps):
    E0s, kTs = (0.0, 1.0, 2.5), (0.25, 0.5, 1.0, 2.0)
    cases = [ps.default_params(n=8, E0=E0, kT=kT, seed=100 + 4 * i + j, chain_id0=7 * j)
             for i, E0 in enumerate(E0s) for j, kT in enumerate(kTs)]
    assert ps.ladders_by(cases).tolist() == [0] * 4 + [1] * 4 + [2] * 4      # seed and chain_id0 do not split a ladder
    assert ps.ladders_by(cases).dtype == np.int32
    cases[6].Fz = 0.2                                                         # one case of the E0 = 1 column deviates
    assert ps.ladders_by(cases).tolist() == [0] * 4 + [1, 1, 2, 1] + [3] * 4
    # a key of the caller's: rows of equal kT instead
    assert ps.ladders_by(cases, key=lambda p: p.kT).tolist() == [0, 1, 2, 3] * 3
    # the rungs of a ladder are its cases by (kT, index), whatever order they were given in
    kT = [c.kT for c in cases]
    assert tw.rungs(ps.ladders_by(cases), kT)[1] == [4, 5, 7]
    assert tw.rungs([0, 0, 0, -1, 0], [2.0, 1.0, 1.0, 0.1, 0.5]) == {0: [4, 1, 2, 0]}


@pytest.mark.parametrize("nrungs", [1, 2, 3, 6])
def test_pairing_schedule(nrungs):
    for t in range(4):
        pairs = tw.schedule(nrungs, t)
        used = [r for p in pairs for r in p]
        assert len(used) == len(set(used)) and all(0 <= r < nrungs for r in used)     # every rung in at most one pair
        assert all(b == a + 1 and a % 2 == t % 2 for a, b in pairs)                   # adjacent rungs, the round's parity
        assert len(pairs) == (nrungs - (t & 1)) // 2                                  # nobody who has a partner sits out
        assert pairs == tw.schedule(nrungs, t + 2)
    both = set(tw.schedule(nrungs, 0)) | set(tw.schedule(nrungs, 1))
    assert both == {(r, r + 1) for r in range(nrungs - 1)}                            # two rounds cover every adjacent pair
    assert not set(tw.schedule(nrungs, 0)) & set(tw.schedule(nrungs, 1))


def test_twin_stream_is_philox(oracle):
    """The twin's Philox4x32-10 against the CPU oracle's, and the uniform's 53 bits."""
    for ctr, key in (((0, 0, 0, 0), (0, 0)), ((5, 3, tw.TAG, 7), (0x12345678, 0x9abcdef0)), ((0xffffffff,) * 4, (0xffffffff,) * 2)):
        assert list(tw.philox4x32_10(ctr, key)) == oracle.philox(ctr, key)
    o = tw.philox4x32_10((5, 3, tw.TAG, 7), (0x12345678, 0x9abcdef0))
    u = tw.uniform(0x9abcdef012345678, 5, 3, 7)
    assert u == ((o[0] << 21) | (o[1] >> 11)) / 2.0 ** 53 and 0.0 <= u < 1.0


def test_product_never_imports_the_twin():
    """tests/tempering_ref.py is a checker (the rule of tests/test_blocking_cpu.py for its twin): the package, tools/, julia/
    and bench.py do not name it in anything that runs."""
    paths = [os.path.join(ROOT, "bench.py")]
    for top in ("polymer_stats_amd", "tools", "julia"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, top)):
            paths += [os.path.join(dirpath, f) for f in files if f.endswith((".py", ".jl", ".sh", "Makefile"))]
    for p in paths:
        assert "tempering_ref" not in open(p, errors="ignore").read(), p


def test_phase_scan_refuses_exchange_with_error_bars():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "phase_scan.py"), "--exchange", "50", "--error-bars", "8"],
                       capture_output=True, text=True)
    assert r.returncode != 0
    assert "--exchange cannot be combined with --error-bars" in r.stderr and "follow-up" in r.stderr
