#!/usr/bin/env python3
"""pstat_blocking_device on seeded matrices uploaded with torch, against the numpy twin (tests/blocking_ref.py); run by
tests/test_gpu_blocking.py in a process of its own, torch imported first.  Exit status 0 and "all shapes agree", or the
traceback of the first shape that does not."""
import os
import sys

import numpy as np
import torch                    # before libpstat: torch's own HIP runtime must be the first one loaded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import blocking_ref as br       # noqa: E402
import polymer_stats_amd as ps  # noqa: E402

NBATCHES = [32, 33, 63, 64, 65, 127, 129, 1000, 4097, 32768]
NCOLS = [1, 3, 4, 5, 19, 65]


def matrix(rng, N, width):
    """Columns of different correlation lengths, offsets and scales (an exponential moving average of white noise)."""
    x = rng.standard_normal((N, width))
    phi = np.linspace(0.0, 0.95, width)
    for t in range(1, N):
        x[t] += phi * x[t - 1]
    return x * np.logspace(-3, 3, width) + np.linspace(-50.0, 50.0, width)


def shapes(N):
    rng = np.random.default_rng(1000 + N)
    for ncols in NCOLS:
        for stride in (ncols, ncols + 3):
            x = matrix(rng, N, stride)
            dev = torch.from_numpy(x).cuda()
            for mb in (2, 32):
                got = ps.blocking_device(dev.data_ptr(), N, ncols, stride, min_blocks=mb, levels=True)
                assert got.nbatches == N and got.mean.shape == (ncols,) and got.levels.shape == (ncols, 24)
                br.compare(got, br.blocking(x[:, :ncols], mb), x[:, :ncols], mb, f"N={N} ncols={ncols} stride={stride} mb={mb}")
            del dev


def constant_and_nan_columns():
    rng = np.random.default_rng(7)
    x = matrix(rng, 257, 6)
    x[:, 1] = 2.5
    x[:, 4] = 0.0
    y = x.copy()
    y[100, 2] = np.nan          # between finite columns
    for m in (x, y):
        dev = torch.from_numpy(m).cuda()
        got = ps.blocking_device(dev.data_ptr(), 257, 6, levels=True)
        br.compare(got, br.blocking(m, 32), m, 32)
        for c in (1, 4):
            assert (got.stderr[c], got.inefficiency[c], got.level[c], got.converged[c]) == (0.0, 1.0, 0, True)
            assert got.mean[c] == m[0, c] and np.all(got.levels[c] == 0.0)
    assert np.isnan(got.stderr[2]) and np.isnan(got.mean[2]) and got.level[2] == -1 and not got.converged[2]
    assert np.all(np.isfinite(got.stderr[[0, 1, 3, 4, 5]]))
    # without `levels`, and with the default min_blocks spelled 0
    again = ps.blocking_device(dev.data_ptr(), 257, 6, min_blocks=0)
    assert again.levels is None and np.array_equal(again.stderr, got.stderr, equal_nan=True)


def the_limit():
    limit = ps._lib.BLOCK_MAX_BATCHES
    dev = torch.zeros(limit + 1, 1, dtype=torch.float64, device="cuda")
    try:
        ps.blocking_device(dev.data_ptr(), limit + 1, 1)
        raise AssertionError("limit + 1 was accepted")
    except ps.PstatError as err:
        assert err.code == -4 and str(limit) in str(err)
    x = np.random.default_rng(3).standard_normal((limit, 2))
    got = ps.blocking_device(torch.from_numpy(x).cuda().data_ptr(), limit, 2, levels=True)      # the limit itself: all of the LDS
    br.compare(got, br.blocking(x, 32), x, 32)


if __name__ == "__main__":
    assert torch.cuda.is_available()
    for N in NBATCHES:
        shapes(N)
        print(f"N = {N}: {len(NCOLS)} widths x 2 strides x 2 min_blocks agree", flush=True)
    constant_and_nan_columns()
    the_limit()
    print("all shapes agree")
