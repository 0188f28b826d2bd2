#!/usr/bin/env python3
"""pstat_histogram_device on crafted matrices uploaded with torch, against the numpy twin of the binning formula
(tests/hist_ref.py); run by tests/test_gpu_hist.py in a process of its own, torch imported first.  Exit status 0 and "all
matrices agree", or the traceback of the first one that does not."""
import os
import sys

import numpy as np
import torch                    # before libpstat: torch's own HIP runtime must be the first one loaded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import hist_ref as hr           # noqa: E402
import polymer_stats_amd as ps  # noqa: E402

NROWS = [1, 63, 64, 65, 100000]

def crafted(lo, hi, nbins):
    edges = lo + (hi - lo) * np.arange(nbins + 1) / nbins
    v = np.concatenate([edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf),
                        [0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, np.nan, np.inf, -np.inf, 1.7e308, -1.7e308]])
    return v


def matrix_case(nrows):
    ranges = [(-1.5, 2.5, 8), (0.1, 0.7, 7), (0.0, 1.0, 64), (-2.0, -1.0, 1)]
    stride = 6                                                       # two columns more than are histogrammed
    rng = np.random.default_rng(800 + nrows)
    x = np.empty((nrows, stride))
    for col in range(stride):
        lo, hi, nbins = ranges[col % len(ranges)]
        special = crafted(lo, hi, nbins)
        column = rng.uniform(lo - 0.3 * (hi - lo), hi + 0.3 * (hi - lo), nrows)
        if nrows >= len(special):
            column[rng.choice(nrows, len(special), replace=False)] = special
        else:                                                        # the short matrices: as many crafted values as fit, another window per column
            column[:] = np.roll(special, -7 * col - nrows)[:nrows]
        x[:, col] = column
    # spec i reads column order[i]: not the identity, and column 3 twice
    order = [2, 0, 3, 1, 3]
    specs = [ps.hist_spec(c, ranges[c][2], ranges[c][0], ranges[c][1]) for c in order[:4]] + [ps.hist_spec(3, 5, -2.5, 0.5)]
    t = torch.from_numpy(x).to("cuda")
    before = torch.cuda.current_device()
    counts, tails = ps.histogram_device(t.data_ptr(), nrows, stride, specs)
    assert torch.cuda.current_device() == before
    for i, sp in enumerate(specs):
        want, want_tails = hr.bin_counts(x[:, sp.channel], sp.lo, sp.hi, sp.nbins)
        assert np.array_equal(counts[i], want), (i, counts[i], want)
        assert np.array_equal(tails[i], want_tails), (i, tails[i], want_tails)
        assert counts[i].sum() + tails[i].sum() == nrows
    if nrows == 100000:
        assert all(tails[i][2] == 3 for i in range(4)) and all(tails[i][0] > 0 and tails[i][1] > 0 for i in range(4))
        # on the caller's stream, and an empty matrix
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            u = t * 1.0
            c2, t2 = ps.histogram_device(u.data_ptr(), nrows, stride, specs, stream=s.cuda_stream)
        assert all(np.array_equal(a, b) for a, b in zip(c2, counts)) and np.array_equal(t2, tails)
        c0, t0 = ps.histogram_device(t.data_ptr(), 0, stride, specs)
        assert all(c.sum() == 0 for c in c0) and t0.sum() == 0


if __name__ == "__main__":
    assert torch.cuda.is_available()
    for nrows in NROWS:
        matrix_case(nrows)
        print(f"{nrows} rows: 5 specs agree", flush=True)
    print("all matrices agree")
