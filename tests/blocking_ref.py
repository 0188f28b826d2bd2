"""The numpy twin of the blocked-standard-error estimator of DESIGN.md section 3.12 (pstat_blocking.hip): batch means from
the rows of a series, and the blocking transform of a matrix.  A checker: the package, tools/, julia/ and bench.py never
import it.  Plain IEEE double arithmetic in the order the section states, so the batch values equal the device's bit for
bit; afterwards only the order of summation differs (numpy's pairwise sums against the kernel's lane partials)."""
import numpy as np

NQ = 19
BLOCK_LEVELS = 24
FIELDS = ("mean", "stderr", "stderr_err", "inefficiency", "level", "converged")


def batches(steps, red, first_row=0, nrows=None):
    """x[N, ncases * NQ] from steps[rows] and red[rows, ncases, NRED] (Series.read()), rows [first_row, first_row + nrows).
    ValueError if the rows are not equally spaced and increasing."""
    steps = np.asarray(steps, dtype=np.int64)
    nrows = len(steps) - first_row if nrows is None else nrows
    st = steps[first_row:first_row + nrows]
    rd = np.asarray(red, dtype=np.float64)[first_row:first_row + nrows]
    d = int(st[1] - st[0]) if nrows >= 2 else int(st[0])
    if d < 1 or np.any(np.diff(st) != d):
        raise ValueError("rows are not equally spaced and increasing")
    S = rd[:, :, 1:1 + NQ] * st.astype(np.float64)[:, None, None]
    chains = rd[:, :, 0:1]
    if st[0] == d:   # the series began at empty averages: the baseline is zero
        S = np.concatenate([np.zeros_like(S[:1]), S])
        chains = np.concatenate([chains[:1], chains])
    x = (S[1:] - S[:-1]) / (float(d) * chains[1:])
    return x.reshape(x.shape[0], -1)


def blocking(x, min_blocks=32):
    """dict of arrays [ncols] (FIELDS) and "levels" [ncols, BLOCK_LEVELS] for x[N, ncols]."""
    x = np.asarray(x, dtype=np.float64)
    N, ncols = x.shape
    assert min_blocks >= 2 and N >= min_blocks
    levels = np.zeros((ncols, BLOCK_LEVELS))
    sizes = []
    v = x
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(BLOCK_LEVELS):
            n = v.shape[0]
            if n < 2:
                break
            m = v.sum(0) / n
            if l == 0:
                mean = m
            levels[:, l] = np.sqrt(((v - m) ** 2).sum(0) / (n - 1) / n)
            sizes.append(n)
            v = 0.5 * (v[0:2 * (n // 2):2] + v[1:2 * (n // 2):2])
    sizes = np.array(sizes)
    elig = np.nonzero(sizes >= min_blocks)[0]   # a prefix of the levels, level 0 among them
    last = elig[-1]
    se = levels[:, elig]
    out = {k: np.zeros(ncols) for k in FIELDS}
    out["mean"] = mean
    out["levels"] = levels
    for c in range(ncols):
        if not np.all(np.isfinite(se[c])):
            star, vals = -1, (np.nan, np.nan, np.nan, -1.0, 0.0)
        elif se[c, 0] == 0.0:
            vals = (0.0, 0.0, 1.0, 0.0, 1.0)
        else:
            star = int(np.argmax(se[c]))   # the first of the largest
            s = se[c, star]
            dse = s / np.sqrt(2.0 * (sizes[star] - 1.0))
            rising = star == last and (star == 0 or s - se[c, star - 1] > dse)      # into the last eligible level
            vals = (s, dse, (s / se[c, 0]) ** 2, float(star), 0.0 if rising else 1.0)
        for k, val in zip(FIELDS[1:], vals):
            out[k][c] = val
    return out


def decided(ref, min_blocks, N, rtol=1e-9):
    """Columns whose two largest eligible se_l differ by more than rtol relative: there level and converged must be equal
    whatever the order of summation."""
    sizes = []
    n = N
    while n >= 2 and len(sizes) < BLOCK_LEVELS:
        sizes.append(n)
        n //= 2
    ne = int(np.sum(np.array(sizes) >= min_blocks))
    se = ref["levels"][:, :ne]
    ok = np.ones(se.shape[0], dtype=bool)
    for c in range(se.shape[0]):
        if not np.all(np.isfinite(se[c])) or ne < 2:
            continue
        top = np.sort(se[c])[::-1]
        ok[c] = top[0] - top[1] > rtol * top[0] or top[0] == 0.0
        star = int(np.argmax(se[c]))
        if ok[c] and star == ne - 1 and star > 0:      # ... and the rise into the last level is not within rtol of its uncertainty
            rise, dse = se[c, star] - se[c, star - 1], se[c, star] / np.sqrt(2.0 * (sizes[star] - 1.0))
            ok[c] = abs(rise - dse) > rtol * se[c, star]
    return ok


def compare(got, ref, x, min_blocks, what=""):
    """An ErrorBars of the device against the twin's dict for the matrix x[N, ncols] (tolerances: only the order
    of summation differs, N <= 40 960 terms of one sign or of a mean: 1e-9 relative is a thousand times that; inefficiency is
    the square of a ratio of two such numbers: 4e-9)."""
    ncols = x.shape[1]
    flat = lambda a: np.asarray(a).reshape(ncols, *np.asarray(a).shape[got.mean.ndim:])
    scale = np.nanmax(np.abs(x)) if np.any(np.isfinite(x)) else 1.0
    fin = np.isfinite(ref["mean"])
    assert np.array_equal(np.isfinite(flat(got.mean)), fin), what
    assert np.all(np.abs(flat(got.mean)[fin] - ref["mean"][fin]) <= 1e-13 * scale), (what, flat(got.mean), ref["mean"])
    np.testing.assert_allclose(flat(got.stderr), ref["stderr"], rtol=1e-9, atol=0, equal_nan=True, err_msg=what)
    if got.levels is not None:
        np.testing.assert_allclose(flat(got.levels), ref["levels"], rtol=1e-9, atol=0, equal_nan=True, err_msg=what)
    ok = decided(ref, min_blocks, x.shape[0])
    assert np.array_equal(flat(got.level)[ok], ref["level"][ok].astype(np.int64)), what
    assert np.array_equal(flat(got.converged)[ok], ref["converged"][ok] != 0), what
    np.testing.assert_allclose(flat(got.stderr_err)[ok], ref["stderr_err"][ok], rtol=1e-9, atol=0, equal_nan=True, err_msg=what)
    np.testing.assert_allclose(flat(got.inefficiency)[ok], ref["inefficiency"][ok], rtol=4e-9, atol=0, equal_nan=True, err_msg=what)
