"""numpy twin of the binning contract of polymer_stats_amd/csrc/pstat_hist.hip (restated here, not shared).

It is the formula, not the real interval: inv = float64(nbins) / (hi - lo) computed once; t = (x - lo) * inv, a subtraction and
a product each rounded to f64 on its own; x not finite -> tails[2]; t < 0 -> tails[0]; t >= nbins -> tails[1]; otherwise bin
int(t), truncated.  Channels 0..6 are the seven doubles of a microstate; 7 is sqrt(r1 r1 + r2 r2 + r3 r3), 8 the same over p,
products rounded singly and added left to right."""
import numpy as np

CHANNELS = ["r1", "r2", "r3", "p1", "p2", "p3", "U", "rmag", "pmag"]


def slots(values, lo, hi, nbins):
    """Per value: its bin, or nbins + (0 below, 1 at or above the range, 2 not finite)."""
    x = np.asarray(values, dtype=np.float64).ravel()
    lo, hi = np.float64(lo), np.float64(hi)
    inv = np.float64(nbins) / (hi - lo)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (x - lo) * inv
    out = np.full(x.shape, -1, dtype=np.int64)
    bad = ~np.isfinite(x)
    below = ~bad & (t < 0)
    above = ~bad & (t >= nbins)
    inside = ~bad & ~below & ~above
    out[bad], out[below], out[above] = nbins + 2, nbins, nbins + 1
    out[inside] = np.trunc(t[inside]).astype(np.int64)
    return out


def bin_counts(values, lo, hi, nbins):
    """(counts int64[nbins], tails int64[3]) of the values under the formula."""
    c = np.bincount(slots(values, lo, hi, nbins), minlength=nbins + 3).astype(np.int64)
    return c[:nbins], c[nbins:nbins + 3]


def channel_values(micro, channel):
    """The channel's value for every row of micro[..., 7] (rows of pstat_microstate)."""
    m = np.asarray(micro, dtype=np.float64)
    if channel < 7:
        return m[..., channel]
    v = m[..., 0:3] if channel == 7 else m[..., 3:6]
    return np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])


def near_edge(values, lo, hi, nbins, ulps=2):
    """True where a value lies within `ulps` ulp of a nominal edge lo + j (hi - lo) / nbins: where a last-bit difference in the
    value (the device's square root against numpy's) may change its bin."""
    x = np.asarray(values, dtype=np.float64).ravel()
    edges = np.float64(lo) + (np.float64(hi) - np.float64(lo)) * np.arange(nbins + 1) / nbins
    j = np.clip(np.searchsorted(edges, x), 0, nbins)
    d = np.minimum(np.abs(x - edges[j]), np.abs(x - edges[np.maximum(j - 1, 0)]))
    return d <= ulps * np.spacing(np.abs(x))
