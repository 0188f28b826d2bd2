"""Generates tests/golden/hist_closed_form.json: bin probabilities of the end-to-end component r_z = b sum_i cos(theta_i) of a
non-interacting dielectric chain in the force ensemble, for tests/test_hist_cpu.py and tests/test_gpu_hist.py.

Our own derivation, not reference output.  With the field along z a monomer's energy is -E0^2 / 2 (K1 cos^2 + K2 sin^2) - Fz b
cos(theta), so z = cos(theta) has the single-monomer density ~ exp(kappa z^2 + f z) on [-1, 1], kappa = E0^2 (K1 - K2) / (2 kT),
f = Fz b / kT.  The monomers are independent: the density of sum_i z_i is that density convolved n times.  density_of_sum does
so on a grid of spacing H whose nodes include the jumps at z = +-1, with the trapezoid weights of a grid-aligned integral; at
kappa = f = 0 the result is the Irwin-Hall density of n uniforms, which validate() compares it with.

Run:  python tests/golden/make_hist_closed_form.py   (rewrites the JSON next to this file)
"""
import json
import math
import os

import numpy as np

H = 1.0 / 1024           # grid spacing of the convolution; a bin edge of every histogram used is a node
NBINS = 32
CASES = [dict(n=8, E0=0.0, K1=1.0, K2=0.0, Fz=0.0), dict(n=8, E0=0.0, K1=1.0, K2=0.0, Fz=1.0),
         dict(n=8, E0=0.0, K1=1.0, K2=0.0, Fz=2.5), dict(n=8, E0=1.5, K1=1.0, K2=0.0, Fz=0.5)]   # all with kT = b = 1


def density_of_sum(n, kappa, f):
    """(s, p): the density p of s = z_1 + ... + z_n on the grid s = -n, -n + H, ..., n."""
    z = np.linspace(-1.0, 1.0, int(round(2 / H)) + 1)
    w = np.exp(kappa * z * z + f * z - abs(kappa) - abs(f))
    w[0] *= 0.5              # trapezoid: the density jumps to 0 at +-1
    w[-1] *= 0.5
    w /= w.sum() * H
    p = w.copy()
    for _ in range(n - 1):
        p = np.convolve(p, w) * H
    # the half weights belong to the quadrature, not to the density: undo them at the two ends (n = 1 only; for n >= 2 the
    # density is continuous and vanishes there)
    if n == 1:
        p[0] *= 2.0
        p[-1] *= 2.0
    return np.linspace(-n, n, len(p)), p


def bin_probabilities(n, kappa, f, nbins, lo=None, hi=None):
    """Probabilities of `nbins` equal bins on [lo, hi] (default [-n, n], in units of b): composite Simpson over the grid nodes
    of each bin, renormalised over the whole support."""
    lo, hi = (-float(n) if lo is None else lo), (float(n) if hi is None else hi)
    s, p = density_of_sum(n, kappa, f)
    per = (hi - lo) / nbins / H
    assert abs(per - round(per)) < 1e-9 and int(round(per)) % 2 == 0, "bin edges must fall on even grid nodes"
    per = int(round(per))
    first = int(round((lo + n) / H))
    simpson = np.ones(per + 1)
    simpson[1:-1:2], simpson[2:-1:2] = 4.0, 2.0
    simpson *= H / 3.0
    total = float(np.sum((p[:-1] + p[1:]) * 0.5 * H))
    out = np.zeros(nbins)
    for j in range(nbins):
        a = first + j * per
        out[j] = float(np.dot(p[a:a + per + 1], simpson))
    return out / total


def irwin_hall_density(n, s):
    """Density of the sum of n uniforms on [-1, 1] at s."""
    x = (np.asarray(s, dtype=np.float64) + n) / 2.0
    out = np.zeros_like(x)
    for k in range(n + 1):
        out += (-1.0) ** k * math.comb(n, k) * np.where(x > k, x - k, 0.0) ** (n - 1)
    return out / math.factorial(n - 1) / 2.0


def validate(n=8):
    """Largest error of density_of_sum(n, 0, 0) against Irwin-Hall, relative to the density's maximum."""
    s, p = density_of_sum(n, 0.0, 0.0)
    exact = irwin_hall_density(n, s)
    return float(np.max(np.abs(p - exact)) / exact.max())


def kappa_f(c, kT=1.0, b=1.0):
    return c["E0"] ** 2 * (c["K1"] - c["K2"]) / (2.0 * kT), c["Fz"] * b / kT


def main():
    err = validate()
    print("Irwin-Hall check, n = 8: max relative error", err)
    assert err < 1e-6
    out = {"_generator": "tests/golden/make_hist_closed_form.py (n-fold grid convolution; not reference output)",
           "kT": 1.0, "b": 1.0, "nbins": NBINS, "cases": []}
    for c in CASES:
        kappa, f = kappa_f(c)
        prob = bin_probabilities(c["n"], kappa, f, NBINS)
        print(c, "sum", prob.sum(), "mode", int(np.argmax(prob)))
        out["cases"].append(dict(c, lo=-float(c["n"]), hi=float(c["n"]), prob=prob.tolist()))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hist_closed_form.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
    print("wrote", path)


if __name__ == "__main__":
    main()
