"""Generates tests/golden/pdist_closed_form.json: closed forms of the pair-distance columns for chains of iid monomers, for
tests/test_pdist_cpu.py and tests/test_gpu_pdist.py.  Our own derivations, formulas only, not reference output.

With the centres x_i = b (sum_{j <= i} n_j - n_i / 2), for j - i = s >= 1:  x_j - x_i = b (n_i / 2 + n_{i+1} + ... + n_{j-1} + n_j / 2).
The monomers of the non-interacting energy are iid with mean m = <n> and |n| = 1, so
  R2(s) = <|x_j - x_i|^2> = b^2 [(1/4 + (s - 1) + 1/4) (1 - |m|^2) + s^2 |m|^2] = b^2 [(s - 1/2) + (s^2 - s + 1/2) |m|^2].
  free (E0 = F = 0)      m = 0:  R2(s) = b^2 (s - 1/2), in 3D and in the plane.
  fixed force F_z, 3D    density ~ sin(theta) exp(f cos(theta)), f = F b / kT:  |m| = L(f) = coth f - 1 / f.
  Debye, free 3D         <sinc(q r)> is the orientational average of <exp(i q . (x_j - x_i))>, and for isotropic monomers that is
                         sinc(q b / 2)^2 sinc(q b)^(s - 1):  S(q) = 1 + (2 / n) sum_{s=1}^{n-1} (n - s) sinc(q b / 2)^2 sinc(q b)^(s-1).
  n = 2, free 3D         r = (b / 2) |n_0 + n_1| = b sqrt((1 + cos g) / 2) with cos g uniform on [-1, 1]: r^2 / b^2 is uniform on
                         [0, 1].  P(r < R) = R^2 / b^2, so with rmax = b bin k of nbins holds (2 k + 1) / nbins^2; <rmin> = 2 b / 3.
  n = 2, free planar     r = b |cos(g / 2)| with g uniform on [0, 2 pi):  P(r < R) = 1 - (2 / pi) arccos(R / b); <rmin> = 2 b / pi.

Every case: `params` (what pstat_params takes), `options` (max_sep, min_sep, nbins, rmax, q), `expect`: `msd_s` and `msd` (the
separations judged and R2 there), `rmin`, `hist` (the share of a chain's counted pairs per column, "above" last), `sq`.

Run:  python tests/golden/make_pdist_closed_form.py   (rewrites the JSON next to this file)
"""
import json
import math
import os

N = 12
MAGNITUDES = (0.0, 0.5, 1.5, 3.0, 6.0)
NBINS = 8


def sinc(x):
    return 1.0 if x == 0.0 else math.sin(x) / x


def langevin(f):
    return 0.0 if f == 0.0 else 1.0 / math.tanh(f) - 1.0 / f


def msd(s, b, m):
    return b * b * ((s - 0.5) + (s * s - s + 0.5) * m * m)


def debye_free(q, n, b):
    return 1.0 + (2.0 / n) * sum((n - s) * sinc(q * b / 2) ** 2 * sinc(q * b) ** (s - 1) for s in range(1, n))


def closed_forms():
    seps = list(range(1, N))
    out = {}
    out["fjc"] = dict(
        params=dict(n=N, E0=0.0, Fz=0.0, Fx=0.0, kT=1.0, b=1.0),
        options=dict(max_sep=-1, min_sep=1, nbins=0, rmax=1.0, q=list(MAGNITUDES)),
        expect=dict(msd_s=seps, msd=[msd(s, 1.0, 0.0) for s in seps], sq=[debye_free(q, N, 1.0) for q in MAGNITUDES]))
    f = 1.5
    out["fixed_force"] = dict(
        params=dict(n=N, E0=0.0, Fz=f, Fx=0.0, kT=1.0, b=1.0),
        options=dict(max_sep=-1, min_sep=1, nbins=0, rmax=1.0, q=[]),
        expect=dict(msd_s=seps, msd=[msd(s, 1.0, langevin(f)) for s in seps]))
    out["planar"] = dict(
        params=dict(n=N, E0=0.0, Fz=0.0, kT=1.0, cluster_prob=0.0),
        options=dict(max_sep=-1, min_sep=1, nbins=0, rmax=1.0, q=[]),
        expect=dict(msd_s=seps, msd=[msd(s, 1.0, 0.0) for s in seps]))
    out["dimer"] = dict(
        params=dict(n=2, E0=0.0, Fz=0.0, Fx=0.0, kT=1.0, b=1.0),
        options=dict(max_sep=-1, min_sep=1, nbins=NBINS, rmax=1.0, q=[]),
        expect=dict(msd_s=[1], msd=[msd(1, 1.0, 0.0)], rmin=2.0 / 3.0,
                    hist=[(2 * k + 1) / NBINS ** 2 for k in range(NBINS)] + [0.0]))
    cdf = lambda R: 1.0 - (2.0 / math.pi) * math.acos(R)
    out["planar_dimer"] = dict(
        params=dict(n=2, E0=0.0, Fz=0.0, kT=1.0, cluster_prob=0.0),
        options=dict(max_sep=-1, min_sep=1, nbins=NBINS, rmax=1.0, q=[]),
        expect=dict(msd_s=[1], msd=[msd(1, 1.0, 0.0)], rmin=2.0 / math.pi,
                    hist=[cdf((k + 1) / NBINS) - cdf(k / NBINS) for k in range(NBINS)] + [0.0]))
    return out


if __name__ == "__main__":
    doc = {"_generator": "tests/golden/make_pdist_closed_form.py (closed forms; not reference output)", **closed_forms()}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pdist_closed_form.json")
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", path)
