"""Generates tests/golden/shape_closed_form.json: the mean gyration tensor and form factor of chains of iid monomers in closed
form, for tests/test_shape_cpu.py and tests/test_gpu_shape.py.  Our own derivations by quadrature (scipy), not
reference output.

The monomers of the non-interacting energy are iid.  With the centres x_i = b (sum_{j <= i} n_j - n_i / 2), for j - i = k >= 1
  x_j - x_i = b (n_i / 2 + n_{i+1} + ... + n_{j-1} + n_j / 2), so
  <exp(i q . (x_j - x_i))> = chi_h(q)^2 chi(q)^(k-1),  chi(q) = <exp(i b q . n)>,  chi_h(q) = <exp(i b q . n / 2)>,
  S(q) = 1 + (2 / n) Re sum_{k=1}^{n-1} (n - k) chi_h^2 chi^(k-1),
  <G_ab> = (1 / n^2) sum_{i<j} <d_a d_b> = (b^2 / n^2) sum_k (n - k) [k^2 m_a m_b + (k - 1/2) C_ab],  m = <n>, C its covariance.
(<trg2> needs fourth moments of the whole chain and has no such form: the fixture does not carry it.)

fjc          3D, E0 = 0, F = 0: n uniform on the sphere, chi(q) = sin(q b) / (q b), m = 0, C = 1 / 3.
fixed_force  3D, E0 = 0, force Fz along z: density ~ sin(theta) exp(Fz b cos(theta) / kT), uniform in phi, so the phi integral of
             exp(i a sin(theta) cos(phi - phi0)) is 2 pi J0(a sin(theta)) with a = b sqrt(q_x^2 + q_y^2); theta by quad.
planar       E0 = 0, force F along the field axis (the z slot): phi has the von Mises density ~ exp(F sin(phi)), n = (cos phi, 0,
             sin phi); chi by quad over phi.

Run:  python tests/golden/make_shape_closed_form.py   (rewrites the JSON next to this file)
"""
import json
import os

import numpy as np
from scipy import integrate, special

N = 12
MAGNITUDES = (0.5, 1.5, 3.0, 6.0)


def _quad(f, lo, hi):
    return integrate.quad(f, lo, hi, epsabs=1e-14, epsrel=1e-13, limit=200)[0]


def monomer_3d(fz):
    """(chi(qvec), m[3], C[3, 3]) of the density ~ sin(theta) exp(fz cos(theta)); chi takes the wave-vector TIMES the length."""
    w = lambda t: np.sin(t) * np.exp(fz * (np.cos(t) - 1.0))
    z0 = _quad(w, 0.0, np.pi)
    avg = lambda g: _quad(lambda t: g(t) * w(t), 0.0, np.pi) / z0

    def chi(k):
        kp, kz = np.hypot(k[0], k[1]), k[2]
        re = avg(lambda t: np.cos(kz * np.cos(t)) * special.j0(kp * np.sin(t)))
        im = avg(lambda t: np.sin(kz * np.cos(t)) * special.j0(kp * np.sin(t)))
        return complex(re, im)

    mz, c2, s2 = avg(np.cos), avg(lambda t: np.cos(t) ** 2), avg(lambda t: np.sin(t) ** 2)
    return chi, np.array([0.0, 0.0, mz]), np.diag([s2 / 2.0, s2 / 2.0, c2 - mz * mz])


def monomer_planar(f):
    """The same for n = (cos phi, 0, sin phi) with the density ~ exp(f sin(phi))."""
    w = lambda p: np.exp(f * (np.sin(p) - 1.0))
    z0 = _quad(w, 0.0, 2.0 * np.pi)
    avg = lambda g: _quad(lambda p: g(p) * w(p), 0.0, 2.0 * np.pi) / z0

    def chi(k):
        ph = lambda p: k[0] * np.cos(p) + k[2] * np.sin(p)
        return complex(avg(lambda p: np.cos(ph(p))), avg(lambda p: np.sin(ph(p))))

    mz, cc, ss = avg(np.sin), avg(lambda p: np.cos(p) ** 2), avg(lambda p: np.sin(p) ** 2)
    cov = np.zeros((3, 3))                      # <cos phi> = <cos phi sin phi> = 0: the density is even about phi = pi / 2
    cov[0, 0], cov[2, 2] = cc, ss - mz * mz
    return chi, np.array([0.0, 0.0, mz]), cov


def form_factor(chi, qvec, b, n):
    k = b * np.asarray(qvec, dtype=float)
    if not np.any(k):
        return float(n)
    c, h = chi(k), chi(k / 2.0)
    return 1.0 + (2.0 / n) * sum((n - j) * (h * h * c ** (j - 1)).real for j in range(1, n))


def gyration(m, cov, b, n):
    g = np.zeros((3, 3))
    for k in range(1, n):
        g += (n - k) * (k * k * np.outer(m, m) + (k - 0.5) * cov)
    return g * b * b / (n * n)


def wave_vectors(extra=()):
    q = [[0.0, 0.0, 0.0]] + [[0.0, 0.0, m] for m in MAGNITUDES] + [[m, 0.0, 0.0] for m in MAGNITUDES] + [list(e) for e in extra]
    return q


def case(params, monomer, q, b, n):
    chi, m, cov = monomer
    g = gyration(m, cov, b, n)
    expect = dict(gxx=g[0, 0], gyy=g[1, 1], gzz=g[2, 2], gxy=g[0, 1], gxz=g[0, 2], gyz=g[1, 2], rg2=float(np.trace(g)),
                  sq=[form_factor(chi, qv, b, n) for qv in q])
    return dict(params=params, q=q, expect=expect)


def closed_forms():
    fjc = case(dict(n=N, E0=0.0, Fz=0.0, Fx=0.0, kT=1.0, b=1.0), monomer_3d(0.0), wave_vectors(), 1.0, N)
    ff = case(dict(n=N, E0=0.0, Fz=1.5, Fx=0.0, kT=1.0, b=1.0), monomer_3d(1.5), wave_vectors([(1.0, 1.0, 1.0)]), 1.0, N)
    pl = case(dict(n=N, E0=0.0, Fz=1.0, kT=1.0, cluster_prob=0.0), monomer_planar(1.0), wave_vectors(), 1.0, N)
    return dict(fjc=fjc, fixed_force=ff, planar=pl)


def main():
    out = closed_forms()
    out["_generator"] = "tests/golden/make_shape_closed_form.py (quadrature; not reference output)"
    # the free chain against its textbook forms
    chi = monomer_3d(0.0)[0]
    assert abs(chi(np.array([0.0, 0.0, 2.0])) - np.sin(2.0) / 2.0) < 1e-12
    assert abs(out["fjc"]["expect"]["rg2"] - 253.0 / 144.0) < 1e-12
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "shape_closed_form.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
    print("wrote", path)
    for name in ("fjc", "fixed_force", "planar"):
        print(name, {k: (np.round(v, 6).tolist() if k == "sq" else round(v, 6)) for k, v in out[name]["expect"].items()})


if __name__ == "__main__":
    main()
