"""Generates tests/golden/corr_closed_form.json: lag correlations in closed form for tests/test_corr_cpu.py and
tests/test_gpu_corr.py.  Our own derivations by quadrature (scipy), not reference output.  kT = b = 1 throughout.

bending      A free chain (E0 = 0, F = 0) whose only energy is kappa / 2 psi_j^2 on the n - 1 bond angles.  In the measure
             prod_i sin(theta_i) dtheta_i dphi_i the successive bonds are independent rotations, each with the polar-angle density
             ~ sin(psi) exp(-kappa psi^2 / (2 kT)) on [0, pi], so <n_i . n_{i+k}> = <cos psi>^k: the freely rotating chain.
fixed_force  Non-interacting dielectric monomers under a field along z and a force (Fx, 0, Fz): a monomer's energy is
             -E0^2 / 2 ((K1 - K2) cos^2 theta + K2) - b (Fz cos theta + Fx sin theta cos phi), the monomers are iid, so for k >= 1
             nn = |<n>|^2, zz = <n_z>^2, mm = |<mu>|^2 and at k = 0 nn = 1, zz = <n_z^2>, mm = <|mu|^2>, with
             mu = (K1 - K2) E0 cos(theta) n + K2 E0 z.  The phi integrals are Bessel functions: int exp(a cos phi) = 2 pi I0(a),
             int cos(phi) exp(a cos phi) = 2 pi I1(a); the theta integral is done by quad.
planar       Non-interacting planar monomers, E0 = 0, force F along the field axis (component 2): phi has the von Mises density
             ~ exp(F sin phi), so <n> = (0, I1(F) / I0(F)), <n_2^2> = (1 + I2(F) / I0(F)) / 2.

Run:  python tests/golden/make_corr_closed_form.py   (rewrites the JSON next to this file)
"""
import json
import os

import numpy as np
from scipy import integrate, special

N = 12


def bending(kappa=2.0, kT=1.0, n=N):
    w = lambda psi: np.sin(psi) * np.exp(-kappa * psi * psi / (2.0 * kT))
    z = integrate.quad(w, 0.0, np.pi, epsabs=1e-14, epsrel=1e-14)[0]
    c = integrate.quad(lambda psi: np.cos(psi) * w(psi), 0.0, np.pi, epsabs=1e-14, epsrel=1e-14)[0] / z
    return dict(params=dict(n=n, E0=0.0, Fz=0.0, Fx=0.0, kT=kT, bend_mod=kappa, bend_angle=0.0, move_set=1, cluster_prob=1.0),
                cos_psi=c, expect=dict(nn=[c ** k for k in range(n)]))


def fixed_force(E0=1.0, K1=0.5, K2=0.2, Fz=0.5, Fx=0.3, kT=1.0, b=1.0, n=N):
    kap, fz, fx = E0 * E0 * (K1 - K2) / (2.0 * kT), Fz * b / kT, Fx * b / kT

    def avg(g0, g1):
        """<g0(theta) + g1(theta) cos(phi)>: the phi integral in closed form (exponentially scaled Bessel functions)."""
        base = lambda t: np.sin(t) * np.exp(kap * np.cos(t) ** 2 + fz * np.cos(t) + fx * np.sin(t))
        num = lambda t: base(t) * (g0(t) * special.ive(0, fx * np.sin(t)) + g1(t) * special.ive(1, fx * np.sin(t)))
        den = lambda t: base(t) * special.ive(0, fx * np.sin(t))
        q = lambda f: integrate.quad(f, 0.0, np.pi, epsabs=1e-13, epsrel=1e-13)[0]
        return q(num) / q(den)

    zero = lambda t: 0.0 * t
    x = avg(zero, np.sin)                                     # <sin theta cos phi>
    z = avg(np.cos, zero)
    z2 = avg(lambda t: np.cos(t) ** 2, zero)
    zx = avg(zero, lambda t: np.cos(t) * np.sin(t))           # <cos theta sin theta cos phi>
    a, c = (K1 - K2) * E0, K2 * E0
    mu_mean = np.array([a * zx, 0.0, a * z2 + c])
    mu2 = a * a * z2 + 2.0 * a * c * z2 + c * c               # |a z n + c z^|^2 = a^2 z^2 + 2 a c z^2 + c^2
    return dict(params=dict(n=n, E0=E0, K1=K1, K2=K2, Fz=Fz, Fx=Fx, kT=kT, b=b),
                expect=dict(nn=[1.0] + [x * x + z * z] * (n - 1), zz=[z2] + [z * z] * (n - 1),
                            mm=[mu2] + [float(mu_mean @ mu_mean)] * (n - 1)))


def planar(F=1.0, kT=1.0, n=N):
    f = F / kT
    m = special.iv(1, f) / special.iv(0, f)
    s2 = 0.5 * (1.0 + special.iv(2, f) / special.iv(0, f))
    return dict(params=dict(n=n, E0=0.0, Fz=F, kT=kT, cluster_prob=0.0),
                expect=dict(nn=[1.0] + [m * m] * (n - 1), zz=[s2] + [m * m] * (n - 1)))


def closed_forms():
    return dict(bending=bending(), fixed_force=fixed_force(), planar=planar())


def main():
    out = closed_forms()
    out["_generator"] = "tests/golden/make_corr_closed_form.py (quadrature; not reference output)"
    print("bending <cos psi> =", out["bending"]["cos_psi"])
    # the theta quadrature against a brute-force double integral
    E0, K1, K2, Fz, Fx = 1.0, 0.5, 0.2, 0.5, 0.3
    w = lambda p, t: np.sin(t) * np.exp(E0 * E0 * (K1 - K2) / 2 * np.cos(t) ** 2 + Fz * np.cos(t) + Fx * np.sin(t) * np.cos(p))
    den = integrate.dblquad(w, 0, np.pi, 0, 2 * np.pi, epsabs=1e-12, epsrel=1e-12)[0]
    x = integrate.dblquad(lambda p, t: np.sin(t) * np.cos(p) * w(p, t), 0, np.pi, 0, 2 * np.pi, epsabs=1e-12, epsrel=1e-12)[0] / den
    z = integrate.dblquad(lambda p, t: np.cos(t) * w(p, t), 0, np.pi, 0, 2 * np.pi, epsabs=1e-12, epsrel=1e-12)[0] / den
    assert abs(x * x + z * z - out["fixed_force"]["expect"]["nn"][1]) < 1e-10, (x, z)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "corr_closed_form.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
    print("wrote", path)


if __name__ == "__main__":
    main()
