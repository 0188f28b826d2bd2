"""Generates tests/golden/energy_closed_form.json: equilibrium ensemble means of the energy recorder's columns that have a
finite variance, by single-monomer (single-bond) quadrature (scipy).  Our own derivation, not reference output.

  field, work   of NON-INTERACTING chains under field and force.  The chain factorises into iid monomers with the density of
                make_closed_form.py (3D, measure sin(theta)) or make_planar_closed_form.py (planar, no Jacobian):
                    rho ~ exp(-[u - b (Fx n_x + Fz n_z)] / kT),   u = -1/2 E0 mu_z   (planar: the second components)
                so  <field> = n <u>  and  <work> = -n b (Fx <n_x> + Fz <n_z>).
  bend          of the freely rotating bending chain of the README's correlation example (E0 = 0, no force, kappa = 2, psi0 = 0,
                single moves only): the n - 1 bond angles are iid with density exp(-kappa psi^2 / (2 kT)) sin(psi) on [0, pi], so
                    <bend> = (n - 1) <kappa psi^2 / 2>.
The PAIR columns are judged by no statistical test: in these ensembles their variance is infinite.  Two neighbours are
r = b |n_i + n_{i+1}| / 2 apart, and for nearly antiparallel neighbours the density of r near 0 goes as r dr (the solid angle
around the antiparallel direction) against a term of order 1 / r^3: the second moment, the integral of r^-6 r dr, diverges, and
even the mean converges only by cancellation over the orientations.  The same holds at every separation for a chain that may
fold back on itself.  The pair columns are pinned exactly instead (tests/test_energy_cpu.py: the oracle's pair sums; closed forms
of a dimer and of the straight chain).

Run:  python tests/golden/make_energy_closed_form.py   (rewrites the JSON next to this file)
"""
import json
import os

import numpy as np
from scipy import integrate

CASES = {
    "fixed_force": dict(planar=False, params=dict(n=20, E0=1.5, K1=0.7, K2=0.3, kT=0.7, Fz=0.4, Fx=0.3, b=1.3)),
    "polar": dict(planar=False, params=dict(n=20, chain_type=1, E0=1.0, mu=1.0, kT=1.0, Fz=1.0, Fx=0.0, b=1.0)),
    "planar": dict(planar=True, params=dict(n=25, E0=1.0, K1=1.0, K2=0.0, kT=1.0, Fz=0.5, Fx=0.25, b=1.0, cluster_prob=0.0)),
    "bend": dict(planar=False, params=dict(n=12, E0=0.0, kT=1.0, bend_mod=2.0, bend_angle=0.0, move_set=1, cluster_prob=1.0)),
}
DEFAULTS = dict(E0=0.0, K1=1.0, K2=0.0, mu=1e-2, kT=1.0, Fz=0.0, Fx=0.0, b=1.0, chain_type=0, bend_mod=0.0, bend_angle=0.0)


def monomer_fields(c, planar):
    """(theta, phi) -> (n_x, n_z, u) of one monomer (planar: theta unused, the second component in the z place)."""
    def fields(th, ph):
        if planar:
            nx, nz = np.cos(ph), np.sin(ph)
        else:
            nx, nz = np.cos(ph) * np.sin(th), np.cos(th)
        mz = c["mu"] * nz if c["chain_type"] == 1 else (c["K1"] - c["K2"]) * c["E0"] * nz * nz + c["K2"] * c["E0"]
        return nx, nz, -0.5 * c["E0"] * mz
    return fields


def field_and_work(c, planar):
    fields = monomer_fields(c, planar)

    def weight(th, ph):
        nx, nz, u = fields(th, ph)
        return (1.0 if planar else np.sin(th)) * np.exp(-(u - c["b"] * (c["Fx"] * nx + c["Fz"] * nz)) / c["kT"])

    def integral(f):
        if planar:
            return integrate.quad(lambda ph: f(0.0, ph) * weight(0.0, ph), 0.0, 2 * np.pi, epsabs=1e-13, epsrel=1e-13, limit=200)[0]
        return integrate.dblquad(lambda ph, th: f(th, ph) * weight(th, ph), 0.0, np.pi, 0.0, 2 * np.pi, epsabs=1e-13, epsrel=1e-13)[0]

    Z = integral(lambda th, ph: 1.0)
    nx, nz, u = (integral(lambda th, ph, k=k: fields(th, ph)[k]) / Z for k in range(3))
    return c["n"] * u, -c["n"] * c["b"] * (c["Fx"] * nx + c["Fz"] * nz)


def bend(c):
    k, kT = c["bend_mod"], c["kT"]
    w = lambda psi: np.exp(-k * (psi - c["bend_angle"]) ** 2 / (2 * kT)) * np.sin(psi)
    Z = integrate.quad(w, 0.0, np.pi, epsabs=1e-14, epsrel=1e-14)[0]
    return (c["n"] - 1) * integrate.quad(lambda psi: 0.5 * k * (psi - c["bend_angle"]) ** 2 * w(psi), 0.0, np.pi, epsabs=1e-14, epsrel=1e-14)[0] / Z


def generate():
    out = {}
    for name, case in CASES.items():
        c = {**DEFAULTS, **case["params"]}
        expect = {}
        if c["bend_mod"] != 0.0:
            expect["bend"] = bend(c)
            expect["field"] = expect["work"] = 0.0
        else:
            expect["field"], expect["work"] = field_and_work(c, case["planar"])
        out[name] = dict(planar=case["planar"], params=case["params"], expect=expect)
    return out


if __name__ == "__main__":
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "energy_closed_form.json")
    with open(path, "w") as f:
        json.dump(generate(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)
