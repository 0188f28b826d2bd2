"""Generates tests/golden/planar_closed_form.json: equilibrium ensemble averages of NON-INTERACTING PLANAR chains by
single-monomer quadrature (scipy).  Our own derivation, not reference output -- the reference holds no fixtures, so
parity stays "unpinned".

A non-interacting planar chain factorises into iid monomers with density (2D/inc/acceptance.jl:18-22,
2D/inc/energy.jl:7-9, 2D/inc/eap_chain.jl:33,64, 2D/inc/dipole_response.jl:7-27), with NO Jacobian:

    rho(phi) ~ exp(-[u(phi) - b (Fx cos(phi) + Fz sin(phi))] / kT),     n = (cos(phi), sin(phi))
    u = -1/2 E0 mu_2,   mu = (K1-K2) E0 sin(phi) n + (0, K2 E0)  (dielectric)   or   mu * n  (polar)

and then   <r> = n b <n>,  <r_j^2> = n b^2 Var(n_j) + <r_j>^2,  <p> = n <mu>,
           <p_j^2> = n Var(mu_j) + <p_j>^2,  <U> = n <w>,  <U^2> = n Var(w) + <U>^2,
with w = u - b F.n the one-monomer energy.  Cross terms vanish by independence.

It is the density that single-monomer Metropolis samples, i.e. the planar main with --cluster-prob 0.  Names are the
16-vector's (r1, r3: components 1 and 2; every y entry is 0).

Run:  python tests/golden/make_planar_closed_form.py   (rewrites the JSON next to this file)
"""
import json
import os

import numpy as np
from scipy import integrate

CASES = {
    "n20_E0_0_Fz1": dict(chain="dielectric", n=20, E0=0.0, K1=1.0, K2=0.0, mu=0.01, kT=1.0, Fz=1.0, Fx=0.0, b=1.0),
    "diel_n25_E0_1_K1_1_Fz05": dict(chain="dielectric", n=25, E0=1.0, K1=1.0, K2=0.0, mu=0.01, kT=1.0, Fz=0.5, Fx=0.0, b=1.0),
    "diel_n100_E0_1_K2_1_Fx1": dict(chain="dielectric", n=100, E0=1.0, K1=0.0, K2=1.0, mu=0.01, kT=1.0, Fz=0.0, Fx=1.0, b=1.0),
    "polar_n25_E0_1_mu09_Fz1_Fx025_kT08_b12": dict(chain="polar", n=25, E0=1.0, K1=1.0, K2=0.0, mu=0.9, kT=0.8, Fz=1.0, Fx=0.25, b=1.2),
}


def one_monomer_moments(c):
    E0, K1, K2, mu, kT, Fz, Fx, b = (c[k] for k in ("E0", "K1", "K2", "mu", "kT", "Fz", "Fx", "b"))

    def fields(ph):
        nh = np.array([np.cos(ph), np.sin(ph)])
        if c["chain"] == "dielectric":
            m = (K1 - K2) * E0 * np.sin(ph) * nh + np.array([0.0, K2 * E0])
        else:
            m = mu * nh
        u = -0.5 * E0 * m[1]
        w = u - b * (Fx * nh[0] + Fz * nh[1])
        return nh, m, w

    def integral(f):
        val, _ = integrate.quad(lambda ph: f(ph) * np.exp(-fields(ph)[2] / kT), 0.0, 2 * np.pi, epsabs=1e-13, epsrel=1e-13,
                                limit=200)
        return val

    Z = integral(lambda ph: 1.0)
    out = {}
    for j in range(2):
        out[f"n{j}"] = integral(lambda ph: fields(ph)[0][j]) / Z
        out[f"n{j}sq"] = integral(lambda ph: fields(ph)[0][j] ** 2) / Z
        out[f"m{j}"] = integral(lambda ph: fields(ph)[1][j]) / Z
        out[f"m{j}sq"] = integral(lambda ph: fields(ph)[1][j] ** 2) / Z
    out["w"] = integral(lambda ph: fields(ph)[2]) / Z
    out["wsq"] = integral(lambda ph: fields(ph)[2] ** 2) / Z
    return out


def chain_averages(c):
    m = one_monomer_moments(c)
    n, b = c["n"], c["b"]
    avg = {k: 0.0 for k in ("r2", "r2sq", "p2", "p2sq")}
    rsq = psq = 0.0
    for j, slot in ((0, 1), (1, 3)):       # component 1 -> the x slots, component 2 -> the z slots
        rj = n * b * m[f"n{j}"]
        rj2 = n * b * b * (m[f"n{j}sq"] - m[f"n{j}"] ** 2) + rj * rj
        pj = n * m[f"m{j}"]
        pj2 = n * (m[f"m{j}sq"] - m[f"m{j}"] ** 2) + pj * pj
        avg[f"r{slot}"], avg[f"r{slot}sq"], avg[f"p{slot}"], avg[f"p{slot}sq"] = rj, rj2, pj, pj2
        rsq += rj2
        psq += pj2
    avg["rsq"], avg["psq"] = rsq, psq
    avg["U"] = n * m["w"]
    avg["Usq"] = n * (m["wsq"] - m["w"] ** 2) + avg["U"] ** 2
    return avg


def main():
    out = {"_generator": "tests/golden/make_planar_closed_form.py (scipy.integrate.quad; not reference output)", "cases": {}}
    for name, c in CASES.items():
        avg = chain_averages(c)
        out["cases"][name] = {"params": c, "avg": avg}
        print(name, {k: round(v, 7) for k, v in avg.items() if k in ("r1", "r3", "r1sq", "r3sq", "p3", "U", "Usq")})
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "planar_closed_form.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote", path)


if __name__ == "__main__":
    main()
