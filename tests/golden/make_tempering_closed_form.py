"""Generates tests/golden/tempering_closed_form.json: closed-form equilibrium averages of the temperature ladder that
tests/test_gpu_tempering.py equilibrates with and without replica exchange.

A dielectric, non-interacting chain of n = 8 monomers at E0 = 3, K1 = 1, K2 = 0, Fz = 0.2, b = 1: every monomer sits in the
symmetric double well u = -4.5 cos^2(theta), tilted by the force; the barrier is 18 kT on the coldest rung.  The integrals are
those of make_closed_form.py (our own derivation, not reference output).

Run:  python tests/golden/make_tempering_closed_form.py   (rewrites the JSON next to this file)
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_closed_form import chain_averages, one_monomer_moments  # noqa: E402,F401  (chain_averages integrates with one_monomer_moments)

LADDER = [0.25, 0.35, 0.5, 0.75, 1.2, 2.0, 4.0]
BASE = dict(chain="dielectric", n=8, E0=3.0, K1=1.0, K2=0.0, mu=0.01, Fz=0.2, Fx=0.0, b=1.0)


def main():
    out = {"_generator": "tests/golden/make_tempering_closed_form.py (scipy.integrate.dblquad; not reference output)",
           "params": BASE, "kT": LADDER, "rungs": []}
    for kT in LADDER:
        c = dict(BASE, kT=kT)
        per_monomer = one_monomer_moments(c)
        avg, var = chain_averages(c)
        out["rungs"].append({"kT": kT, "avg": avg, "var1": var, "n3": per_monomer["n2"]})
        print(kT, {k: round(avg[k], 6) for k in ("r3", "r3sq", "p3", "U")})
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tempering_closed_form.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote", path)


if __name__ == "__main__":
    main()
