"""numpy twin of the replica-exchange contract (the device's statement is polymer_stats_amd/csrc/pstat_exchange.hip).

TEST INFRASTRUCTURE ONLY.  The contract is restated here, not shared:
  ladder     cases that differ in nothing but kT, seed, chain_id0; rungs = its cases by (kT, case index) ascending
  pairing    round t pairs rungs (2j + (t & 1), 2j + 1 + (t & 1)); a rung without a partner sits the round out
  criterion  f64: d = (1 / kT_a - 1 / kT_b) * (U_a - U_b); accept iff U_a, U_b finite and (d >= 0 or u < exp(d))
  stream     o = Philox4x32-10(key = (seed_lo, seed_hi), ctr = (k, lower rung's case, 0x7e3a9e0d, t)),
             u = ((o[0] << 21) | (o[1] >> 11)) * 2^-53
"""
import numpy as np

M32 = 0xFFFFFFFF
TAG = 0x7E3A9E0D


def philox4x32_10(ctr, key):
    """Philox4x32-10 of one counter (4 words) under one key (2 words): Salmon et al., SC'11."""
    c0, c1, c2, c3 = (int(x) & M32 for x in ctr)
    k0, k1 = (int(x) & M32 for x in key)
    for _ in range(10):
        p0 = 0xD2511F53 * c0
        p1 = 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0 = (k0 + 0x9E3779B9) & M32
        k1 = (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def uniform(seed, k, lower_case, t):
    o = philox4x32_10((k, lower_case, TAG, t), (seed & M32, (seed >> 32) & M32))
    return float((o[0] << 21) | (o[1] >> 11)) * 2.0 ** -53


def rungs(ladder, kT):
    """{ladder id: [case indices by (kT, index) ascending]} of the cases with ladder id >= 0."""
    out = {}
    for i, l in enumerate(ladder):
        if l >= 0:
            out.setdefault(int(l), []).append(i)
    return {l: sorted(c, key=lambda i: (kT[i], i)) for l, c in out.items()}


def schedule(nrungs, t):
    """The pairs (lower rung, upper rung) of round t in a ladder of `nrungs` rungs."""
    return [(r, r + 1) for r in range(t & 1, nrungs - 1, 2)]


def pairs(ladder, kT, t):
    """The pairs (lower case, upper case) of round t over all ladders."""
    return [(c[a], c[b]) for c in rungs(ladder, kT).values() for a, b in schedule(len(c), t)]


def decide(seed, t, a, b, kT, U, per):
    """Round t, pair of cases (a, b), a the lower rung: (accept[per], margin[per]) from the energies U[ncases * per] and the
    cases' kT; margin = |u - exp(d)| where the draw decides (d < 0), inf where it does not."""
    acc = np.zeros(per, dtype=bool)
    margin = np.full(per, np.inf)
    for k in range(per):
        Ua, Ub = np.float64(U[a * per + k]), np.float64(U[b * per + k])
        with np.errstate(all="ignore"):
            d = (np.float64(1.0) / np.float64(kT[a]) - np.float64(1.0) / np.float64(kT[b])) * (Ua - Ub)
            u = uniform(seed, k, a, t)
            if not (np.isfinite(Ua) and np.isfinite(Ub)):
                continue
            if d >= 0:
                acc[k] = True
            else:
                e = float(np.exp(d))
                acc[k] = u < e
                margin[k] = abs(u - e)
    return acc, margin
