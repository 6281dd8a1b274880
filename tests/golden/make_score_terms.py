"""Generate tests/golden/score_terms.npz: the Gaussian CRPS and log-score terms of single
predictive points (crps KF:60-68, logs KF:52-57; c is the VARIANCE), evaluated with mpmath at
60 digits from the float64 inputs and stored as float64 hi/lo pairs (hi = float(r),
lo = float(r − hi): 106 bits of the value).  numpy and scipy have no extended-precision erf,
and the GPU tests must not need mpmath, so they load this file.

Grid: z over the fixed list below (the centre, the tails where pdf and 1 − cdf underflow, the
point z ≈ 38.6 where exp(−z²/2) leaves the normal range) crossed with every variance, plus 200
draws z ~ 3·N(0, 1) with the variances taken in turn; y = fl(m + z·√c), m = 0.3 (m = 0 at
c = 1e200, so that z survives the rounding of y at both ends of the range).

Usage:  python tests/golden/make_score_terms.py   (rewrites the file; needs mpmath)
"""
import math
import os

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "score_terms.npz")
DIGITS = 60
Z_PAIRS = (1e-300, 1e-8, 0.5, 1.0, 2.0, 5.0, 8.3, 26.0, 37.5, 38.6, 40.0)
Z_FIXED = (0.0,) + tuple(s * z for z in Z_PAIRS for s in (1.0, -1.0)) + (1e5, -1e10)
VARIANCES = (1e-300, 1e-12, 0.25, 1.0, 3.7, 1e12, 1e200)
N_RANDOM = 200


def grid():
    """(m, c, y) float64 arrays of the fixture's points."""
    zs = [(z, c) for z in Z_FIXED for c in VARIANCES]
    draws = 3.0 * np.random.default_rng(60).standard_normal(N_RANDOM)
    zs += [(float(z), VARIANCES[i % len(VARIANCES)]) for i, z in enumerate(draws)]
    m = np.array([0.0 if c == 1e200 else 0.3 for _, c in zs])
    c = np.array([c for _, c in zs])
    y = np.array([mi + z * math.sqrt(ci) for (z, _), mi, ci in zip(zs, m, c)])
    return m, c, y


def reference(m, c, y):
    """CRPS and LogS terms of the points as (hi, lo) float64 pairs, from mpmath."""
    import mpmath as mp
    mp.mp.dps = DIGITS
    out = {k: np.empty(len(m)) for k in ("crps_hi", "crps_lo", "logs_hi", "logs_lo")}
    for i, (mi, ci, yi) in enumerate(zip(m, c, y)):
        mi, ci, yi = mp.mpf(float(mi)), mp.mpf(float(ci)), mp.mpf(float(yi))
        s = mp.sqrt(ci)
        z = (yi - mi) / s
        pdf = mp.exp(-z * z / 2) / mp.sqrt(2 * mp.pi)
        crps = s * (z * mp.erf(z / mp.sqrt(2)) + 2 * pdf - 1 / mp.sqrt(mp.pi))
        logs = (yi - mi) ** 2 / (2 * ci) + mp.log(s) + mp.log(2 * mp.pi) / 2
        for name, r in (("crps", crps), ("logs", logs)):
            hi = float(r)
            out[name + "_hi"][i] = hi
            out[name + "_lo"][i] = float(r - mp.mpf(hi))
    return out


if __name__ == "__main__":
    m, c, y = grid()
    np.savez(OUT, m=m, c=c, y=y, **reference(m, c, y))
    print("wrote %s: %d points" % (OUT, len(m)))
