"""Generate tests/golden/vec_terms.npz: the inputs of the row finalisers' cases
(tests/vec_cases.py build_pool: full_loo, fitc_lambda, fitc_loo, surface_point) and, per row,
erf(z/√2) and exp(−z²/2) at the standardised residual z that the row's float64 inputs define,
evaluated with mpmath at 60 digits and stored as float64 hi/lo pairs (hi = float(r),
lo = float(r − hi)).  numpy has no extended-precision erf, and the GPU tests must not need
mpmath, so they load this file; the rest of every reference is numpy longdouble arithmetic.

Four families of z, all from the values the kernels start from (α, d and r are the in-order
float64 sums of the stored slabs):
  full   z = α/√d                                  (full_loo: μ = y − α/d, σ² = 1/d)
  fitc   a = (y − g)/λ, d = 1/λ − r/λ², z = a/√d   (fitc_loo)
  surf0, surf1   z = s²α/√(2s² − s⁴d), s² = SURF_S2[0], [1]   (surface_point's first sum)

Usage:  python tests/golden/make_vec_terms.py   (rewrites the file; needs mpmath)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import vec_cases as C  # noqa: E402

OUT = os.path.join(HERE, "vec_terms.npz")
DIGITS = 60


def reference(g):
    """erf(z/√2) and exp(−z²/2) of every row of every family as (hi, lo) pairs."""
    import mpmath as mp
    mp.mp.dps = DIGITS
    f = lambda v: mp.mpf(float(v))
    v = C.pool_z_inputs(g)
    n = len(g["y"])
    out = {}

    def store(name, zs):
        for key, fn in (("erf", lambda z: mp.erf(z / mp.sqrt(2))), ("exp", lambda z: mp.exp(-z * z / 2))):
            hi, lo = np.empty(n), np.empty(n)
            for i, z in enumerate(zs):
                r = fn(z)
                hi[i] = float(r)
                lo[i] = float(r - mp.mpf(hi[i]))
            out["%s_%s_hi" % (name, key)] = hi
            out["%s_%s_lo" % (name, key)] = lo

    store("full", [f(a) / mp.sqrt(f(d)) for a, d in zip(v["alpha"], v["dinv"])])
    zs = []
    for y, lam, r, gg in zip(g["y"], g["fitc_lam"], v["r"], g["fitc_g"]):
        a = (f(y) - f(gg)) / f(lam)
        d = 1 / f(lam) - f(r) / (f(lam) * f(lam))
        zs.append(a / mp.sqrt(d))
    store("fitc", zs)
    for k, s2 in enumerate(C.SURF_S2):
        s2 = f(s2)
        store("surf%d" % k, [s2 * f(a) / mp.sqrt(2 * s2 - s2 * s2 * f(d)) for a, d in zip(v["alpha"], v["dinv"])])
    return out


if __name__ == "__main__":
    g = C.build_pool()
    np.savez(OUT, **g, **reference(g))
    print("wrote %s: %d rows per family" % (OUT, len(g["y"])))
