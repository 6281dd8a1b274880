"""Generate tests/golden/grad_terms.npz: the inputs of the per-point gradient kernels
(loo_grad_terms, fitc_grad_terms, fold_terms) and, for each point, erf(z/√2) and exp(−z²/2) at
the standardised LOO residual z that the point's float64 inputs define, evaluated with mpmath at
60 digits and stored as float64 hi/lo pairs (hi = float(r), lo = float(r − hi)).  numpy has no
extended-precision erf, and the GPU tests must not need mpmath, so they load this file; the rest
of every reference is numpy longdouble arithmetic (tests/grad_cases.py).

Three families over one grid — z over the list below (score_terms' list plus ±0.8325546, where
2φ(z) = 1/√π and the variance derivative cancels) crossed with d (or 1/λ) and y, plus 200 draws
z ~ 3·N(0, 1):
  full  (y, alpha, dinv):  z = (alpha/dinv)·√dinv
  fitc  (y, lam, r, g):    a = (y − g)/lam, d = 1/lam − r/lam², z = (a/d)·√d
  fold  (y, r, c):         z = r/√c
Each family's inputs are built in float64 so that z lands near the grid value; the stored erf
and exp are those of the z the inputs define exactly, whatever rounding did to it.

Usage:  python tests/golden/make_grad_terms.py   (rewrites the file; needs mpmath)
"""
import math
import os

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "grad_terms.npz")
DIGITS = 60
Z_PAIRS = (1e-300, 1e-8, 0.5, 0.8325546, 1.0, 2.0, 5.0, 8.3, 26.0, 37.5, 38.6, 40.0)
Z_FIXED = (0.0,) + tuple(s * z for z in Z_PAIRS for s in (1.0, -1.0)) + (1e5, -1e10)
D_LIST = (1e-6, 1e-3, 0.3, 1.0, 50.0, 1e4, 1e8)
Y_LIST = (0.0, 0.3, -7.0, 1e6)
RHO = (0.0, 0.25, 0.5)          # fitc: r/λ, so that d = (1 − ρ)/λ
N_RANDOM = 200


def grid():
    """{name: float64 array} of the three families' inputs."""
    pts = [(z, d, y) for z in Z_FIXED for d in D_LIST for y in Y_LIST]
    draws = 3.0 * np.random.default_rng(61).standard_normal(N_RANDOM)
    pts += [(float(z), D_LIST[i % len(D_LIST)], Y_LIST[(i // 7) % len(Y_LIST)])
            for i, z in enumerate(draws)]
    z = np.array([p[0] for p in pts])
    d = np.array([p[1] for p in pts])
    y = np.array([p[2] for p in pts])
    g = {"z_target": z, "y": y}
    # full: alpha = z·√d
    g["full_dinv"] = d
    g["full_alpha"] = z * np.sqrt(d)
    # fitc: 1/λ = d (the grid value), r = ρλ, g = y − aλ with a = z·√(d(1 − ρ))
    rho = np.array([RHO[i % len(RHO)] for i in range(len(pts))])
    lam = 1.0 / d
    g["fitc_lam"] = lam
    g["fitc_r"] = rho * lam
    g["fitc_g"] = y - (z * np.sqrt(d * (1.0 - rho))) * lam
    # fold: c = 1/d, r = z·√c
    g["fold_c"] = 1.0 / d
    g["fold_r"] = z * np.sqrt(g["fold_c"])
    return g


def reference(g):
    """erf(z/√2) and exp(−z²/2) of every point of every family as (hi, lo) pairs."""
    import mpmath as mp
    mp.mp.dps = DIGITS
    f = lambda v: mp.mpf(float(v))
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

    store("full", [f(a) / mp.sqrt(f(d)) for a, d in zip(g["full_alpha"], g["full_dinv"])])
    zs = []
    for y, lam, r, gg in zip(g["y"], g["fitc_lam"], g["fitc_r"], g["fitc_g"]):
        a = (f(y) - f(gg)) / f(lam)
        d = 1 / f(lam) - f(r) / (f(lam) * f(lam))
        zs.append(a / mp.sqrt(d))
    store("fitc", zs)
    store("fold", [f(r) / mp.sqrt(f(c)) for r, c in zip(g["fold_r"], g["fold_c"])])
    return out


if __name__ == "__main__":
    g = grid()
    np.savez(OUT, **g, **reference(g))
    print("wrote %s: %d points per family" % (OUT, len(g["y"])))
