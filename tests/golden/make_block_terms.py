"""Generate tests/golden/blk_terms.npz: the transcendental references of the block-LOO,
energy-score and joint kernels' cases (tests/block_cases.py term_inputs), evaluated with mpmath at
60 digits and stored as float64 hi/lo pairs (hi = float(r), lo = float(r − hi)):
  log       log λ over fold_logdet's pool of 300 λ;
  pow0.5, pow1.5   D^β over es_reduce's 33 × 34 pool of distances;
  exp_b*_d* exp of joint_cov's arguments −½‖(x_i − x_j)/ℓ‖² on the sampled lower-triangle entries of
            each (b, d): the diagonal and up to 200 below it (the argument itself is a longdouble,
            handed over as a hi/lo pair).
The GPU tests must not need mpmath, so they load this file; the rest of every reference is numpy
longdouble arithmetic.  The inputs are not stored: they are m·2^e from numpy's generator, the same
bits everywhere.

Usage:  python tests/golden/make_block_terms.py   (rewrites the file; needs mpmath)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import block_cases as C  # noqa: E402

OUT = os.path.join(HERE, "blk_terms.npz")
DIGITS = 60


def reference(g):
    """{name_hi, name_lo} for every family of g = block_cases.term_inputs()."""
    import mpmath as mp
    mp.mp.dps = DIGITS
    out = {}

    def store(name, values, shape):
        hi, lo = np.empty(len(values)), np.empty(len(values))
        for i, r in enumerate(values):
            hi[i] = float(r)
            lo[i] = float(r - mp.mpf(hi[i]))
        out[name + "_hi"], out[name + "_lo"] = hi.reshape(shape), lo.reshape(shape)

    f = lambda v: mp.mpf(float(v))
    store("log", [mp.log(f(v)) for v in g["log"]], g["log"].shape)
    for beta in (0.5, 1.5):
        store("pow%g" % beta, [mp.power(f(v), f(beta)) for v in g["pow"].reshape(-1)], g["pow"].shape)
    for k in sorted(g):
        if k.startswith("arg_"):
            hi, lo = g[k]
            store("exp_" + k[4:], [mp.exp(f(a) + f(b)) for a, b in zip(hi, lo)], hi.shape)
    return out


if __name__ == "__main__":
    ref = reference(C.term_inputs())
    np.savez(OUT, **ref)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(ref), os.path.getsize(OUT)))
