"""Inputs, extended-precision references, error bounds and float64 restatements of the gradient
layer's kernels (kernels_grad.hip, kernels_fitc_grad.hip, fold_terms in kernels_block.hip),
shared by test_grad_terms_host.py (CPU: every bound holds, with room, for a numpy float64
restatement of each kernel, and every listed defect built into a restatement fails a named check)
and test_gpu_grad_terms.py (the kernels, through the gps_*_diag entry points).  Nothing here
touches the GPU or imports mpmath.  DESIGN §23 has the derivations in full.

u = 2^-53.  References are numpy longdouble from the float64 values the kernel receives; erf and
exp of the per-point terms come from tests/golden/grad_terms.npz (mpmath, 60 digits, hi/lo).
"""
import math
import os

import numpy as np

from elementwise_cases import CLUSTER_POS, GOLDEN, LD, SUBNORMAL, U, inv_ell_of, need_extended

OBJ_NLML, OBJ_CRPS, OBJ_LOGS = 0, 1, 2
FIXTURE = os.path.join(GOLDEN, "grad_terms.npz")
PI_LD = LD(math.pi) + LD(1.2246467991473532e-16)          # π to 2^-106
INV_SQRT_PI = 1 / np.sqrt(PI_LD)
INV_SQRT_2PI = 1 / np.sqrt(2 * PI_LD)
K_PDF, K_SQRT_HALF, K_ISP = 0.39894228040143267794, 0.70710678118654752440, 0.56418958354775628695
K_ISP_SHORT = 0.5641895835                                 # the defect: ten digits
_erf = np.vectorize(math.erf, otypes=[np.float64])


def ld(a):
    return np.asarray(a, np.float64).astype(LD)


def load_fixture():
    """The fixture's inputs (float64) and, per family, erf(z/√2) and exp(−z²/2) as longdouble."""
    need_extended()
    with np.load(FIXTURE, allow_pickle=False) as z:
        g = {k: z[k] for k in z.files}
    for fam in ("full", "fitc", "fold"):
        for key in ("erf", "exp"):
            g["%s_%s" % (fam, key)] = ld(g["%s_%s_hi" % (fam, key)]) + ld(g["%s_%s_lo" % (fam, key)])
    return g


# ====================================================================== per-point terms
# n (and its padding) of the seam cases; the whole fixture runs once more as one call
TERM_N = (1, 255, 256, 257)
FOLD_B = (1, 255, 256, 257, 650)
MDIAG_MPAD = (2, 126, 128, 130, 384)


def pads_of(n):
    return sorted({-(-n // 32) * 32, -(-n // 128) * 128})


def score_derivs_ref(obj, res, c, erf, ex, N):
    """(gm, gc, S_gm, S_gc) in longdouble: the derivatives of the mean score w.r.t. the LOO mean
    and variance at residual res = y − μ and variance c, and the natural scale of each —
    CRPS: gm = −erf(z/√2)/N against 1/N, gc = (2φ(z) − 1/√π)/(2sN) against 1/(2sN);
    LogS: gm = −res/(cN) against |res|/(cN), gc = (1/2c − res²/2c²)/N against the sum of both."""
    if obj == OBJ_CRPS:
        s = np.sqrt(c)
        return (-erf / N, (2 * INV_SQRT_2PI * ex - INV_SQRT_PI) / (2 * s * N), 1 / (N * np.ones_like(c)),
                1 / (2 * s * N))
    return (-res / c / N, (1 / (2 * c) - res * res / (2 * c * c)) / N, np.abs(res) / c / N,
            (1 / (2 * c) + res * res / (2 * c * c)) / N)


def deriv_consts(obj, ea, kap):
    """Operation counts (in u, against the natural scales) of gm and gc as the kernels form them.
    ea, kap: relative error (in u) of the α and d the formulas start from — 0 where they are
    inputs (full GP, folds), 3 and κ_d where fitc_grad_terms computes them itself.
      z = r/s with r = α/d (u), c = 1/d (u), s = √c (c's u/2 + u): 3.5u + ea + kap/2
      CRPS gm: w = z·(1/√2) (1.5u more); erf <= 16 ulp (§18) plus |w·erf'(w)| <= 0.484 times w's
        error; 1 + erf, the halving is exact: cdf <= [16 + 0.484(5 + ea + kap/2)]/2 + 1; doubled,
        subtracted from 1 (u), divided by N (u):            20 + (5 + ea + kap/2)/2
      CRPS gc: the argument −½z² carries 2·(z's error) + 2u relative, x·e^-x <= 1/e turns that
        into 0.368·(9 + 2ea + kap) of exp; exp <= 3 ulp (§18), the product with 1/√2π 1.5u:
        2φ <= 0.798·(that); the constant and the subtraction 1.1u; the denominator 2sN
        (3.5 + kap/2)u of a quotient <= 0.564:               10 + 0.6(ea + kap)
      LogS gm = −r/c/N: four roundings:                       5 + ea
      LogS gc = 0.5/c − r·r/(2c·c): 2u on the first term, 8u on the second, the subtraction and
        the division by N:                                    10 + 2ea + kap"""
    if obj == OBJ_CRPS:
        return 20 + (5 + ea + kap / 2) / 2, 10 + 0.6 * (ea + kap)
    return 5 + ea + 0 * kap, 10 + 2 * ea + kap


def point_reference(obj, a, d, res_c_erf_exp, N, ea=0.0, kap=0.0):
    """References and bounds of (gm, gc, u, h) for LOO points with α = a, d (longdouble):
      u = −gm/d:             (C_gm + 1 + kap)·u·S_gm/|d|
      h = (gm·α − gc)/d²:    (max(C_gm, C_gc) + 4 + ea + 2kap)·u·(S_gm|α| + S_gc)/d²
    (the product, the subtraction, d·d and the quotient; |gm| <= S_gm and |gc| <= S_gc)."""
    res, c, erf, ex = res_c_erf_exp
    gm, gc, Sm, Sc = score_derivs_ref(obj, res, c, erf, ex, N)
    Cm, Cc = deriv_consts(obj, ea, kap)
    u = LD(U)
    ref = {"gm": gm, "gc": gc, "u": -gm / d, "h": (gm * a - gc) / (d * d)}
    Sh = (Sm * np.abs(a) + Sc) / (d * d)
    tol = {"gm": Cm * u * Sm, "gc": Cc * u * Sc, "u": (Cm + 1 + kap) * u * Sm / np.abs(d),
           "h": (np.maximum(Cm, Cc) + 4 + ea + 2 * kap) * u * Sh}
    return ref, tol, {"Cm": Cm, "Cc": Cc, "Sm": Sm, "Sc": Sc, "Sh": Sh}


def full_point_reference(g, obj, idx, N):
    a, d = ld(g["full_alpha"][idx]), ld(g["full_dinv"][idx])
    return point_reference(obj, a, d, (a / d, 1 / d, g["full_erf"][idx], g["full_exp"][idx]), N)


def fitc_point_reference(g, obj, idx, N):
    """fitc_grad_terms' six outputs.  α = (y − g)·(1/λ): 3u;  d = 1/λ − r·(1/λ)·(1/λ):
    u·(1/λ + 4|r|/λ² + |d|) absolutely, κ_d·u relatively with κ_d = (1/λ + 4|r|/λ²)/|d| + 1.
    ulam = u/λ adds 2u to u's constant, hl2 = h/λ² adds 4u to h's."""
    y, lam, r, gg = (ld(g[k][idx]) for k in ("y", "fitc_lam", "fitc_r", "fitc_g"))
    il = 1 / lam
    a = (y - gg) * il
    d = il - r * il * il
    kap = (il + 4 * np.abs(r) * il * il) / np.abs(d) + 1
    u = LD(U)
    ref = {"alpha": a, "dinv": d}
    tol = {"alpha": 3 * u * np.abs(a), "dinv": kap * u * np.abs(d)}
    if obj == OBJ_NLML:
        z = np.zeros_like(a)
        ref.update(v=a / 2, ulam=z, h=z, hl2=z)
        tol.update(v=tol["alpha"] / 2, ulam=z, h=z, hl2=z)
        return ref, tol
    pr, pt, k = point_reference(obj, a, d, (a / d, 1 / d, g["fitc_erf"][idx], g["fitc_exp"][idx]),
                                N, ea=3.0, kap=kap)
    ref.update(v=np.zeros_like(a), ulam=pr["u"] * il, h=pr["h"], hl2=pr["h"] * il * il)
    tol.update(v=np.zeros_like(a), ulam=(k["Cm"] + 3 + kap) * u * k["Sm"] / np.abs(d) * il,
               h=pt["h"], hl2=(np.maximum(k["Cm"], k["Cc"]) + 8 + 3 + 2 * kap) * u * k["Sh"] * il * il)
    return ref, tol


def fold_point_reference(g, idx, b):
    """fold_terms' gm and gc (CRPS, N = b, residual and variance are inputs: ea = kap = 0)."""
    r, c = ld(g["fold_r"][idx]), ld(g["fold_c"][idx])
    gm, gc, Sm, Sc = score_derivs_ref(OBJ_CRPS, r, c, g["fold_erf"][idx], g["fold_exp"][idx], b)
    Cm, Cc = deriv_consts(OBJ_CRPS, 0.0, 0.0)
    return {"gm": gm, "gc": gc}, {"gm": Cm * LD(U) * Sm, "gc": Cc * LD(U) * Sc}


# ---- float64 restatements (numpy's IEEE operations, libm erf / exp), in the kernels' order
def score_derivs_f64(obj, r, c, N, isp=K_ISP):
    with np.errstate(all="ignore"):
        if obj == OBJ_CRPS:
            s = np.sqrt(c)
            z = r / s
            cdf = 0.5 * (1.0 + _erf(z * K_SQRT_HALF))
            pdf = K_PDF * np.exp(-0.5 * z * z)
            return 1.0 - 2.0 * cdf, (2.0 * pdf - isp) / (2.0 * s)
        return -r / c, 0.5 / c - r * r / (2.0 * c * c)


def loo_terms_f64(y, alpha, dinv, n, obj, detour=False, isp=K_ISP):
    """loo_grad_terms_kernel; detour: the residual as y − (y − α/d), as the kernel had it."""
    with np.errstate(all="ignore"):
        d, a = dinv, alpha
        c = 1.0 / d
        r = y - (y - a / d) if detour else a / d
        gm, gc = score_derivs_f64(obj, r, c, n, isp)
        gm, gc = gm / n, gc / n
        return -gm / d, (gm * a - gc) / (d * d)


def fitc_terms_f64(y, lam, r, g, obj, n_total, hl2_once=False):
    """fitc_grad_terms_kernel; hl2_once: the defect h/λ in place of h/λ²."""
    with np.errstate(all="ignore"):
        il = 1.0 / lam
        a = (y - g) * il
        d = il - r * il * il
        z = np.zeros_like(a)
        if obj == OBJ_NLML:
            return {"alpha": a, "dinv": d, "v": 0.5 * a, "ulam": z, "h": z, "hl2": z}
        c, res = 1.0 / d, a / d
        gm, gc = score_derivs_f64(obj, res, c, n_total)
        gm, gc = gm / n_total, gc / n_total
        u, hh = -gm / d, (gm * a - gc) / (d * d)
        return {"alpha": a, "dinv": d, "v": z, "ulam": u * il, "h": hh,
                "hl2": hh * il if hl2_once else hh * il * il}


def crps_terms_f64(r, c):
    """The fold value's per-point terms as fold_terms_kernel writes them."""
    s = np.sqrt(c)
    z = r / s
    cdf = 0.5 * (1.0 + _erf(z * K_SQRT_HALF))
    pdf = K_PDF * np.exp(-0.5 * z * z)
    return s * (z * (2.0 * cdf - 1.0) + 2.0 * pdf - K_ISP)


def wave_sum(v):
    """The xor butterfly over the last axis (64 lanes); every lane ends with the same sum."""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    return v[..., 0]


def block_sum(v):
    """block_sum of 256 threads (last axis): the butterfly per wave, then the waves in order."""
    w = wave_sum(v.reshape(v.shape[:-1] + (4, 64)))
    t = np.zeros(w.shape[:-1])
    for k in range(4):
        t = t + w[..., k]
    return t


def strided_block_sum(x):
    """Thread t adds x[t], x[t + 256], ... in order (axis 0), then block_sum."""
    cnt = x.shape[0]
    pad = np.zeros((-(-cnt // 256) * 256,) + x.shape[1:])
    pad[:cnt] = x
    v = np.zeros((256,) + x.shape[1:])
    for k in range(pad.shape[0] // 256):
        v = v + pad[256 * k:256 * (k + 1)]
    return block_sum(np.moveaxis(v, 0, -1))


def fold_terms_f64(r, c, b):
    """fold_terms_kernel: (gm, gc, value) with the value summed in the kernel's order."""
    s = np.sqrt(c)
    z = r / s
    cdf = 0.5 * (1.0 + _erf(z * K_SQRT_HALF))
    pdf = K_PDF * np.exp(-0.5 * z * z)
    gm = (1.0 - 2.0 * cdf) / b
    gc = (2.0 * pdf - K_ISP) / (2.0 * s * b)
    return gm, gc, float(strided_block_sum(crps_terms_f64(r, c))) / b


def fold_sum_reference(r, c, b):
    """math.fsum of the float64 terms / b, with §18's reduction bound 128u·Σ|t_i|/b (it holds the
    64u a device term may differ from the host's by and the depth of the sum, <= 3 + 10)."""
    t = crps_terms_f64(r, c)
    return math.fsum(t) / b, 128 * U * math.fsum(np.abs(t)) / b


# ---- fitc_grad_mdiag
MDIAG_N, MDIAG_NPAD = 37, 64


def mdiag_inputs(m_pad):
    """37 rows: KN and K with entries over eight decades and mixed signs, λ over the d grid."""
    rng = np.random.default_rng(900 + m_pad)
    n = MDIAG_N

    def wide(*shape):
        return rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-4.0, 4.0, shape)

    lam = 1.0 / np.array([(1e-6, 1e-3, 0.3, 1.0, 50.0, 1e4, 1e8)[i % 7] for i in range(n)])
    return dict(KN=wide(n, m_pad), K=wide(n, m_pad), lam=lam, r=0.4 * lam * rng.uniform(0, 1, n),
                dinv=wide(n), alpha=wide(n), v=wide(n), h=wide(n), a=0.5)


def mdiag_reference(p, m_pad, with_kn=True, with_h=True):
    """mdiag = a·d − v·α − (h/λ² − 2hr/λ³ + q/λ²), q = Σ_j KN_ij K_ij, against the sum of the five
    terms' absolute values: products u, 1/λ u each time it enters, so the terms carry <= 1, 1, 4,
    7 and 4u, the four subtractions u each of a partial sum <= the total: 12u·Σ|T|; q itself is
    two fmas a lane and trip of the j += 128 loop and the six-level butterfly:
    (2·⌈m_pad/128⌉ + 6)u·Σ_j|KN_ij K_ij|/λ².  s1 = 2(a/λ − h/λ²): 6u·(|a/λ| + |h/λ²|);
    s2 = 2/λ: one rounding; s3 = −2·mdiag exactly."""
    lam, r, dinv, al, v = (ld(p[k]) for k in ("lam", "r", "dinv", "alpha", "v"))
    h = ld(p["h"]) if with_h else np.zeros_like(lam)
    il = 1 / lam
    prod = ld(p["KN"]) * ld(p["K"]) if with_kn else np.zeros((len(lam), m_pad), LD)
    q, qa = prod.sum(1), np.abs(prod).sum(1)
    T = [p["a"] * dinv, v * al, h * il * il, 2 * h * r * il ** 3, q * il * il]
    md = T[0] - T[1] - (T[2] - T[3] + T[4])
    u = LD(U)
    tol_md = u * (12 * sum(np.abs(t) for t in T) + (2 * -(-m_pad // 128) + 6) * qa * il * il)
    s1 = 2 * (p["a"] * il - h * il * il)
    return ({"mdiag": md, "s1": s1, "s2": 2 * il},
            {"mdiag": tol_md, "s1": 6 * u * 2 * (np.abs(p["a"] * il) + np.abs(h * il * il)),
             "s2": u * 2 * il})


def mdiag_f64(p, m_pad, with_kn=True, with_h=True):
    """fitc_grad_mdiag_kernel: lane l takes columns 2l, 2l + 1, then j += 128."""
    n = len(p["lam"])
    q = np.zeros(n)
    if with_kn:
        acc = np.zeros((n, 64))
        for j0 in range(0, m_pad, 128):
            for l in range(64):
                for j in (j0 + 2 * l, j0 + 2 * l + 1):
                    if j0 + 2 * l < m_pad:
                        acc[:, l] = p["KN"][:, j] * p["K"][:, j] + acc[:, l]
        q = wave_sum(acc)
    il = 1.0 / p["lam"]
    hi = p["h"] if with_h else np.zeros(n)
    md = p["a"] * p["dinv"] - p["v"] * p["alpha"] - (hi * il * il - 2.0 * hi * p["r"] * il * il * il
                                                     + q * il * il)
    return {"mdiag": md, "s1": 2.0 * (p["a"] * il - hi * il * il), "s2": 2.0 * il, "s3": -2.0 * md}


# ====================================================================== the contractions
COEF_SETS = {"nlml": (0.5, -0.5, 0.0, 0.0), "loo": (0.0, 0.0, -1.0, -1.0),
             "all": (0.7, -0.3, 1.3, -0.9)}
FULL_N = (1, 2, 63, 64, 65, 129, 200)
FULL_D_EVERY_N = (8, 17)
FULL_D_OTHER = (1, 16, 2, 15, 32, 33, 64)
FULL_CASES = ([(n, d) for d in FULL_D_EVERY_N for n in FULL_N]
              + [(n, d) for d in FULL_D_OTHER for n in (65, 200)])
FULL_LARGE = (1473, 2)          # 24 tile rows: 300 tiles, the slab reduction's second trip
LOG_SF2 = -0.75


def cluster_features(rng, d, k, inv):
    """§18's clustered line in scaled units (clusters at 0, 1, 3, 8, 18, 46.1 and 300, spread
    0.6/√d), returned as raw features x = scaled/inv_ell."""
    dirn = rng.standard_normal(d)
    dirn /= np.linalg.norm(dirn)
    c = rng.integers(0, len(CLUSTER_POS), k)
    return (np.outer(CLUSTER_POS[c], dirn) + 0.6 / math.sqrt(d) * rng.standard_normal((k, d))) / inv


def wide(rng, *shape):
    """Magnitudes log-uniform over eight decades, mixed signs."""
    return rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-4.0, 4.0, shape)


class FullCase:
    """One launch_grad_contract call: features with exact and near duplicates (a quarter of
    the rows, at the end), Ainv / Mx [n][ld] with the strict upper triangle and the columns from
    n on NaN, α and v over eight decades; the reference terms in longdouble."""

    def __init__(self, n, d, seed=0):
        need_extended()
        rng = np.random.default_rng(7000 + 100 * d + n + seed)
        self.n, self.d, self.ld = n, d, n + 3
        self.log_ell = 0.3 * rng.standard_normal(d)
        self.inv = inv_ell_of(self.log_ell, d)
        self.sf2 = math.exp(LOG_SF2)
        x = cluster_features(rng, d, n, self.inv)
        k = n // 8
        if k:
            x[n - 2 * k:n - k] = x[:k]
            x[n - k:] = x[k:2 * k] * (1.0 + 2.0 ** -50)
        self.x = np.ascontiguousarray(x)
        self.alpha, self.v = wide(rng, n), wide(rng, n)
        low = np.tril(np.ones((n, n), bool))
        self.Ainv, self.Mx = np.full((n, self.ld), np.nan), np.full((n, self.ld), np.nan)
        self.Ainv[:, :n][low] = wide(rng, int(low.sum()))
        self.Mx[:, :n][low] = wide(rng, int(low.sum()))
        self.low = low
        self.tiles = (-(-n // 64)) * (-(-n // 64) + 1) // 2
        self.passes = -(-d // 16)
        self._ref = None

    def operands(self, coef):
        """(Ainv, Mx, v) as a call with these coefficients passes them: None where absent."""
        a0, _, a2, a3 = coef
        return (self.Ainv if a0 else None, self.Mx if a3 else None, self.v if a2 else None)

    def geometry(self):
        """xs = fl(x·inv_ell) as the kernel stages it in LDS, then Δ, arg, K in longdouble."""
        if self._ref is None:
            xs = ld(self.x * self.inv)
            dl = xs[:, None, :] - xs[None, :, :]
            arg = -0.5 * (dl * dl).sum(2)
            self._ref = (dl, arg, LD(self.sf2) * np.exp(arg))
        return self._ref

    def reference(self, coef):
        """(out [passes][18], tol) — out[p][0] = Σ w·m·K, out[p][1] = Σ_diag m, out[p][2 + q] =
        Σ w·m·K·Δ_k² (k = 16p + q), every sum bounded by
            u·Σ_ij |t_ij|·(c_term + c_sum + (d + 6)|arg_ij|) + underflow
        with |t| taken with m's parts in absolute value.  c_term: m is a product of three (2u)
        and an fma chain over up to three more parts, the a2 part a sum of two products halved:
        each part <= 3u of itself and three additions u each of a partial sum <= Σ|parts|: 6u;
        K = sf2·exp_neg: 3u (§18; its argument is the (d + 6)|arg| term); (w·m)·K: u — 10u for
        out[0], 6u for out[1] (no K, no argument); Δ_k² a rounded difference squared, 3u: 13u.
        c_sum: 16 rows a thread, block_sum (6 levels + 4 waves), ⌈tiles/256⌉ slab entries a
        thread, block_sum again: 36 + ⌈tiles/256⌉.  Underflow: K below the normal range is off
        by 1.5·2^-1074 (§18) times w|m|Δ², and each product may lose 2^-1074."""
        n, d = self.n, self.d
        a0, a1, a2, a3 = (LD(c) for c in coef)
        dl, arg, K = self.geometry()
        al, v = ld(self.alpha), ld(self.v)
        A = np.where(self.low, ld(np.nan_to_num(self.Ainv[:, :n])), 0)
        X = np.where(self.low, ld(np.nan_to_num(self.Mx[:, :n])), 0)
        parts = [a0 * A, a1 * al[:, None] * al[None, :],
                 a2 * (v[:, None] * al[None, :]) / 2, a2 * (al[:, None] * v[None, :]) / 2, a3 * X]
        m = np.where(self.low, sum(parts), 0)
        mabs = np.where(self.low, sum(np.abs(p) for p in parts), 0)
        w = np.where(np.eye(n, dtype=bool), LD(1), LD(2))
        csum = 36 + -(-self.tiles // 256)
        u = LD(U)
        out = np.zeros((self.passes, 18), LD)
        tol = np.zeros((self.passes, 18), LD)
        aarg = (d + 6) * np.abs(arg)
        mk, mka = w * m * K, w * mabs * K
        sub = LD(SUBNORMAL) * (2 * n * n + 1.5 * (w * mabs).sum())
        out[:, 0], tol[:, 0] = mk.sum(), u * (mka * (10 + csum + aarg)).sum() + sub
        out[:, 1] = np.trace(m)
        tol[:, 1] = u * np.trace(mabs) * (6 + csum)
        for k in range(d):
            d2 = dl[:, :, k] ** 2
            out[k // 16, 2 + k % 16] = (mk * d2).sum()
            tol[k // 16, 2 + k % 16] = (u * (mka * d2 * (13 + csum + aarg)).sum()
                                        + LD(SUBNORMAL) * (2 * n * n + 1.5 * (w * mabs * d2).sum()))
        return out, tol


def benign_full(n, d):
    """A FullCase with the older tests' kind of input: N(0, I) features, length-scales near 1,
    N(0, 1) entries everywhere and finite zeros where the kernel must not read."""
    case = FullCase(n, d)
    rng = np.random.default_rng(5 + n + d)
    case.log_ell = 0.1 * rng.standard_normal(d)
    case.inv = inv_ell_of(case.log_ell, d)
    case.x = rng.standard_normal((n, d))
    case.alpha, case.v = rng.standard_normal(n), rng.standard_normal(n)
    case.Ainv = np.where(np.tril(np.ones((n, case.ld), bool)), rng.standard_normal((n, case.ld)), 0.0)
    case.Mx = np.where(np.tril(np.ones((n, case.ld), bool)), rng.standard_normal((n, case.ld)), 0.0)
    case._ref = None
    return case


def benign_fitc(nr, nc, d, config):
    case = FitcCase(nr, nc, -(-nc // 128) * 128, d, config)
    rng = np.random.default_rng(6 + nr + nc + d)
    case.log_ell = 0.1 * rng.standard_normal(d)
    case.inv = inv_ell_of(case.log_ell, d)
    case.xr, case.xc = rng.standard_normal((nr, d)), rng.standard_normal((nc, d))
    case.R = [np.where(np.arange(m.shape[1]) < nc, rng.standard_normal(m.shape), 0.0) for m in case.R]
    case.rs = [None if r is None else rng.uniform(0.5, 2.0, nr) for r in case.rs]
    case.pv = [None if v is None else rng.standard_normal(nr) for v in case.pv]
    case.qv = [None if v is None else rng.standard_normal(nc) for v in case.qv]
    return case


def emulate_full(case, coef, operands=None, defect=None):
    """grad_contract_kernel and grad_slab_reduce_kernel in numpy float64, thread for thread:
    thread (rg, cj) of a tile adds its rows rg, rg + 4, ... in order, block_sum, the slab
    reduction; an fma is a rounded product and a rounded sum (no more accurate).  operands:
    (Ainv, Mx, v) arrays as the device holds them (NaN where absent).  defect: one of
    'diag_weight', 'row_guard', 'pass_offset', 'ungated_a0', 'ungated_a2', 'ungated_a3'.  (The
    template instances differ only in where the features live: one restatement serves all.)"""
    n, d, sf2 = case.n, case.d, case.sf2
    a0, a1, a2, a3 = coef
    Ain, Mxn, vn = operands if operands is not None else (case.Ainv, case.Mx, case.v)
    nan_m, nan_v = np.full((n, case.ld), np.nan), np.full(n, np.nan)
    Ain = nan_m if Ain is None else Ain
    Mxn = nan_m if Mxn is None else Mxn
    vn = nan_v if vn is None else vn
    xs = case.x * case.inv
    T = -(-n // 64)
    ti = np.array([i for i in range(T) for j in range(i + 1)])
    tj = np.array([j for i in range(T) for j in range(i + 1)])
    nt = len(ti)
    cj = np.arange(64)
    j = (tj[:, None, None] * 64 + cj[None, None, :])                  # [tiles][1][64]
    jc = np.minimum(j, n - 1)
    slab = np.zeros((case.passes, nt, 18))
    g0, g2, g3 = (a0 != 0.0 or defect == "ungated_a0", a2 != 0.0 or defect == "ungated_a2",
                  a3 != 0.0 or defect == "ungated_a3")
    with np.errstate(all="ignore"):
        for p in range(case.passes):
            d0 = 16 * p
            acc = np.zeros((18, nt, 4, 64))
            for step in range(16):
                i = ti[:, None, None] * 64 + (np.arange(4)[None, :, None] + 4 * step)
                ic = np.minimum(i, n - 1)
                ok = (i < n) & (j < n) & ((i > j) if defect == "row_guard" else (i >= j))
                r2 = np.zeros((nt, 4, 64))
                for k in range(d):
                    t = xs[ic, k] - xs[jc, k]
                    r2 = t * t + r2
                K = sf2 * np.exp(-0.5 * r2)
                ai, aj = case.alpha[ic], case.alpha[jc]
                m = a1 * ai * aj
                if g0:
                    m = a0 * Ain[ic, jc] + m
                if g2:
                    m = a2 * (0.5 * (vn[ic] * aj + ai * vn[jc])) + m
                if g3:
                    m = a3 * Mxn[ic, jc] + m
                w = np.where((i == j) & (defect != "diag_weight"), 1.0, 2.0)
                mk = w * m * K
                acc[0] += np.where(ok, mk, 0.0)
                acc[1] += np.where(ok & (i == j), m, 0.0)
                for q in range(16):
                    if d0 + q < d:
                        kk = q if defect == "pass_offset" else d0 + q
                        t = xs[ic, kk] - xs[jc, kk]
                        acc[2 + q] = np.where(ok, mk * (t * t) + acc[2 + q], acc[2 + q])
            slab[p] = block_sum(acc.reshape(18, nt, 256)).T
    return np.stack([strided_block_sum(slab[p]) for p in range(case.passes)])


# ---- the FITC contraction
FITC_NR = (1, 255, 256, 257, 513)
FITC_NC = (1, 63, 64, 65, 130)
FITC_D_EVERY = (8, 17)
FITC_D_OTHER = (1, 16, 2, 33, 64)
# term configurations (nt, which terms carry a row scale, which rank-one terms are on), cycled
# over the cases: every one runs at d = 8 and d = 17
FITC_CONFIGS = ((4, (0, 2), (1, 1)), (1, (), (1, 0)), (0, (), (1, 1)), (1, (0,), (0, 0)),
                (4, (), (0, 1)), (4, (0, 1, 2, 3), (0, 0)))


def fitc_cases():
    """(nr, nc, nc_pad, d, config) of every FITC contraction case but the two large ones."""
    out, k = [], 0
    for d in FITC_D_EVERY:
        for nr in FITC_NR:
            for nc in FITC_NC:
                out.append((nr, nc, -(-nc // 128) * 128, d, FITC_CONFIGS[k % len(FITC_CONFIGS)]))
                k += 1
    for d in FITC_D_OTHER:
        out.append((257, 65, 128, d, FITC_CONFIGS[k % len(FITC_CONFIGS)]))
        k += 1
    out.append((257, 65, 66, 8, FITC_CONFIGS[0]))        # nc_pad = nc rounded up to 2
    out.append((40, 5, 128, 3, (0, (), (0, 0))))         # no term at all: everything is 0
    return out


FITC_LARGE = ((70000, 3, 128, 2, (1, (0,), (1, 0))),      # fitc_chunk_rows = 320
              (4097, 1000, 1024, 1, (1, (), (0, 0))))     # 17 chunks × 16 column blocks = 272


def fitc_chunk_rows(nr):
    c = -(-(-(-nr // 256)) // 64) * 64
    return max(c, 256)


class FitcCase:
    """One launch_fitc_grad_contract call.  R_t [nr][ldr_t] with unequal ldr_t >= nc, the columns
    from nc on NaN; column zero_col of every term (and of qv) is zero, so G's column is."""

    def __init__(self, nr, nc, nc_pad, d, config):
        need_extended()
        rng = np.random.default_rng(8000 + 1000 * d + 7 * nr + nc)
        self.nr, self.nc, self.nc_pad, self.d = nr, nc, nc_pad, d
        self.nt, rs_on, pc_on = config
        self.log_ell = 0.3 * rng.standard_normal(d)
        self.inv = inv_ell_of(self.log_ell, d)
        self.sf2 = math.exp(LOG_SF2)
        xr = cluster_features(rng, d, nr, self.inv)
        xc = cluster_features(rng, d, nc, self.inv)
        k = min(nr, nc) // 4
        if k:
            xc[:k] = xr[:k]
            xc[k:2 * k] = xr[k:2 * k] * (1.0 + 2.0 ** -50)
        self.xr, self.xc = np.ascontiguousarray(xr), np.ascontiguousarray(xc)
        self.zero_col = nc // 2
        self.R, self.coef, self.rs = [], [], []
        for t in range(self.nt):
            m = np.full((nr, nc + 1 + 2 * t), np.nan)
            m[:, :nc] = wide(rng, nr, nc)
            m[:, self.zero_col] = 0.0
            self.R.append(m)
            self.coef.append(float(wide(rng, 1)[0]) if t else 2.0)
            self.rs.append(wide(rng, nr) if t in rs_on else None)
        self.pc = [float(c) * (-0.5 if q else 1.0) for q, c in enumerate(pc_on)]
        self.pv = [wide(rng, nr) if c else None for c in pc_on]
        self.qv = [wide(rng, nc) if c else None for c in pc_on]
        for q in self.qv:
            if q is not None:
                q[self.zero_col] = 0.0
        self.rchunk = fitc_chunk_rows(nr)
        self.chunks = -(-nr // self.rchunk)
        self.cb = -(-nc_pad // 64)
        self.passes = -(-d // 16)

    def call_args(self):
        return dict(R=self.R, coef=self.coef, rs=self.rs if self.nt else None, pc=self.pc,
                    pv=self.pv, qv=self.qv)

    def reference(self):
        """(out [passes][17], zout [nc][d], tol_out, tol_zout).  As the full contraction's bound
        with: G = Σ_t (coef_t·rs_t)·R_t + Σ_q (pc_q·pv_q)·qv_q, an fma chain over up to six parts,
        <= 2u a part and 6u of Σ|parts|: 8u; K 3u; G·K u — c_term 12, Δ_k² 15, Δ_k 13.
        c_sum = rchunk/4 rows a thread + block_sum (10) + ⌈blocks/256⌉ + block_sum (10); zout:
        rchunk/4 + 3 (row groups) + chunks.  The row side forms xr·inv_ell − xs_j, which the
        compiler may contract into one fma: Δ_k then differs from the reference's (rounded
        product) by <= u|xs_ik|, the argument by u·R_ij, R_ij = Σ_k |Δ_k||xs_ik| (§18), Δ_k² by
        2u|Δ_k||xs_ik|: both forms are inside the bound."""
        d, nr, nc = self.d, self.nr, self.nc
        xs, xcs = ld(self.xr * self.inv), ld(self.xc * self.inv)
        axs = np.abs(xs)
        G, Ga = np.zeros((nr, nc), LD), np.zeros((nr, nc), LD)
        for t in range(self.nt):
            part = LD(self.coef[t]) * ld(self.R[t][:, :nc])
            if self.rs[t] is not None:
                part = part * ld(self.rs[t])[:, None]
            G, Ga = G + part, Ga + np.abs(part)
        for q in range(2):
            if self.pc[q] != 0.0:
                part = LD(self.pc[q]) * ld(self.pv[q])[:, None] * ld(self.qv[q])[None, :]
                G, Ga = G + part, Ga + np.abs(part)
        arg, Rr = np.zeros((nr, nc), LD), np.zeros((nr, nc), LD)
        for k in range(d):
            dk = xs[:, k][:, None] - xcs[:, k][None, :]
            arg += dk * dk
            Rr += np.abs(dk) * axs[:, k][:, None]
        arg *= -0.5
        K = LD(self.sf2) * np.exp(arg)
        gk, gka = G * K, Ga * K
        bpp = self.cb * self.chunks
        csum = self.rchunk // 4 + 20 + -(-bpp // 256)
        cz = self.rchunk // 4 + 3 + self.chunks
        u, sn = LD(U), LD(SUBNORMAL)
        common = (d + 6) * np.abs(arg) + Rr
        out, tol = np.zeros((self.passes, 17), LD), np.zeros((self.passes, 17), LD)
        zout, ztol = np.zeros((nc, d), LD), np.zeros((nc, d), LD)
        out[:, 0] = gk.sum()
        tol[:, 0] = u * (gka * (12 + csum + common)).sum() + sn * (2 * nr * nc + 1.5 * Ga.sum())
        for k in range(d):
            dk = xs[:, k][:, None] - xcs[:, k][None, :]
            ad, ax = np.abs(dk), axs[:, k][:, None]
            out[k // 16, 1 + k % 16] = (gk * dk * dk).sum()
            tol[k // 16, 1 + k % 16] = (u * (gka * (dk * dk * (15 + csum + common) + 2 * ad * ax)).sum()
                                        + sn * (2 * nr * nc + 1.5 * (Ga * dk * dk).sum()))
            zout[:, k] = (gk * dk).sum(0)
            ztol[:, k] = (u * (gka * (ad * (13 + cz + common) + ax)).sum(0)
                          + sn * (2 * nr + 1.5 * (Ga * ad).sum(0)))
        return out, zout, tol, ztol


def _fma_sub(a, b, c):
    """fl(a·b − c) with one rounding, element-wise (exact rational arithmetic)."""
    from fractions import Fraction
    a, b, c = np.broadcast_arrays(a, b, c)
    out = np.empty(a.shape)
    flat = out.reshape(-1)
    for i, (x, y, z) in enumerate(zip(a.reshape(-1), b.reshape(-1), c.reshape(-1))):
        flat[i] = float(Fraction(float(x)) * Fraction(float(y)) - Fraction(float(z)))
    return out


def emulate_fitc(case, defect=None, fused=False, poison_off=False):
    """fitc_grad_contract_kernel and its two reductions in numpy float64, thread for thread (all
    column blocks at once: a thread's sums do not depend on its block).  fused: the row-side
    difference in one rounding.  defect: 'row_group' (zsh summed over three row groups),
    'missing_rs' (the first row scale left out), 'pass_offset'.  poison_off: the rank-one terms
    that are off get NaN vectors and are used (the ungated defect)."""
    nr, nc, d, sf2 = case.nr, case.nc, case.d, case.sf2
    ncol = case.cb * 64
    xcs = case.xc * case.inv
    j = np.arange(ncol)
    jc = np.minimum(j, nc - 1)
    steps = case.rchunk // 4
    r0 = (np.arange(case.chunks) * case.rchunk)[:, None, None]
    r1 = np.minimum(nr, r0 + case.rchunk)
    rg = np.arange(4)[None, :, None]
    shape = (case.chunks, 4, ncol)
    out = np.zeros((case.passes, 17))
    zout = np.zeros((nc, d))

    def delta(ic, k):
        if fused:
            return _fma_sub(case.xr[ic, k], case.inv[k], xcs[jc, k][None, None, :])
        return case.xr[ic, k] * case.inv[k] - xcs[jc, k][None, None, :]

    with np.errstate(all="ignore"):
        for p in range(case.passes):
            d0 = 16 * p
            acc = np.zeros((17,) + shape)
            zacc = np.zeros((16,) + shape)
            for step in range(steps):
                i = r0 + rg + 4 * step                                   # [chunks][4][1]
                ic = np.minimum(i, nr - 1)
                ok = (i < r1) & (j[None, None, :] < nc)
                r2 = np.zeros(shape)
                for k in range(d):
                    t = delta(ic, k)
                    r2 = t * t + r2
                Kij = sf2 * np.exp(-0.5 * r2)
                G = np.zeros(shape)
                for t in range(case.nt):
                    use_rs = case.rs[t] is not None and not (defect == "missing_rs" and t == 0)
                    sc = case.coef[t] * case.rs[t][ic] if use_rs else case.coef[t]
                    G = sc * case.R[t][ic, jc[None, None, :]] + G
                for q in range(2):
                    if case.pc[q] != 0.0:
                        G = (case.pc[q] * case.pv[q][ic]) * case.qv[q][jc][None, None, :] + G
                    elif poison_off:
                        G = (case.pc[q] * np.nan) * np.nan + G
                gk = G * Kij
                acc[0] += np.where(ok, gk, 0.0)
                for q in range(16):
                    if d0 + q < d:
                        tq = delta(ic, q if defect == "pass_offset" else d0 + q)
                        acc[1 + q] = np.where(ok, gk * (tq * tq) + acc[1 + q], acc[1 + q])
                        zacc[q] = np.where(ok, gk * tq + zacc[q], zacc[q])
            z = zacc[:, :, 0] + zacc[:, :, 1] + zacc[:, :, 2]
            if defect != "row_group":
                z = z + zacc[:, :, 3]
            zs = np.zeros((16, ncol))
            for c in range(case.chunks):
                zs = zs + z[:, c]
            for q in range(16):
                if d0 + q < d:
                    zout[:, d0 + q] = zs[q, :nc]
            # block (chunk, column block): threads (rg, cj) -> 256
            blk = acc.reshape(17, case.chunks, 4, case.cb, 64).transpose(0, 1, 3, 2, 4)
            slab = block_sum(blk.reshape(17, case.chunks * case.cb, 256))
            out[p] = strided_block_sum(slab.T)
    return out, zout


def worst_ratio(got, ref, tol):
    """max |got − ref| / tol over the entries (0/0 counts as 0; a non-finite entry as inf)."""
    got = np.asarray(got, np.float64)
    err = np.abs(ld(got) - ref)
    with np.errstate(all="ignore"):
        q = np.where(err == 0, LD(0), err / tol)
    q = np.where(np.isfinite(got), q, LD(np.inf))
    return float(np.max(q)) if q.size else 0.0
