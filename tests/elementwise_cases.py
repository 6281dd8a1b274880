"""Inputs, extended-precision references and error bounds of the element-wise device math
(exp_neg, the Gram kernels, the score terms), shared by test_elementwise_host.py (CPU: the
bounds hold for plain float64 arithmetic on these very inputs) and test_gpu_elementwise.py (the
kernels).  Nothing here touches the GPU.

Notation: u = 2^-53 (the unit roundoff of float64); "reference" is numpy longdouble, the 80-bit
x87 format (64-bit significand), evaluated from the float64 values the kernel receives.
"""
import math
import os
from fractions import Fraction

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
SUBNORMAL = 2.0 ** -1074          # the spacing of float64 below 2^-1022
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def need_extended():
    """The references need a longdouble wider than float64 (x86: 64-bit significand)."""
    assert np.finfo(LD).nmant >= 63, "numpy longdouble is not extended precision here"


def f64_spacing(ref):
    """Spacing of float64 at |ref| (longdouble array, ref != 0): 2^(e-53) for ref = f·2^e with
    f in [0.5, 1), and the subnormal spacing 2^-1074 below the normal range."""
    _, e = np.frexp(np.abs(ref))
    return np.ldexp(LD(1), np.maximum(e.astype(np.int64) - 53, -1074).astype(np.int32))


# ------------------------------------------------------------------ 1a: exp_neg in isolation
EXP_N = 1024
EXP_FINE = 860            # columns on the fine grid; the rest are the powers of ten
LN2_64 = float.fromhex("0x1.71547652b82fep+6")   # 64 / ln 2, the constant exp_neg multiplies by


def exp_inputs():
    """x, x' (1024 × 1 each) whose 2^20 pairwise arguments −½(x_i − x'_j)² cover exp_neg's
    domain.  t = |x_i − x'_j| runs over [0, 40.04] in 1024 coarse steps (x) times 860 jittered
    fine steps (x'): consecutive arguments are at most t·Δt ≈ 1.9e-3 apart down to −801, and
    Δlog|arg| = 2Δt/t <= 7e-5 for |arg| >= 1.  The other 164 columns are 10^-k, k = 0..163, which
    against x_0 = 0 give |arg| = ½·10^-2k down to 5e-301, through the subnormal squares, to the
    squares that underflow to −0.  x_0 = x'_0 = 0 gives the argument 0 itself."""
    rng = np.random.default_rng(20240)
    h = 40.0 / (EXP_N - 1)
    x = h * np.arange(EXP_N)
    x[1:] += 1e-3 * h * rng.uniform(-1.0, 1.0, EXP_N - 1)
    xp = np.empty(EXP_N)
    xp[:EXP_FINE] = -h * (np.arange(EXP_FINE) + rng.uniform(0.0, 1.0, EXP_FINE)) / EXP_FINE
    xp[0] = 0.0
    xp[EXP_FINE:] = 10.0 ** -np.arange(EXP_N - EXP_FINE, dtype=np.float64)
    return np.ascontiguousarray(x.reshape(-1, 1)), np.ascontiguousarray(xp.reshape(-1, 1))


def exp_args(x, xp):
    """The device argument bit for bit: with d = 1 and inv_ell = 1 the kernels form
    e = fl(x_i − x'_j), a = fma(e, e, 0) = fl(e²) and −0.5·a — three plain IEEE operations."""
    e = x[:, 0][:, None] - xp[:, 0][None, :]
    return -0.5 * (e * e)


def exp_table_index(arg):
    """exp_neg's table index (j & 63 with j = rint(64·x/ln 2)) after its clamp at −746."""
    j = np.rint(np.maximum(arg, -746.0) * LN2_64).astype(np.int64)
    return j & 63


def exp_reference(arg):
    need_extended()
    return np.exp(arg.astype(LD))


def exp_check(out, arg, ref):
    """The project's claim for exp_neg, |out − exp(x)| <= 1 spacing of float64 at exp(x) (the
    subnormal spacing below the normal range), exactly 0 where exp(x) < 2^-1075, exactly 1 at
    x = 0.  Returns the largest error in spacings; raises on a violation."""
    err = np.abs(out.astype(LD) - ref) / f64_spacing(ref)
    worst = float(err.max())
    k = np.unravel_index(int(np.argmax(err)), err.shape)
    assert worst <= 1.0, ("exp_neg off by %.3f spacings at arg %r: got %r, exp is %r"
                          % (worst, arg[k], out[k], ref[k]))
    gone = ref < np.ldexp(LD(1), -1075)
    assert gone.any() and np.all(out[gone] == 0.0)
    zero = arg == 0.0
    assert zero.any() and np.all(out[zero] == 1.0)
    return worst


EXP_BIAS_MIN_SAMPLES = 10000
EXP_BIAS_BOUND = 0.1


def exp_table_bias(out, arg, ref):
    """Mean signed error of exp_neg, in spacings of the result, per table entry over the
    arguments with a normal result.  A one-ulp bound cannot see a table entry whose tail is lost
    (at most half an ulp, on top of a rounding error that reaches half an ulp only in the limit);
    the mean over the >= 10000 arguments that read one entry can.  What the design leaves:
    the truncated Taylor term r⁶/720, always positive, r uniform on ±ln2/128, is 5.0e-18
    relative on average = 0.0225·(head of the entry) <= 0.045 spacings; every rounding is to
    nearest and unbiased; the table pair and the Cody–Waite constants are exact to 2^-79 or
    better.  Sampling: each error is within 1 spacing (the claim), so the mean of N >= 10000
    has σ <= 0.01 and 6σ <= 0.055: EXP_BIAS_BOUND = 0.1 spacings."""
    idx = exp_table_index(arg)
    sel = (ref >= np.ldexp(LD(1), -1022)) & (arg < 0)
    err = ((out.astype(LD) - ref) / f64_spacing(ref)).astype(np.float64)
    bias = np.empty(64)
    for k in range(64):
        pick = sel & (idx == k)
        assert int(pick.sum()) >= EXP_BIAS_MIN_SAMPLES, (k, int(pick.sum()))
        bias[k] = err[pick].mean()
    return bias


# ------------------------------------------------------------------ 1b: Gram entries
GRAM_DIMS = (1, 2, 8, 16, 63, 64)
# (n, m, uplo); uplo 1: x' = x, lower, diag_add.  gps_gram pads rows to 32 and columns to 128, and
# a lower build goes to the matrix-core kernel only when the two agree: 333 (352 × 384) stays on
# the direct-difference kernels under every mode, 256 reaches the matrix-core kernel's lower
# mask and diagonal add.
GRAM_SHAPES = ((333, 201, 0), (333, 333, 1), (256, 256, 1))
GRAM_DIAG_ADD = 0.01
# sf2 = exp(−0.75) ≈ 0.47.  Below the normal range exp_neg is within one subnormal spacing and
# the product with sf2 is rounded again: sf2·1 + ½ spacings, which is inside the bound's one
# spacing only for sf2 <= ½ (a larger sf2 can legitimately be 1.5 spacings off).
GRAM_LOG_SF2 = -0.75
CLUSTER_POS = np.array([0.0, 1.0, 3.0, 8.0, 18.0, 46.1, 300.0])


def inv_ell_of(log_ell, d, rbf=False):
    """The library's inverse length-scales (set_theta): exp(−b) for ARD, exp(−b/2) for RBF with
    b = log ℓ²; std::exp there, math.exp here — the same libm."""
    b = np.broadcast_to(np.asarray(log_ell, np.float64), (d,))
    return np.array([math.exp(-0.5 * v) if rbf else math.exp(-v) for v in b])


def gram_inputs(d, n, m, uplo, rbf=False):
    """(x, x', log_ell) with, in scaled units, seven clusters of spread 0.6/√d on a line at
    0, 1, 3, 8, 18, 46.1 and 300: within a cluster the argument −½r² is near −0.4, between the
    clusters it runs through −0.5, −2, ... −726 (46.1 − 8: subnormal results), −929 (past the
    clamp at −746), −1063 to −45000; 40 exact
    duplicates and 40 near-duplicates (one part in 2^-50 apart: r² ≈ 1e-30 around the origin)
    between x and x'.  The far clusters put the data far from the origin, which the matrix-core
    kernel's centring must absorb.  uplo 1: x' is x (the square lower build)."""
    rng = np.random.default_rng(1000 * d + n + 7 * uplo + (3 if rbf else 0))
    log_ell = np.array([0.4]) if rbf else np.ascontiguousarray(0.3 * rng.standard_normal(d))
    inv = inv_ell_of(log_ell, d, rbf)
    dirn = rng.standard_normal(d)
    dirn /= np.linalg.norm(dirn)

    def draw(k):
        c = rng.integers(0, len(CLUSTER_POS), k)
        return (np.outer(CLUSTER_POS[c], dirn) + 0.6 / math.sqrt(d) * rng.standard_normal((k, d))) / inv

    x = draw(n)
    if uplo:
        x[n - 80:n - 40] = x[5:45]
        x[n - 40:] = x[50:90] * (1.0 + 2.0 ** -50)
        xp = x
    else:
        xp = draw(m)
        xp[:40] = x[5:45]
        xp[40:80] = x[50:90] * (1.0 + 2.0 ** -50)
        xp = np.ascontiguousarray(xp)
    return np.ascontiguousarray(x), xp, log_ell


def gram_duplicates(uplo, n):
    """(rows, columns) of the exact duplicate pairs planted by gram_inputs."""
    i = np.arange(5, 45)
    return (np.arange(n - 80, n - 40), i) if uplo else (i, np.arange(40))


class GramCase:
    """Reference and bounds of one Gram build.  xs, xps: the scaled features as the
    direct-difference kernels hold them, fl(x·inv_ell); arg, K: −½‖xs_i − xs'_j‖² and
    sf2·exp(arg) (+ diag_add on i == j) in longdouble."""

    def __init__(self, d, n, m, uplo, rbf=False):
        need_extended()
        self.d, self.n, self.m, self.uplo, self.rbf = d, n, m, uplo, rbf
        self.x, self.xp, self.log_ell = gram_inputs(d, n, m, uplo, rbf)
        self.inv = inv_ell_of(self.log_ell, d, rbf)
        self.sf2 = math.exp(GRAM_LOG_SF2)
        self.diag_add = GRAM_DIAG_ADD if uplo else 0.0
        self.xs, self.xps = self.x * self.inv, self.xp * self.inv
        arg = np.zeros((n, m), LD)
        for k in range(d):
            e = self.xs[:, k].astype(LD)[:, None] - self.xps[:, k].astype(LD)[None, :]
            arg += e * e
        self.arg = -0.5 * arg
        self.K = LD(self.sf2) * np.exp(self.arg)
        if self.diag_add:
            self.K[np.arange(n), np.arange(n)] += LD(self.diag_add)
        self.mask = np.tril(np.ones((n, m), bool)) if uplo else np.ones((n, m), bool)
        # launch_gram: d = 8, 16 under GPS_OPT_GRAM_REG 2, a lower build only if M == N
        self.matrix_core = d in (8, 16) and (not uplo or -(-n // 32) * 32 == -(-n // 128) * 128)

    def tol_direct(self):
        """K·u·((d + 6)·|arg| + 4) + 2^-1074 (derivation: test_gpu_elementwise.py)."""
        return self.K * LD(U) * ((self.d + 6) * np.abs(self.arg) + 4) + LD(SUBNORMAL)

    def centre_rows(self):
        """Row of x whose scaled features centre each 128-row tile (its first row)."""
        return [min(128 * t, self.n - 1) for t in range((self.n + 127) // 128)]

    def tol_centred(self):
        """K·u·((d + 6)·(‖p_i‖² + ‖q_j‖²) + R_ij + 4) + 2^-1074 with p, q the scaled features
        minus the centre of i's tile and R_ij = Σ_k |e_k|·(|xs_ik| + |xs'_jk|) (derivation:
        test_gpu_elementwise.py)."""
        S = np.zeros((self.n, self.m), LD)
        for t, r in enumerate(self.centre_rows()):
            c = self.xs[r].astype(LD)
            rows = slice(128 * t, min(128 * t + 128, self.n))
            p2 = ((self.xs[rows].astype(LD) - c) ** 2).sum(1)
            q2 = ((self.xps.astype(LD) - c) ** 2).sum(1)
            S[rows] = p2[:, None] + q2[None, :]
        R = np.zeros((self.n, self.m))
        axs, axps = np.abs(self.xs), np.abs(self.xps)
        for k in range(self.d):
            R += np.abs(self.xs[:, k][:, None] - self.xps[:, k][None, :]) * (axs[:, k][:, None] + axps[:, k][None, :])
        return self.K * LD(U) * ((self.d + 6) * S + R.astype(LD) + 4) + LD(SUBNORMAL)

    def worst(self, out, tol, normal_only=False):
        """max |out − K| / tol over the written part (<= 1 passes), and where; normal_only: over
        the entries in float64's normal range (a figure to report: below it the one-spacing
        term dominates)."""
        mask = self.mask & (self.K >= np.ldexp(LD(1), -1022)) if normal_only else self.mask
        q = np.where(mask, np.abs(out.astype(LD) - self.K) / tol, LD(0))
        k = np.unravel_index(int(np.argmax(q)), q.shape)
        return float(q[k]), (int(k[0]), int(k[1]), float(self.arg[k]), float(out[k]), float(self.K[k]))


def emulate_direct(case):
    """The direct-difference kernels in numpy float64: e = xs_i − xs'_j, a accumulated over k in
    order (a rounded product and a rounded sum where the kernel has one fma: no more accurate),
    sf2·exp(−½a) with the libm exp, + diag_add on i == j."""
    a = np.zeros((case.n, case.m))
    for k in range(case.d):
        e = case.xs[:, k][:, None] - case.xps[:, k][None, :]
        a = e * e + a
    out = case.sf2 * np.exp(-0.5 * a)
    if case.diag_add:
        out[np.arange(case.n), np.arange(case.n)] += case.diag_add
    return out


def _fma_sub(a, b, c):
    """fl(a·b − c) with one rounding, element-wise (exact rational arithmetic)."""
    out = np.empty(a.shape)
    flat = out.reshape(-1)
    bb = np.broadcast_to(b, a.shape).reshape(-1)
    cc = np.broadcast_to(c, a.shape).reshape(-1)
    for i, v in enumerate(a.reshape(-1)):
        flat[i] = float(Fraction(float(v)) * Fraction(float(bb[i])) - Fraction(float(cc[i])))
    return out


def emulate_centred(case, fused=True, centred=True):
    """The matrix-core kernel's arithmetic in numpy float64: p = x·inv_ell − c per 128-row tile
    with c = fl(x_first·inv_ell) — in one rounding (fused, what the compiler makes of
    gram_stage_half) or with the product rounded first — the cross products accumulated over k,
    ½‖p‖² from two half sums, res/2 = (p·q − ½‖p‖²) − ½‖q‖², sf2·exp, + diag_add.  centred =
    False drops the shift (the reference's own expansion), for the host test that shows the
    bound tells the two apart."""
    n, m, d = case.n, case.m, case.d
    out = np.empty((n, m))

    def half_norm(v):
        h0, h1 = np.zeros(v.shape[0]), np.zeros(v.shape[0])
        for k in range(d // 2):
            h0 = v[:, k] * v[:, k] + h0
        for k in range(d // 2, d):
            h1 = v[:, k] * v[:, k] + h1
        return 0.5 * (h0 + h1)

    for t, r in enumerate(case.centre_rows()):
        c = case.x[r] * case.inv if centred else np.zeros(d)
        rows = slice(128 * t, min(128 * t + 128, n))
        if fused:
            p, q = _fma_sub(case.x[rows], case.inv, c), _fma_sub(case.xp, case.inv, c)
        else:
            p, q = case.x[rows] * case.inv - c, case.xp * case.inv - c
        acc = np.zeros((p.shape[0], m))
        for k in range(d):
            acc = p[:, k][:, None] * q[:, k][None, :] + acc
        res = (acc - half_norm(p)[:, None]) - half_norm(q)[None, :]
        out[rows] = case.sf2 * np.exp(res)
    if case.diag_add:
        out[np.arange(n), np.arange(n)] += case.diag_add
    return out


# ------------------------------------------------------------------ 1c-1f: score terms
SCORE_FIXTURE = os.path.join(GOLDEN, "score_terms.npz")
YTR_MEAN, YTR_VAR = 0.1, 1.7     # the train-target statistics handed to gps_scores
SC_CRPS, SC_LOGS, SC_MSLL, SC_SMSE, SC_MSE, SC_COVER = range(6)


def load_score_fixture():
    """m, c, y and the 60-digit CRPS / LogS terms as longdouble (hi + lo)."""
    need_extended()
    with np.load(SCORE_FIXTURE, allow_pickle=False) as z:
        g = {k: z[k] for k in z.files}
    g["crps"] = g["crps_hi"].astype(LD) + g["crps_lo"].astype(LD)
    g["logs"] = g["logs_hi"].astype(LD) + g["logs_lo"].astype(LD)
    return g


def score_terms_f64(m, c, y, ytr_mean=YTR_MEAN, ytr_var=YTR_VAR):
    """The six per-point terms [crps, logs, msll, (m − y)², (ȳ − y)², cover] in float64, written
    as crps_term / logs_term / score_rows_kernel write them, with math.erf.  Non-finite inputs
    propagate as IEEE arithmetic has it (nothing is clamped)."""
    m, c, y = (np.asarray(a, np.float64) for a in (m, c, y))
    with np.errstate(all="ignore"):
        s = np.sqrt(c)
        z = (y - m) / s
        erf = np.array([math.erf(v) for v in (z * 0.70710678118654752440).ravel()]).reshape(z.shape)
        cdf = 0.5 * (1.0 + erf)
        pdf = 0.39894228040143267794 * np.exp(-z * z * 0.5)
        crps = s * (z * (2.0 * cdf - 1.0) + 2.0 * pdf - 0.56418958354775628695)
        e = y - m
        logs = e * e / (2.0 * c) + np.log(s) + 0.91893853320467274178
        e0 = y - ytr_mean
        msll = logs - (0.5 * math.log(6.28318530717958647692 * ytr_var) + e0 * e0 / (2.0 * ytr_var))
        cover = (((m + 2.0 * s - y) > 0.0) & ((y - (m - 2.0 * s)) > 0.0)).astype(np.float64)
    return np.stack([crps, logs, msll, (m - y) * (m - y), e0 * e0, cover])


def term_references(g, ytr_mean=YTR_MEAN, ytr_var=YTR_VAR):
    """Longdouble references and bounds of the five real-valued scores of ONE point (gps_scores
    with nt = 1), per fixture point: {score: (ref, bound)}.
      CRPS  64u·|ref|;  LogS  8u·(|q| + |log s| + 1 + |ref|), q = (y − m)²/2c;
      MSLL  8u·(|q| + |log s| + 1 + |½log 2πv| + |q0| + |ref|), q0 = (y − ȳ)²/2v;
      MSE   4u·ref (a difference, a square);  SMSE  8u·ref (two of those and a quotient);
      both + 2^-1074 where the square underflows (y − m = 1e-200)."""
    m, c, y = (g[k].astype(LD) for k in ("m", "c", "y"))
    q = (y - m) ** 2 / (2 * c)
    ls = np.abs(0.5 * np.log(c))
    trivc = 0.5 * np.log(2 * LD(np.pi) * LD(ytr_var))   # |Δπ| ~ 1e-16 relative: far below 8u·1
    q0 = (y - LD(ytr_mean)) ** 2 / (2 * LD(ytr_var))
    msll = g["logs"] - (trivc + q0)
    mse = (m - y) ** 2
    smse = mse / (y - LD(ytr_mean)) ** 2
    u = LD(U)
    return {
        SC_CRPS: (g["crps"], 64 * u * np.abs(g["crps"])),
        SC_LOGS: (g["logs"], 8 * u * (q + ls + 1 + np.abs(g["logs"]))),
        SC_MSLL: (msll, 8 * u * (q + ls + 1 + np.abs(trivc) + q0 + np.abs(msll))),
        SC_MSE: (mse, 4 * u * mse + LD(SUBNORMAL)),
        SC_SMSE: (smse, 8 * u * smse + LD(SUBNORMAL)),
    }


def sum_references(m, c, y, ytr_mean=YTR_MEAN, ytr_var=YTR_VAR):
    """gps_scores' six outputs from math.fsum of the float64 per-point terms, with the bound
    128u·Σ|t_i| on each sum carried to the output (÷ nt; SMSE, a quotient of two sums of
    non-negative terms: 256u·ref); the coverage is an exact count."""
    t = score_terms_f64(m, c, y, ytr_mean, ytr_var)
    nt = t.shape[1]
    s = [math.fsum(row) for row in t]
    a = [math.fsum(np.abs(row)) for row in t]
    ref = {SC_CRPS: s[0] / nt, SC_LOGS: s[1] / nt, SC_MSLL: s[2] / nt, SC_SMSE: s[3] / s[4],
           SC_MSE: s[3] / nt, SC_COVER: s[5] / nt}
    tol = {SC_CRPS: 128 * U * a[0] / nt, SC_LOGS: 128 * U * a[1] / nt, SC_MSLL: 128 * U * a[2] / nt,
           SC_SMSE: 256 * U * s[3] / s[4], SC_MSE: 128 * U * a[3] / nt, SC_COVER: 0.0}
    return ref, tol


SEAM_NT = (1, 255, 256, 257, 1000, 262145)


def seam_inputs(nt):
    """nt predictive points with variances log-uniform over [1e-6, 1e6] and y = m + z·sd,
    z ~ 1.2·N(0, 1): terms of very different magnitude in one sum."""
    rng = np.random.default_rng(500 + nt)
    m = rng.standard_normal(nt)
    c = 10.0 ** rng.uniform(-6.0, 6.0, nt)
    y = m + 1.2 * rng.standard_normal(nt) * np.sqrt(c)
    return m, c, y
