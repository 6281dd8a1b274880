"""The element-wise device math, entry by entry and term by term, against extended precision.

Every other accuracy test here is normwise (max|a − b| / max|b|) on benign inputs, which sees
neither a wrong small Gram entry nor a wrong score term in the tails.  These tests reach the
same kernels through gps_gram and gps_scores with inputs built to cover the whole domain of
exp_neg (csrc/gps_internal.h), every Gram kernel's arithmetic, and crps_term / logs_term and
the two-level score reduction (kernels_vec.hip), and bound each output separately.

u = 2^-53.  References are numpy longdouble (64-bit significand) from the float64 values the
kernel receives, or the mpmath fixture tests/golden/score_terms.npz for the terms that need erf.
No bound below was taken from a kernel's output: each is the project's own claim (1 ulp for
exp_neg) or is derived in the docstring of its test, and test_elementwise_host.py shows that
plain float64 arithmetic meets every one of them on the same inputs (elementwise_cases.py).
"""
import math

import numpy as np
import pytest

import elementwise_cases as E
from conftest import record_floors

pytestmark = pytest.mark.gpu

U, LD = E.U, E.LD


def _gram(ctx, mode, x, xp, log_sf2, log_ell, diag_add, uplo, rbf=False):
    from gpscore._lib import GPS_ARD, GPS_RBF, ptr
    n, m, d = x.shape[0], xp.shape[0], x.shape[1]
    out = np.full((n, m), -7.0)
    ctx.set_gram_reg(mode)
    try:
        ctx.call("gps_gram", GPS_RBF if rbf else GPS_ARD, ptr(x), n, ptr(xp), m, d, log_sf2,
                 ptr(log_ell), len(log_ell), diag_add, uplo, ptr(out))
    finally:
        ctx.set_gram_reg(True)
    return out


def _scores(ctx, m, c, y):
    from gpscore._lib import ptr
    m, c, y = (np.ascontiguousarray(a, dtype=np.float64) for a in (m, c, y))
    out = np.full(6, -7.0)
    ctx.call("gps_scores", ptr(m), ptr(c), ptr(y), m.size, E.YTR_MEAN, E.YTR_VAR, ptr(out))
    return out


def _record(test, **ratios):
    """measured error / bound, next to the parity floors (conftest.record_floors)."""
    print(test, ratios)
    record_floors(test, ratios, {}, {k: 1.0 for k in ratios})


# ------------------------------------------------------------------ a. exp_neg
def test_exp_neg_whole_domain(gpu_ctx):
    """exp_neg alone: d = 1, log_sf2 = 0 and log_ell = 0 make sf2 and inv_ell exactly 1, so a
    1024 × 1024 full Gram is exp_neg(−½·fl(fl(x_i − x'_j)²)) and nothing else, under
    GPS_OPT_GRAM_REG 0 (gram_kernel<1>) and 1 (gram_reg_kernel<1>).  The 2^20 arguments
    (elementwise_cases.exp_inputs; their coverage is asserted in test_elementwise_host.py) hold
    0, |x| down to 5e-301 and the subnormal squares, [−1, 0] with no gap above 1e-3, [−708, −1]
    dense both uniformly and logarithmically, the subnormal results' band [−745.2, −708.4] and
    arguments past the clamp down to −801 — every table entry in each band.

    Bound: the comment's own claim, |out − exp(x)| <= 1 spacing of float64 at exp(x) (2^-1074
    below the normal range), exactly 0 where exp(x) < 2^-1075 (nothing but 0 is within reach of
    round-to-nearest there), exactly 1 at x = 0; and the two kernels bitwise equal.  On top of
    the claim, the mean signed error over the >= 10000 arguments that read one table entry is
    below 0.1 spacings for every entry: a lost or wrong table tail (up to half an ulp, which
    the one-ulp bound cannot tell from rounding) shows there."""
    x, xp = E.exp_inputs()
    arg = E.exp_args(x, xp)
    ref = E.exp_reference(arg)
    outs = [_gram(gpu_ctx, mode, x, xp, 0.0, np.zeros(1), 0.0, 0) for mode in (0, 1)]
    worst = E.exp_check(outs[0], arg, ref)
    normal = ref >= np.ldexp(LD(1), -1022)
    err = np.abs(outs[0].astype(LD) - ref) / E.f64_spacing(ref)
    _record("exp_neg", all=worst, normal=float(err[normal].max()), subnormal=float(err[~normal].max()))
    assert np.array_equal(outs[0], outs[1])
    assert np.all(outs[0] <= 1.0) and np.all(outs[0] >= 0.0)
    # no table entry is off by a fraction of an ulp (elementwise_cases.exp_table_bias)
    bias = E.exp_table_bias(outs[0], arg, ref)
    _record("exp_neg_bias", worst=float(np.abs(bias).max()) / E.EXP_BIAS_BOUND)
    assert np.all(np.abs(bias) <= E.EXP_BIAS_BOUND), (int(np.abs(bias).argmax()), bias)


# ------------------------------------------------------------------ b. Gram entries
def _check_gram_case(gpu_ctx, case, name):
    """Direct-difference kernels (modes 0 and 1; mode 2 where d is not 8 or 16).  The scaled
    features xs = fl(x·inv_ell) are mirrored exactly (one IEEE product; inv_ell from the same
    libm exp).  e_k = fl(xs_ik − xs'_jk) = e_k(1 + δ), |δ| <= u, so e_k² carries 2u; the fma
    chain a = Σ_k e_k² adds at most d roundings to a term: |Δa| <= (d + 2)u·a, and −½a is exact.
    K = sf2·exp(arg), so |ΔK|/K <= (d + 2)u·|arg| from the argument, 2u for exp_neg's one ulp,
    u for the product with sf2 and u for the diagonal add: (d + 2)·|arg| + 4.  The bound asserted
    is  K·u·((d + 6)·|arg| + 4) + 2^-1074 : the further 4·|arg| would admit inverse
    length-scales one ulp apart (2u on every e_k², twice over), which the shared libm makes
    unnecessary — it is slack, not a tuned constant.  2^-1074: one subnormal spacing, exp_neg's
    claim below the normal range; the product with sf2 rounds again (sf2·1 + ½ spacings), so
    the cases use sf2 = e^-0.75 < ½.

    Matrix-core kernel (mode 2, d in {8, 16}).  Per 128-row tile it holds p = x·inv_ell − c and
    q = x'·inv_ell − c, c = fl(x_first·inv_ell), and forms res/2 = (p·q − ½‖p‖²) − ½‖q‖² =
    −½‖p − q‖².  With S = ‖p‖² + ‖q‖²: the d-term fma dot product errs by at most d·u·Σ|p_k q_k|
    <= (d/2)u·S; each half norm (d/2 terms and the pair's sum) by (d/2 + 1)u·½‖·‖², together
    (d/4 + ½)u·S; the two subtractions by u·(|p·q| + ½‖p‖²) + u·½S <= (3/2)u·S; the roundings
    of p and q themselves by u·‖p − q‖(‖p‖ + ‖q‖) <= 2u·S: (3d/4 + 4.5)·u·S in all, inside
    (d + 6)·S for every d (the rest, again, is room for a one-ulp inv_ell).  One
    term that bound lacks: hipcc contracts the scaling into the subtraction, p = fma(x, inv_ell,
    −c), so this kernel's scaled features are NOT rounded to xs first, while the reference (one
    for every kernel: what the direct kernels compute) starts from the rounded xs.  The two
    differ by up to u·|xs_k| per coordinate, i.e. by u·R_ij in the argument, R_ij = Σ_k |e_k|·
    (|xs_ik| + |xs'_jk|) — the fused emulation on the CPU is 1.7 to 12 times over the
    bound without it and inside with it, fused or not.  Asserted:
    K·u·((d + 6)·S_ij + R_ij + 4) + 2^-1074.  For data off the origin R is small beside what
    the uncentred expansion loses, u·(‖xs‖² + ‖xs'‖²): the host test finds that 30 to 30 000
    times over this bound.

    The persistent matrix-core grid needs thousands of tiles and keeps its normwise tests
    (test_gpu_parity.py); it runs this same per-element code, so these shapes cover its
    arithmetic.  Shapes: ragged row and column tiles (333, 201); a square lower build with
    diag_add whose diagonal tiles take the per-element selects (333: 352 padded rows against 384
    padded columns, which launch_gram keeps on the direct-difference kernels under every mode);
    and 256, the lower build that does reach the matrix-core kernel's mask and diagonal add."""
    n, m, d, uplo = case.n, case.m, case.d, case.uplo
    outs = [_gram(gpu_ctx, mode, case.x, case.xp, E.GRAM_LOG_SF2, case.log_ell, case.diag_add,
                  uplo, case.rbf) for mode in (0, 1, 2)]
    assert np.array_equal(outs[0], outs[1])
    matrix_core = case.matrix_core
    ratios = {}
    for mode, out in ((1, outs[1]), (2, outs[2])):
        tol = case.tol_centred() if mode == 2 and matrix_core else case.tol_direct()
        worst, where = case.worst(out, tol)
        ratios["mode%d" % mode] = worst
        ratios["mode%d_normal" % mode] = case.worst(out, tol, normal_only=True)[0]
        assert worst <= 1.0, (mode, worst, where)
        if uplo:
            assert np.all(out[~case.mask] == 0.0)   # the unwritten half
    _record(name, **ratios)
    if matrix_core:
        assert not np.array_equal(outs[2], outs[1])  # the matrix-core kernel ran
    else:
        assert np.array_equal(outs[2], outs[1])
    # exact duplicates: the argument is exactly 0 and exp_neg(0) exactly 1
    i, j = E.gram_duplicates(uplo, n)
    assert np.all(outs[1][i, j] == case.sf2)
    if uplo:
        # the diagonal carries diag_add (the matrix-core kernel's: inside its bound, above)
        assert np.all(np.diag(outs[1]) == case.sf2 + case.diag_add)


@pytest.mark.parametrize("n,m,uplo", E.GRAM_SHAPES)
@pytest.mark.parametrize("d", E.GRAM_DIMS)
def test_gram_entries_componentwise(gpu_ctx, d, n, m, uplo):
    """Every entry of an ARD Gram with per-dimension length-scales, under modes 0, 1 and 2, at
    d = 1, 2, 8, 16, 63 and 64 (GPS_MAX_D), inside its own bound (_check_gram_case has the
    derivation); arguments from 0 (exact duplicates) and 1e-30 through the subnormal results to
    −45000 in one matrix."""
    _check_gram_case(gpu_ctx, E.GramCase(d, n, m, uplo), "gram_d%d_%dx%d_%s" % (d, n, m, "lower" if uplo else "full"))


def test_gram_entries_componentwise_rbf(gpu_ctx):
    """The RBF parametrisation (one b = log ℓ², inv_ell = exp(−b/2)) at d = 8, same bounds."""
    _check_gram_case(gpu_ctx, E.GramCase(8, 333, 201, 0, rbf=True), "gram_d8_rbf")


@pytest.mark.parametrize("d", [1, 2, 8, 16, 64])
def test_gram_full_square_is_bitwise_symmetric(gpu_ctx, d):
    """K(x, x) built in full by the direct-difference kernels: fl(a − b) = −fl(b − a) and the
    squares are summed in the same order on both sides of the diagonal, so the matrix is
    symmetric to the bit, with exactly sf2 on its diagonal."""
    case = E.GramCase(d, 333, 333, 1)
    for mode in (0, 1):
        out = _gram(gpu_ctx, mode, case.x, case.x, E.GRAM_LOG_SF2, case.log_ell, 0.0, 0)
        assert np.array_equal(out, out.T)
        assert np.all(np.diag(out) == case.sf2)


# ------------------------------------------------------------------ c. score terms
@pytest.fixture(scope="module")
def score_fixture():
    return E.load_score_fixture()


def test_score_terms_one_at_a_time(gpu_ctx, score_fixture):
    """gps_scores with nt = 1 returns crps_term and logs_term of that point unchanged (block_sum
    over one value and zeros is exact, and the division is by 1).  375 points: z from 0 and
    1e-300 to the tails (26, 37.5, 38.6 where exp(−z²/2) goes subnormal, 40, 1e5, −1e10),
    variances from 1e-300 to 1e200; references from mpmath at 60 digits.

    CRPS: relative error <= 64u.  The device math library meets the OpenCL double-precision
    limits erf <= 16 ulp, exp <= 3, log <= 3, sqrt and divide correctly rounded; z carries
    about 2u and enters with |∂/∂z| <= 1; CRPS/s >= 0.2337 everywhere (its value at z = 0),
    so no term of s·(z·(2Φ − 1) + 2φ − 1/√π) is large against the result.
    LogS: |Δ| <= 8u·(|q| + |log s| + 1 + |ref|), q = (y − m)²/2c: q carries 4u (a difference,
    a square, a quotient), log s 3 ulp = 6u and u/2 from the square root, the two sums u each of
    their partial results; the three terms can cancel, hence the absolute form.
    MSLL adds the trivial model's two terms in the same way; MSE is 4u relative, SMSE 8u."""
    g = score_fixture
    got = np.array([_scores(gpu_ctx, g["m"][i:i + 1], g["c"][i:i + 1], g["y"][i:i + 1])
                    for i in range(len(g["m"]))])
    ratios = {}
    for k, (ref, tol) in E.term_references(g).items():
        err = np.abs(got[:, k].astype(LD) - ref)
        bad = int(np.argmax(err - tol))
        ratios["sc%d" % k] = float(np.max(err / np.where(tol > 0, tol, 1)))
        assert np.all(err <= tol), (k, g["m"][bad], g["c"][bad], g["y"][bad], got[bad, k], float(ref[bad]))
    _record("score_terms", **ratios)


# ------------------------------------------------------------------ d. coverage boundary
def test_coverage_boundary_is_open(gpu_ctx):
    """The 95 % interval is open on both sides (strict > in the reference and in
    score_rows_kernel).  m = 0 and c in {1, 0.25} make sd and m ± 2·sd exact: y on the boundary
    is not covered, the next float64 towards m is, the next one away is not."""
    pts = []
    for c in (1.0, 0.25):
        b = 2.0 * math.sqrt(c)
        for edge in (b, -b):
            pts += [(c, edge, 0.0), (c, np.nextafter(edge, 0.0), 1.0),
                    (c, np.nextafter(edge, 2.0 * edge), 0.0)]
    for c, y, want in pts:
        got = _scores(gpu_ctx, np.zeros(1), np.array([c]), np.array([y]))[E.SC_COVER]
        assert got == want, (c, y, got)
    c = np.array([p[0] for p in pts] + [1.0, 0.25, 1.0])
    y = np.array([p[1] for p in pts] + [0.0, 0.3, 5.0])
    want = sum(p[2] for p in pts) + 2.0
    got = _scores(gpu_ctx, np.zeros(c.size), c, y)[E.SC_COVER]
    assert got == want / c.size, (got, want, c.size)


# ------------------------------------------------------------------ e. non-finite inputs
def test_nonfinite_variance_propagates(gpu_ctx):
    """include/gpscore.h: NaN / Inf propagate, nothing is clamped.  A negative variance, and a
    zero variance with and without a residual, give NaN in CRPS, LogS and MSLL exactly where
    the float64 formula does (each of these three rows; no ordinary row), leave MSE and SMSE
    finite and equal to the reference, and count 0 towards the coverage."""
    rng = np.random.default_rng(5)
    nt = 300
    m = rng.standard_normal(nt)
    c = 10.0 ** rng.uniform(-2, 2, nt)
    y = m + rng.standard_normal(nt) * np.sqrt(c)
    bad = {17: (-0.5, 0.4), 130: (0.0, 0.4), 257: (0.0, 0.0)}   # row: (variance, y − m)
    for r, (v, e) in bad.items():
        c[r], y[r] = v, m[r] + e
    terms = E.score_terms_f64(m, c, y)
    nan_rows = np.isnan(terms[0])
    assert sorted(np.flatnonzero(nan_rows)) == sorted(bad) and np.all(terms[5][nan_rows] == 0.0)
    assert np.array_equal(np.isnan(terms[1]), nan_rows) and np.array_equal(np.isnan(terms[2]), nan_rows)
    for r in list(bad) + [0, 16, 131, 299]:      # row by row: NaN exactly where the formula's is
        one = _scores(gpu_ctx, m[r:r + 1], c[r:r + 1], y[r:r + 1])
        for k in (E.SC_CRPS, E.SC_LOGS, E.SC_MSLL):
            assert np.isnan(one[k]) == bool(nan_rows[r]), (r, k, one[k])
        assert one[E.SC_COVER] == terms[5][r]
        assert np.isfinite(one[E.SC_MSE]) and np.isfinite(one[E.SC_SMSE])
    out = _scores(gpu_ctx, m, c, y)
    assert np.isnan(out[E.SC_CRPS]) and np.isnan(out[E.SC_LOGS]) and np.isnan(out[E.SC_MSLL])
    mse, sq0 = math.fsum(terms[3]), math.fsum(terms[4])
    assert abs(out[E.SC_MSE] - mse / nt) <= 128 * U * mse / nt
    assert abs(out[E.SC_SMSE] - mse / sq0) <= 256 * U * mse / sq0
    assert out[E.SC_COVER] == terms[5].sum() / nt
    good = ~nan_rows                               # and the ordinary rows alone are finite
    assert np.all(np.isfinite(_scores(gpu_ctx, m[good], c[good], y[good])))


# ------------------------------------------------------------------ f. reduction seams
@pytest.mark.parametrize("nt", E.SEAM_NT)
def test_score_reduction_seams(gpu_ctx, nt):
    """The two-level fixed-order sum at its seams: one point, one workgroup less a lane, exactly
    one, one plus a lane, four ragged ones, and 262145 points = 1025 workgroups, where
    partials_sum_kernel's 1024 threads take a second trip through their loop.  Variances over
    twelve decades, so the terms of one sum differ widely.  Reference: math.fsum (exact
    summation) of the float64 terms with math.erf.  Bound per sum: 128u·Σ|t_i| — 64u for each
    term (the CRPS bound above, the largest) and a tree of depth below 64 (lane, wave, block,
    1024 partials, block again: u per level); SMSE, a quotient of two such sums of non-negative
    terms, 256u relative; the coverage an exact count.  Two calls agree to the bit."""
    m, c, y = E.seam_inputs(nt)
    ref, tol = E.sum_references(m, c, y)
    out = _scores(gpu_ctx, m, c, y)
    ratios = {}
    for k in ref:
        err = abs(out[k] - ref[k])
        ratios["sc%d" % k] = float(err / tol[k] if tol[k] else err)
        assert err <= tol[k], (k, out[k], ref[k], tol[k])
    _record("score_sums_nt%d" % nt, **ratios)
    assert np.array_equal(out, _scores(gpu_ctx, m, c, y))
