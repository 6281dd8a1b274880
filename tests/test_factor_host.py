"""The factorisation's bounds on the CPU (no GPU): a float64 numpy restatement of the device
algorithm — the 128-leaf as right-looking 16-column panels with a·rsqrt(d) multipliers and the
block-row inverse, the recursion of potrf_inv_rec, the tile tasks LEAF / TRSM / UPD / UPDX / FIN
of the persistent kernel — meets every bound of tests/factor_cases.py on every input that
tests/test_gpu_factor.py gives the device, and each defect built into a COPY of it (never into a
kernel) fails a named check.  DESIGN §21 records the ratios printed here."""
import numpy as np
import pytest

import factor_cases as FC

T = FC.TILE


# ------------------------------------------------------------------ the restatement
def _rsqrt(d):
    """The pivot's multiplier: NaN for d <= 0, NaN or +Inf (the device's Newton steps turn the
    seeds rsq(0) = Inf and rsq(Inf) = 0 into NaN)."""
    if not (d > 0.0) or not np.isfinite(d):
        return np.nan
    return 1.0 / np.sqrt(d)


def _invert16(Lpp):
    """X_pp = L_pp⁻¹ column by column (right-looking substitution, lane c forms column c)."""
    r = 1.0 / np.diag(Lpp)
    acc = np.zeros((16, 16))
    x = np.zeros((16, 16))
    c = np.arange(16)
    for k in range(16):
        x[k] = np.where(k < c, 0.0, np.where(k == c, r[k], -acc[k] * r[k]))
        acc[k + 1:] += np.outer(Lpp[k + 1:, k], x[k])
    return x


def leaf_model(A, nreal, base, mut, tile):
    """One 128-block: (L, X, logdiag, flagged minors).  mut: the defects aimed at leaf `tile`."""
    S = np.tril(A).copy()
    t16 = lambda i, j: (slice(16 * i, 16 * i + 16), slice(16 * j, 16 * j + 16))
    for p in range(8):
        J0, hi = 16 * p, 16 * p + 16
        for j in range(J0, hi):
            d = S[j, j]
            rs = _rsqrt(d)
            S[j + 1:, j] = S[j + 1:, j] * rs
            S[j, j] = d * rs
            if j + 1 < hi:   # the rest of the panel (its rows above the diagonal are cleared below)
                S[j + 1:, j + 1:hi] -= np.outer(S[j + 1:, j], S[j + 1:hi, j])
        S[J0:hi, J0:hi] = np.tril(S[J0:hi, J0:hi])
        for tj in range(p + 1, 8):      # column p+1: the lookahead (phase B); the rest: phase A
            for ti in range(tj, 8):
                if mut.get("skip_tile") == (tile, p, ti, tj):
                    continue
                reps = 2 if (mut.get("lookahead_twice") == (tile, p) and tj == p + 1) else 1
                for _ in range(reps):
                    S[t16(ti, tj)] -= S[t16(ti, p)] @ S[t16(tj, p)].T
    L = np.tril(S)
    X = np.zeros((T, T))
    for p in range(8):
        Xpp = _invert16(L[t16(p, p)])
        X[t16(p, p)] = Xpp
        for k in range(p):
            Tk = np.zeros((16, 16))
            for j in range(k, p):
                Tk += L[t16(p, j)] @ X[t16(j, k)]
            X[t16(p, k)] = -(Xpp @ Tk)
    dg = np.diag(L).copy()
    with np.errstate(invalid="ignore", divide="ignore"):
        logdiag = np.log(dg)
    lim = T if mut.get("ignore_nreal") else nreal
    off = 0 if mut.get("info_off_by_one") else 1
    flagged = [base + t + off for t in range(T) if not (dg[t] > 0.0) and t < lim]
    return L, X, logdiag, flagged


class Model:
    """potrf_inv on the padded matrix: L, X, logdiag, info and the plan, as gps_potrf_diag
    reports them."""

    def __init__(self, A, dag=True, dag_tiles=20, mut=None):
        self.n = n = A.shape[0]
        self.mut = mut or {}
        self.dag, self.dag_tiles = dag, dag_tiles
        self.W = FC.pad_identity(A)
        n_pad = self.W.shape[0]
        self.L = np.zeros((n_pad, n_pad))
        self.X = np.zeros((n_pad, n_pad))
        self.logdiag = np.zeros(n_pad)
        self.flagged = []
        self.plan = {"n_pad": n_pad, "leaves": 0, "dags": [], "gemms": 0}
        with np.errstate(invalid="ignore", over="ignore"):
            self.rec(0, n_pad // T)
        pick = max if self.mut.get("info_max") else min
        self.info = pick(self.flagged) if self.flagged else 0

    def blk(self, r0, i, j):
        return (slice(r0 + T * i, r0 + T * (i + 1)), slice(r0 + T * j, r0 + T * (j + 1)))

    def leaf(self, r0, standalone):
        d = slice(r0, r0 + T)
        L, X, ld, fl = leaf_model(self.W[d, d], self.n - r0, r0, self.mut, r0 // T)
        self.L[d, d], self.X[d, d], self.logdiag[d] = L, X, ld
        self.W[d, d] = L
        self.flagged += fl
        self.plan["leaves"] += standalone

    def rec(self, r0, nb):
        if nb == 1:
            return self.leaf(r0, 1)
        if self.dag and nb <= self.dag_tiles:
            return self.dag_block(r0, nb)
        n1b = nb // 2
        a, b = slice(r0, r0 + T * n1b), slice(r0 + T * n1b, r0 + T * nb)
        W, L, X = self.W, self.L, self.X
        self.rec(r0, n1b)
        L21 = W[b, a] @ X[a, a].T              # L21 = A21·X11ᵀ
        L[b, a] = L21
        W[b, b] -= L21 @ L21.T                 # trailing update (the lower tiles are read later)
        Tm = L21 @ X[a, a]                     # T = L21·X11
        self.rec(r0 + T * n1b, nb - n1b)
        X[b, a] = -(X[b, b] @ Tm)              # X21 = −X22·T
        self.plan["gemms"] += 4

    def dag_block(self, r0, nt):
        W, L, X, mut = self.W, self.L, self.X, self.mut
        B = lambda i, j: self.blk(r0, i, j)
        self.plan["dags"].append(nt)
        stale = {}
        for k in range(nt):
            self.leaf(r0 + T * k, 0)                                   # LEAF(k)
            for i in range(k + 1, nt):                                  # TRSM(i, k)
                W[B(i, k)] = W[B(i, k)] @ X[B(k, k)].T
                L[B(i, k)] = W[B(i, k)]
            for j in range(k + 1, nt):                                  # UPD(i, j, k)
                for i in range(j, nt):
                    a, b = W[B(i, k)], W[B(j, k)]
                    if mut.get("upd_drop_k4") == (i, j, k):
                        a, b = a[:, :T - 4], b[:, :T - 4]
                    if k == j - 1:
                        stale[(i, j)] = W[B(i, j)].copy()               # A_ij before its last update
                    W[B(i, j)] -= a @ b.T
        for j in range(nt):
            for k in range(j):                                          # FIN(j, k)
                sgn = 1.0 if mut.get("fin_sign") == (j, k) else -1.0
                X[B(j, k)] = sgn * (X[B(j, j)] @ X[B(j, k)])
            for i in range(j + 1, nt):                                  # UPDX(i, k, j)
                for k in range(j + 1):
                    Lij = W[B(i, j)]
                    if mut.get("updx_stale") == (i, k, j):
                        Lij = stale[(i, j)] @ X[B(j, j)].T
                    term = Lij @ X[B(j, k)]
                    X[B(i, k)] = term if j == k else X[B(i, k)] + term


def run(A, dag=True, dag_tiles=20, mut=None):
    return Model(A, dag, dag_tiles, mut)


# ------------------------------------------------------------------ the named checks
LOG_ULP_HOST = 1.0   # numpy's log is within 1 ulp of the longdouble reference


def failed_checks(m, A, expect_info=0, rows=None):
    """Names of the checks the result m (a Model, or anything with its fields) fails."""
    bad = []
    if m.info != expect_info:
        bad.append("info")
    if any(f > m.n for f in m.flagged):
        bad.append("flags")
    if expect_info == 0 and m.info == 0:
        f, _ = FC.check_factor(FC.pad_identity(A), m.L, m.X, rows, m.dag, m.dag_tiles)
        bad += f
        bad += FC.check_structure(m.L, m.X, m.logdiag, m.n)
        if not np.all(FC.log_ulps(m.logdiag, m.L, m.L.shape[0]) <= LOG_ULP_HOST):
            bad.append("logs")
    return bad


RATIOS = {}   # (plan, family) -> largest ratio per bound, printed at the end of the module


def note(plan, fam, r):
    cur = RATIOS.setdefault((plan, fam), {"F": 0.0, "X": 0.0, "R": 0.0})
    for k in cur:
        cur[k] = max(cur[k], r[k])


def clean_case(n, fam, dag, dag_tiles, plan_name, expect_plan):
    A = FC.family(fam, n)
    m = run(A, dag, dag_tiles)
    got = (m.plan["leaves"], m.plan["dags"], m.plan["gemms"])
    assert got == expect_plan == FC.plan_of(m.plan["n_pad"] // T, dag, dag_tiles), got
    rows = FC.rows_for(n, dag, dag_tiles)
    bad, r = FC.check_factor(FC.pad_identity(A), m.L, m.X, rows, dag, dag_tiles)
    note(plan_name, fam, r)
    print(f"factor host {plan_name:9s} n={n:4d} {fam:2s} " +
          " ".join(f"{k}={v:.3g}" for k, v in r.items()))
    assert bad == [], (n, fam, r)
    assert m.info == 0 and m.flagged == []
    assert FC.check_structure(m.L, m.X, m.logdiag, n) == []
    assert np.all(FC.log_ulps(m.logdiag, m.L, m.L.shape[0]) <= LOG_ULP_HOST)


@pytest.mark.parametrize("fam", FC.FAMILIES)
def test_leaf_meets_the_bounds(fam):
    for n in FC.LEAF_NS:
        clean_case(n, fam, True, 20, "leaf", (1, [], 0))


@pytest.mark.parametrize("fam", FC.FAMILIES)
def test_recursion_meets_the_bounds(fam):
    for n in FC.REC_NS:
        nb = FC.n_pad_of(n) // T
        clean_case(n, fam, False, 20, "recursion", (nb, [], 4 * (nb - 1)))


@pytest.mark.parametrize("n,nt", FC.DAG_CASES)
def test_persistent_meets_the_bounds(n, nt):
    for fam in FC.FAMILIES:
        clean_case(n, fam, True, nt, "dag", (0, [nt], 0))


def test_mixed_and_large_meet_the_bounds():
    n, tiles = FC.MIXED
    for fam in FC.FAMILIES:
        clean_case(n, fam, True, tiles, "mixed", (1, [2, 2], 8))
    clean_case(FC.BIG_N, "a", True, 20, "big", (0, [10, 11], 4))
    clean_case(FC.BIG_N, "b6", True, 20, "big", (0, [10, 11], 4))


def test_zz_print_ratio_table():
    """The table DESIGN §21 quotes (run with -s)."""
    for (plan, fam), r in sorted(RATIOS.items()):
        print(f"factor host max  {plan:9s} {fam:2s} F={r['F']:.3g} X={r['X']:.3g} R={r['R']:.3g}")


def test_scaling_is_exact_in_the_restatement():
    """D A D with D = diag(2^k): every operation of the algorithm scales exactly (the numpy
    1/sqrt pivots are exact under 4^k), so L(DAD) = D·L(A) and X(DAD) = X(A)·D⁻¹ bitwise."""
    n = 300
    A = FC.fam_a(n)
    k = FC.scale_exponents(n, 100)
    kp = np.zeros(FC.n_pad_of(n), np.int32)
    kp[:n] = k
    for dag in (False, True):
        m0, m1 = run(A, dag), run(FC.scaled(A, k), dag)
        assert np.array_equal(m1.L, np.ldexp(m0.L, kp[:, None]))
        assert np.array_equal(m1.X, np.ldexp(m0.X, -kp[None, :]))


# ------------------------------------------------------------------ defects (CPU copies only)
# (on the ill-conditioned families a defect of the factor can push a later pivot below zero: the
#  wrong matrix is then caught by 'info' before the value checks run)
def mutated(n, dag, dag_tiles, mut, fam="a"):
    A = FC.family(fam, n)
    assert failed_checks(run(A, dag, dag_tiles), A) == []      # the clean copy passes them all
    return failed_checks(run(A, dag, dag_tiles, mut), A), A


def test_defect_one_tile_update_skipped():
    for fam in FC.FAMILIES:
        bad, _ = mutated(128, True, 20, {"skip_tile": (0, 2, 5, 4)}, fam)
        assert ("F" in bad) if fam in "ac" else bool({"F", "info"} & set(bad)), (fam, bad)


def test_defect_last_k_slice_of_one_upd_dropped():
    for fam in FC.FAMILIES:
        bad, _ = mutated(384, True, 3, {"upd_drop_k4": (2, 1, 0)}, fam)
        assert ("F" in bad) if fam in "ac" else bool({"F", "info"} & set(bad)), (fam, bad)
    bad, _ = mutated(384, True, 3, {"upd_drop_k4": (2, 2, 1)})
    assert "F" in bad, bad


def test_defect_one_fin_tile_with_the_wrong_sign():
    for fam in FC.FAMILIES:
        bad, _ = mutated(384, True, 3, {"fin_sign": (2, 1)}, fam)
        assert "X" in bad and "R" in bad and "F" not in bad, (fam, bad)


def test_defect_updx_reads_l_before_its_last_update():
    for fam in FC.FAMILIES:
        bad, _ = mutated(384, True, 3, {"updx_stale": (2, 0, 1)}, fam)
        assert "X" in bad and "R" in bad and "F" not in bad, (fam, bad)


def test_defect_lookahead_update_applied_twice():
    for fam in FC.FAMILIES:
        bad, _ = mutated(128, True, 20, {"lookahead_twice": (0, 3)}, fam)
        assert ("F" in bad) if fam in "ac" else bool({"F", "info"} & set(bad)), (fam, bad)
    bad, _ = mutated(300, True, 3, {"lookahead_twice": (2, 0)})   # a padded leaf inside a block
    assert "F" in bad, bad


class Perturbed:
    def __init__(self, m, L=None, X=None):
        self.__dict__.update(m.__dict__)
        self.L = m.L if L is None else L
        self.X = m.X if X is None else X


def nrel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@pytest.mark.parametrize("n,dag,lij,xij", [(128, True, (100, 3), (100, 99)),
                                           (128, True, (127, 90), (127, 127)),
                                           (300, False, (299, 2), (299, 299)),
                                           (300, True, (200, 3), (130, 130)),
                                           (300, True, (260, 260), (257, 256))])
def test_defect_one_entry_off_by_1e12_relative(n, dag, lij, xij):
    """One entry of L, and separately of L⁻¹, off by 1e-12 relative (9007 u) on family (a): the
    componentwise checks see it, the suite's older normwise assertions do not.  (The bounds grow
    with the number of terms behind an entry, so what they resolve depends on the entry: these
    are entries with few terms behind them or with a dominant term — the diagonal, the first
    columns, the columns next to the diagonal; DESIGN §21 gives the threshold.)"""
    A = FC.fam_a(n)
    m = run(A, dag, 3)
    assert failed_checks(m, A) == []
    Lr = np.linalg.cholesky(A)
    L2 = m.L.copy()
    L2[lij] *= 1.0 + 1e-12
    assert "F" in failed_checks(Perturbed(m, L=L2), A)
    assert nrel(np.tril(L2[:n, :n]), Lr) < 1e-12                # the old assertion passes
    X2 = m.X.copy()
    X2[xij] *= 1.0 + 1e-12
    bad = failed_checks(Perturbed(m, X=X2), A)
    assert "X" in bad and "R" in bad, bad
    assert nrel(np.sum(X2[:, :n] ** 2, axis=0), np.diag(np.linalg.inv(A))) < 1e-10   # diag_inv's


BAD_CASES = [(128, True, 20, (k,)) for k in (0, 15, 16, 63, 64, 111, 112, 127)] + \
    [(100, True, 20, (99,))] + \
    [(384, dag, 3, (k,)) for dag in (False, True) for k in (128, 255, 256, 383)] + \
    [(640, True, 2, (k,)) for k in (100, 300, 600)] + \
    [(300, True, 20, (200, 70))]


@pytest.mark.parametrize("n,dag,tiles,ks", BAD_CASES)
def test_first_non_pd_minor_in_the_restatement(n, dag, tiles, ks):
    A, info = FC.bad_pivot_matrix(n, ks)
    m = run(A, dag, tiles)
    assert failed_checks(m, A, info) == []
    # the defects of the index
    assert "info" in failed_checks(run(A, dag, tiles, {"info_off_by_one": True}), A, info)
    if len(ks) > 1:
        assert "info" in failed_checks(run(A, dag, tiles, {"info_max": True}), A, info)
    if n % T:
        # a bad pivot's NaNs reach the padding rows: without the tid < nreal mask they are
        # flagged too (the minimum hides them from info: only the flags show it)
        bad = failed_checks(run(A, dag, tiles, {"ignore_nreal": True}), A, info)
        assert bad == ["flags"], bad
        assert "info" in failed_checks(run(A, dag, tiles, {"ignore_nreal": True, "info_max": True}),
                                       A, info)


@pytest.mark.parametrize("val", [np.nan, np.inf])
def test_nan_and_inf_pivots_in_the_restatement(val):
    A, info = FC.bad_pivot_matrix(384, (150,), values={150: val})
    assert failed_checks(run(A, True, 3), A, info) == []
    assert failed_checks(run(A, False, 3), A, info) == []


def test_unmodified_padded_matrix_flags_nothing():
    A = FC.fam_a(100)
    m = run(A)
    assert m.info == 0 and m.flagged == []
    assert failed_checks(run(A, mut={"ignore_nreal": True}), A) == []   # (identity pivots are 1)


def test_constants_are_the_documented_formulas():
    assert FC.C_R_LEAF == 146 and FC.c_r(1) == 146
    assert FC.c_r(3, True, 3) == 128 * 2 + 2 + 128 + 146
    assert FC.c_r(3, False) == (128 + 8) + (256 + 8) + FC.c_r(2, False)
    assert FC.c_r(2, False) == 2 * (128 + 8) + 146
    K, R = FC.c_f_tiles(3, False)
    assert K[1, 0] == 136 and K[2, 0] == 136 and K[2, 1] == 136 and K[0, 0] == 0
    assert R[2, 1] == 146 and np.all(np.triu(K, 0) == 0)
    assert FC.plan_of(5, True, 2) == (1, [2, 2], 8)
    assert FC.plan_of(21, True, 20) == (0, [10, 11], 4)
    assert FC.split_rows(5, True, 2) == [256, 384]
    for nb, dag, tiles in ((1, True, 20), (3, False, 20), (3, True, 3), (5, True, 2), (5, True, 5),
                           (21, True, 20)):
        C = FC.c_r_entries(nb, dag, tiles)
        assert C.max() == FC.c_r(nb, dag, tiles)                # the flat constant is its maximum
        low = np.tril(np.ones_like(C, dtype=bool))
        assert np.all(C[low] >= FC.SUBST16) and not C[~low].any()
        # never decreasing down a column: what lets one matrix bound X̂ − L̂⁻¹ = L̂⁻¹·R as well
        assert np.all((np.diff(C, axis=0) >= 0) | ~low[1:])


def test_bad_arguments_are_refused_without_a_device():
    """gps_potrf_diag judges its arguments before it binds a device: -1, nothing written."""
    from gpscore import _lib
    lib = _lib.load()
    A = FC.fam_a(8)
    L, X, ld = np.zeros((128, 128)), np.zeros((128, 128)), np.zeros(128)
    info, plan = np.zeros(1, np.int32), np.full(8, -7, np.int32)
    ip, pp = info.ctypes.data_as(_lib._PI), plan.ctypes.data_as(_lib._PI)
    p = _lib.ptr
    f = lib.gps_potrf_diag
    assert f(None, 0, p(A), 8, p(L), p(X), p(ld), ip, pp) == -1
    assert f(None, 8, p(A), 7, p(L), p(X), p(ld), ip, pp) == -1
    assert f(None, 8, None, 8, p(L), p(X), p(ld), ip, pp) == -1
    assert f(None, 8, p(A), 8, p(L), p(X), p(ld), ip, None) == -1
    assert b"gps_potrf_diag" in lib.gps_last_error(None)
    assert np.all(plan == -7) and not L.any() and not X.any()
