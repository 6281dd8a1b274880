"""Inputs, extended-precision references and componentwise error bounds of the factorisation with
its fused inverse (csrc/kernels_potrf.hip, potrf_inv_rec in csrc/api.hip), shared by
test_factor_host.py (CPU: a float64 restatement of the device algorithm meets the bounds, and
built-in defects miss them) and test_gpu_factor.py (the kernels, through gps_potrf_diag).
Nothing here touches the GPU.  DESIGN §21 holds the derivations.

Notation: u = 2^-53; L̂, X̂ the returned float64 factor and inverse on the padded n_pad × n_pad
square (n_pad = n rounded up to 128, A padded with the identity); "reference" is numpy longdouble
(64-bit significand) evaluated from the returned float64 values.  The signed quantities — the
residual A − L̂L̂ᵀ, L̂⁻¹, L̂X̂ − I — are formed in longdouble; the magnitude products of the bounds
(sums of non-negative terms, relative error <= 5·n_pad·u < 2e-12) in float64.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
TILE = 128
SUBNORMAL = 2.0 ** -1074          # the spacing of float64 below 2^-1022


def need_extended():
    """The references need a longdouble wider than float64 (x86: 64-bit significand)."""
    assert np.finfo(LD).nmant >= 63, "numpy longdouble is not extended precision here"


def n_pad_of(n):
    return (n + TILE - 1) // TILE * TILE


# ------------------------------------------------------------------ input families
def fam_a(n, seed=0):
    """M Mᵀ + 0.5 I, M = N(0,1)/√n: condition number about 9 (the suite's older family)."""
    rng = np.random.default_rng(1000 + 7 * n + seed)
    M = rng.standard_normal((n, n)) / np.sqrt(n)
    A = M @ M.T + 0.5 * np.eye(n)
    return (A + A.T) / 2


def fam_b(n, sigma2, seed=0):
    """RBF Gram (unit length scale) of n sorted 1-D inputs on [0, n/40] plus σ² I: the largest
    eigenvalue is about 40·√(2π) = 100, so cond ≈ 1e4 at σ² = 1e-2 and 1e8 at 1e-6 (for n >= 64;
    smaller n are better conditioned) — the project's regime."""
    rng = np.random.default_rng(2000 + 7 * n + seed)
    x = np.sort(rng.uniform(0.0, max(n, 2) / 40.0, n))
    d = x[:, None] - x[None, :]
    return np.exp(-0.5 * d * d) + sigma2 * np.eye(n)


def scale_exponents(n, kmax, seed=0):
    rng = np.random.default_rng(3000 + 7 * n + seed)
    return rng.integers(-kmax, kmax + 1, n)


def scaled(A, k):
    """D A D with D = diag(2^k_i): exact in float64 (powers of two, no over/underflow here)."""
    d = np.ldexp(1.0, np.asarray(k, dtype=np.int32))
    return A * d[:, None] * d[None, :]


def fam_c(n, seed=0):
    """Family (a) scaled as D A D, D = diag(2^k_i), |k_i| <= 40: entries spread over 2^±80 while
    every componentwise ratio of family (a) is unchanged."""
    return scaled(fam_a(n, seed), scale_exponents(n, 40, seed))


FAMILIES = ("a", "b2", "b6", "c")


def family(name, n, seed=0):
    if name == "a":
        return fam_a(n, seed)
    if name == "b2":
        return fam_b(n, 1e-2, seed)
    if name == "b6":
        return fam_b(n, 1e-6, seed)
    if name == "c":
        return fam_c(n, seed)
    raise KeyError(name)


def pad_identity(A):
    """A on the padded square, as the library pads it: identity in the padding."""
    n = A.shape[0]
    P = np.eye(n_pad_of(n))
    P[:n, :n] = A
    return P


def sample_rows(n, n_pad, splits=()):
    """At most 32 rows for the checks of a large factor: both sides of every 128 boundary (thinned
    evenly if there are many), the rows either side of the given split rows, row 0, row n−1 and
    the last padded row."""
    must = {0, n - 1, n_pad - 1}
    for s in splits:
        must |= {s - 1, s}
    edges = [b for b in range(TILE, n_pad, TILE)]
    room = (32 - len(must)) // 2
    if len(edges) > room:
        edges = [edges[int(round(i))] for i in np.linspace(0, len(edges) - 1, room)]
    for b in edges:
        must |= {b - 1, b}
    rows = sorted(r for r in must if 0 <= r < n_pad)
    return np.array(rows[:32])


# ------------------------------------------------------------------ the cases both files run
LEAF_NS = (1, 2, 15, 16, 17, 63, 64, 65, 112, 127, 128)      # one stand-alone leaf launch
REC_NS = (129, 256, 300, 384)                                # GPS_OPT_DAG = 0 (3 tiles: 1 + 2)
DAG_CASES = ((256, 2), (300, 3), (384, 3), (500, 4), (640, 5))   # (n, T): one persistent launch
MIXED = (640, 2)        # n, GPS_OPT_DAG_TILES: one leaf, two T = 2 launches, eight GEMMs
BIG_N = 2561            # defaults: persistent blocks of 10 and 11 tiles under one level
FULL_MAX = 384          # full-matrix checks up to this n_pad, 32 sampled rows above


def rows_for(n, dag=True, dag_tiles=20):
    """None (every row) up to FULL_MAX, else the sampled rows of this plan."""
    n_pad = n_pad_of(n)
    if n_pad <= FULL_MAX:
        return None
    return sample_rows(n, n_pad, split_rows(n_pad // TILE, dag, dag_tiles))


# ------------------------------------------------------------------ the launch plan, restated
def plan_of(nb, dag=True, dag_tiles=20):
    """What potrf_inv_rec launches for nb tiles: (leaves, [T of each persistent launch], GEMMs)."""
    if nb == 1:
        return 1, [], 0
    if dag and 2 <= nb <= dag_tiles:
        return 0, [nb], 0
    a, b = plan_of(nb // 2, dag, dag_tiles), plan_of(nb - nb // 2, dag, dag_tiles)
    return a[0] + b[0], a[1] + b[1], a[2] + b[2] + 4


def split_rows(nb, dag=True, dag_tiles=20, base=0):
    """First rows of the A22 sides of every recursion level (the rows near which a wrong offset
    would show)."""
    if nb == 1 or (dag and nb <= dag_tiles):
        return []
    n1b = nb // 2
    return ([base + TILE * n1b] + split_rows(n1b, dag, dag_tiles, base) +
            split_rows(nb - n1b, dag, dag_tiles, base + TILE * n1b))


# ------------------------------------------------------------------ constants
# Operation counts of the device algorithm, first order in u.
PIVOT = 8          # l_ij·l_jj and l_jj² against the pivot d: r = rsqrt(d) within 3u after the two
                   # Newton steps, the products a·r and d·r one rounding each: 2·(3 + 1)
SUBST16 = 18       # a 16×16 diagonal tile inverted column by column: <= 15 fma terms, the
                   # reciprocal 1/l_kk, the product with it, and the final negation's operand
SPLITK = 8         # a GEMM launch may combine up to 8 partial sums (split-K / stream-K): <= 8
                   # extra additions on top of its K fma terms
C_R_LEAF = 112 + 16 + SUBST16   # right residual of the leaf's X: T_k has <= 112 terms, the product
                                # −X_pp·T_k 16, and X_pp's own residual


def c_r(nb, dag=True, dag_tiles=20):
    """c_R with |L̂X̂ − I| <= c_R·u·(|L̂||X̂|)² for a diagonal block of nb tiles: by block row,
    X_ik = −X_ii·S with S = Σ_j L_ij X_jk — the terms of S, the terms of the product with X_ii,
    and X_ii's own residual constant."""
    if nb == 1:
        return C_R_LEAF
    if dag and nb <= dag_tiles:
        # S_ik: 128 terms per UPDX task, one rounding per task that adds into the tile; FIN: 128
        return TILE * (nb - 1) + (nb - 1) + TILE + C_R_LEAF
    n1b, n2b = nb // 2, nb - nb // 2
    # T = L21·X11 (n1 terms), X21 = −X22·T (n2 terms), each one GEMM launch
    return (TILE * n1b + SPLITK) + (TILE * n2b + SPLITK) + max(c_r(n1b, dag, dag_tiles),
                                                               c_r(n2b, dag, dag_tiles))


def c_r_entries(nb, dag=True, dag_tiles=20):
    """c_R per entry (i >= k) of L̂X̂ − I, tightened by block: the terms actually behind the entry.
    Inside a leaf, 16-tile rows p >= q: the diagonal tile SUBST16, below it 16·(p − q) terms of
    T_q, 16 of the product with X_pp, and SUBST16.  Between the tiles of a persistent block:
    128·(i − j) terms of S_ij and one rounding per UPDX task, 128 of FIN, and the leaf's constant.
    Across a recursion split: the two GEMMs and the constant of the X22 block (c_r).  Down every
    column the constant never decreases (the host test asserts it), so the same matrix bounds
    X̂ − L̂⁻¹ = L̂⁻¹(L̂X̂ − I) — plus one for the longdouble reference's own error there
    (n_pad·2^-64 relative to the same magnitudes)."""
    C = np.zeros((nb * TILE, nb * TILE))
    p = np.arange(TILE) // 16
    dp = p[:, None] - p[None, :]
    leaf = np.where(dp > 0, 16.0 * dp + 16 + SUBST16, np.where(dp == 0, SUBST16, 0.0))

    def rec(b0, m):
        s = lambda i: slice(TILE * (b0 + i), TILE * (b0 + i + 1))
        if m == 1:
            C[s(0), s(0)] = leaf
            return
        if dag and m <= dag_tiles:
            for i in range(m):
                C[s(i), s(i)] = leaf
                for j in range(i):
                    C[s(i), s(j)] = TILE * (i - j) + (i - j) + TILE + C_R_LEAF
            return
        m1 = m // 2
        C[TILE * (b0 + m1):TILE * (b0 + m), TILE * b0:TILE * (b0 + m1)] = \
            (TILE * m1 + SPLITK) + (TILE * (m - m1) + SPLITK) + c_r(m - m1, dag, dag_tiles)
        rec(b0, m1)
        rec(b0 + m1, m - m1)

    rec(0, nb)
    return np.tril(C)


def c_f_tiles(nb, dag=True, dag_tiles=20):
    """Per pair of tiles (ti >= tj): (K, cR) of the product L_ij = A_ij·X_bbᵀ that formed the tile
    — K its inner dimension (plus the split-K allowance), cR the residual constant of the X block
    it multiplied by; zeros on the diagonal tiles, which no such product touches."""
    K = np.zeros((nb, nb))
    R = np.zeros((nb, nb))

    def rec(b0, m):
        if m == 1:
            return
        if dag and m <= dag_tiles:
            for i in range(m):
                for j in range(i):
                    K[b0 + i, b0 + j] = TILE
                    R[b0 + i, b0 + j] = C_R_LEAF
            return
        m1 = m // 2
        K[b0 + m1:b0 + m, b0:b0 + m1] = TILE * m1 + SPLITK
        R[b0 + m1:b0 + m, b0:b0 + m1] = c_r(m1, dag, dag_tiles)
        rec(b0, m1)
        rec(b0 + m1, m - m1)

    rec(0, nb)
    return K, R


def c_s(n_pad):
    """Per column j: the Schur-complement sum behind entry (i, j) has j product terms and the
    original entry (fma chains: one rounding per term), the pivot's PIVOT, and one rounding per
    separate task or launch that adds into the entry (at most one per tile column, each possibly
    a split-K combine)."""
    nb = n_pad // TILE
    return np.arange(n_pad) + 1.0 + PIVOT + (1 + SPLITK) * nb


# ------------------------------------------------------------------ references (longdouble)
def chol_ld(A):
    """Longdouble Cholesky (left-looking by rows).  Returns (pivots, info): the pivots
    d_j = A_jj − Σ_k l_jk² up to and including the first non-positive (or non-finite) one, and
    info = its 1-based index, 0 if there is none."""
    n = A.shape[0]
    A = A.astype(LD)
    L = np.zeros((n, n), LD)
    piv = []
    for j in range(n):
        row = L[j, :j]
        d = A[j, j] - row @ row
        piv.append(d)
        if not (d > 0 and np.isfinite(d)):
            return np.array(piv, LD), j + 1
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ row) / L[j, j]
    return np.array(piv, LD), 0


def residual_rows(A_pad, L, rows):
    """Rows of A − L̂L̂ᵀ in longdouble (A symmetric, L̂ as returned: its upper part is zero)."""
    Ll = L.astype(LD)
    return A_pad[rows].astype(LD) - Ll[rows] @ Ll.T


def inv_rows(L, rows):
    """Rows of L̂⁻¹ in longdouble: xᵀL̂ = e_iᵀ by substitution from column i down."""
    n = L.shape[0]
    Ll = L.astype(LD)
    rows = np.asarray(rows)
    X = np.zeros((len(rows), n), LD)
    top = int(rows.max())
    for j in range(top, -1, -1):
        rhs = (rows == j).astype(LD) - X[:, j + 1:top + 1] @ Ll[j + 1:top + 1, j]
        X[:, j] = np.where(rows >= j, rhs / Ll[j, j], LD(0))
    return X


def right_residual_rows(L, X, rows):
    """Rows of L̂X̂ − I in longdouble."""
    R = L[rows].astype(LD) @ X.astype(LD)
    R[np.arange(len(rows)), rows] -= 1
    return R


def left_residual_rows(L, X, rows):
    """Rows of X̂L̂ − I in longdouble."""
    R = X[rows].astype(LD) @ L.astype(LD)
    R[np.arange(len(rows)), rows] -= 1
    return R


# ------------------------------------------------------------------ bounds
class Bounds:
    """The componentwise bounds of one returned pair (L̂, X̂) on the given rows, each as
    (error, bound) longdouble arrays of shape (rows, n_pad):

      F   |A − L̂L̂ᵀ|  <=  u·[ c_S(j)·P + K·P·M + c_R·P·M² ]     P = |L̂||L̂ᵀ|, M = |X̂ᵀ||L̂ᵀ|
                           (K, c_R per tile pair: zero inside the diagonal 128-tiles)
      X   |X̂ − L̂⁻¹|   <=  (c_R + 1)·u·|L̂⁻¹|·(|L̂||X̂|)²        c_R per entry: c_r_entries
      R   |L̂X̂ − I|    <=  c_R·u·(|L̂||X̂|)²

    Every term is invariant under A -> DAD with D a diagonal of powers of two."""

    def __init__(self, A_pad, L, X, rows=None, dag=True, dag_tiles=20):
        need_extended()
        n_pad = L.shape[0]
        nb = n_pad // TILE
        self.rows = rows = np.arange(n_pad) if rows is None else np.asarray(rows)
        aL, aX = np.abs(L), np.abs(X)
        # float64 products underflow (the far-off-diagonal entries of an RBF Gram are exact zeros
        # and tiny numbers) where the longdouble reference does not: each of the <= n_pad terms
        # behind an entry may lose up to one subnormal spacing
        floor = LD(n_pad) * LD(SUBNORMAL)
        # ---- F
        self.res = np.abs(residual_rows(A_pad, L, rows))
        P = aL[rows] @ aL.T                       # (rows, n_pad)
        PM = (P @ aX.T) @ aL.T
        PMM = (PM @ aX.T) @ aL.T
        Kt, Rt = c_f_tiles(nb, dag, dag_tiles)
        rt = rows // TILE
        Ke = np.repeat(Kt[rt], TILE, axis=1)      # per entry of the sampled rows
        Re = np.repeat(Rt[rt], TILE, axis=1)
        self.res_bound = (U * (c_s(n_pad)[None, :] * P + Ke * PM + Re * PMM)).astype(LD) + floor
        # the residual is symmetric and the bound is derived for i >= j: upper entries are judged
        # by their mirror, so only the lower triangle counts
        low = rows[:, None] >= np.arange(n_pad)[None, :]
        self.res = np.where(low, self.res, 0)
        # ---- X, R
        Q = aL @ aX                               # |L̂||X̂|, lower triangular
        Li = inv_rows(L, rows)
        self.xerr = np.abs(X[rows].astype(LD) - Li)
        CR = c_r_entries(nb, dag, dag_tiles)[rows]
        self.x_bound = (U * (CR + 1.0) *
                        ((np.abs(Li).astype(np.float64) @ Q) @ Q)).astype(LD) + floor
        self.rres = np.abs(right_residual_rows(L, X, rows))
        self.r_bound = (U * CR * (Q[rows] @ Q)).astype(LD) + floor

    @staticmethod
    def _ratio(err, bound):
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(bound > 0, err / bound, np.where(err == 0, 0, np.inf))
        r = np.where(np.isnan(err) | np.isnan(bound), np.inf, r)   # a NaN never passes
        return float(r.max())

    def ratios(self):
        """Largest error / bound per check (<= 1 passes)."""
        return {"F": self._ratio(self.res, self.res_bound),
                "X": self._ratio(self.xerr, self.x_bound),
                "R": self._ratio(self.rres, self.r_bound)}


def check_factor(A_pad, L, X, rows=None, dag=True, dag_tiles=20):
    """The named checks on values: 'F', 'X', 'R'.  Returns (failed names, ratios)."""
    r = Bounds(A_pad, L, X, rows, dag, dag_tiles).ratios()
    return [k for k, v in r.items() if not v <= 1.0], r


def check_structure(L, X, logdiag, n):
    """The named checks on structure; returns the failed names.
      'upper'    strict upper triangles of L̂ and X̂ exactly zero (inside the diagonal tiles too)
      'padding'  padding rows and columns exactly the identity in both
      'padlog'   the padding's log-diagonal exactly 0 (+0 or −0 never arises: log(1) = +0)"""
    bad = []
    n_pad = L.shape[0]
    iu = np.triu_indices(n_pad, 1)
    if np.any(L[iu] != 0) or np.any(X[iu] != 0) or np.any(np.signbit(L[iu])) or \
            np.any(np.signbit(X[iu])):
        bad.append("upper")
    eye = np.eye(n_pad)
    for F in (L, X):
        if not (np.array_equal(F[n:], eye[n:]) and np.array_equal(F[:, n:], eye[:, n:])):
            if "padding" not in bad:
                bad.append("padding")
    if not np.array_equal(logdiag[n:], np.zeros(n_pad - n)) or np.any(np.signbit(logdiag[n:])):
        bad.append("padlog")
    return bad


def log_ulps(logdiag, L, n):
    """Error of each logdiag[i] against the longdouble log of the returned L̂_ii, in float64 ulps
    of the reference (spacing 2^(e−53) at |ref| in [2^(e−1), 2^e); an exact zero reference — the
    padding — must be met exactly)."""
    d = np.diag(L)[:n].astype(LD)
    ref = np.log(d)
    _, e = np.frexp(np.abs(ref))
    ulp = np.ldexp(LD(1), np.maximum(e.astype(np.int64) - 53, -1074).astype(np.int32))
    err = np.abs(logdiag[:n].astype(LD) - ref)
    return np.where(ref == 0, np.where(err == 0, 0, np.inf), err / ulp).astype(np.float64)


def logdet_bound(logdiag, log_ulp_max):
    """|logdet − 2·Σ log L̂_ii| for logdet = 2·fl(Σ logdiag_i) summed in any order:
    2·(n_pad − 1)·u·Σ|logdiag_i| for the summation, plus the per-entry term
    2·Σ log_ulp_max·ulp(logdiag_i) <= 2·log_ulp_max·2u·Σ|logdiag_i|."""
    s = float(np.sum(np.abs(logdiag)))
    return 2.0 * (len(logdiag) - 1) * U * s + 2.0 * log_ulp_max * 2.0 * U * s


def logdet_ref(L):
    """2·Σ log L̂_ii in longdouble."""
    return 2 * np.sum(np.log(np.diag(L).astype(LD)))


# ------------------------------------------------------------------ non-PD inputs
def bad_pivot_matrix(n, ks, seed=0, values=None):
    """A family-(a) matrix with A[k,k] lowered (or set to values[k]) at every k in ks so that, in
    the longdouble Cholesky, every pivot before min(ks) is >= 0.25 and pivot min(ks) is <= −0.25
    (checked here, on the CPU).  Returns (A, expected info = min(ks) + 1)."""
    A = fam_a(n, seed)
    values = values or {}
    for k in ks:
        A[k, k] = values.get(k, A[k, k] - 2.0)   # family (a): pivots within (0.3, 1.6)
    k0 = min(ks)
    piv, info = chol_ld(A)
    assert info == k0 + 1, (info, k0)
    assert np.all(piv[:k0] >= 0.25), float(piv[:k0].min())
    v = values.get(k0)
    if v is None or np.isfinite(v):
        assert piv[k0] <= -0.25, float(piv[k0])
    return A, k0 + 1
