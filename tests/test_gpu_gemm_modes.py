"""The FP64 GEMM launcher (csrc/kernels_gemm.hip launch_gemm), variant by variant, against a
plain numpy product in EXACT arithmetic.

Each case is one internal launch through gps_gemm_diag.  Operands are small integers (A, B, w in
[-4, 4], |C0| <= 1000, kscale / alpha in {1, -1, 2, 0.5}, beta in {0, 1, -2}, K <= 4096), so every
partial sum in every summation order is exactly representable: `Case` computes the bound from
the case's actual ranges and asserts it stays below 2^53.  The comparison is np.array_equal — a
dropped, repeated or misplaced k-slice or tile fails in the element where it happened, while a
correct kernel passes in whatever order it sums.  Every test also asserts, from the plan
launch_gemm hands back, that the variant it names is the one that ran.

What the reference computes (kernel comments of kernels_gemm.hip, checked while writing this):
  EPI_STORE      C = alpha·op(A·diag(kscale))·op(B) + beta·C0
  EPI_ROWSQ      out0[tj][row] = alpha²·Σ_{col in 128-tile tj} acc²
  EPI_ROWSQ_DOT  as ROWSQ, plus out1[row] = (A·diag(kscale))[row, :]·w
  EPI_COLRED     out0[ti][col] = alpha·Σ_{row in tile ti} w[row]·acc, out1[ti][col] = alpha²·Σ acc²

Triangular modes: the operand is zero outside its documented k-range at element level and holds
NaN outside the 128-tile-granular range the Tri enum documents (every kernel clips at least that
tightly), so a finite, equal result shows the clip is applied, not merely harmless.  No
production variant was found to read past that range, so no case substitutes zeros.  Padding
columns of A and B (leading dimensions above the minimum) hold NaN as well; padding columns of C
and of the epilogue slabs hold a sentinel that must come back untouched.  With kend, A's columns
from kend on are zero (the contract) and B there is ordinary data.

Call sites of the triangular modes (layouts A/B as production passes them):
  TRI_K_LE_I  N/T: pred_rows (api.hip, EPI_COLRED, tri_off), joint_cov's V (api_joint.hip);
              N/N: potrf_inv_rec's L⁻¹21 product (api.hip, alpha −1), gps_potrs (api.hip)
  TRI_K_LE_J  N/T: fitc_rowsq_cols (api.hip, EPI_ROWSQ, tri_off, kend), potrf_inv_rec's TRSM
              (api.hip), the FITC row norms / ROWSQ_DOT and fitc_tri_right (api_fitc.hip), the
              joint draws (api_joint.hip), the FITC block-LOO W_f (api_block.hip)
  TRI_K_GE_J  N/N: potrf_inv_rec's T product (api.hip), fitc_tri_right's other side (api_fitc.hip)
  TRI_K_GE_I  T/N: L⁻ᵀL⁻¹ with lower_out (api_full.hip, api_block.hip [mirror], api_fitc.hip),
              fitc_tri_left_t (api_fitc.hip)
  TRI_KR_J    N/N: the block-LOO gradient's block-diagonal product (api_block.hip)

Not reachable, hence not covered: the small kernel's `!valid` path with more than one wave per
block needs a block count that is no multiple of the blocks per workgroup (2 or 1), and with M
and N multiples of 128 every count is a multiple of 4.
"""
import time
from types import SimpleNamespace

import numpy as np
import pytest

from gpscore import _lib

pytestmark = pytest.mark.gpu

STORE, ROWSQ, COLRED, ROWSQ_DOT = 0, 1, 2, 3
NONE, K_LE_I, K_LE_J, K_GE_J, K_GE_I, KR_J = 0, 1, 2, 3, 4, 5
OPT_STREAM_K, OPT_SLAB_XCD = 18, 26
SENT = 77777.0  # padding sentinel (finite, not a value any case produces in a padding column)
U = 2.0 ** -53


def gamma(n):
    return n * U / (1.0 - n * U)


def kr_of_blocks(sizes16, N):
    """TRI_KR_J ranges of a block-diagonal B with blocks of 16·sizes16 columns (repeated to N)."""
    kr = np.zeros(2 * (N // 16), np.int32)
    g = 0
    while g < N // 16:
        for s in sizes16:
            for q in range(g, min(g + s, N // 16)):
                kr[2 * q], kr[2 * q + 1] = 16 * g, 16 * min(g + s, N // 16)
            g += s
            if g >= N // 16:
                break
    return kr


def tri_masks(tri, off, M, N, K, kr):
    """(operand, zero mask, NaN mask): where the triangular operand (as op(A) M×K or op(B) K×N)
    is structurally zero, and where it lies outside the 128-tile-granular k-range."""
    if tri in (K_LE_I, K_GE_I):
        i, k = np.arange(M)[:, None], np.arange(K)[None, :]
        if tri == K_LE_I:
            return "A", k > off + i, k >= off + (i // 128 + 1) * 128
        return "A", k < off + i, k < off + (i // 128) * 128
    k, j = np.arange(K)[:, None], np.arange(N)[None, :]
    if tri == K_LE_J:
        return "B", k > off + j, k >= off + (j // 128 + 1) * 128
    if tri == K_GE_J:
        return "B", k < off + j, k < off + (j // 128) * 128
    g = np.arange(N) // 16
    g0, g1 = (np.arange(N) // 128) * 8, (np.arange(N) // 128) * 8 + 7
    lo, hi = kr[2 * g][None, :], kr[2 * g + 1][None, :]
    tlo, thi = kr[2 * g0][None, :], kr[2 * g1 + 1][None, :]
    return "B", (k < lo) | (k >= hi), (k < tlo) | (k >= thi)


def Case(ctx, M, N, K, la=0, lb=1, epi=STORE, alpha=1.0, beta=0.0, tri=NONE, tri_off=0,
         blocks=None, lower_out=0, mirror=0, kscale=False, kend=0, tile=0, ksplit=1, map_mode=0,
         use_ws=1, sk_alone=0, pad=2, seed=0, real=False, nan_c=False, syrk=False, run=True):
    """Build one launch (operands, stored arrays with NaN outside what may be read, expected
    results), run it, return everything.  Integer cases assert their own exactness bound."""
    rng = np.random.default_rng([seed, M, N, K, la, lb, tri, tile])
    draw = (lambda *s: rng.standard_normal(s)) if real else \
        (lambda *s: rng.integers(-4, 5, s).astype(np.float64))
    opA = draw(M, K)
    opB = draw(K, N)
    kr = kr_of_blocks(blocks, N) if tri == KR_J else None
    nanA, nanB = np.zeros((M, K), bool), np.zeros((K, N), bool)
    if tri:
        which, zero, nan = tri_masks(tri, tri_off, M, N, K, kr)
        if which == "A":
            opA[zero], nanA = 0.0, nan
        else:
            opB[zero], nanB = 0.0, nan
        assert not (nan & ~zero).any()
    if kend:
        opA[:, kend:] = 0.0
    if syrk:  # a symmetric product (L⁻ᵀL⁻¹, KᵀΛ⁻¹K): B is A's transpose, structural zeros included
        opB = opA.T.copy()
    ks = rng.choice([1.0, -1.0, 2.0, 0.5], K) if kscale else None
    opAs = opA * ks[None, :] if kscale else opA

    def store(op, nan, transposed, ld_pad):
        m = np.where(nan, np.nan, op)
        m = m.T if transposed else m
        out = np.full((m.shape[0], m.shape[1] + ld_pad), np.nan)
        out[:, :m.shape[1]] = m
        return np.ascontiguousarray(out)

    A = store(opA, nanA, la == 1, pad)          # LAY_T: stored [k][i]
    B = store(opB, nanB, lb == 1, 2 * pad)      # LAY_T: stored [j][k]
    acc = opAs @ opB
    # Σ_k |a_ik|·|b_kj|: elementwise for the real-valued bounds, its range's maximum otherwise
    absacc = np.abs(opAs) @ np.abs(opB) if real else None
    accmax = float(absacc.max()) if real else K * 4.0 * 4.0 * (2.0 if kscale else 1.0)
    d = _lib.GemmDesc(lay_a=la, lay_b=lb, epi=epi, M=M, N=N, K=K, lda=A.shape[1], ldb=B.shape[1],
                      ldc=0, alpha=alpha, beta=beta, tri=tri, tri_off=tri_off, lower_out=lower_out,
                      mirror=mirror, kend=kend, tile=tile, ksplit=ksplit, map_mode=map_mode,
                      use_ws=use_ws, sk_alone=sk_alone, dep_mode=0, ld_out=0, c_kslice_stride=0)
    r = SimpleNamespace(desc=d, A=A, B=B, kr=kr, kscale=ks, acc=acc, absacc=absacc, opA=opA,
                        opAs=opAs, opB=opB, C=None, w=None, out0=None, out1=None, M=M, N=N, K=K)
    g_acc = 0.5 if kscale else 1.0
    g_alpha = 0.5 if alpha == 0.5 else 1.0
    if epi == STORE:
        ldc = N + 3 * pad
        C0 = draw(M, N) if real else rng.integers(-1000, 1001, (M, N)).astype(np.float64)
        if syrk:
            C0 = np.tril(C0) + np.tril(C0, -1).T
        unslab = ksplit > 1 and not use_ws and tile not in (16, 32)
        nsl = ksplit if unslab else 1
        stride = M * ldc + 6
        buf = np.full(nsl * stride if unslab else M * ldc, SENT)
        Cv = [buf[s * stride: s * stride + M * ldc].reshape(M, ldc) for s in range(nsl)]
        for c in Cv:
            c[:, :N] = np.nan if (nan_c or unslab) else C0
        d.ldc, d.c_kslice_stride = ldc, stride if unslab else 0
        r.C, r.Cv, r.C0 = buf, Cv, C0
        r.exp = alpha * acc + (beta * C0 if beta != 0.0 else 0.0)
        if real:
            r.bound = gamma(K + 2) * (abs(alpha) * absacc + abs(beta) * np.abs(C0))
        mag, gran = abs(alpha) * accmax + abs(beta) * 1000.0, g_acc * g_alpha
    else:
        rows = N // 128 if epi != COLRED else M // 128
        width = M if epi != COLRED else N
        d.ld_out = width + 5
        r.out0 = np.full((rows, d.ld_out), SENT)
        e = gamma(K + 2) * absacc if real else np.zeros_like(acc)  # elementwise bound on acc
        if epi == COLRED:
            r.w = draw(M)
            r.out1 = np.full((rows, d.ld_out), SENT)
            a3, w3 = acc.reshape(rows, 128, N), r.w.reshape(rows, 128, 1)
            e3, c3 = e.reshape(rows, 128, N), np.abs(a3)
            r.exp0 = alpha * (w3 * a3).sum(1)
            r.exp1 = alpha * alpha * (a3 * a3).sum(1)
            r.bound0 = abs(alpha) * ((np.abs(w3) * e3).sum(1) + gamma(130) * (np.abs(w3) * (c3 + e3)).sum(1))
            r.bound1 = alpha * alpha * ((2 * c3 * e3 + e3 * e3).sum(1) + gamma(130) * ((c3 + e3) ** 2).sum(1))
            mag = max(abs(alpha) * 128 * 4 * accmax, alpha * alpha * 128 * accmax ** 2)
        else:
            a3 = acc.reshape(M, rows, 128)
            e3, c3 = e.reshape(M, rows, 128), np.abs(a3)
            r.exp0 = (alpha * alpha * (a3 * a3).sum(2)).T
            r.bound0 = (alpha * alpha * ((2 * c3 * e3 + e3 * e3).sum(2) + gamma(130) * ((c3 + e3) ** 2).sum(2))).T
            mag = alpha * alpha * 128 * accmax ** 2
            if epi == ROWSQ_DOT:
                r.w = draw(K)
                r.out1 = np.full(M, SENT)
                r.exp1 = opAs @ r.w
                mag = max(mag, K * 8.0 * 4.0)
        gran = (g_acc * g_alpha) ** 2
    if not real:
        assert K <= 4096 and mag / gran < 2.0 ** 53, (mag, gran)  # every partial sum is exact
    if run:
        r.plan = ctx.gemm_diag(d, A, B, r.C, ks, r.w, kr, r.out0, r.out1)
    return r


def check_store(r, what, lower_out=0, mirror=0):
    """EPI_STORE result: exact where written, C0 (or the padding sentinel) bitwise elsewhere."""
    C = r.Cv[0]
    N = r.N
    assert np.array_equal(C[:, N:], np.full_like(C[:, N:], SENT)), (what, "padding columns of C written")
    got = C[:, :N]
    if not lower_out or mirror:
        bad = np.argwhere(got != r.exp)
        assert bad.size == 0, (what, r.plan, "first wrong element", bad[:1], got[tuple(bad[0])],
                               r.exp[tuple(bad[0])]) if bad.size else what
        if mirror:
            assert np.array_equal(got, got.T), (what, "mirror is not bitwise symmetric")
        return
    i, j = np.arange(r.M)[:, None], np.arange(N)[None, :]
    low, up_tile = j <= i, j // 128 > i // 128
    assert np.array_equal(got[low], r.exp[low]), (what, r.plan, "lower part")
    assert np.array_equal(got[up_tile], r.C0[up_tile]), (what, r.plan, "strictly-upper 128-tiles written")
    rest = ~low & ~up_tile  # above the diagonal inside a diagonal 128-tile: untouched or exact
    assert np.all((got[rest] == r.C0[rest]) | (got[rest] == r.exp[rest])), (what, r.plan, "diagonal tiles")


def set_opt(ctx, key, value):
    ctx.call("gps_ctx_set_option", key, value)


AB = [(1.0, 1.0), (-1.0, 1.0), (2.0, -2.0), (0.5, 0.0)]
LAYOUTS = [(0, 1), (0, 0), (1, 0), (1, 1)]


# ------------------------------------------------------------------ the LDS kernel, dense
@pytest.mark.parametrize("la,lb", LAYOUTS)
@pytest.mark.parametrize("tile", [128, 64])
def test_lds_kernel_dense(gpu_ctx, tile, la, lb):
    """128- and 64-tile EPI_STORE kernel, forced: four layouts, tile grids with tiles_m != tiles_n,
    K = 16 (one slice, no loop), 32 / 48 (even / odd slice count: double-buffer parity), 272;
    leading dimensions above the minimum; beta = 0 over a NaN-filled C must not propagate."""
    n = 0
    for (M, N) in ((128, 128), (256, 384), (384, 128)):
        for K in (16, 32, 48, 272):
            alpha, beta = AB[n % 4]
            n += 1
            r = Case(gpu_ctx, M, N, K, la, lb, alpha=alpha, beta=beta, tile=tile, nan_c=beta == 0.0,
                     pad=2 + 2 * (n % 3))
            p = r.plan
            assert (p["tile"], p["ksplit"], p["sk_wgs"], p["grid_y"]) == (tile, 1, 0, 1), p
            assert p["grid_x"] == (M // tile) * (N // tile), p
            check_store(r, (tile, la, lb, M, N, K, alpha, beta))


# ------------------------------------------------------------------ split-K
@pytest.mark.parametrize("ks", [2, 3, 4])
@pytest.mark.parametrize("tile", [64, 128])
def test_splitk_slabbed(gpu_ctx, tile, ks):
    """Slabbed split-K at K = 48 (3 slices of 16: ks 2 has a remainder slice, ks 4 an empty one
    that must contribute zeros): splitk_reduce_kernel with and without lower_out,
    splitk_reduce_sym_kernel (mirror), kscale with mixed signs on both A layouts (the joint
    covariance's launch is T/N, lower_out, kscale ±1), slab_xcd on and off."""
    try:
        for xcd in (1, 0):
            set_opt(gpu_ctx, OPT_SLAB_XCD, xcd)
            n = 0
            for (la, lb) in LAYOUTS:
                for (lower, mirror) in ((0, 0), (1, 0), (1, 1)):
                    for K in (48, 272):
                        alpha, beta = AB[n % 4]
                        n += 1
                        M, N = (256, 256) if lower else (256, 384)
                        r = Case(gpu_ctx, M, N, K, la, lb, alpha=alpha, beta=beta, tile=tile,
                                 ksplit=ks, lower_out=lower, mirror=mirror, syrk=bool(mirror),
                                 kscale=(n % 2 == 0), seed=n)
                        p = r.plan
                        tiles = (M // tile) * (M // tile + 1) // 2 if lower else (M // tile) * (N // tile)
                        assert (p["tile"], p["ksplit"], p["grid_x"], p["grid_y"], p["slab_xcd"],
                                p["sk_wgs"]) == (tile, ks, tiles, ks, xcd, 0), p
                        check_store(r, (tile, ks, xcd, la, lb, lower, mirror, K), lower, mirror)
    finally:
        set_opt(gpu_ctx, OPT_SLAB_XCD, 1)


@pytest.mark.parametrize("ks", [2, 3, 4])
def test_splitk_unslabbed(gpu_ctx, ks):
    """The unslabbed split (the FITC SYRK and the joint covariance: T/N, kscale, lower_out, the
    automatic 128-tile): slice s writes C + s·stride.  Every slice block is fully written (the
    NaN prefill is gone from every tile the launch owns, the sentinel between blocks intact) and
    the slices sum to the product."""
    n = 0
    for (la, lb) in ((1, 0), (0, 1)):
        for lower in (0, 1):
            for K in (48, 272):
                for tile in (0, 128):
                    n += 1
                    M, N = (384, 384) if lower else (256, 384)
                    alpha = (1.0, -1.0, 2.0, 0.5)[n % 4]
                    r = Case(gpu_ctx, M, N, K, la, lb, alpha=alpha, tile=tile, ksplit=ks, use_ws=0,
                             lower_out=lower, kscale=(n % 2 == 1), seed=n)
                    p = r.plan
                    assert (p["tile"], p["ksplit"], p["grid_y"]) == (128, ks, ks), p
                    what = (ks, la, lb, lower, K, tile)
                    i, j = np.arange(M)[:, None], np.arange(N)[None, :]
                    own = (j // 128 <= i // 128) if lower else np.ones((M, N), bool)
                    own = np.broadcast_to(own, (M, N))
                    total = np.zeros((M, N))
                    for s, c in enumerate(r.Cv):
                        assert np.array_equal(c[:, N:], np.full_like(c[:, N:], SENT)), (what, s)
                        assert np.isfinite(c[:, :N][own]).all(), (what, "slice not fully written", s)
                        assert np.isnan(c[:, :N][~own]).all(), (what, "upper tiles written", s)
                        total += np.where(own, c[:, :N], 0.0)
                    gaps = r.C.reshape(ks, -1)[:, -6:]  # between the slice blocks
                    assert np.array_equal(gaps, np.full((ks, 6), SENT)), what
                    assert np.array_equal(total[own], (alpha * r.acc)[own]), (what, p)


# ------------------------------------------------------------------ triangular modes
TRI_SITES = [(K_LE_I, 0, 1), (K_LE_I, 0, 0), (K_LE_J, 0, 1), (K_GE_J, 0, 0), (K_GE_I, 1, 0)]
GRIDS = [(1, 1), (1, 9), (9, 1), (7, 3), (8, 8), (9, 17)]
MAP_RESULT = {0: 3, 1: 1, 2: 2, 3: 3, 4: 0, 5: 5}  # launch_gemm: 0 -> 3 for a triangular operand, 4 -> 0
OFFK = [(0, 0), (128, 0), (384, 0), (0, 128), (128, 256), (384, 128)]  # (tri_off, K beyond the extent)


@pytest.mark.parametrize("tri,la,lb", TRI_SITES)
@pytest.mark.parametrize("tile", [128, 64])
def test_tri_modes_lds(gpu_ctx, tile, tri, la, lb):
    """Each k-range mode in the layouts production passes (module docstring), tile grids (in
    128-tiles) 1×1 .. 9×17 so the banded maps 3 and 5 run with holes at the band edges (grids
    that are no multiple of 8), map_mode forced to every value launch_gemm accepts for the shape,
    tri_off in {0, 128, 384} with K equal to and larger than tri_off + extent."""
    for gi, (tm, tn) in enumerate(GRIDS):
        M, N = 128 * tm, 128 * tn
        for mi, mm in enumerate(MAP_RESULT):
            off, extra = OFFK[(gi + mi) % 6]
            K = off + (M if tri in (K_LE_I, K_GE_I) else N) + extra
            alpha, beta = AB[(gi + mi) % 4]
            r = Case(gpu_ctx, M, N, K, la, lb, alpha=alpha, beta=beta, tri=tri, tri_off=off,
                     tile=tile, map_mode=mm, nan_c=beta == 0.0, seed=mi)
            p = r.plan
            assert (p["tile"], p["ksplit"], p["map_mode"]) == (tile, 1, MAP_RESULT[mm]), (mm, p)
            assert p["grid_x"] >= (M // tile) * (N // tile), p
            check_store(r, (tile, tri, la, lb, tm, tn, mm, off, K))


@pytest.mark.parametrize("tri,la,lb", [(K_GE_I, 1, 0)])
@pytest.mark.parametrize("tile", [128, 64, 32, 16])
def test_tri_lower_out(gpu_ctx, tile, tri, la, lb):
    """L⁻ᵀL⁻¹ as production forms it: TRI_K_GE_I with lower_out (and mirror), every kernel."""
    for M in (128, 384, 1152 if tile >= 64 else 256):
        for mirror in (0, 1):
            r = Case(gpu_ctx, M, M, M, la, lb, alpha=-1.0, beta=1.0, tri=tri, lower_out=1,
                     mirror=mirror, syrk=True, tile=tile, ksplit=4 if tile < 64 else 1, seed=M)
            assert r.plan["tile"] == tile, r.plan
            check_store(r, (tile, M, mirror), 1, mirror)


@pytest.mark.parametrize("tile,ks", [(128, 1), (64, 1), (64, 2), (32, 1), (32, 4), (16, 2), (0, 1)])
def test_tri_kr_j(gpu_ctx, tile, ks):
    """TRI_KR_J with unaligned block boundaries (blocks of 16·{1, 3, 9, 3} columns: 128- and
    64-tiles hold parts of several blocks), in the LDS and the small kernel and as planned."""
    for (M, N) in ((128, 256), (256, 512)):
        r = Case(gpu_ctx, M, N, N, 0, 0, alpha=2.0, beta=1.0, tri=KR_J, blocks=(1, 3, 9, 3),
                 tile=tile, ksplit=ks)
        want = (16, 4) if (tile == 0 and M * N <= 256 * 256) else (32, 4) if tile == 0 else (tile, ks)
        assert (r.plan["tile"], r.plan["ksplit"]) == want, r.plan
        check_store(r, (tile, ks, M, N))


# ------------------------------------------------------------------ the small kernel
@pytest.mark.parametrize("la,lb", LAYOUTS)
@pytest.mark.parametrize("waves", [1, 2, 4])
@pytest.mark.parametrize("tile", [16, 32])
def test_small_kernel(gpu_ctx, tile, waves, la, lb):
    """16- and 32-blocks × 1 / 2 / 4 waves × four layouts: K = 16 (one chunk: waves beyond the
    first get nothing), 80 (uneven parts per wave), 272 (more than two load groups per wave: both
    fragment buffers cycle); lower_out at 128 / 256 / 384 with and without mirror; every tri mode."""
    n = 0
    for (M, N) in ((128, 128), (128, 384)):
        for K in (16, 80, 272):
            alpha, beta = AB[n % 4]
            n += 1
            r = Case(gpu_ctx, M, N, K, la, lb, alpha=alpha, beta=beta, tile=tile, ksplit=waves,
                     nan_c=beta == 0.0)
            blocks = (M // tile) * (N // tile)
            assert (r.plan["tile"], r.plan["ksplit"], r.plan["grid_x"]) == \
                (tile, waves, (blocks * waves + 3) // 4), r.plan
            check_store(r, (tile, waves, la, lb, M, N, K))
    for M in (128, 256, 384):
        for mirror in (0, 1):
            r = Case(gpu_ctx, M, M, 80, la, lb, alpha=-1.0, beta=1.0, tile=tile, ksplit=waves,
                     lower_out=1, mirror=mirror, syrk=bool(mirror))
            u, a = 64 // tile, M // 64
            assert r.plan["grid_x"] == (u * u * a * (a + 1) // 2 * waves + 3) // 4, r.plan
            check_store(r, (tile, waves, la, lb, M, mirror), 1, mirror)
    for tri in (K_LE_I, K_LE_J, K_GE_J, K_GE_I):
        off = 128 if tri in (K_LE_I, K_LE_J) else 0
        r = Case(gpu_ctx, 256, 384, 640, la, lb, alpha=0.5, beta=-2.0, tri=tri, tri_off=off,
                 tile=tile, ksplit=waves)
        assert (r.plan["tile"], r.plan["ksplit"]) == (tile, waves), r.plan
        check_store(r, (tile, waves, la, lb, "tri", tri))


# ------------------------------------------------------------------ epilogues
def check_slab(out, exp, width, what):
    assert np.array_equal(out[:, width:], np.full_like(out[:, width:], SENT)), (what, "slab padding written")
    bad = np.argwhere(out[:, :width] != exp)
    assert bad.size == 0, (what, "first wrong (slab row, index)", bad[:1])


@pytest.mark.parametrize("epi", [ROWSQ, ROWSQ_DOT])
@pytest.mark.parametrize("mm,want", [(0, 6), (6, 6), (5, 5)])
def test_epilogue_rowsq(gpu_ctx, epi, mm, want):
    """The FITC row norms (fitc_rowsq_cols / the ROWSQ_DOT launch): TRI_K_LE_J, tri_off 0 / 256,
    kend < K, grids 3×1, 3×4, 3×5 (map 6 pairs column tiles T−1−q and q and runs the middle tile
    alone when the count is odd), maps 6 (the automatic choice) and 5.  Slab row tj holds column
    tile tj's row sums and no other; ROWSQ_DOT's last column tile also gives the row dot."""
    for tn in (1, 4, 5):
        for off in (0, 256):
            for kend in (0, off + 128 * tn - 48):
                M, N = 384, 128 * tn
                r = Case(gpu_ctx, M, N, off + N, 0, 1, epi=epi, alpha=(0.5 if kend else -1.0),
                         tri=K_LE_J, tri_off=off, kend=kend, map_mode=mm, kscale=(epi == ROWSQ_DOT),
                         seed=tn)
                p = r.plan
                assert (p["tile"], p["map_mode"]) == (128, want), p
                if want == 6:
                    assert p["grid_x"] == 3 * ((tn + 1) // 2), p
                what = (epi, mm, tn, off, kend)
                check_slab(r.out0, r.exp0, M, what)
                if epi == ROWSQ_DOT:
                    assert np.array_equal(r.out1, r.exp1), (what, "row dot")


@pytest.mark.parametrize("mm,want", [(0, 3), (5, 5), (1, 1)])
def test_epilogue_colred(gpu_ctx, mm, want):
    """pred_rows' launch: EPI_COLRED with TRI_K_LE_I, tri_off 0 / 256.  Slab row ti holds row
    tile ti's column partials and no other."""
    for (tm, tn) in ((3, 2), (4, 3), (1, 1)):
        for off in (0, 256):
            M, N = 128 * tm, 128 * tn
            r = Case(gpu_ctx, M, N, off + M, 0, 1, epi=COLRED, alpha=(-1.0 if off else 2.0),
                     tri=K_LE_I, tri_off=off, map_mode=mm, seed=tm)
            assert (r.plan["tile"], r.plan["map_mode"]) == (128, want), r.plan
            check_slab(r.out0, r.exp0, N, ("colred s1", mm, tm, tn, off))
            check_slab(r.out1, r.exp1, N, ("colred s2", mm, tm, tn, off))


# ------------------------------------------------------------------ the stream-K tail
@pytest.mark.parametrize("M,K,la,lb,lower", [(2944, 32, 0, 1, 0), (2944, 64, 0, 0, 0),
                                             (2944, 48, 1, 0, 0), (4096, 32, 0, 1, 1),
                                             (2944, 496, 0, 1, 0)])  # 527 slices on all 512 slots
def test_stream_k_tail_exact(gpu_ctx, M, K, la, lb, lower):
    """529 tiles on 512 slots (remainder 17; K = 32 / 64 / 48: 2, 4 and 3 slices per tile) and
    the trailing update's lower_out shape (528 lower tiles, remainder 16), sk_alone, alpha −1,
    beta 1.  The tail engaged (plan), the same launch again gives the same bits (the tickets were
    left zero), and GPS_OPT_STREAM_K = 0 gives the same exact result.

    These shapes have fewer tail slices than workgroup slots (34 .. 68 on 512).  Before this test
    launch_gemm still cut them into 512 runs, most of them empty; the combine counts on every
    block between a tile's first and last owner having run part of it, so no tile of the tail
    was ever completed (C kept C0 there) and the tickets stayed raised.  launch_gemm now starts
    at most one workgroup per slice (sk_wgs = min(slots, remainder·K/16))."""
    t0 = time.perf_counter()
    r = Case(gpu_ctx, M, M, K, la, lb, alpha=-1.0, beta=1.0, tile=128, sk_alone=1, lower_out=lower)
    dt = time.perf_counter() - t0
    p = r.plan
    tiles = 23 * 23 if not lower else 32 * 33 // 2
    wgs = min(512, (tiles % 512) * (K // 16))
    assert p["sk_wgs"] == wgs > 0 and p["sk_dp"] == tiles - tiles % 512, p
    assert p["grid_x"] == p["sk_dp"] + wgs, p
    check_store(r, ("stream-K", M, K), lower, 0)
    first = r.C.copy()
    r2 = Case(gpu_ctx, M, M, K, la, lb, alpha=-1.0, beta=1.0, tile=128, sk_alone=1, lower_out=lower)
    assert r2.plan == p and np.array_equal(r2.C, first), "second launch differs: tickets not reset?"
    try:
        set_opt(gpu_ctx, OPT_STREAM_K, 0)
        r3 = Case(gpu_ctx, M, M, K, la, lb, alpha=-1.0, beta=1.0, tile=128, sk_alone=1, lower_out=lower)
    finally:
        set_opt(gpu_ctx, OPT_STREAM_K, 2)
    assert r3.plan["sk_wgs"] == 0 and r3.plan["grid_x"] == tiles, r3.plan
    check_store(r3, ("no stream-K", M, K), lower, 0)
    assert np.array_equal(r3.Cv[0][:, :M][np.tril_indices(M)], r.Cv[0][:, :M][np.tril_indices(M)])
    print(f"stream-K case M={M} K={K}: first launch incl. operand build {dt:.2f} s")


# ------------------------------------------------------------------ the automatic plan
# (tile, ksplit) from the thresholds in gemm_plan's comment: 16-blocks up to M·N = 256² (K <= 1024),
# 32-blocks up to M·N = 1280² for triangular products (K <= 1280) and for K <= 640 otherwise, waves
# 4 from K = 64; 128-tiles from 512 of them; else 64-tiles, K split (by doubling, >= 64 of K per
# slice) until about 1024 workgroups
AUTO = [
    (256, 256, 64, NONE, (16, 4)),
    (256, 256, 16, NONE, (16, 1)),
    (256, 256, 32, NONE, (16, 2)),
    (256, 384, 64, NONE, (32, 4)),        # just above 256²
    (256, 256, 1024, NONE, (16, 4)),
    (256, 256, 1040, NONE, (64, 8)),      # 16 64-tiles: split 8 ways (130 of K per slice)
    (256, 384, 1040, K_LE_J, (32, 4)),
    (256, 384, 640, NONE, (32, 4)),
    (256, 384, 656, NONE, (64, 8)),       # 24 64-tiles, 82 of K per slice
    (256, 768, 656, K_LE_J, (32, 4)),
    (2048, 4096, 32, NONE, (128, 1)),     # 512 128-tiles
    (2816, 2944, 32, NONE, (64, 1)),      # 506 128-tiles -> 2024 64-tiles, no split
]


@pytest.mark.parametrize("M,N,K,tri,want", AUTO)
def test_automatic_plan(gpu_ctx, M, N, K, tri, want):
    r = Case(gpu_ctx, M, N, K, 0, 1, alpha=-1.0, beta=1.0, tri=tri, tile=0)
    assert (r.plan["tile"], r.plan["ksplit"]) == want, r.plan
    check_store(r, ("auto", M, N, K, tri))


# ------------------------------------------------------------------ real-valued, per kernel family
def longdouble_ref(r, rows=slice(None)):
    assert np.finfo(np.longdouble).eps < 1e-18
    A, B = r.opAs[rows].astype(np.longdouble), r.opB.astype(np.longdouble)
    return A @ B


@pytest.mark.parametrize("family,kw", [
    ("lds128", dict(M=128, N=256, K=272, tile=128)),
    ("lds64", dict(M=128, N=256, K=272, tile=64)),
    ("small16", dict(M=128, N=128, K=272, tile=16, ksplit=4)),
    ("small32", dict(M=128, N=128, K=272, tile=32, ksplit=2)),
    ("splitk", dict(M=256, N=256, K=272, tile=64, ksplit=3, kscale=True)),
    ("splitk_sym", dict(M=256, N=256, K=272, tile=128, ksplit=3, lower_out=1, mirror=1, syrk=True)),
    ("streamk", dict(M=2944, N=2944, K=48, tile=128, sk_alone=1)),
    ("streamk_full", dict(M=2944, N=2944, K=512, tile=128, sk_alone=1)),  # 544 slices: all 512 slots
])
def test_real_valued_componentwise(gpu_ctx, family, kw):
    """Reduced-precision accumulation, which integers cannot see: standard-normal operands against
    an np.longdouble product, componentwise |Ĉ − C| <= γ_{K+2}·(|alpha|·|A|·|B| + |beta|·|C0|) with
    γ_n = n·u/(1 − n·u), u = 2^-53 — valid for any summation order of FMA / MFMA accumulation (K
    products and at most K − 1 additions per element, one rounding for alpha, one for beta·C0's
    fused add), so it needs no measured margin."""
    lower, mirror = kw.get("lower_out", 0), kw.get("mirror", 0)
    r = Case(gpu_ctx, la=0, lb=1, alpha=-0.7, beta=1.3, real=True, **kw)
    if family.startswith("streamk"):
        assert r.plan["sk_wgs"] == min(512, 17 * kw["K"] // 16), r.plan
    assert r.plan["tile"] == kw["tile"], r.plan
    # stream-K: the rows of the tail's tiles only (tile rows 16.. / the last tile row)
    rows = {"streamk": slice(1920, None), "streamk_full": slice(2816, None)}.get(family, slice(None))  # the tail's tiles and some before
    ref = (np.longdouble(-0.7) * longdouble_ref(r, rows) +
           np.longdouble(1.3) * r.C0[rows].astype(np.longdouble))
    got = r.Cv[0][rows, :r.N].astype(np.longdouble)
    err = np.abs(got - ref).astype(np.float64)
    ok = err <= r.bound[rows]
    if lower and not mirror:
        ok |= np.arange(r.N)[None, :] > np.arange(r.M)[:, None]
    worst = float(np.max(err / r.bound[rows]))
    print(f"{family}: max |err| / bound = {worst:.3f}")
    assert ok.all(), (family, worst)


@pytest.mark.parametrize("epi", [ROWSQ, COLRED])
def test_real_valued_epilogues(gpu_ctx, epi):
    """The reducing epilogues in real arithmetic.  With c_j the exact accumulators of a row (or
    column) of a 128-tile and e_j = γ_{K+2}·(|A|·|B|)_j their elementwise bound, the computed ĉ_j
    satisfy |ĉ_j² − c_j²| <= 2·|c_j|·e_j + e_j²; summing 128 squares and scaling by alpha² takes
    at most 130 roundings of non-negative terms each at most (|c_j| + e_j)², so
      |out − alpha²·Σ c_j²| <= alpha²·[Σ_j (2·|c_j|·e_j + e_j²) + γ_130·Σ_j (|c_j| + e_j)²].
    COLRED's weighted sum likewise: |alpha|·[Σ_i |w_i|·e_i + γ_130·Σ_i |w_i|·(|c_i| + e_i)]."""
    if epi == ROWSQ:
        r = Case(gpu_ctx, 256, 384, 384, 0, 1, epi=ROWSQ, alpha=-0.7, tri=K_LE_J, real=True)
        acc = longdouble_ref(r).reshape(256, 3, 128)
        refs = [((np.longdouble(-0.7) ** 2 * (acc * acc).sum(2)).T, r.out0[:, :256], r.bound0)]
    else:
        r = Case(gpu_ctx, 384, 256, 384, 0, 1, epi=COLRED, alpha=-0.7, tri=K_LE_I, real=True)
        acc = longdouble_ref(r).reshape(3, 128, 256)
        w = r.w.astype(np.longdouble).reshape(3, 128, 1)
        refs = [(np.longdouble(-0.7) * (w * acc).sum(1), r.out0[:, :256], r.bound0),
                (np.longdouble(-0.7) ** 2 * (acc * acc).sum(1), r.out1[:, :256], r.bound1)]
    for ref, got, bound in refs:
        err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
        print(f"epilogue {epi}: max |err| / bound = {float(np.max(err / bound)):.3f}")
        assert (err <= bound).all(), (epi, float(np.max(err / bound)))
