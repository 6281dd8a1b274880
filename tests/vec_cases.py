"""Cases, extended-precision references, error bounds and float64 restatements of the vector
layer's kernels (csrc/kernels_vec.hip), one production launch at a time through gps_vec_diag
(which 0..13, include/gpscore.h), shared by test_vec_host.py (CPU: a numpy float64 restatement of
each kernel meets every bound with room, every listed defect fails a named check) and
test_gpu_vec.py (the kernels).  Nothing here touches the GPU or imports mpmath; DESIGN §30 has
the derivations in full.

u = 2^-53.  References are numpy longdouble from the float64 values the kernel receives; erf and
exp of the score terms come from tests/golden/vec_terms.npz (mpmath, 60 digits, hi/lo pairs,
written by tests/golden/make_vec_terms.py from build_pool() below).

The two bound shapes:
  * a sum of k terms (products included), in any order, with or without fma:
        |err| <= (k + c)·u·Σ|a_i||b_i|,   c the count of further roundings per term (sum_tol);
    the two-level row sums are trees of known depth D, for which (D + 1)·u·Σ|t_i| holds
    (tree_depth) on top of the terms' own bounds;
  * a row formula: an operation count times u against the output's natural scale (each case's
    docstring states its own).
Copies, zeros, the pad identity, the pad rows of Λ and the in-order slab sums are compared bit
for bit ("exact ..." checks).

A Case holds the arguments of one call; check(case, outs) returns {check name: ratio}, the error
as a multiple of the bound (0 or inf for the exact and the all-finite checks; <= 1 passes).
with_ld() and poison_upper() restate what gps_vec_diag puts on the device around the inputs —
NaN in the strict-upper 128-tiles of the lower forms, in the row gaps, in one slab past the real
ones — so that a restatement which reads what the kernel must not read turns non-finite just as
the kernel would.
"""
import math
import os

import numpy as np

from elementwise_cases import GOLDEN, LD, U, need_extended
from grad_cases import INV_SQRT_2PI, INV_SQRT_PI, K_ISP, K_PDF, K_SQRT_HALF, _erf, ld, wave_sum, worst_ratio

TILE, CR_ROWS, CR_COLS = 128, 256, 512
FIXTURE = os.path.join(GOLDEN, "vec_terms.npz")
LOG_2PI = 1.83787706640934548356          # the constant full_loo_obj_kernel carries
HALF_LOG_2PI = 0.91893853320467274178     # logs_term's
uL = LD(U)


def pad_to(n, t=TILE):
    return (n + t - 1) // t * t


def wide(rng, *shape, lo=-40.0, hi=40.0, signed=True):
    """Magnitudes log-uniform over 2^lo..2^hi, mixed signs."""
    v = np.exp2(rng.uniform(lo, hi, shape))
    return v * rng.choice([-1.0, 1.0], shape) if signed else v


def inorder(slabs, init=None):
    """Σ_t slabs[t] in float64, in slab order from 0.0 (or init) — slab_sum_kernel's sum."""
    s = np.zeros(slabs.shape[1:]) if init is None else init.copy()
    for t in range(slabs.shape[0]):
        s = s + slabs[t]
    return s


def sum_tol(k, c, absterms):
    """(k + c)·u·Σ|terms| (absterms: the longdouble Σ|a_i||b_i|)."""
    return (k + c) * uL * absterms


def tree_depth(nrows):
    """Additions on the longest path of a two-level row sum over nrows rows: block_sum of 256
    threads (6 butterfly levels, 4 waves in order), the strided walk of partials_sum_kernel
    (one add per 1024 blocks), its block_sum of 1024 threads (6 + 16)."""
    nblk = max(1, -(-nrows // 256))
    return 10 + -(-nblk // 1024) + 22


def exact(got, want):
    """0 if the arrays agree bit for bit (NaN matching NaN), else inf."""
    got, want = np.asarray(got), np.asarray(want)
    same = got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64))
    if not same and got.shape == want.shape:   # ±0 and NaN payloads do not matter
        same = bool(np.all((got == want) | (np.isnan(got) & np.isnan(want))))
    return 0.0 if same else float("inf")


def finite(*arrays):
    return 0.0 if all(np.isfinite(a).all() for a in arrays) else float("inf")


def nanlike(*shape):
    return np.full(shape, np.nan)


class Case:
    """One gps_vec_diag call: which, dims, scal, ins (arrays or None) and the outputs' initial
    contents (NaN unless the call reads them; None where an output is absent)."""

    def __init__(self, which, name, dims, ins, outs, scal=(), **extra):
        self.which, self.name, self.dims, self.scal = which, name, tuple(int(v) for v in dims), tuple(scal)
        self.ins = [None if a is None else np.ascontiguousarray(a, np.float64) for a in ins]
        self.outs0 = outs
        self.__dict__.update(extra)

    def fresh_outs(self):
        return [None if a is None else a.copy() for a in self.outs0]

    def __repr__(self):
        return "Case(%d, %s)" % (self.which, self.name)


def run(ctx, case):
    """The call on the device (ctx: gpscore.Context)."""
    outs = case.fresh_outs()
    ctx.vec_diag(case.which, case.dims, case.ins, outs, case.scal)
    return outs


def poison_upper(M):
    """NaN over the strict-upper 128-tiles of a square matrix (in place)."""
    for t in range(M.shape[0] // TILE):
        M[t * TILE:(t + 1) * TILE, (t + 1) * TILE:] = np.nan
    return M


def with_ld(M, ldm):
    """The device copy of a dense matrix with row stride ldm: NaN in the gap."""
    out = nanlike(M.shape[0], ldm)
    out[:, :M.shape[1]] = M
    return out


# ====================================================================== 0: gemv
GEMV_LOWER = (128, 256, 384)
GEMV_ROWS, GEMV_COLS = (1, 3, 4, 5, 9), (2, 126, 128, 130, 258)


def cases_gemv():
    """y_i = Σ_{k < kend} M_ik x_k, kend = cols (full) or (i/128 + 1)·128 (tile-lower: the diagonal
    tile is read whole).  Bound per row: (kend + 2)·u·Σ|M_ik||x_k| — kend products and adds in the
    lanes' order, the pair sum and the butterfly among them, c = 2 for the second-order terms."""
    rng = np.random.default_rng(3000)
    for k, np_ in enumerate(GEMV_LOWER):
        for mode in (1, 2) if np_ == 256 else (1,):
            ldm = np_ + (2 if k == 1 else 0)
            yield Case(0, "lower%d_mode%d" % (np_, mode), (mode, np_, np_, ldm, 0),
                       [wide(rng, np_, np_), wide(rng, np_)], [nanlike(np_)])
    for i, rows in enumerate(GEMV_ROWS):
        for j, cols in enumerate(GEMV_COLS):
            ldm = cols + (6 if (i + j) % 2 else 0)
            yield Case(0, "full%dx%d_ld%d" % (rows, cols, ldm), (0, rows, cols, ldm, 0),
                       [wide(rng, rows, cols), wide(rng, cols)], [nanlike(rows)])


def _gemv_kend(case):
    mode, rows, cols = case.dims[:3]
    i = np.arange(rows)
    return np.minimum(cols, (i // TILE + 1) * TILE) if mode else np.full(rows, cols)


def check_gemv(case, outs):
    M, x = case.ins
    kend = _gemv_kend(case)
    mask = np.arange(M.shape[1])[None, :] < kend[:, None]
    P = np.where(mask, ld(M) * ld(x)[None, :], LD(0))
    ref, tol = P.sum(1), sum_tol(kend, 2, np.abs(P).sum(1))
    return {"finite": finite(outs[0]), "y": worst_ratio(outs[0], ref, tol)}


def restate_gemv(case, defect=None):
    """gemv_rows_kernel: lane l takes the column pairs 2l + 128t in order, two accumulators,
    their sum, the butterfly.  defect 'kend_short' / 'kend_long': the tile-lower range one tile
    short / long."""
    mode, rows, cols, ldm = case.dims[:4]
    M = with_ld(case.ins[0], ldm)
    if mode:
        poison_upper(M[:, :cols])
    x = case.ins[1]
    kend = _gemv_kend(case)
    if defect == "kend_short":
        kend = kend - TILE
    if defect == "kend_long":
        kend = np.minimum(cols, kend + TILE)
    trips = -(-cols // 128)
    Mp, xp = nanlike(rows, trips * 128), nanlike(trips * 128)
    Mp[:, :cols], xp[:cols] = M[:, :cols], x
    kk = np.arange(trips * 128)
    prod = np.where(kk[None, :] < kend[:, None], Mp * xp[None, :], 0.0)
    acc = np.zeros((rows, 64, 2))
    for t in range(trips):
        acc = acc + prod[:, 128 * t:128 * (t + 1)].reshape(rows, 64, 2)
    return [wave_sum(acc[:, :, 0] + acc[:, :, 1])]


# ====================================================================== 1, 2: colred
COLRED_ROWS, COLRED_COLS = (1, 255, 256, 257, 513), (2, 510, 512, 514, 1026)
# (w, s1, s2, rowscale) present
COLRED_COMBOS = {"w_s1_s2": (1, 1, 1, 0), "w_s1": (1, 1, 0, 0), "s2": (0, 0, 1, 0), "rs_s1_s2": (1, 1, 1, 1)}
COLRED_LOWER = ((128, 256), (384, 256), (640, 256), (256, 32))    # (n_pad, crows)


def _colred_case(rng, rows, cols, ldm, lower, crows, combo):
    w, s1, s2, rs = COLRED_COMBOS[combo]
    ins = [wide(rng, rows, cols), wide(rng, rows, lo=-20, hi=20) if w else None,
           wide(rng, rows, lo=-10, hi=10) if rs else None]
    name = "%s%dx%d_ld%d_cr%d_%s" % ("lower" if lower else "full", rows, cols, ldm, crows, combo)
    return Case(1, name, (rows, cols, ldm, lower, crows), ins,
                [nanlike(cols) if s1 else None, nanlike(cols) if s2 else None])


def cases_colred():
    """s1_c = Σ_r (M_rc·sc_r)·w_r and s2_c = Σ_r (M_rc·sc_r)² over the rows r >= (c/128)·128 in
    the lower form, all rows otherwise, in chunks of crows rows whose partials are then added in
    chunk order.  Bound per column: (k + 4)·u·Σ|terms| with k the number of rows summed — each
    term carries the row scale's rounding and its own product (two for the square), c = 4."""
    rng = np.random.default_rng(3100)
    names = list(COLRED_COMBOS)
    for i, rows in enumerate(COLRED_ROWS):
        for j, cols in enumerate(COLRED_COLS):
            yield _colred_case(rng, rows, cols, cols + (4 if (i + j) % 3 == 0 else 0), 0, CR_ROWS,
                               names[(i + j) % 4])
    for combo in names:
        yield _colred_case(rng, 257, 514, 514, 0, CR_ROWS, combo)
    for np_, crows in COLRED_LOWER:
        for combo in names if np_ == 640 else names[:1]:
            yield _colred_case(rng, np_, np_, np_, 1, crows, combo)
    yield _colred_case(rng, 300, 130, 130, 0, 7, "w_s1_s2")     # crows that divides nothing


def _colred_terms(case):
    """Longdouble terms [rows][cols] of s1 and s2 (0 outside the column's row range)."""
    rows, cols, _, lower = case.dims[:4]
    M, w, rs = case.ins
    V = ld(M) * (ld(rs)[:, None] if rs is not None else LD(1))
    if lower:
        r = np.arange(rows)[:, None]
        V = np.where(r >= (np.arange(cols)[None, :] // TILE) * TILE, V, LD(0))
    return (V * ld(w)[:, None] if w is not None else None), V * V


def check_colred(case, outs):
    rows, cols, _, lower = case.dims[:4]
    T1, T2 = _colred_terms(case)
    k = rows - (np.arange(cols) // TILE) * TILE if lower else np.full(cols, rows)
    res = {"finite": finite(*[o for o in outs if o is not None])}
    for name, o, T in (("s1", outs[0], T1), ("s2", outs[1], T2)):
        if o is not None:
            res[name] = worst_ratio(o, T.sum(0), sum_tol(k, 4, np.abs(T).sum(0)))
    return res


def colred_slabs(case, crows, defect=None):
    """colred_kernel: (slab1, slab2) [nchunk][cols], each chunk's rows in order; NaN where nothing
    is written.  defect 'no_clip': the lower form without r0 = max(r0, tile start)."""
    rows, cols, ldm, lower = case.dims[:4]
    M = with_ld(case.ins[0], ldm)
    if lower:
        poison_upper(M[:, :cols])
    M = M[:, :cols]
    w, rs = case.ins[1], case.ins[2] if len(case.ins) > 2 else None
    nchunk = -(-rows // crows)
    s1, s2 = nanlike(nchunk, cols), nanlike(nchunk, cols)
    c0 = (np.arange(cols) // TILE) * TILE
    for ch in range(nchunk):
        a, b = np.zeros(cols), np.zeros(cols)
        for r in range(ch * crows, min(rows, ch * crows + crows)):
            v = M[r] * rs[r] if rs is not None else M[r]
            on = (r >= c0) if (lower and defect != "no_clip") else np.ones(cols, bool)
            if w is not None:
                a = np.where(on, v * w[r] + a, a)
            b = np.where(on, v * v + b, b)
        s1[ch], s2[ch] = a, b
    return s1, s2


def restate_colred(case, defect=None):
    """launch_colred: the chunk partials, then slab_sum over the chunks.  defect
    'drop_last_chunk': nchunk = rows / crows rounded down."""
    rows, crows = case.dims[0], case.dims[4]
    s1, s2 = colred_slabs(case, crows, defect)
    if defect == "drop_last_chunk":
        s1, s2 = s1[:rows // crows], s2[:rows // crows]
    return [None if case.outs0[0] is None else inorder(s1), None if case.outs0[1] is None else inorder(s2)]


def cases_colred_partials():
    """launch_colred_partials (crows = 256): the chunk slabs themselves.  Each chunk's entry is
    a sum over its own rows: (k_chunk + 4)·u·Σ|terms|, exactly 0 for a chunk that lies wholly
    above the column's tile (lower form), and the call returns the chunk count."""
    rng = np.random.default_rng(3200)
    for rows, cols, lower in ((640, 640, 1), (384, 384, 1), (513, 514, 0), (1, 2, 0)):
        nchunk = -(-rows // CR_ROWS)
        yield Case(2, "%s%dx%d" % ("lower" if lower else "full", rows, cols), (rows, cols, cols + 2, lower),
                   [wide(rng, rows, cols), wide(rng, rows, lo=-20, hi=20)],
                   [nanlike(2, nchunk, cols), nanlike(1)])


def check_colred_partials(case, outs):
    rows, cols, _, lower = case.dims[:4]
    T = _colred_terms(Case(1, "", case.dims, case.ins + [None], []))
    nchunk = -(-rows // CR_ROWS)
    res = {"finite": finite(*outs), "exact count": exact(outs[1], np.array([float(nchunk)]))}
    worst, zeros = 0.0, 0.0
    for q in range(2):
        for ch in range(nchunk):
            sl = slice(ch * CR_ROWS, min(rows, (ch + 1) * CR_ROWS))
            k = sl.stop - sl.start
            worst = max(worst, worst_ratio(outs[0][q, ch], T[q][sl].sum(0),
                                           sum_tol(k, 4, np.abs(T[q][sl]).sum(0))))
            if lower:
                empty = (np.arange(cols) // TILE) * TILE >= sl.stop
                zeros = max(zeros, exact(outs[0][q, ch][empty], np.zeros(int(empty.sum()))))
    res["partials"] = worst
    res["exact empty chunks"] = zeros
    return res


def restate_colred_partials(case, defect=None):
    s1, s2 = colred_slabs(Case(1, "", case.dims, case.ins + [None], []), CR_ROWS, defect)
    return [np.stack([s1, s2]), np.array([float(s1.shape[0])])]


# ====================================================================== 3: slab_sum
SLAB_N, SLAB_LEN = (1, 7, 8, 9, 17), (1, 255, 256, 257)


def cases_slab_sum():
    """out_j = init_j + Σ_t slab_t[j]: (nslab + 1 + 1)·u·(|init_j| + Σ|slab_t[j]|)."""
    rng = np.random.default_rng(3300)
    for i, ns in enumerate(SLAB_N):
        for j, ln in enumerate(SLAB_LEN):
            init = wide(rng, ln) if (i + j) % 2 else None
            yield Case(3, "ns%d_len%d_%s" % (ns, ln, "init" if init is not None else "noinit"),
                       (ns, ln, ln + (3 if (i + j) % 3 == 0 else 0)), [wide(rng, ns, ln), init], [nanlike(ln)])


def check_slab_sum(case, outs):
    slab, init = case.ins
    i0 = ld(init) if init is not None else LD(0)
    ref = i0 + ld(slab).sum(0)
    tol = sum_tol(slab.shape[0] + 1, 1, np.abs(i0) + np.abs(ld(slab)).sum(0))
    return {"finite": finite(outs[0]), "out": worst_ratio(outs[0], ref, tol)}


def restate_slab_sum(case, defect=None):
    """defects 'skip_last' (the loop one slab short) and 'no_init'."""
    ns, ln, ldd = case.dims[:3]
    img = nanlike(ns + 1, ldd)
    img[:ns, :ln] = case.ins[0]
    img = img[:, :ln]
    init = None if defect == "no_init" else case.ins[1]
    return [inorder(img[:ns - 1] if defect == "skip_last" else img[:ns], init)]


# ====================================================================== 4, 5: symmetric sums
SYM_M = (128, 256, 384)
PACK_MM = ((1, 128), (37, 128), (128, 128), (129, 256), (200, 256), (37, 256), (200, 384), (384, 384))
PACK_R = (1, 64, 128, 129)
PACK_LARGE = (2047, 2048)


def lower_tiles(M):
    i = np.arange(M)
    return (i[None, :] // TILE) <= (i[:, None] // TILE)


def cases_sym_slab_sum():
    """dst = base + Σ_t slab_t on the lower 128-tiles: (nslab + 2)·u·(|base| + Σ|slab_t|); the
    strict-upper tiles are exactly 0 (and are NaN in every operand on the device)."""
    rng = np.random.default_rng(3400)
    for i, M in enumerate(SYM_M):
        for ns in (1, 9):
            for base in (0, 1):
                yield Case(4, "M%d_ns%d_base%d" % (M, ns, base), (ns, M, M * M + (2 if i == 1 else 0)),
                           [wide(rng, ns, M * M), wide(rng, M * M) if base else None], [nanlike(M * M)])


def check_sym_slab_sum(case, outs):
    ns, M = case.dims[:2]
    slab, base = case.ins
    low = lower_tiles(M).reshape(-1)
    b = ld(base) if base is not None else np.zeros(M * M, LD)
    ref = np.where(low, b + ld(slab).sum(0), LD(0))
    tol = sum_tol(ns + 1, 1, np.abs(b) + np.abs(ld(slab)).sum(0))
    o = outs[0]
    return {"finite": finite(o), "exact upper tiles": exact(o[~low], np.zeros(int((~low).sum()))),
            "dst": worst_ratio(o[low], ref[low], tol[low])}


def _sym_images(case):
    ns, M, stride = case.dims[:3]
    slabs = nanlike(ns + 1, stride)
    for q in range(ns):
        slabs[q, :M * M] = poison_upper(case.ins[0][q].reshape(M, M).copy()).reshape(-1)
    base = case.ins[1]
    if base is not None and not (case.which == 5 and case.dims[7]):
        base = poison_upper(base.reshape(M, M).copy()).reshape(-1)
    return slabs, base


def restate_sym_slab_sum(case, defect=None):
    ns, M = case.dims[:2]
    slabs, base = _sym_images(case)
    low = lower_tiles(M).reshape(-1)
    v = np.zeros(M * M)
    v[low] = inorder(slabs[:ns, :M * M][:, low])
    if base is not None:
        v[low] = base[low] + v[low]
    return [v]


def tri(i):
    return i * (i + 1) // 2


def sym_slabs(rng, ns, m, M, symmetric=False):
    """ns slabs of an M×M accumulator: real on the element-wise lower triangle of the leading
    m×m block, NaN everywhere else; symmetric: mirrored, zero in the padding (what the SYRK
    leaves), for the comparison with sym_slab_sum."""
    S = nanlike(ns, M, M)
    il = np.tril_indices(m)
    for q in range(ns):
        S[q][il] = wide(rng, len(il[0]))
    if symmetric:
        for q in range(ns):
            full = np.zeros((M, M))
            full[:m, :m] = np.tril(np.nan_to_num(S[q][:m, :m])) + np.tril(np.nan_to_num(S[q][:m, :m]), -1).T
            S[q] = full
    return S.reshape(ns, M * M)


def cases_sym_pack():
    """launch_sym_pack over the rows [r0, r1), then (unpack) launch_sym_unpack.
      packed[e], e in [r0(r0+1)/2, r1(r1+1)/2): Σ_t slab_t[i][j] of the row-major lower-packed
        index e = i(i+1)/2 + j: (nslab + 1)·u·Σ|slab_t|, and bitwise the in-order float64 sum;
        every other entry keeps the bits it had;
      dst: packed[hi(hi+1)/2 + lo] + base, one rounding from the device's own packed values, so
        bitwise; 0 + base past m; exactly 0 on the strict-upper tiles unless full.
    The slabs are NaN above the element diagonal and past row m."""
    rng = np.random.default_rng(3500)
    for k, (m, M) in enumerate(PACK_MM):
        ranges = [(0, m)] + [rr for r in PACK_R if r < m for rr in ((0, r), (r, m))]
        for j, (r0, r1) in enumerate(ranges):
            ns = 9 if (k + j) % 2 else 1
            unpack = j < 3 or m == 200
            full = (k + j) % 2
            base = wide(rng, M * M) if (unpack and (j % 3 != 1)) else None
            yield Case(5, "m%d_M%d_r%d_%d_ns%d_un%d_full%d_base%d" % (m, M, r0, r1, ns, unpack, full,
                                                                      base is not None),
                       (ns, M, M * M, m, r0, r1, unpack, full), [sym_slabs(rng, ns, m, M), base],
                       [wide(rng, tri(m)), nanlike(M * M) if unpack else None])


def case_sym_pack_large():
    """e up to 2047·2048/2: the square root of 8e + 1 and its correction at large e.  nslab = 1,
    so packed is the slab's lower triangle bit for bit."""
    m, M = PACK_LARGE
    rng = np.random.default_rng(3501)
    return Case(5, "m%d_M%d_large" % (m, M), (1, M, M * M, m, 0, m, 0, 0), [sym_slabs(rng, 1, m, M), None],
                [nanlike(tri(m)), None])


def roundtrip_cases():
    """(sym_slab_sum case, pack + unpack case) on the same symmetric slabs and base: the lower
    tiles must agree bit for bit."""
    rng = np.random.default_rng(3502)
    for m, M, ns in ((37, 128, 9), (200, 256, 3), (129, 384, 9)):
        S, base = sym_slabs(rng, ns, m, M, symmetric=True), wide(rng, M * M)
        yield (Case(4, "rt_m%d_M%d" % (m, M), (ns, M, M * M), [S, base], [nanlike(M * M)]),
               Case(5, "rt_m%d_M%d" % (m, M), (ns, M, M * M, m, 0, m, 1, 0), [S, base],
                    [nanlike(tri(m)), nanlike(M * M)]))


def check_sym_pack(case, outs):
    ns, M, _, m, r0, r1, unpack, full = case.dims
    slab, base = case.ins
    S = slab.reshape(ns, M, M)
    il = np.tril_indices(m)
    e0, e1 = tri(r0), tri(r1)
    packed = outs[0]
    terms = ld(S[:, il[0], il[1]])
    res = {"finite": finite(packed[e0:e1]),
           "exact untouched": max(exact(packed[:e0], case.outs0[0][:e0]), exact(packed[e1:], case.outs0[0][e1:])),
           "packed": worst_ratio(packed[e0:e1], terms.sum(0)[e0:e1], sum_tol(ns, 1, np.abs(terms).sum(0)[e0:e1])),
           "exact packed": exact(packed[e0:e1], inorder(S[:, il[0], il[1]])[e0:e1])}
    if unpack:
        P = np.zeros((M, M))
        P[il] = packed
        P[:m, :m] = np.tril(P[:m, :m]) + np.tril(P[:m, :m], -1).T
        want = P + base.reshape(M, M) if base is not None else P
        if not full:
            want = np.where(lower_tiles(M), want, 0.0)
        res["finite dst"] = finite(outs[1])
        res["exact dst"] = exact(outs[1].reshape(M, M), want)
    return res


def restate_sym_pack(case, defect=None):
    """sym_pack_kernel / sym_unpack_kernel.  defects 'pack_row_off': the row index of e from
    the truncated square root alone, one short where 8e + 1 is a perfect square's neighbour
    (restated as: one short at every triangular number); 'unpack_swap': hi and lo exchanged."""
    ns, M, stride, m, r0, r1, unpack, full = case.dims
    slabs, base = _sym_images(case)
    packed = case.outs0[0].copy()
    e = np.arange(tri(r0), tri(r1))
    i = ((np.sqrt(8.0 * e + 1.0) - 1.0) * 0.5).astype(np.int64)
    i = np.where(tri(i + 1) <= e, i + 1, i)
    i = np.where(tri(i) > e, i - 1, i)
    if defect == "pack_row_off":
        i = np.where((tri(i) == e) & (i > 0), i - 1, i)
    j = e - tri(i)
    packed[e] = inorder(slabs[:ns][:, i * M + j])
    outs = [packed, None]
    if unpack:
        ii, jj = np.meshgrid(np.arange(M), np.arange(M), indexing="ij")
        hi, lo = np.maximum(ii, jj), np.minimum(ii, jj)
        if defect == "unpack_swap":
            hi, lo = lo, hi
        inside = (ii < m) & (jj < m)
        idx = np.where(inside, tri(hi) + lo, 0)
        v = np.where(inside, packed[np.minimum(idx, len(packed) - 1)], 0.0)
        region = np.ones((M, M), bool) if full else lower_tiles(M)
        if base is not None:
            v = v + np.where(region, base.reshape(M, M), 0.0)
        outs[1] = np.where(region, v, 0.0).reshape(-1)
    return outs


# ====================================================================== the row pools
POOL_P = 640
POOL_NS = 9
POOL_Z = (0.0, 1e-8, -0.5, 0.8325546, -1.0, 2.0, -5.0, 8.3, -26.0, 37.5, 40.0, -1e5)
POOL_D = (1e-6, 1e-3, 0.3, 1.0, 50.0, 1e4)
POOL_Y = (0.0, 0.3, -7.0, 1e6)
POOL_RHO = (0.0, 0.25, 0.5, 1.0 - 2.0 ** -20)       # r/λ: the last one leaves d = 2^-20/λ
SURF_S2 = (1.5e-4, 1e-7)                            # s2·d < 2 for every d of the pool
LAM_SF2 = 1.7
LAM_SN2 = (1e-6, 0.01)
POOL_INPUTS = ("y", "full_s1", "full_s2", "beta", "logdiag", "fitc_lam", "fitc_rs", "fitc_g", "lam_qs")


def _split(rng, target, signed):
    """POOL_NS slabs per row whose in-order float64 sum is near target: eight pieces over
    2^-40..2^2 of the target's size (signed) or positive weights over 2^-40..1 that add up to
    it, the last piece closing the gap.  A zero target gets ± pieces that cancel exactly."""
    P = len(target)
    scale = np.where(target == 0, 1.0, np.abs(target))
    if signed:
        S = wide(rng, POOL_NS, P, lo=-40, hi=2) * scale
        S[-1] = np.where(target == 0, 0.0, target) - inorder(S[:-1])
    else:
        W = wide(rng, POOL_NS, P, lo=-40, hi=0, signed=False)
        S = target * W / W.sum(0)
    return S


def build_pool():
    """The float64 inputs of the row finalisers' cases, 640 rows (the first 288 the full cross
    of POOL_Z × POOL_D × POOL_Y, then z ~ 3·N(0, 1)); make_vec_terms.py stores them with erf and
    exp at the z each row defines.
      full  (which 6, 10): slabs full_s1 / full_s2 whose in-order sums are α ≈ z·√d and d;
      fitc  (which 8): λ = 1/d, slabs fitc_rs summing to r ≈ ρλ, g = y − z·√(d(1 − ρ))·λ;
      lam   (which 7): slabs lam_qs summing to q — the first 16 rows within 1..4 ulp below
            sf2 = 1.7, the rest over 2^-40..1 of it with mixed signs."""
    rng = np.random.default_rng(3600)
    P = POOL_P
    i = np.arange(P)
    z = np.where(i < 288, np.array(POOL_Z)[i % 12], 3.0 * rng.standard_normal(P))
    d = np.array(POOL_D)[(i // 12) % 6]
    y = np.array(POOL_Y)[(i // 72) % 4]
    rho = np.array(POOL_RHO)[(i + i // 12) % 4]
    g = {"y": y}
    g["full_s1"] = _split(rng, z * np.sqrt(d), True)
    g["full_s2"] = _split(rng, d, False)
    g["beta"] = rng.standard_normal(P) * np.exp2(rng.uniform(-3, 3, P))
    g["logdiag"] = rng.standard_normal(P)
    lam = 1.0 / d
    g["fitc_lam"] = lam
    g["fitc_rs"] = _split(rng, rho * lam, False)
    g["fitc_g"] = y - (z * np.sqrt(d * (1.0 - rho))) * lam
    q = LAM_SF2 * rng.uniform(0.0, 1.0, P) * np.exp2(rng.choice([0.0, -10.0, -40.0], P))
    q[:16] = LAM_SF2 - (1 + np.arange(16) % 4) * np.spacing(LAM_SF2)
    g["lam_qs"] = _split(rng, q, True)
    return g


def pool_z_inputs(g):
    """What erf and exp are evaluated from, per family: the float64 values the kernels start
    from (the slabs' in-order sums among them)."""
    a, dd = inorder(g["full_s1"]), inorder(g["full_s2"])
    return {"alpha": a, "dinv": dd, "r": inorder(g["fitc_rs"])}


def load_pool():
    need_extended()
    with np.load(FIXTURE, allow_pickle=False) as z:
        g = {k: z[k] for k in z.files}
    g.update(pool_z_inputs(g))
    for fam in ("full", "fitc", "surf0", "surf1"):
        for key in ("erf", "exp"):
            g["%s_%s" % (fam, key)] = ld(g["%s_%s_hi" % (fam, key)]) + ld(g["%s_%s_lo" % (fam, key)])
    return g


_POOL = None


def pool():
    global _POOL
    if _POOL is None:
        _POOL = load_pool()
    return _POOL


def rows_of(n, lo):
    """Row indices into the pool of a case with n rows starting at lo (cyclic)."""
    return (lo + np.arange(n)) % POOL_P


def score_terms_ref(res, c, erf, ex, dm, dc):
    """Longdouble CRPS and LogS terms at residual res = y − μ and variance c, with their bounds
    when the kernel's μ and c carry the absolute errors dm and dc:
      CRPS = s(z·erf(z/√2) + 2φ(z) − 1/√π): 64u·|CRPS| for crps_term itself, plus
        |∂/∂μ| = |erf| times dm and |∂/∂c| = |2φ − 1/√π|/(2s) times dc;
      LogS = res²/2c + log s + ½log 2π: 8u·(q + |log s| + 1 + |LogS|) (§18), plus |res|/c·dm and
        (q/c + 1/2c)·dc."""
    s = np.sqrt(c)
    z = res / s
    phi2 = 2 * INV_SQRT_2PI * ex
    crps = s * (z * erf + phi2 - INV_SQRT_PI)
    q = res * res / (2 * c)
    logs = q + np.log(s) + LD(HALF_LOG_2PI)
    tc = 64 * uL * np.abs(crps) + np.abs(erf) * dm + np.abs(phi2 - INV_SQRT_PI) / (2 * s) * dc
    tl = 8 * uL * (q + np.abs(np.log(s)) + 1 + np.abs(logs)) + np.abs(res) / c * dm + (q / c + 1 / (2 * c)) * dc
    return crps, logs, tc, tl


def tree_sum_ref(terms, tb, nrows):
    """(Σ terms, Σ tb + (D + 1)·u·Σ|terms|) of a two-level row sum over nrows rows."""
    return terms.sum(), tb.sum() + (tree_depth(nrows) + 1) * uL * np.abs(terms).sum()


def crps_f64(m, c, y):
    with np.errstate(all="ignore"):
        s = np.sqrt(c)
        z = (y - m) / s
        cdf = 0.5 * (1.0 + _erf(z * K_SQRT_HALF))
        pdf = K_PDF * np.exp(-z * z * 0.5)
        return s * (z * (2.0 * cdf - 1.0) + 2.0 * pdf - K_ISP)


def logs_f64(m, c, y):
    with np.errstate(all="ignore"):
        e = y - m
        return e * e / (2.0 * c) + np.log(np.sqrt(c)) + HALF_LOG_2PI


def block_sum_n(v, nt):
    """block_sum of nt threads (last axis): the butterfly per wave, the waves in order from 0."""
    w = wave_sum(v.reshape(v.shape[:-1] + (nt // 64, 64)))
    t = np.zeros(w.shape[:-1])
    for k in range(nt // 64):
        t = t + w[..., k]
    return t


def two_level_sum(x, nrows, defect=None):
    """One value per row (x: [nrows], zeros where the kernel adds none): per-block block_sum of
    256, then partials_sum_kernel — thread b takes blocks b, b + 1024, ... in order, block_sum
    of 1024.  defect 'first_trip_only': the blocks >= 1024 are ignored."""
    nblk = max(1, -(-nrows // 256))
    xp = np.zeros(nblk * 256)
    xp[:len(x)] = x
    part = block_sum_n(xp.reshape(nblk, 256), 256)
    trips = 1 if defect == "first_trip_only" else -(-nblk // 1024)
    pp = np.zeros(-(-nblk // 1024) * 1024)
    pp[:nblk] = part
    v = np.zeros(1024)
    for t in range(trips):
        v = v + pp[1024 * t:1024 * (t + 1)]
    return float(block_sum_n(v, 1024))


FIN_N = (1, 127, 128, 129, 300, 513)
FIN_LARGE_N = 1024 * 256 + 1          # n_pad = 262 272: 1025 blocks, the second trip


def _slabs_of(S, rows, ns, n_pad):
    """[ns][n_pad] slabs of the pool rows: the nine pool slabs, or their in-order sum as one."""
    out = S[:, rows] if ns == POOL_NS else inorder(S[:, rows])[None, :]
    assert out.shape == (ns, n_pad)
    return np.ascontiguousarray(out)


# ====================================================================== 6: full_loo
def case_full_loo(n, ns, lo=0, ld_extra=0):
    g = pool()
    n_pad = pad_to(n)
    rows = rows_of(n_pad, lo)
    ins = [g["y"][rows[:n]], _slabs_of(g["full_s1"], rows, ns, n_pad), _slabs_of(g["full_s2"], rows, ns, n_pad),
           g["beta"][rows], g["logdiag"][rows]]
    return Case(6, "n%d_ns%d" % (n, ns), (n, ns, n_pad + ld_extra), ins,
                [nanlike(n_pad) for _ in range(4)] + [nanlike(5), nanlike(4)], rows=rows)


def cases_full_loo():
    """launch_full_loo.  α and d (all n_pad rows) bitwise the in-order slab sums; per real row
      μ = y − α/d: 2u·(|y| + |α/d|) (a quotient and a difference);  σ² = 1/d: u/d;
    rows past n of μ and σ² stay unwritten.  The sums: Σ CRPS and Σ LogS with the terms' bounds
    at dm = 2u·(|y| + |α/d|), dc = u/d (score_terms_ref) and the tree's (D + 1)·u·Σ|t|; Σ log L_ii
    and Σ β² over all n_pad rows, (D + 1) and (D + 2)·u·Σ|t|.  The objectives: logdet = 2Σ exactly,
    quad, the means (their sum's bound / n + u·|ref|), and nlml = ½n·log 2π + ½logdet + ½quad:
    the sums' bounds plus 4u·(½n·log 2π + ½|logdet| + ½quad)."""
    for k, n in enumerate(FIN_N):
        for ns in (1, POOL_NS):
            yield case_full_loo(n, ns, lo=37 * k, ld_extra=2 if k % 2 else 0)


def check_full_loo(case, outs):
    g, rows = pool(), case.rows
    n, ns = case.dims[:2]
    n_pad = pad_to(n)
    alpha, dinv, mu, var, obj, sums = outs
    y, s1, s2, beta, logdiag = case.ins
    res = {"finite": finite(alpha, dinv, mu[:n], var[:n], obj, sums),
           "exact alpha": exact(alpha, inorder(s1)), "exact dinv": exact(dinv, inorder(s2)),
           "exact unwritten": exact(np.concatenate([mu[n:], var[n:]]), nanlike(2 * (n_pad - n)))}
    r = rows[:n]
    a, d, yl = ld(g["alpha"][r]), ld(g["dinv"][r]), ld(y)
    dm, dc = 2 * uL * (np.abs(yl) + np.abs(a / d)), uL / d
    res["mu"] = worst_ratio(mu[:n], yl - a / d, dm)
    res["var"] = worst_ratio(var[:n], 1 / d, dc)
    crps, logs, tc, tl = score_terms_ref(a / d, 1 / d, g["full_erf"][r], g["full_exp"][r], dm, dc)
    D = tree_depth(n_pad)
    S = [tree_sum_ref(crps, tc, n_pad), tree_sum_ref(logs, tl, n_pad),
         (ld(logdiag).sum(), (D + 1) * uL * np.abs(ld(logdiag)).sum()),
         ((ld(beta) ** 2).sum(), (D + 2) * uL * (ld(beta) ** 2).sum())]
    for k, name in enumerate(("sum crps", "sum logs", "sum logdiag", "sum beta2")):
        res[name] = worst_ratio(sums[k], S[k][0], S[k][1])
    logdet, quad = 2 * S[2][0], S[3][0]
    c0 = LD(0.5) * n * np.log(2 * LD(np.pi))
    refs = [c0 + logdet / 2 + quad / 2, S[0][0] / n, S[1][0] / n, logdet, quad]
    tols = [S[2][1] + S[3][1] / 2 + 4 * uL * (c0 + np.abs(logdet) / 2 + quad / 2),
            S[0][1] / n + uL * np.abs(refs[1]), S[1][1] / n + uL * np.abs(refs[2]), 2 * S[2][1], S[3][1]]
    for k, name in enumerate(("nlml", "loo_crps", "loo_logs", "logdet", "quad")):
        res["obj " + name] = worst_ratio(obj[k], refs[k], tols[k])
    return res


def restate_full_loo(case, defect=None):
    """full_loo_rows_kernel, partials_sum_kernel<4>, full_loo_obj_kernel.  defects
    'first_trip_only', 'nlml_const' (log 2π to ten digits), 'nlml_half' (logdet not halved)."""
    n, ns = case.dims[:2]
    n_pad = pad_to(n)
    y, s1, s2, beta, logdiag = case.ins
    a, dd = inorder(s1), inorder(s2)
    mu, var = nanlike(n_pad), nanlike(n_pad)
    m, c = y - a[:n] / dd[:n], 1.0 / dd[:n]
    mu[:n], var[:n] = m, c
    sums = np.array([two_level_sum(crps_f64(m, c, y), n_pad, defect), two_level_sum(logs_f64(m, c, y), n_pad, defect),
                     two_level_sum(logdiag, n_pad, defect), two_level_sum(beta * beta, n_pad, defect)])
    logdet, quad = 2.0 * sums[2], sums[3]
    k = 1.8378770664 if defect == "nlml_const" else LOG_2PI
    obj = np.array([0.5 * n * k + (1.0 if defect == "nlml_half" else 0.5) * logdet + 0.5 * quad,
                    sums[0] / n, sums[1] / n, logdet, quad])
    return [a, dd, mu, var, obj, sums]


# ====================================================================== 7: fitc_lambda
def case_fitc_lambda(n, ns, sn2, lo=0, n_pad=None, ld_extra=0):
    g = pool()
    n_pad = pad_to(n) if n_pad is None else n_pad
    rows = rows_of(n_pad, lo)
    return Case(7, "n%d_pad%d_ns%d_sn%g" % (n, n_pad, ns, sn2), (n, n_pad, ns, n_pad + ld_extra),
                [_slabs_of(g["lam_qs"], rows, ns, n_pad), g["y"][rows[:n]]],
                [nanlike(n_pad) for _ in range(4)] + [nanlike(2)], scal=(LAM_SF2, sn2), rows=rows)


def cases_fitc_lambda():
    """launch_fitc_lambda.  q (all n_pad rows) bitwise the in-order slab sum; per real row, with
    S = sf2 + |q| + sn2:
      λ = sf2 − q + sn2: 2u·S = dλ;   1/λ: (dλ/λ² + u/λ)(1 + 2dλ/λ) = di;   y/λ: |y|·di + u·|y|/λ;
    pad rows exactly λ = 1, 1/λ = 0, y/λ = 0.  Σ log λ: per term dλ/λ·(1 + dλ/λ) + 4u·|log λ| (the
    device log within 2 ulp), Σ y²/λ: per term y²·di + 2u·y²/λ; both with the tree's
    (D + 1)·u·Σ|t|."""
    for k, n in enumerate(FIN_N):
        for ns in (1, POOL_NS):
            yield case_fitc_lambda(n, ns, LAM_SN2[k % 2], lo=0 if k % 2 == 0 else 41 * k, ld_extra=2 if k % 2 else 0)
    yield case_fitc_lambda(300, POOL_NS, LAM_SN2[0], n_pad=320)      # a 32-row padding


def check_fitc_lambda(case, outs):
    n, n_pad, ns = case.dims[:3]
    sf2, sn2 = (LD(v) for v in case.scal)
    slab, y = case.ins
    q, lam, il, ys, sums = outs
    qf = inorder(slab)
    pads = n_pad - n
    res = {"finite": finite(*outs), "exact q": exact(q, qf),
           "exact pads": max(exact(lam[n:], np.ones(pads)), exact(il[n:], np.zeros(pads)),
                             exact(ys[n:], np.zeros(pads)))}
    ql, yl = ld(qf[:n]), ld(y)
    lref = sf2 - ql + sn2
    dl = 2 * uL * (sf2 + np.abs(ql) + sn2)
    di = (dl / lref ** 2 + uL / lref) * (1 + 2 * dl / lref)
    res["lam"] = worst_ratio(lam[:n], lref, dl)
    res["inv_lam"] = worst_ratio(il[:n], 1 / lref, di)
    res["ys"] = worst_ratio(ys[:n], yl / lref, np.abs(yl) * di + uL * np.abs(yl) / lref)
    t0, t1 = np.log(lref), yl * yl / lref
    S0 = tree_sum_ref(t0, dl / lref * (1 + dl / lref) + 4 * uL * np.abs(t0), n_pad)
    S1 = tree_sum_ref(t1, yl * yl * di + 2 * uL * t1, n_pad)
    res["sum loglam"] = worst_ratio(sums[0], *S0)
    res["sum y2/lam"] = worst_ratio(sums[1], *S1)
    return res


def restate_fitc_lambda(case, defect=None):
    """defect 'pad_inv_lam': pad rows with 1/λ = 1 instead of 0; 'first_trip_only'."""
    n, n_pad = case.dims[:2]
    sf2, sn2 = case.scal
    slab, y = case.ins
    q = inorder(slab)
    lam, il, ys = np.ones(n_pad), np.zeros(n_pad), np.zeros(n_pad)
    lam[:n] = sf2 - q[:n] + sn2
    il[:n] = 1.0 / lam[:n]
    ys[:n] = y * il[:n]
    if defect == "pad_inv_lam":
        il[n:] = 1.0 / lam[n:]
    d2 = "first_trip_only" if defect == "first_trip_only" else None
    sums = np.array([two_level_sum(np.log(lam[:n]), n_pad, d2), two_level_sum(y * y * il[:n], n_pad, d2)])
    return [q, lam, il, ys, sums]


# ====================================================================== 8: fitc_loo
def case_fitc_loo(n, ns, lo=0, n_pad=None, ld_extra=0):
    g = pool()
    n_pad = pad_to(n) if n_pad is None else n_pad
    rows = rows_of(n_pad, lo)
    r = rows[:n]
    return Case(8, "n%d_pad%d_ns%d" % (n, n_pad, ns), (n, n_pad, ns, n_pad + ld_extra),
                [g["y"][r], g["fitc_lam"][r], _slabs_of(g["fitc_rs"], rows, ns, n_pad), g["fitc_g"][r]],
                [nanlike(n_pad) for _ in range(3)] + [nanlike(2)], rows=rows)


def cases_fitc_loo():
    """launch_fitc_loo.  r (all n_pad rows) bitwise the in-order slab sum; per real row
      d = 1/λ − r/λ²: u·(1/λ + 4|r|/λ² + |d|) = dd, κ = dd/|d|;
      a = (y − g)/λ: 3u·|a|;
      μ = y − a/d: |a/d|·(4u + κ)/(1 − κ) + u·(|y| + |a/d|) = dm;
      σ² = 1/d: (κ + u)/(1 − κ)/|d| = dc;
    μ and σ² past n unwritten.  Σ CRPS, Σ LogS: the terms' bounds at dm, dc and the tree's."""
    for k, n in enumerate(FIN_N):
        for ns in (1, POOL_NS):
            yield case_fitc_loo(n, ns, lo=53 * k, ld_extra=2 if k % 2 else 0)
    yield case_fitc_loo(300, POOL_NS, n_pad=320)


def fitc_loo_reference(y, lam, r, gg):
    """(a, d, μ, σ², dm, dc) in longdouble from the float64 inputs."""
    y, lam, r, gg = (ld(v) for v in (y, lam, r, gg))
    il = 1 / lam
    a, d = (y - gg) * il, il - r * il * il
    kap = uL * (il + 4 * np.abs(r) * il * il + np.abs(d)) / np.abs(d)
    dm = np.abs(a / d) * (4 * uL + kap) / (1 - kap) + uL * (np.abs(y) + np.abs(a / d))
    dc = (kap + uL) / (1 - kap) / np.abs(d)
    return a, d, y - a / d, 1 / d, dm, dc


def check_fitc_loo(case, outs):
    g, rows = pool(), case.rows
    n, n_pad = case.dims[:2]
    y, lam, slab, gg = case.ins
    r, mu, var, sums = outs
    rf = inorder(slab)
    res = {"finite": finite(r, mu[:n], var[:n], sums), "exact r": exact(r, rf),
           "exact unwritten": exact(np.concatenate([mu[n:], var[n:]]), nanlike(2 * (n_pad - n)))}
    a, d, mref, cref, dm, dc = fitc_loo_reference(y, lam, rf[:n], gg)
    res["mu"] = worst_ratio(mu[:n], mref, dm)
    res["var"] = worst_ratio(var[:n], cref, dc)
    k = rows[:n]
    crps, logs, tc, tl = score_terms_ref(a / d, cref, g["fitc_erf"][k], g["fitc_exp"][k], dm, dc)
    res["sum crps"] = worst_ratio(sums[0], *tree_sum_ref(crps, tc, n_pad))
    res["sum logs"] = worst_ratio(sums[1], *tree_sum_ref(logs, tl, n_pad))
    return res


def restate_fitc_loo(case, defect=None):
    n, n_pad = case.dims[:2]
    y, lam, slab, gg = case.ins
    r = inorder(slab)
    il = 1.0 / lam
    d = il - r[:n] * il * il
    a = (y - gg) * il
    mu, var = nanlike(n_pad), nanlike(n_pad)
    mu[:n], var[:n] = y - a / d, 1.0 / d
    sums = np.array([two_level_sum(crps_f64(mu[:n], var[:n], y), n_pad, defect),
                     two_level_sum(logs_f64(mu[:n], var[:n], y), n_pad, defect)])
    return [r, mu, var, sums]


# ====================================================================== 9: the predictive
PRED_NT = (1, 255, 256, 257)


def cases_pred():
    """launch_pred_finalize: mu = s1 bit for bit, var = base − s2: u·(base + |s2|).
    launch_fitc_pred_finalize: var = base − qm + qb: 2u·(base + |qm| + |qb|) (two roundings).
    A quarter of the rows have s2 (or qm) within 2^-30 of base (+ qb), where the result is
    the difference's low bits."""
    rng = np.random.default_rng(3900)
    for k, nt in enumerate(PRED_NT):
        base = (1.01, 3.7e5)[k % 2]
        s1 = wide(rng, nt)
        qb = base * wide(rng, nt, lo=-40, hi=3, signed=False)
        near = np.arange(nt) % 4 == 0
        s2 = np.where(near, base * (1 - wide(rng, nt, lo=-50, hi=-30)), base * wide(rng, nt, lo=-40, hi=0, signed=False))
        qm = np.where(near, (base + qb) * (1 - wide(rng, nt, lo=-50, hi=-30)), s2)
        yield Case(9, "full_nt%d" % nt, (nt, 0), [s1, s2], [nanlike(nt), nanlike(nt)], scal=(base,))
        yield Case(9, "fitc_nt%d" % nt, (nt, 1), [qm, qb], [None, nanlike(nt)], scal=(base,))


def check_pred(case, outs):
    nt, fitc = case.dims[:2]
    base = LD(case.scal[0])
    a, b = (ld(v) for v in case.ins)
    res = {"finite": finite(*[o for o in outs if o is not None])}
    if fitc:
        res["var"] = worst_ratio(outs[1], base - a + b, 2 * uL * (base + np.abs(a) + np.abs(b)))
    else:
        res["exact mu"] = exact(outs[0], case.ins[0])
        res["var"] = worst_ratio(outs[1], base - b, uL * (base + np.abs(b)))
    return res


def restate_pred(case, defect=None):
    """defect 'qb_sign': var = base − qm − qb."""
    a, b = case.ins
    base = case.scal[0]
    if case.dims[1]:
        return [None, base - a - b if defect == "qb_sign" else base - a + b]
    return [a.copy(), base - b]


# ====================================================================== 10: the surface point
def cases_surface():
    """launch_surface_point_sums from (y, α, d).  The first sum's terms are CRPS at
      μ_w = y − s²α: 2u·(|y| + s²|α|),   c_w = 2s² − s⁴d: 3u·(2s² + s⁴d)
    (s²·s², ·d, the difference; the doubling is exact), the second's LogS at μ = y − α/d and
    σ² = 1/d (+ s²: one more rounding, u·(1/d + s²)) with full_loo's dm and dc."""
    for k, n in enumerate(FIN_N):
        for add in (0, 1):
            yield case_surface(n, k % 2, add, lo=29 * k)


def case_surface(n, s2k, add, lo=0):
    g = pool()
    r = rows_of(n, lo)
    return Case(10, "n%d_s2_%d_add%d" % (n, s2k, add), (n, add), [g["y"][r], g["alpha"][r], g["dinv"][r]],
                [nanlike(2)], scal=(SURF_S2[s2k],), rows=r, s2k=s2k)


def check_surface(case, outs):
    g, r = pool(), case.rows
    n, add = case.dims[:2]
    s2 = LD(case.scal[0])
    y, a, d = (ld(v) for v in case.ins)
    cw = 2 * s2 - s2 * s2 * d
    crps, _, tc, _ = score_terms_ref(s2 * a, cw, g["surf%d_erf" % case.s2k][r], g["surf%d_exp" % case.s2k][r],
                                     2 * uL * (np.abs(y) + s2 * np.abs(a)), 3 * uL * (2 * s2 + s2 * s2 * d))
    c = 1 / d + (s2 if add else 0)
    dm, dc = 2 * uL * (np.abs(y) + np.abs(a / d)), uL / d + (uL * c if add else 0)
    # LogS needs no erf: the terms with erf = exp = 0 placeholders, only logs and its bound used
    _, logs, _, tl = score_terms_ref(a / d, c, LD(0) * d, LD(0) * d, dm, dc)
    return {"finite": finite(outs[0]), "sum crps": worst_ratio(outs[0][0], *tree_sum_ref(crps, tc, n)),
            "sum logs": worst_ratio(outs[0][1], *tree_sum_ref(logs, tl, n))}


def restate_surface(case, defect=None):
    n, add = case.dims[:2]
    s2 = case.scal[0]
    y, a, d = case.ins
    mu, c = y - a / d, 1.0 / d
    v0 = crps_f64(y - s2 * a, 2.0 * s2 - s2 * s2 * d, y)
    v1 = logs_f64(mu, c + s2 if add else c, y)
    return [np.array([two_level_sum(v0, n, defect), two_level_sum(v1, n, defect)])]


# ====================================================================== 11: dot
DOT_N = (1, 1023, 1024, 1025, 5000)


def cases_dot():
    """out = Σ a_i b_i (or Σ a_i): (n + 2)·u·Σ|a_i||b_i|."""
    rng = np.random.default_rng(4100)
    for n in DOT_N:
        for b in (0, 1):
            yield Case(11, "n%d_b%d" % (n, b), (n,), [wide(rng, n), wide(rng, n, lo=-20, hi=20) if b else None],
                       [nanlike(1)])


def check_dot(case, outs):
    a, b = case.ins
    t = ld(a) * (ld(b) if b is not None else LD(1))
    return {"finite": finite(outs[0]), "out": worst_ratio(outs[0][0], t.sum(), sum_tol(len(a), 2, np.abs(t).sum()))}


def restate_dot(case, defect=None):
    a, b = case.ins
    t = a * b if b is not None else a
    n = len(t)
    tp = np.zeros(-(-n // 1024) * 1024)
    tp[:n] = t
    v = np.zeros(1024)
    for k in range(len(tp) // 1024):
        v = v + tp[1024 * k:1024 * (k + 1)]
    return [np.array([float(block_sum_n(v, 1024))])]


# ====================================================================== 12: pad_copy
# (rows, cols, lds, rows_pad, cols_pad, ldd)
PAD_SHAPES = ((5, 3, 3, 128, 128, 128), (128, 128, 128, 128, 128, 128), (129, 1, 1, 256, 1, 1),
              (37, 37, 300, 128, 128, 128), (5, 3, 10, 128, 256, 258), (200, 130, 256, 256, 256, 256))


def cases_pad_copy():
    """dst = src zero-padded, the identity on the padded diagonal when asked; everything bit for
    bit, the gap of dst's rows (ldd > cols_pad) untouched."""
    rng = np.random.default_rng(4200)
    for sh in PAD_SHAPES:
        for ident in (0, 1):
            yield Case(12, "%dx%d_lds%d_to_%dx%d_ldd%d_id%d" % (sh + (ident,)), sh + (ident,),
                       [wide(rng, sh[0], sh[1])], [nanlike(sh[3], sh[5])])


def _pad_want(case):
    rows, cols, lds, rp, cp, ldd, ident = case.dims
    want = nanlike(rp, ldd)
    want[:, :cp] = np.eye(rp, cp) if ident else 0.0
    want[:rows, :cols] = case.ins[0]
    return want


def check_pad_copy(case, outs):
    return {"exact dst": exact(outs[0], _pad_want(case))}


def restate_pad_copy(case, defect=None):
    """defect 'identity_inside': the diagonal set to 1 inside the real block too."""
    rows, cols, lds, rp, cp, ldd, ident = case.dims
    src = with_ld(case.ins[0], lds)
    dst = nanlike(rp, ldd)
    i, j = np.meshgrid(np.arange(rp), np.arange(cp), indexing="ij")
    inside = (i < rows) & (j < cols)
    v = np.where((i == j) & bool(ident), 1.0, 0.0)
    v[inside] = src[:rows, :cols].reshape(-1)
    if defect == "identity_inside" and ident:
        v[(i == j)] = 1.0
    dst[:, :cp] = v
    return [dst]


# ====================================================================== 13: local_sum
def cases_local_sum():
    """out_i = Σ_q src_q[i] in rank order from 0.0: (n + 1)·u·Σ|src_q[i]|, and bitwise the in-order
    float64 sum (the device sum must equal the group's host path)."""
    rng = np.random.default_rng(4300)
    for n in (1, 2, 3, 64):
        for count in (1, 255, 257):
            yield Case(13, "n%d_count%d" % (n, count), (n, count), [wide(rng, n, count)], [nanlike(count)])


def check_local_sum(case, outs):
    src = case.ins[0]
    return {"finite": finite(outs[0]), "exact out": exact(outs[0], inorder(src)),
            "out": worst_ratio(outs[0], ld(src).sum(0), sum_tol(src.shape[0], 1, np.abs(ld(src)).sum(0)))}


def restate_local_sum(case, defect=None):
    return [inorder(case.ins[0])]


# ====================================================================== the table
NAMES = ("gemv", "colred", "colred_partials", "slab_sum", "sym_slab_sum", "sym_pack", "full_loo",
         "fitc_lambda", "fitc_loo", "pred_finalize", "surface_point", "dot", "pad_copy", "local_sum")
CASES = (cases_gemv, cases_colred, cases_colred_partials, cases_slab_sum, cases_sym_slab_sum, cases_sym_pack,
         cases_full_loo, cases_fitc_lambda, cases_fitc_loo, cases_pred, cases_surface, cases_dot,
         cases_pad_copy, cases_local_sum)
CHECK = (check_gemv, check_colred, check_colred_partials, check_slab_sum, check_sym_slab_sum, check_sym_pack,
         check_full_loo, check_fitc_lambda, check_fitc_loo, check_pred, check_surface, check_dot,
         check_pad_copy, check_local_sum)
RESTATE = (restate_gemv, restate_colred, restate_colred_partials, restate_slab_sum, restate_sym_slab_sum,
           restate_sym_pack, restate_full_loo, restate_fitc_lambda, restate_fitc_loo, restate_pred,
           restate_surface, restate_dot, restate_pad_copy, restate_local_sum)
# the checks whose bound is a count of one to three roundings, which plain rounding may approach
SHARP = ("mu", "var", "lam", "inv_lam", "ys")


def few_terms(case):
    """True where a sum has at most four terms (three slabs and a base): its (k + c)·u bound is
    then a count of a few roundings, as sharp as those of SHARP, and plain rounding may approach
    it."""
    w, d = case.which, case.dims
    if w == 0:
        return d[2] <= 2
    return w in (1, 2, 3, 4, 5, 11, 13) and d[0] <= 3


def check(case, outs):
    return CHECK[case.which](case, outs)


def restate(case, defect=None):
    return RESTATE[case.which](case, defect)


def large_cases():
    """n_pad = 262 272 > 1024·256 with one slab: partials_sum_kernel<4> and <2> take their
    second trip (which 6 and 7)."""
    return [case_full_loo(FIN_LARGE_N, 1), case_fitc_lambda(FIN_LARGE_N, 1, LAM_SN2[0])]


# ====================================================================== the FITC forward chain
# gps_fitc_fit at shapes ragged in both dimensions, its stages recomputed from the device's own
# Knm, λ, Lm⁻¹ and Lb⁻¹ (gps_fitc_intermediates): this checks the slab counts, offsets and operand
# choice between the kernels, which no single-launch case sees.
CHAIN_SHAPES = ((300, 37, 3), (513, 129, 8))      # (n, m, d)
CHAIN_THETA = (0.2, 0.3, -2.5)                    # log sf2, log ell (every dimension), log sn2


def chain_data(n, m, d):
    rng = np.random.default_rng(5000 + n)
    X = rng.standard_normal((n, d))
    w = rng.standard_normal(d) / math.sqrt(d)
    y = np.sin(2.0 * X @ w) + 0.1 * rng.standard_normal(n)
    Z = np.ascontiguousarray(X[rng.choice(n, m, replace=False)] + 0.05 * rng.standard_normal((m, d)))
    return X, y, Z, (CHAIN_THETA[0], CHAIN_THETA[1] * np.ones(d), CHAIN_THETA[2])


def _rowsq(K, aK, L, aL, m):
    """Row norms q_i = ‖L k_i‖² with their bound: each of the m dot products of length <= m within
    (m + 2)·u·(|L||k_i|), the m squares summed within (m + 4)·u·q (the column tiles' partials and
    their in-order sum among the additions)."""
    v, w = K @ L.T, aK @ aL.T
    dv = (m + 2) * uL * w
    q = (v * v).sum(1)
    return q, (2 * np.abs(v) * dv + dv * dv).sum(1) + (m + 4) * uL * q


def fitc_chain(y, sf2, sn2, Knm, lam, Lm_inv, Lb_inv):
    """Longdouble references and bounds of the FITC forward's outputs from the float64 stage
    arrays, every bound the same chain with absolute values and operation counts:
      λ = sf2 − q + sn2, q = ‖Lm⁻¹k_i‖²: dq (rowsq above) + 2u·(sf2 + q + sn2) — compared with the λ
        handed in, which every later stage then starts from;
      b = Knmᵀ(y/λ): (n + 4)·u·Σ_i|K_ij||y_i|/λ_i;   t = Lb⁻¹b, c = Lb⁻ᵀt: |Lb⁻¹|·(the operand's
        bound) + (m + 4)·u·|Lb⁻¹||operand| each;   g = Knm c: |Knm|·dc + (m + 4)·u·|Knm||c|;
      r = ‖Lb⁻¹k_i‖²: rowsq;   d = 1/λ − r/λ²: dr/λ² + u·(1/λ + 4r/λ² + |d|), κ = dd/|d|;
      a = (y − g)/λ: dg/λ + 3u·(|y| + |g|)/λ;
      μ = y − a/d: (da/|d| + |a/d|·κ)/(1 − κ) + 2u·(|y| + |a/d|);   σ² = 1/d: (κ + u)/(1 − κ)/|d|;
      Σ log λ, Σ y²/λ, Σ CRPS, Σ LogS: the terms' bounds (erf from the float64 libm here, within
        8u·s·(|z| + 1) of a term) and the tree's; Σ log L_ii of both factors from the inverses'
        diagonals, each within 8u (L⁻¹_ii against 1/L_ii) + 4u·|log| and the sum's (m + 2)·u;
      bᵀc: Σ(db|c| + |b|dc) + (m + 2)·u·Σ|b_j c_j|;
      logdet = Σ log λ + 2Σ log Lb_ii − 2Σ log Lm_ii and quad = Σ y²/λ − bᵀc: the parts' bounds
        plus 2u (u) of the parts' absolute sum; nlml and the two means as in full_loo."""
    need_extended()
    n, m = Knm.shape
    yl, K, Lm, Lb = ld(y), ld(Knm), ld(np.tril(Lm_inv)), ld(np.tril(Lb_inv))
    aK, aLm, aLb = np.abs(K), np.abs(Lm), np.abs(Lb)
    sf2, sn2 = LD(sf2), LD(sn2)
    q, dq = _rowsq(K, aK, Lm, aLm, m)
    ref, tol = {"lam": sf2 - q + sn2}, {"lam": dq + 2 * uL * (sf2 + q + sn2)}
    lam = ld(lam)
    ys = yl / lam
    b, ab = K.T @ ys, aK.T @ np.abs(ys)
    db = (n + 4) * uL * ab
    t, dt = Lb @ b, aLb @ db + (m + 4) * uL * (aLb @ np.abs(b))
    c, dc = Lb.T @ t, aLb.T @ dt + (m + 4) * uL * (aLb.T @ np.abs(t))
    g, dg = K @ c, aK @ dc + (m + 4) * uL * (aK @ np.abs(c))
    r, dr = _rowsq(K, aK, Lb, aLb, m)
    il = 1 / lam
    d = il - r * il * il
    kap = (dr * il * il + uL * (il + 4 * r * il * il + np.abs(d))) / np.abs(d)
    a = (yl - g) * il
    da = dg * il + 3 * uL * (np.abs(yl) + np.abs(g)) * il
    mu, var = yl - a / d, 1 / d
    dm = (da / np.abs(d) + np.abs(a / d) * kap) / (1 - kap) + 2 * uL * (np.abs(yl) + np.abs(a / d))
    dv = (kap + uL) / (1 - kap) / np.abs(d)
    ref.update(mu=mu, var=var)
    tol.update(mu=dm, var=dv)
    np_ = pad_to(n)
    s = np.sqrt(var)
    z = (a / d) / s
    erf = ld(_erf(z.astype(np.float64) * K_SQRT_HALF))
    crps, logs, tc, tl = score_terms_ref(a / d, var, erf, np.exp(-z * z / 2), dm, dv)
    tc = tc + 8 * uL * s * (np.abs(z) + 1)
    S_crps, S_logs = tree_sum_ref(crps, tc, np_), tree_sum_ref(logs, tl, np_)
    t0, t1 = np.log(lam), yl * yl * il
    S_ll, S_yy = tree_sum_ref(t0, 4 * uL * np.abs(t0), np_), tree_sum_ref(t1, 3 * uL * t1, np_)

    def logdiag(Li):
        t = -np.log(np.diag(Li))
        return t.sum(), m * 8 * uL + (4 + pad_to(m) + 2) * uL * np.abs(t).sum()

    ldm, ldb = logdiag(Lm), logdiag(Lb)
    btc = (b * c).sum(), (db * np.abs(c) + np.abs(b) * dc).sum() + (m + 2) * uL * np.abs(b * c).sum()
    logdet = S_ll[0] + 2 * ldb[0] - 2 * ldm[0]
    d_logdet = S_ll[1] + 2 * ldb[1] + 2 * ldm[1] + 2 * uL * (np.abs(S_ll[0]) + 2 * np.abs(ldb[0]) + 2 * np.abs(ldm[0]))
    quad = S_yy[0] - btc[0]
    d_quad = S_yy[1] + btc[1] + uL * (S_yy[0] + np.abs(btc[0]))
    c0 = LD(0.5) * n * np.log(2 * LD(np.pi))
    ref.update(nlml=c0 + logdet / 2 + quad / 2, loo_crps=S_crps[0] / n, loo_logs=S_logs[0] / n, logdet=logdet, quad=quad)
    tol.update(nlml=d_logdet / 2 + d_quad / 2 + 4 * uL * (c0 + np.abs(logdet) / 2 + np.abs(quad) / 2),
               loo_crps=S_crps[1] / n + uL * np.abs(ref["loo_crps"]),
               loo_logs=S_logs[1] / n + uL * np.abs(ref["loo_logs"]), logdet=d_logdet, quad=d_quad)
    return ref, tol


CHAIN_OUTPUTS = ("lam", "mu", "var", "nlml", "loo_crps", "loo_logs", "logdet", "quad")


def chain_ratios(got, ref, tol):
    """{output: worst |got − ref| / tol}; got: dict with CHAIN_OUTPUTS' names."""
    return {k: worst_ratio(got[k], ref[k], tol[k]) for k in CHAIN_OUTPUTS}
