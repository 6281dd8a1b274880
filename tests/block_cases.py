"""Cases, extended-precision references, error bounds and float64 restatements of the block-LOO,
energy-score and joint-predictive kernels (csrc/kernels_block.hip, csrc/kernels_joint.hip, and
fitc_grad_v / fitc_grad_y of csrc/kernels_fitc_grad.hip), one production launch at a time through
gps_block_diag (which 0..23, include/gpscore.h), shared by test_block_host.py (CPU: a numpy float64
restatement of each kernel meets every bound with room, every listed defect fails a named check)
and test_gpu_block.py (the kernels).  Nothing here touches the GPU or imports mpmath; DESIGN §39
has the derivations.

u = 2^-53.  References are numpy longdouble from the float64 values the kernel receives; log, pow
and (on a sample of the entries) exp come from tests/golden/blk_terms.npz (mpmath, 60 digits,
hi/lo pairs, written by tests/golden/make_block_terms.py from term_inputs() below).  Inputs are
m·2^e with m uniform on [1, 2) and e a uniform integer, so they are the same bits on every libm.

The device build contracts a*b + c, so "exact" is claimed only where the kernel does one rounding
per output or calls fma itself (the fused results come from exact rational arithmetic, _fma_sub);
everything else gets one of §30's two bound shapes — a sum of k terms, (k + c)·u·Σ|terms|, or a
count of roundings times u against the formula's terms — and each cases_* docstring states its
count.

An output comes back as its device image, [rows][ld] and the 16-double gap after it (view(),
tail()): what the kernel must leave alone is NaN there afterwards ("exact untouched").
check(case, outs) returns {check name: ratio} as in vec_cases.
"""
import math
import os

import numpy as np

from elementwise_cases import GOLDEN, LD, SUBNORMAL, U, need_extended
from grad_cases import _fma_sub, ld, wave_sum, worst_ratio
from vec_cases import exact, finite, nanlike, uL

GAP = 16
FIXTURE = os.path.join(GOLDEN, "blk_terms.npz")
LOG_2PI = 1.83787706640934548356          # the constant joint_dss_kernel carries
# worst error of pow over the fixture's D values (es_pool, β = 0.5 and 1.5) against mpmath, in ulps
# of the reference, and the allowance c = twice that, rounded up to a whole ulp (1 ulp <= 2u
# relative): numpy's pow on the host (0.646; test_block_host.py holds it to the figure) and the
# device pow on an MI355X (1.056 at β = 0.5, 1.118 at 1.5; tools/pow_probe.hip)
POW_MEASURED_ULP = {"host": 0.65, "device": 1.12}
POW_ALLOW_ULP = {k: None if v is None else math.ceil(2 * v) for k, v in POW_MEASURED_ULP.items()}
POW_WHERE = "host"                        # test_gpu_block.py sets "device"


def pow_c():
    """The pow allowance in units of u."""
    return 2 * POW_ALLOW_ULP[POW_WHERE]


def wide(rng, *shape, lo=-40, hi=40, signed=True):
    """m·2^e, m uniform on [1, 2), e a uniform integer in lo..hi, mixed signs."""
    v = np.ldexp(rng.uniform(1.0, 2.0, shape), rng.integers(lo, hi + 1, shape))
    return v * rng.choice([-1.0, 1.0], shape) if signed else v


def image(M, ldm=None):
    """The device image of a dense matrix (or vector) with row stride ldm: NaN in the row gaps
    and in the gap after it."""
    M = np.atleast_2d(np.asarray(M, np.float64))
    ldm = M.shape[1] if ldm is None else ldm
    out = nanlike(M.shape[0] * ldm + GAP)
    out[:M.shape[0] * ldm].reshape(M.shape[0], ldm)[:, :M.shape[1]] = M
    return out


def blank(rows, ldm):
    return nanlike(rows * ldm + GAP)


def view(o, rows, ldm):
    return o[:rows * ldm].reshape(rows, ldm)


def untouched(o, rows, cols, ldm):
    """0 if the row gaps and the gap after the array are still NaN."""
    ok = np.isnan(o[rows * ldm:]).all() and np.isnan(view(o, rows, ldm)[:, cols:]).all()
    return 0.0 if ok else float("inf")


def vec(o, n):
    return o[:n]


def hilo(g, key):
    return ld(g[key + "_hi"]) + ld(g[key + "_lo"])


_G = {}


def fixture():
    if not _G:
        _G.update(np.load(FIXTURE))
    return _G


class Case:
    """One gps_block_diag call: which, dims, scal, ins (dense arrays or None) and the outputs'
    first contents as device images (NaN unless the kernel reads them; None where absent)."""

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
    outs = case.fresh_outs()
    ctx.block_diag(case.which, case.dims, case.ins, outs, case.scal)
    return outs


def with_ld(M, ldm):
    out = nanlike(M.shape[0], ldm)
    out[:, :M.shape[1]] = M
    return out


def block_sum_f64(v):
    """block_sum over the last axis (a multiple of 64 threads): the butterfly per wave, then the
    waves in order."""
    w = wave_sum(v.reshape(v.shape[:-1] + (v.shape[-1] // 64, 64)))
    t = np.zeros(w.shape[:-1])
    for k in range(w.shape[-1]):
        t = t + w[..., k]
    return t


def strided_sum_f64(x, threads):
    """Thread t adds x[t], x[t + threads], ... in order from 0.0; returns the per-thread sums."""
    cnt = len(x)
    pad = np.zeros(-(-max(cnt, 1) // threads) * threads)
    pad[:cnt] = x
    v = np.zeros(threads)
    for k in range(len(pad) // threads):
        v = v + pad[threads * k:threads * (k + 1)]
    return v


# ====================================================================== 0: fold_grad
FOLD_B = (1, 15, 16, 17, 37)
# (c0, c1, c2, c3, gr, gw), H present, w present: api_block.hip's three launches
FOLD_SETS = {"es": ((0.0, 0.0, -1.0, -1.0, 0.0, 1.0), 1, 1), "dss": ((-0.5, -0.5, 0.0, 0.0, 1.0, 0.0), 0, 0),
             "kc": ((0.0, 0.0, 1.0, -1.0, 0.0, -1.0), 1, 1)}


def cases_fold_grad():
    """G_ij = c0·PI_ij + c1·r_i r_j + c2·½(w_i r_j + r_i w_j) + c3·H_ij and g_i = gr·r_i + gw·w_i.
    Longest path of G: the c2 term's four roundings (c2·½, two products and their sum, the
    scaling), then three additions: 7u·Σ|terms|.  g: two products and a sum, 3u·(|gr r| + |gw w|)."""
    rng = np.random.default_rng(6000)
    for b in FOLD_B:
        for name, (sc, hasH, hasw) in FOLD_SETS.items():
            ins = [wide(rng, b, b), wide(rng, b, b) if hasH else None, wide(rng, b, lo=-20, hi=20),
                   wide(rng, b, lo=-20, hi=20) if hasw else None]
            yield Case(0, "b%d_%s" % (b, name), (b, b + 1, b + 2, b + 3), ins, [blank(b, b + 3), blank(1, b)], sc)


def check_fold_grad(case, outs):
    b = case.dims[0]
    c0, c1, c2, c3, gr, gw = (LD(v) for v in case.scal)
    PI, H, r, w = (None if a is None else ld(a) for a in case.ins)
    T = [c0 * PI, c1 * r[:, None] * r[None, :]]
    if w is not None:
        T += [c2 * w[:, None] * r[None, :] / 2, c2 * r[:, None] * w[None, :] / 2]
    if H is not None:
        T.append(c3 * H)
    G, g = view(outs[0], b, b + 3), vec(outs[1], b)
    tg = [gr * r] + ([gw * w] if w is not None else [])
    return {"finite": finite(G[:, :b], g),
            "exact untouched": max(untouched(outs[0], b, b, b + 3), untouched(outs[1], 1, b, b)),
            "G": worst_ratio(G[:, :b], sum(T), 7 * uL * sum(np.abs(t) for t in T)),
            "g": worst_ratio(g, sum(tg), 3 * uL * sum(np.abs(t) for t in tg))}


def restate_fold_grad(case, defect=None):
    """defect 'half_missing': the c2 term without its ½; 'g_every_column': g written from the
    last column's thread with r_j in place of r_i."""
    b = case.dims[0]
    c0, c1, c2, c3, gr, gw = case.scal
    PI, H, r, w = case.ins
    PI = with_ld(PI, b + 1)[:, :b]
    v = c0 * PI + c1 * r[:, None] * r[None, :]
    if c2 != 0.0:
        v = v + c2 * (1.0 if defect == "half_missing" else 0.5) * (w[:, None] * r[None, :] + r[:, None] * w[None, :])
    if c3 != 0.0:
        v = v + c3 * with_ld(H, b + 2)[:, :b]
    rr = r[::-1] if defect == "g_every_column" else r
    g = gr * rr + (gw * w if gw != 0.0 else 0.0)
    return [image(v, b + 3), image(g)]


# ====================================================================== 1: row_dots
DOT_ROWS, DOT_COLS = (1, 3, 4, 5, 9), (2, 126, 128, 130, 258)
DOT_SETS = ("t", "B", "same_t", "B_apart")     # t only; B only; B = A with t (423); B != A (454)


def cases_row_dots():
    """at_i = Σ_k A_ik t_k, ab_i = Σ_k A_ik B_ik, one wave per row, lane l taking the column pairs
    2l + 128·trip in order, then the butterfly.  Bound per row: (cols + 2)·u·Σ|a||b|."""
    rng = np.random.default_rng(6100)
    for i, rows in enumerate(DOT_ROWS):
        for j, cols in enumerate(DOT_COLS):
            kind = DOT_SETS[(i + j) % 4]
            lda = cols + (6 if (i + j) % 2 else 0)
            A = wide(rng, rows, cols, lo=-20, hi=20)
            B = wide(rng, rows, cols, lo=-20, hi=20) if kind in ("B", "B_apart") else None
            t = wide(rng, cols, lo=-20, hi=20) if kind in ("t", "same_t") else None
            same = kind == "same_t"
            yield Case(1, "%dx%d_ld%d_%s" % (rows, cols, lda, kind), (rows, cols, lda, lda if same else cols + 2, same),
                       [A, B, t], [blank(1, rows) if t is not None else None,
                                   blank(1, rows) if (B is not None or same) else None])


def _dots_ops(case):
    A, B, t = case.ins
    return A, (A if case.dims[4] else B), t


def check_row_dots(case, outs):
    rows, cols = case.dims[:2]
    A, B, t = _dots_ops(case)
    res = {"finite": finite(*[vec(o, rows) for o in outs if o is not None]),
           "exact untouched": max(untouched(o, 1, rows, rows) for o in outs if o is not None)}
    for name, o, other in (("at", outs[0], None if t is None else ld(t)[None, :]), ("ab", outs[1], None if B is None else ld(B))):
        if o is not None:
            P = ld(A) * other
            res[name] = worst_ratio(vec(o, rows), P.sum(1), (cols + 2) * uL * np.abs(P).sum(1))
    return res


def restate_row_dots(case, defect=None):
    """defect 'stride_short': the loop one 128-stride short."""
    rows, cols, lda, ldb = case.dims[:4]
    A, B, t = _dots_ops(case)
    A = with_ld(A, lda)
    B = None if B is None else (A if case.dims[4] else with_ld(B, ldb))
    trips = -(-cols // 128) - (1 if defect == "stride_short" else 0)
    outs = []
    for other in (None if t is None else np.broadcast_to(t, (rows, cols)), B):
        if other is None:
            outs.append(None)
            continue
        acc = np.zeros((rows, 64))
        for trip in range(trips):
            for half in (0, 1):
                k = 128 * trip + 2 * np.arange(64) + half
                on = (k - half) < cols
                kc = np.minimum(k, A.shape[1] - 1)
                oc = np.minimum(k, other.shape[1] - 1)
                acc = np.where(on[None, :], A[:, kc] * other[:, oc] + acc, acc)
        outs.append(image(wave_sum(acc)))
    return outs


# ====================================================================== 2: lr_fold_vec
LRV_SHAPES = ((1, 1), (1, 128), (255, 256), (256, 256), (257, 384))     # (b, bp)


def cases_lr_fold_vec():
    """Mode 0: o1 = fma(λ, x, at), o2 = λ + ab and mode 1: o1 alone (o2 NULL): one rounding each,
    exact.  Mode 2: o1 = w·r − (λ²gc + 2λ·gc·(c − λ) + q) within 8u·(|wr| + λ²|gc| + 2λ|gc||c − λ| +
    |q|) (the longest path: 2λ·gc·(c − λ) has four roundings, then three additions, one more for
    the second order), o2 = −w exact; rows with c − λ down to 2^-40·λ among them.  Mode 3:
    o1 = −½(c + r²) within 3u·(|c| + r²)/2, o2 = r exact.  Rows b..bp-1 are exactly 0."""
    rng = np.random.default_rng(6200)
    for mode in range(4):
        for b, bp in LRV_SHAPES:
            lam = wide(rng, b, lo=-20, hi=20, signed=False)
            v = [lam] + [None] * 8
            if mode < 2:
                v[1], v[2] = wide(rng, b), wide(rng, b)
                if mode == 0:
                    v[3] = wide(rng, b, lo=-20, hi=20, signed=False)
            else:
                c = wide(rng, b, lo=-20, hi=20, signed=False)
                near = np.arange(b) % 3 == 0
                c[near] = lam[near] * (1.0 + np.ldexp(1.0, -(np.arange(b)[near] % 41)))
                v[4], v[5] = wide(rng, b, lo=-20, hi=20), c
                if mode == 2:
                    v[6], v[7], v[8] = wide(rng, b, lo=-20, hi=20), wide(rng, b, lo=-20, hi=20), wide(rng, b)
            yield Case(2, "mode%d_b%d_bp%d" % (mode, b, bp), (mode, b, bp), v,
                       [blank(1, bp), None if mode == 1 else blank(1, bp)])


def check_lr_fold_vec(case, outs):
    mode, b, bp = case.dims
    lam, x, at, ab, r, c, w, gc, q = case.ins
    o1 = vec(outs[0], bp)
    o2 = None if outs[1] is None else vec(outs[1], bp)
    res = {"finite": finite(o1, *([] if o2 is None else [o2])),
           "exact untouched": max(untouched(o, 1, bp, bp) for o in outs if o is not None),
           "exact pads": max(exact(o[b:], np.zeros(bp - b)) for o in (o1, o2) if o is not None)}
    if mode < 2:
        res["exact o1"] = exact(o1[:b], _fma_sub(lam, x, -at))
        if mode == 0:
            res["exact o2"] = exact(o2[:b], lam + ab)
    elif mode == 2:
        l, g = ld(lam), ld(gc)
        T = [ld(w) * ld(r), l * l * g, 2 * l * g * (ld(c) - l), ld(q)]
        res["o1 kc"] = worst_ratio(o1[:b], T[0] - (T[1] + T[2] + T[3]), 8 * uL * sum(np.abs(t) for t in T))
        res["exact o2"] = exact(o2[:b], -w)
    else:
        res["o1 dss"] = worst_ratio(o1[:b], -(ld(c) + ld(r) * ld(r)) / 2, 3 * uL * (ld(c) + ld(r) * ld(r)) / 2)
        res["exact o2"] = exact(o2[:b], r)
    return res


def restate_lr_fold_vec(case, defect=None):
    """defect 'pads_unwritten': rows >= b left as they were; 'no_two': mode 2 without the 2."""
    mode, b, bp = case.dims
    lam, x, at, ab, r, c, w, gc, q = case.ins
    pad = np.nan if defect == "pads_unwritten" else 0.0
    o1, o2 = np.full(bp, pad), np.full(bp, pad)
    if mode < 2:
        o1[:b] = _fma_sub(lam, x, -at)
        if mode == 0:
            o2[:b] = lam + ab
    elif mode == 2:
        two = 1.0 if defect == "no_two" else 2.0
        o1[:b] = w * r - (lam * lam * gc + two * lam * gc * (c - lam) + q)
        o2[:b] = -w
    else:
        o1[:b] = -0.5 * (c + r * r)
        o2[:b] = r
    return [image(o1), None if mode == 1 else image(o2)]


# ====================================================================== 3: lr_combine
LRC_SHAPES = ((1, 1, 2), (5, 8, 3), (37, 128, 20), (129, 256, 130))     # (rows, rows_pad, cols)
# (c0, c1, c2), rs, first and second rank-one term present: api_block.hip:435, 446, 450
LRC_SETS = {"dss": ((-0.5, -0.5, 0.0), 0, 1, 0), "x2": ((1.0, 0.0, 0.0), 1, 0, 0), "kc": ((-1.0, 0.5, 0.5), 0, 1, 1)}


def cases_lr_combine():
    """out_ij = rs_i·c0·(X_ij + λ_i Y_ij) + c1·u1_i v1_j + c2·u2_i v2_j.  The X term passes through
    the fma, the two scalings and the two rank-one fmas (five roundings), one more for the second
    order: 6u·Σ|terms|.  Rows rows..rows_pad-1 exactly 0."""
    rng = np.random.default_rng(6300)
    for rows, rp, cols in LRC_SHAPES:
        for k, (name, (sc, rs, t1, t2)) in enumerate(LRC_SETS.items()):
            w = lambda *s: wide(rng, *s, lo=-20, hi=20)
            ins = [w(rows, cols), w(rows, cols), wide(rng, rows, lo=-20, hi=20, signed=False), w(rows) if rs else None,
                   w(rows) if t1 else None, w(cols) if t1 else None, w(rows) if t2 else None, w(cols) if t2 else None]
            yield Case(3, "%d_%dx%d_%s" % (rows, rp, cols, name), (rows, rp, cols, cols + 1, cols + 2, cols + 3 + k),
                       ins, [blank(rp, cols + 3 + k)], sc)


def check_lr_combine(case, outs):
    rows, rp, cols, _, _, ldo = case.dims
    X, Y, lam, rs, u1, v1, u2, v2 = (None if a is None else ld(a) for a in case.ins)
    c0, c1, c2 = (LD(v) for v in case.scal)
    s = c0 * (rs[:, None] if rs is not None else LD(1))
    T = [s * X, s * lam[:, None] * Y]
    if u1 is not None:
        T.append(c1 * u1[:, None] * v1[None, :])
    if u2 is not None:
        T.append(c2 * u2[:, None] * v2[None, :])
    o = view(outs[0], rp, ldo)
    return {"finite": finite(o[:, :cols]), "exact untouched": untouched(outs[0], rp, cols, ldo),
            "exact pads": exact(o[rows:, :cols], np.zeros((rp - rows, cols))),
            "out": worst_ratio(o[:rows, :cols], sum(T), 6 * uL * sum(np.abs(t) for t in T))}


def restate_lr_combine(case, defect=None):
    """defect 'pads_unwritten'; 'rs_skipped': the row scale left out."""
    rows, rp, cols, ldx, ldy, ldo = case.dims
    X, Y, lam, rs, u1, v1, u2, v2 = case.ins
    c0, c1, c2 = case.scal
    v = c0 * (lam[:, None] * with_ld(Y, ldy)[:, :cols] + with_ld(X, ldx)[:, :cols])
    if rs is not None and defect != "rs_skipped":
        v = v * rs[:, None]
    if u1 is not None:
        v = (c1 * u1)[:, None] * v1[None, :] + v
    if u2 is not None:
        v = (c2 * u2)[:, None] * v2[None, :] + v
    out = np.full((rp, cols), np.nan if defect == "pads_unwritten" else 0.0)
    out[:rows] = v
    return [image(out, ldo)]


# ====================================================================== 4: fold_sum
FS_NSLAB, FS_LEN = (1, 4, 9), (1, 255, 256, 257)


def cases_fold_sum():
    """dst = base (+ base2) + sgn·Σ_{g != skip} slab_g in slab order: with sgn = ±1 every step is
    one rounded addition, so the result is the in-order float64 sum bit for bit.  The slab past
    the real ones is NaN on the device, and so is the skipped slab."""
    rng = np.random.default_rng(6400)
    k = 0
    for ns in FS_NSLAB:
        for skip in sorted({-1, 0, ns // 2, ns - 1}):
            for ln in FS_LEN:
                k += 1
                slab = wide(rng, ns, ln)
                if skip >= 0:
                    slab[skip] = np.nan
                base = wide(rng, ln) if k % 3 else None
                base2 = wide(rng, ln) if k % 4 == 1 else None
                inplace = base is not None and k % 2 == 0
                sgn = -1.0 if k % 5 < 2 else 1.0
                name = "ns%d_skip%d_len%d%s%s%s_%s" % (ns, skip, ln, "_base" if base is not None else "",
                                                       "_base2" if base2 is not None else "", "_inplace" if inplace else "",
                                                       "minus" if sgn < 0 else "plus")
                yield Case(4, name, (ns, skip, ln, ln + 3, inplace), [slab, None if inplace else base, base2],
                           [image(base) if inplace else blank(1, ln)], (sgn,), base=base)


def _fold_sum_f64(case, skip):
    ns, _, ln = case.dims[:3]
    slab = np.vstack([case.ins[0], nanlike(1, ln)])      # the NaN slab past the real ones
    v = np.zeros(ln) if case.base is None else case.base.copy()
    if case.ins[2] is not None:
        v = v + case.ins[2]
    for g in range(ns):
        if g != skip:
            v = v + case.scal[0] * slab[g]
    return v


def check_fold_sum(case, outs):
    ln = case.dims[2]
    return {"finite": finite(vec(outs[0], ln)), "exact untouched": untouched(outs[0], 1, ln, ln),
            "exact dst": exact(vec(outs[0], ln), _fold_sum_f64(case, case.dims[1]))}


def restate_fold_sum(case, defect=None):
    """defect 'skip_off_by_one': slab skip + 1 is left out in place of slab skip."""
    return [image(_fold_sum_f64(case, case.dims[1] + (1 if defect == "skip_off_by_one" else 0)))]


# ====================================================================== 5: fold_logdet
FL_M, FL_B = (1, 20, 255, 257), (1, 125, 256, 300)
FL_POOL = 300


def logdet_lam():
    return wide(np.random.default_rng(6501), FL_POOL, lo=-20, hi=20, signed=False)


def cases_fold_logdet():
    """out = Σ_{i<m}(ldf_i − ldb_i) − ½Σ_{i<b} log λ_i, thread t adding its strided terms in order,
    then block_sum of 256 (6 butterfly levels, 4 waves): depth ⌈m/256⌉ + ⌈b/256⌉ + 10, so
    (depth + 1)·u·Σ|terms| on top of the terms' own u·|ldf − ldb| and 2 ulp = 4u·|½ log λ| (§30's
    figure for the device log)."""
    rng = np.random.default_rng(6500)
    lam = logdet_lam()
    for m in FL_M:
        for b in FL_B:
            yield Case(5, "m%d_b%d" % (m, b), (m, b), [wide(rng, m, lo=-10, hi=10), wide(rng, m, lo=-10, hi=10), lam[:b]],
                       [blank(1, 1)])


def check_fold_logdet(case, outs):
    m, b = case.dims
    ldf, ldb, _ = (ld(a) for a in case.ins)
    t0, t1 = ldf - ldb, hilo(fixture(), "log")[:b] / 2
    depth = -(-m // 256) + -(-b // 256) + 10
    tot = np.abs(t0).sum() + np.abs(t1).sum()
    tol = uL * np.abs(t0).sum() + 4 * uL * np.abs(t1).sum() + (depth + 1) * uL * tot
    return {"finite": finite(outs[0][:1]), "exact untouched": untouched(outs[0], 1, 1, 1),
            "out": worst_ratio(outs[0][:1], (t0.sum() - t1.sum()).reshape(1), tol)}


def restate_fold_logdet(case, defect=None):
    """defect 'lam_to_m': the log λ loop runs to m in place of b; 'no_half'."""
    m, b = case.dims
    ldf, ldb, lam = case.ins
    nb = m if defect == "lam_to_m" else b
    lam_dev = np.concatenate([lam, nanlike(GAP)])        # what lies past λ on the device
    h = 1.0 if defect == "no_half" else 0.5
    v = strided_sum_f64(ldf - ldb, 256)
    lg = np.concatenate([lam_dev, nanlike(max(0, nb - len(lam_dev)))])[:nb]
    nt = -(-max(nb, 1) // 256) * 256
    pad = np.zeros(nt)
    pad[:nb] = h * np.log(lg)
    for k in range(nt // 256):
        v = v - pad[256 * k:256 * (k + 1)]
    return [image(block_sum_f64(v))]


# ====================================================================== the one-rounding kernels
VEC_N = (1, 255, 256, 257)
MAT_N = (1, 2, 17, 128, 130)


def cases_row_scale():
    """M_ij *= scale_i (cols even): one rounding, exact; the row gaps stay NaN."""
    rng = np.random.default_rng(6600)
    for n in MAT_N:
        cols = n + (n & 1)
        yield Case(6, "%dx%d" % (n, cols), (n, cols, cols + 2), [wide(rng, n, lo=-20, hi=20)],
                   [image(wide(rng, n, cols), cols + 2)])


def _inout(case, q=0):
    rows, cols, ldm = case.shape
    return view(case.outs0[q], rows, ldm)[:, :cols].copy()


def _one(case, outs, want, rows, cols, ldm, name="exact out"):
    o = view(outs[0], rows, ldm)[:, :cols]
    return {"finite": finite(o), "exact untouched": untouched(outs[0], rows, cols, ldm), name: exact(o, want)}


def check_row_scale(case, outs):
    n, cols, ldm = case.dims
    M = view(case.outs0[0], n, ldm)[:, :cols]
    return _one(case, outs, M * case.ins[0][:, None], n, cols, ldm)


def restate_row_scale(case, defect=None):
    """defect 'scale_by_pair': the scale indexed by the pair, not the row."""
    n, cols, ldm = case.dims
    M = view(case.outs0[0], n, ldm)[:, :cols]
    s = case.ins[0]
    sc = s[(np.arange(n * cols) // 2 % n).reshape(n, cols)] if defect == "scale_by_pair" else s[:, None]
    return [image(M * sc, ldm)]


def cases_vec_mul():
    """out_i = a_i·b_i: exact."""
    rng = np.random.default_rng(6700)
    for n in VEC_N:
        yield Case(7, "n%d" % n, (n,), [wide(rng, n), wide(rng, n)], [blank(1, n)])


def check_vec_mul(case, outs):
    n = case.dims[0]
    return _one(case, outs, (case.ins[0] * case.ins[1])[None, :], 1, n, n)


def restate_vec_mul(case, defect=None):
    """defect 'last_missing': i < n − 1."""
    v = case.ins[0] * case.ins[1]
    if defect == "last_missing":
        v[-1] = np.nan
    return [image(v)]


NS_INIT_SHAPES = ((1, 64), (63, 64), (64, 64), (65, 128))


def cases_ns_init():
    """Y = diag(scale·C_b, pad·I), scale·I for C NULL: one rounding, exact."""
    rng = np.random.default_rng(6800)
    for b, bp in NS_INIT_SHAPES:
        for hasC in (1, 0):
            for pad in (0.0, 1.0):
                yield Case(9, "b%d_bp%d_%s_pad%d" % (b, bp, "C" if hasC else "noC", pad), (b, bp, b + 2),
                           [wide(rng, b, b) if hasC else None], [blank(bp, bp)], (1.75, pad))


def _ns_init_want(case, defect=None):
    b, bp, _ = case.dims
    scale, pad = case.scal
    Y = np.zeros((bp, bp))
    Y[np.arange(bp), np.arange(bp)] = pad
    Y[:b, :b] = scale * case.ins[0] if case.ins[0] is not None else scale * np.eye(b)
    if defect == "pad_from_b_plus_1" and b < bp:
        Y[b, b] = 0.0 if case.ins[0] is not None else scale
    return Y


def check_ns_init(case, outs):
    bp = case.dims[1]
    return _one(case, outs, _ns_init_want(case), bp, bp, bp)


def restate_ns_init(case, defect=None):
    """defect 'pad_from_b_plus_1': row b treated as a real row."""
    return [image(_ns_init_want(case, defect))]


def cases_diag_add_const():
    """M_ii += c: exact; the off-diagonal entries (NaN going in) and the row gaps stay NaN."""
    rng = np.random.default_rng(6900)
    for n in MAT_N:
        M = nanlike(n, n)
        M[np.arange(n), np.arange(n)] = wide(rng, n, lo=-4, hi=4)
        yield Case(10, "n%d" % n, (n, n + 2), [], [image(M, n + 2)], (0.3,))


def _diag_want(case, defect=None):
    n, ldm = case.dims
    M = view(case.outs0[0], n, ldm)[:, :n].copy()
    i = np.arange(n)
    if defect == "ld_is_n":                   # i·n + i in place of i·ld + i
        flat = view(case.outs0[0], n, ldm).copy().reshape(-1)
        flat[i * n + i] += case.scal[0]
        return flat.reshape(n, ldm)[:, :n]
    M[i, i] += case.scal[0]
    return M


def check_diag_add_const(case, outs):
    n, ldm = case.dims
    o = view(outs[0], n, ldm)[:, :n]
    return {"finite": finite(np.diag(o)), "exact untouched": untouched(outs[0], n, n, ldm),
            "exact out": exact(o, _diag_want(case))}


def restate_diag_add_const(case, defect=None):
    return [image(_diag_want(case, defect), case.dims[1])]


def cases_sym_avg():
    """M ← ½(M + Mᵀ): one rounded addition and an exact halving per pair, the diagonal as it was."""
    rng = np.random.default_rng(7000)
    for n in MAT_N:
        yield Case(11, "n%d" % n, (n, n + 2), [], [image(wide(rng, n, n, lo=-20, hi=20), n + 2)])


def _sym_want(case, defect=None):
    n, ldm = case.dims
    M = view(case.outs0[0], n, ldm)[:, :n]
    A = 0.5 * (M + M.T)
    A[np.arange(n), np.arange(n)] = np.diag(M)
    if defect == "lower_only":
        A = np.where(np.arange(n)[:, None] >= np.arange(n)[None, :], A, M)
    return A


def check_sym_avg(case, outs):
    n, ldm = case.dims
    return _one(case, outs, _sym_want(case), n, n, ldm)


def restate_sym_avg(case, defect=None):
    """defect 'lower_only': the upper entry not written."""
    return [image(_sym_want(case, defect), case.dims[1])]


def cases_scaled_row():
    """dst_j = scale·src_j (j < b), 0 (b <= j < bp): exact."""
    rng = np.random.default_rng(7100)
    for k, b in enumerate(VEC_N):
        bp = b + (0, 1, 128, 127)[k]
        yield Case(12, "b%d_bp%d" % (b, bp), (b, bp), [wide(rng, b)], [blank(1, bp)], (-1.3,))


def _padded(v, bp, defect):
    out = np.full(bp, np.nan if defect == "pads_unwritten" else 0.0)
    out[:len(v)] = v
    return out


def check_scaled_row(case, outs):
    b, bp = case.dims
    return _one(case, outs, _padded(case.scal[0] * case.ins[0], bp, None)[None, :], 1, bp, bp)


def restate_scaled_row(case, defect=None):
    """defect 'pads_unwritten'."""
    return [image(_padded(case.scal[0] * case.ins[0], case.dims[1], defect))]


def cases_joint_resid():
    """r_i = y_i − mu_i (i < b), 0 on the padding: exact."""
    rng = np.random.default_rng(7200)
    for k, b in enumerate(VEC_N):
        bp = b + (127, 1, 0, 127)[k]
        yield Case(18, "b%d_bp%d" % (b, bp), (b, bp), [wide(rng, b), wide(rng, b)], [blank(1, bp)])


def check_joint_resid(case, outs):
    b, bp = case.dims
    return _one(case, outs, _padded(case.ins[0] - case.ins[1], bp, None)[None, :], 1, bp, bp)


def restate_joint_resid(case, defect=None):
    """defect 'pads_unwritten'."""
    return [image(_padded(case.ins[0] - case.ins[1], case.dims[1], defect))]


def cases_sign_fill():
    """dst_i = +1 (i < npos), −1 (npos <= i < n): exact."""
    for n in VEC_N:
        for npos in sorted({0, n // 2, n}):
            yield Case(20, "npos%d_n%d" % (npos, n), (npos, n), [], [blank(1, n)])


def _sign_want(case, defect=None):
    npos, n = case.dims
    return np.where(np.arange(n) < npos + (1 if defect == "le" else 0), 1.0, -1.0)


def check_sign_fill(case, outs):
    return _one(case, outs, _sign_want(case)[None, :], 1, case.dims[1], case.dims[1])


def restate_sign_fill(case, defect=None):
    """defect 'le': i <= npos."""
    return [image(_sign_want(case, defect))]


def cases_row_add():
    """M_ij += mu_j: exact."""
    rng = np.random.default_rng(7300)
    for n in MAT_N:
        rows = n + 1 if n == 17 else n
        yield Case(21, "%dx%d" % (rows, n), (rows, n, n + 2), [wide(rng, n)], [image(wide(rng, rows, n), n + 2)])


def _row_add_want(case, defect=None):
    rows, cols, ldm = case.dims
    M = view(case.outs0[0], rows, ldm)[:, :cols]
    mu = case.ins[0]
    return M + (mu[np.arange(rows) % cols][:, None] if defect == "mu_by_row" else mu[None, :])


def check_row_add(case, outs):
    rows, cols, ldm = case.dims
    return _one(case, outs, _row_add_want(case), rows, cols, ldm)


def restate_row_add(case, defect=None):
    """defect 'mu_by_row': mu indexed by the row."""
    return [image(_row_add_want(case, defect), case.dims[2])]


def cases_fitc_grad_v():
    """v = ulam − z/λ, or ulam − z with λ NULL: a division and a subtraction, nothing to contract:
    exact."""
    rng = np.random.default_rng(7400)
    for n in VEC_N:
        for has in (1, 0):
            yield Case(22, "n%d_%s" % (n, "lam" if has else "nolam"), (n,),
                       [wide(rng, n), wide(rng, n), wide(rng, n, lo=-20, hi=20, signed=False) if has else None],
                       [blank(1, n)])


def _grad_v_want(case, defect=None):
    ulam, z, lam = case.ins
    if lam is None:
        return ulam - z
    return ulam - (z * (1.0 / lam) if defect == "reciprocal" else z / lam)


def check_fitc_grad_v(case, outs):
    n = case.dims[0]
    return _one(case, outs, _grad_v_want(case)[None, :], 1, n, n)


def restate_fitc_grad_v(case, defect=None):
    """defect 'reciprocal': z·(1/λ) in place of z/λ (two roundings where the kernel has one)."""
    return [image(_grad_v_want(case, defect))]


# ====================================================================== 13: row_axpy, 23: fitc_grad_y
AXPY_SHAPES = ((1, 2), (5, 64), (17, 66), (129, 130))


def cases_row_axpy():
    """C_ij = fma(s_i, Z_ij, C_ij): exact."""
    rng = np.random.default_rng(7500)
    for rows, cols in AXPY_SHAPES:
        yield Case(13, "%dx%d" % (rows, cols), (rows, cols, cols + 2, cols + 4),
                   [wide(rng, rows, cols, lo=-20, hi=20), wide(rng, rows, lo=-20, hi=20)],
                   [image(wide(rng, rows, cols), cols + 2)])


def _axpy_want(case, defect=None):
    rows, cols, ldc, _ = case.dims
    C = view(case.outs0[0], rows, ldc)[:, :cols]
    Z, sv = case.ins
    if defect == "two_roundings":
        return sv[:, None] * Z + C
    return _fma_sub(Z, sv[:, None], -C)


def check_row_axpy(case, outs):
    rows, cols, ldc, _ = case.dims
    return _one(case, outs, _axpy_want(case), rows, cols, ldc)


def restate_row_axpy(case, defect=None):
    """defect 'two_roundings': the product rounded before the sum."""
    return [image(_axpy_want(case, defect), case.dims[2])]


def cases_fitc_grad_y():
    """Y = diag(s1)·U (UP NULL: one rounding, exact), + diag(s2)·UP (two roundings:
    2u·(|s1 U| + |s2 UP|)); UP distinct and UP == Y."""
    rng = np.random.default_rng(7600)
    for rows, cols in AXPY_SHAPES:
        for kind in ("noup", "up", "alias"):
            w = lambda *s: wide(rng, *s, lo=-20, hi=20)
            UP = None if kind == "noup" else w(rows, cols)
            ldm = cols + 2
            yield Case(23, "%dx%d_%s" % (rows, cols, kind), (rows, cols, ldm, kind == "alias"),
                       [w(rows, cols), UP if kind == "up" else None, w(rows), None if kind == "noup" else w(rows)],
                       [image(UP, ldm) if kind == "alias" else blank(rows, ldm)], UP=UP)


def check_fitc_grad_y(case, outs):
    rows, cols, ldm, _ = case.dims
    U_, _, s1, s2 = case.ins
    o = view(outs[0], rows, ldm)[:, :cols]
    res = {"finite": finite(o), "exact untouched": untouched(outs[0], rows, cols, ldm)}
    if case.UP is None:
        res["exact Y"] = exact(o, s1[:, None] * U_)
    else:
        T = [ld(s1)[:, None] * ld(U_), ld(s2)[:, None] * ld(case.UP)]
        res["Y"] = worst_ratio(o, T[0] + T[1], 2 * uL * (np.abs(T[0]) + np.abs(T[1])))
    return res


def restate_fitc_grad_y(case, defect=None):
    """defect 's1_for_both': s1 scales UP too."""
    U_, _, s1, s2 = case.ins
    y = s1[:, None] * U_
    if case.UP is not None:
        y = _fma_sub(case.UP, (s1 if defect == "s1_for_both" else s2)[:, None], -y)
    return [image(y, case.dims[2])]


# ====================================================================== 8: blk_mdiag
MD_N, MD_MPAD = ((1, 4), (5, 8), (6, 6), (130, 256)), (2, 126, 128, 130, 258)


def cases_blk_mdiag():
    """p_i = Σ_j F_ij U_ij, q_i = Σ_j US_ij U_ij (one wave per row, the lanes' column pairs in
    order, then the butterfly: (m_pad + 2)·u·Σ|terms| each), md = −gd/λ² + 2p/λ − q − vα with λ over
    2^±20: the reciprocal enters the first term twice and the second once, with their products at
    most four roundings a term, three additions, one more for the second order: 8u·Σ|terms|, plus
    the dots' (m_pad + 2)·u·(2Σ|F U|/λ + Σ|US U|); sc = −2·md exactly; Y = fma(−2/λ, F, 2·US): two
    roundings, 2u·(|2F/λ| + |2US|).  Pad rows: md = sc = 0 and the row of Y 0, exactly.  Y over US
    (production) and apart."""
    rng = np.random.default_rng(7700)
    k = 0
    for n, n_pad in MD_N:
        for m_pad in MD_MPAD:
            k += 1
            alias = k % 2
            w = lambda *s: wide(rng, *s, lo=-20, hi=20)
            lds = (m_pad + 2, m_pad + 4, m_pad + 6, m_pad + 4 if alias else m_pad + 8)
            US = w(n, m_pad)
            Y0 = blank(n_pad, lds[3])
            if alias:
                view(Y0, n_pad, lds[3])[:n, :m_pad] = US
            yield Case(8, "n%d_pad%d_m%d_%s" % (n, n_pad, m_pad, "alias" if alias else "apart"),
                       (n, n_pad, m_pad) + lds + (alias,),
                       [w(n, m_pad), None if alias else US, w(n, m_pad), w(n), wide(rng, n, lo=-20, hi=20, signed=False),
                        w(n), w(n)], [blank(1, n_pad), blank(1, n_pad), Y0], US=US)


def check_blk_mdiag(case, outs):
    n, n_pad, m_pad = case.dims[:3]
    ldy = case.dims[6]
    F, _, U_, gd, lam, v, al = (None if a is None else ld(a) for a in case.ins)
    US = ld(case.US)
    il = 1 / lam
    p, q, pa, qa = (F * U_).sum(1), (US * U_).sum(1), np.abs(F * U_).sum(1), np.abs(US * U_).sum(1)
    T = [gd * il * il, 2 * p * il, q, v * al]
    ref = -T[0] + T[1] - T[2] - T[3]
    tol = uL * (8 * sum(np.abs(t) for t in T) + (m_pad + 2) * (2 * pa * il + qa))
    md, sc, Y = vec(outs[0], n_pad), vec(outs[1], n_pad), view(outs[2], n_pad, ldy)
    TY = [2 * F * il[:, None], 2 * US]
    return {"finite": finite(md, sc, Y[:, :m_pad]),
            "exact untouched": max(untouched(outs[0], 1, n_pad, n_pad), untouched(outs[1], 1, n_pad, n_pad),
                                   untouched(outs[2], n_pad, m_pad, ldy)),
            "exact pads": max(exact(md[n:], np.zeros(n_pad - n)), exact(sc[n:], np.zeros(n_pad - n)),
                              exact(Y[n:, :m_pad], np.zeros((n_pad - n, m_pad)))),
            "exact sc": exact(sc[:n], -2.0 * md[:n]),
            "md": worst_ratio(md[:n], ref, tol),
            "Y": worst_ratio(Y[:n, :m_pad], TY[1] - TY[0], 2 * uL * (np.abs(TY[0]) + np.abs(TY[1])))}


def restate_blk_mdiag(case, defect=None):
    """defect 'pads_kept': the pad rows of Y left as they were; 'p_once': 2p/λ without the 2."""
    n, n_pad, m_pad = case.dims[:3]
    ldy = case.dims[6]
    F, _, U_, gd, lam, v, al = case.ins
    US = case.US
    il = 1.0 / lam
    accp, accq = np.zeros((n, 64)), np.zeros((n, 64))
    for j0 in range(0, m_pad, 128):
        for half in (0, 1):
            j = j0 + 2 * np.arange(64) + half
            on = (j - half) < m_pad
            jc = np.minimum(j, m_pad - 1)
            accp = np.where(on[None, :], F[:, jc] * U_[:, jc] + accp, accp)
            accq = np.where(on[None, :], US[:, jc] * U_[:, jc] + accq, accq)
    p, q = wave_sum(accp), wave_sum(accq)
    mi = -gd * il * il + (1.0 if defect == "p_once" else 2.0) * p * il - q - v * al
    md, sc = np.zeros(n_pad), np.zeros(n_pad)
    md[:n], sc[:n] = mi, -2.0 * mi
    Y = view(case.outs0[2].copy(), n_pad, ldy)[:, :m_pad] if defect == "pads_kept" else np.zeros((n_pad, m_pad))
    Y[:n] = _fma_sub(F, (-2.0 * il)[:, None], -2.0 * US)
    return [image(md), image(sc), image(Y, ldy)]


# ====================================================================== 14: ns_resid
NSR_N = (1, 31, 32, 33, 128)
NSR_THRESHOLD = 1e-24          # gps_energy_score compares the residual with 1e-24·bp


def cases_ns_resid():
    """out = Σ_ij (T_ij − δ_ij)² with T = I + E, thread t adding its ⌈n²/1024⌉ squares in order,
    then block_sum of 1024 (6 + 16).  All terms >= 0, so relative: (⌈n²/1024⌉ + 22 + 3)·u (the
    subtraction, the square and one for the second order).  |E| ~ 2^U(−50, −30), one case |E| ~ 1,
    and ‖E‖²_F placed a factor 1.7 below and above 1e-24·n, where the verdict of the convergence
    test must be the reference's."""
    rng = np.random.default_rng(7800)
    for k, n in enumerate(NSR_N):
        kinds = ("small", "below", "above") + (("unit",) if n == 33 else ())
        for kind in kinds:
            E = wide(rng, n, n, lo=-50, hi=-30) if kind != "unit" else wide(rng, n, n, lo=-2, hi=0)
            if kind in ("below", "above"):
                target = NSR_THRESHOLD * n * (1.7 if kind == "above" else 1 / 1.7)
                E = E * math.sqrt(target / float((E * E).sum()))
            ldm = n + (2 if k % 2 else 0)
            yield Case(14, "n%d_ld%d_%s" % (n, ldm, kind), (n, ldm), [np.eye(n) + E], [blank(1, 1)], kind=kind)


def _resid_ref(case):
    n = case.dims[0]
    D = ld(case.ins[0]) - np.eye(n).astype(LD)
    return (D * D).sum()


def check_ns_resid(case, outs):
    n = case.dims[0]
    ref = _resid_ref(case)
    got = outs[0][0]
    thr = NSR_THRESHOLD * n
    return {"finite": finite(outs[0][:1]), "exact untouched": untouched(outs[0], 1, 1, 1),
            "exact verdict": 0.0 if (got <= thr) == (ref <= thr) else float("inf"),
            "out": worst_ratio(outs[0][:1], ref.reshape(1), (-(-n * n // 1024) + 25) * uL * ref)}


def restate_ns_resid(case, defect=None):
    """defect 'no_delta': Σ T_ij²; 'ld_is_n'."""
    n, ldm = case.dims
    T = with_ld(case.ins[0], ldm)
    D = (T.reshape(-1)[:n * n].reshape(n, n) if defect == "ld_is_n" else T[:, :n]) - (0.0 if defect == "no_delta" else np.eye(n))
    return [image(block_sum_f64(strided_sum_f64((D * D).reshape(-1), 1024)))]


# ====================================================================== 15: es_dist
ESD_S, ESD_BP = (2, 15, 16, 17, 33), (64, 128, 192)


def cases_es_dist():
    """D_ij = ‖z_i − ẑ_j‖ for i < S, j <= S over rows of length bp (zero past b): a subtraction, a
    square and an addition per coordinate, then the square root.  All terms >= 0; relative bound
    ((bp + 3)/2 + 1)·u on D (bp + 3 roundings under the root, halved by it, and the root's own).
    ẑ_1 is z_0 but for one ulp of one coordinate, ẑ_2 is z_1 but for 2^-40 relative of one.
    Everything outside i < S, j <= S stays NaN."""
    rng = np.random.default_rng(7900)
    for S in ESD_S:
        for bp in ESD_BP:
            b = bp - (0 if bp == 64 else 5)
            Z, Zh = np.zeros((S, bp)), np.zeros((S + 1, bp))
            Z[:, :b], Zh[:, :b] = wide(rng, S, b, lo=-10, hi=10), wide(rng, S + 1, b, lo=-10, hi=10)
            Zh[1] = Z[0]
            Zh[1, 3] = np.nextafter(Z[0, 3], np.inf)
            Zh[2] = Z[1]
            Zh[2, b - 1] = Z[1, b - 1] * (1.0 + 2.0 ** -40)
            yield Case(15, "S%d_bp%d" % (S, bp), (S, bp, S + 3), [Z, Zh], [blank(S + 3, S + 3)])


def check_es_dist(case, outs):
    S, bp, ldd = case.dims
    Z, Zh = (ld(a) for a in case.ins)
    ref = np.sqrt(((Z[:, None, :] - Zh[None, :, :]) ** 2).sum(2))
    D = view(outs[0], ldd, ldd)
    rest = D.copy()
    rest[:S, :S + 1] = np.nan
    return {"finite": finite(D[:S, :S + 1]),
            "exact untouched": max(untouched(outs[0], ldd, ldd, ldd), 0.0 if np.isnan(rest).all() else float("inf")),
            "D": worst_ratio(D[:S, :S + 1], ref, ((bp + 3) / 2 + 1) * uL * ref)}


def restate_es_dist(case, defect=None):
    """No fma: a rounded square and a rounded sum.  defect 'j_lt_S': column S not written;
    'one_chunk': only the first 64 coordinates."""
    S, bp, ldd = case.dims
    Z, Zh = case.ins
    acc = np.zeros((S, S + 1))
    for k in range(64 if defect == "one_chunk" else bp):
        t = Z[:, k][:, None] - Zh[:, k][None, :]
        acc = t * t + acc
    D = nanlike(ldd, ldd)
    ncol = S if defect == "j_lt_S" else S + 1
    D[:S, :ncol] = np.sqrt(acc)[:, :ncol]
    return [image(D)]


# ====================================================================== 16: es_reduce
ESR_S, ESR_BETA = (2, 15, 17, 33), (1.0, 0.5, 1.5)
ESR_POOL = (33, 34)


def es_pool():
    """The D values every es_reduce case takes its S × (S + 1) corner from: 2^U(−20, 20)."""
    return wide(np.random.default_rng(8001), *ESR_POOL, lo=-20, hi=20, signed=False)


def cases_es_reduce():
    """ES = (1/S)Σ_i D_iS^β − Σ_{i,j<S} D_ij^β/(2S(S−1)): thread i adds its S + 1 powers in order,
    block_sum of 1024 (6 + 16); (S + 1 + 22 + c)·u·Σ|terms| with c the allowance for pow (0 for
    β = 1, pow_c() otherwise).  With grad, W_ij = coef_j/D_ij (β = 1: the coefficient, the
    reciprocal, the product, one for the second order: 4u·|W|) or coef_j·β·D^β/D² ((6 + c)·u·|W|);
    rs_i the in-order sum over j <= S ((S + 1 + 6 + c)·u·Σ|W|), cs_j over i < S ((S + 6 + c)·u·Σ|W|);
    rows >= S and columns > S (NaN going in) exactly 0 in W, rs and cs.  Without grad D is left
    as it was."""
    pool = es_pool()
    k = 0
    for S in ESR_S:
        for Sp in (S + 1, 64, 128):
            for beta in ESR_BETA:
                for grad in (0, 1):
                    k += 1
                    ldd = Sp + (2 if k % 2 else 0)
                    D = nanlike(Sp, Sp)
                    D[:S, :S + 1] = pool[:S, :S + 1]
                    yield Case(16, "S%d_Sp%d_ld%d_beta%g_grad%d" % (S, Sp, ldd, beta, grad), (S, Sp, ldd, grad), [],
                               [image(D, ldd), blank(1, Sp) if grad else None, blank(1, Sp) if grad else None,
                                blank(1, 1)], (beta,))


def _es_terms(case):
    """(D^β in longdouble, the coefficient of each column, W's reference)."""
    S = case.dims[0]
    beta = case.scal[0]
    D = ld(es_pool()[:S, :S + 1])
    P = D if beta == 1.0 else hilo(fixture(), "pow%g" % beta)[:S, :S + 1]
    cz, cy = 1 / (LD(S) * (S - 1)), 1 / LD(S)
    coef = np.full(S + 1, -cz / 2)
    coef[S] = cy
    return D, P, coef, coef[None, :] * LD(beta) * P / (D * D)


def check_es_reduce(case, outs):
    S, Sp, ldd, grad = case.dims
    beta = case.scal[0]
    c = 0 if beta == 1.0 else pow_c()
    D, P, coef, W = _es_terms(case)
    T = coef[None, :] * P
    Do = view(outs[0], Sp, ldd)
    res = {"finite": finite(outs[3][:1]),
           "exact untouched": max([untouched(outs[0], Sp, Sp, ldd), untouched(outs[3], 1, 1, 1)]
                                  + [untouched(o, 1, Sp, Sp) for o in outs[1:3] if o is not None]),
           "out": worst_ratio(outs[3][:1], T.sum().reshape(1), (S + 1 + 22 + c) * uL * np.abs(T).sum())}
    if not grad:
        res["exact D kept"] = exact(Do[:, :Sp], view(case.outs0[0], Sp, ldd)[:, :Sp])
        return res
    rs, cs = vec(outs[1], Sp), vec(outs[2], Sp)
    Wz = Do[:, :Sp].copy()
    Wz[:S, :S + 1] = 0.0
    aW = np.abs(W)
    res.update({"finite": finite(outs[3][:1], Do[:, :Sp], rs, cs),
                "exact zeros": max(exact(Wz, np.zeros((Sp, Sp))), exact(rs[S:], np.zeros(Sp - S)),
                                   exact(cs[S + 1:], np.zeros(Sp - S - 1))),
                "W": worst_ratio(Do[:S, :S + 1], W, ((4 if beta == 1.0 else 6) + c) * uL * aW),
                "rs": worst_ratio(rs[:S], W.sum(1), (S + 1 + 6 + c) * uL * aW.sum(1)),
                "cs": worst_ratio(cs[:S + 1], W.sum(0), (S + 6 + c) * uL * aW.sum(0))})
    return res


def restate_es_reduce(case, defect=None):
    """numpy's pow.  defect 'last_col_coef': column S gets −½cz; 'pads_kept': the rows >= S and
    columns > S of W not zeroed."""
    S, Sp, ldd, grad = case.dims
    beta = case.scal[0]
    Dm = view(case.outs0[0].copy(), Sp, ldd)
    Dm[S:, :Sp] = np.nan
    Dm[:S, S + 1:Sp] = np.nan
    D = Dm[:S, :S + 1].copy()
    cz, cy = 1.0 / (float(S) * (S - 1)), 1.0 / S
    P = D if beta == 1.0 else np.power(D, beta)
    v0, v1 = np.zeros(1024), np.zeros(1024)
    for j in range(S):
        v0[:S] = v0[:S] + P[:, j]
    v1[:S] = v1[:S] + P[:, S]
    out = cy * block_sum_f64(v1) - 0.5 * cz * block_sum_f64(v0)
    if not grad:
        return [image(Dm[:, :Sp], ldd), None, None, image(out)]
    coef = np.full(S + 1, -0.5 * cz)
    coef[S] = -0.5 * cz if defect == "last_col_coef" else cy
    W = coef[None, :] * (1.0 / D if beta == 1.0 else beta * P / (D * D))
    Wf = Dm[:, :Sp].copy() if defect == "pads_kept" else np.zeros((Sp, Sp))
    Wf[:S, :S + 1] = W
    rs, cs = np.zeros(Sp), np.zeros(Sp)
    for j in range(S + 1):
        rs[:S] = rs[:S] + W[:, j]
    for i in range(S):
        cs = cs + Wf[i]
    return [image(Wf, ldd), image(rs), image(cs), image(out)]


def pow_error_ulps(W, case):
    """The error of the power behind one W = coef·β·pow/D², in ulps of the power, from the
    returned W: within the five other roundings (u each, at most 5 ulp) of pow's own."""
    S = case.dims[0]
    _, P, _, Wref = _es_terms(case)
    rel = np.abs(ld(W[:S, :S + 1]) - Wref) / np.abs(Wref)
    return float(np.max(rel * np.abs(P) / np.spacing(np.abs(P.astype(np.float64))).astype(LD)))


# ====================================================================== 17: joint_cov
JC_B, JC_D, JC_KS = (1, 31, 32, 33, 100, 129), (1, 2, 8, 16), (1, 3)
JC_SF2, JC_SN2 = 0.47, 0.01
JC_SAMPLE = 200


def jc_inputs(b, d):
    """x [b][d] uniform on ±2 and the inverse length-scales ½, ¾, 1, 1¼ in turn."""
    rng = np.random.default_rng(8100 + 100 * b + d)
    return rng.uniform(-2.0, 2.0, (b, d)), 0.5 + 0.25 * (np.arange(d) % 4)


def jc_args(b, d):
    """−½‖xs_i − xs_j‖² in longdouble from the scaled features the kernel holds, fl(x·inv_ell)."""
    x, inv = jc_inputs(b, d)
    xs = ld(x * inv)
    return -((xs[:, None, :] - xs[None, :, :]) ** 2).sum(2) / 2


def jc_sample(b, d):
    """The lower-triangle entries whose exp the fixture holds: the diagonal and up to 200 drawn
    below it."""
    rng = np.random.default_rng(8200 + 100 * b + d)
    i, j = rng.integers(0, b, JC_SAMPLE), rng.integers(0, b, JC_SAMPLE)
    i, j = np.maximum(i, j), np.minimum(i, j)
    return np.concatenate([np.arange(b), i]), np.concatenate([np.arange(b), j])


def jc_exp(b, d):
    """exp(arg) [b][b]: mpmath's on the sample, numpy longdouble's elsewhere (the host test holds
    the two together to 2^-62 on the sample, a 2^-9 of the bound's one spacing)."""
    E = np.exp(jc_args(b, d))
    i, j = jc_sample(b, d)
    E[i, j] = hilo(fixture(), "exp_b%d_d%d" % (b, d))
    E[j, i] = E[i, j]
    return E


def cases_joint_cov():
    """Sigma_ij = sf2·exp(−½‖(x_i − x_j)/ℓ‖²) + sn2·δ_ij − Σ_q slab_q[i][j] on the real entries:
    §18's Gram-entry bound K·u·((d + 6)·|arg| + 4) + 2^-1074 for K**, plus (ks + 1)·u·(|K| + Σ|slab|)
    for the slice sum, the noise and the subtraction.  On a quarter of the entries the slabs sum
    to K·(1 − 2^-20).  out == out.T bit for bit; the padding is the identity exactly; the slabs are
    NaN in the strict-upper 32-tiles and in the rows and columns >= b (gps_block_diag), and differ
    between the two halves of a diagonal tile."""
    for b in JC_B:
        bp = 256 if b > 128 else 128
        for d in JC_D:
            x, inv = jc_inputs(b, d)
            for ks in JC_KS:
                rng = np.random.default_rng(8300 + 100 * b + 10 * d + ks)
                K = np.zeros((bp, bp))
                K[:b, :b] = (LD(JC_SF2) * np.exp(jc_args(b, d))).astype(np.float64)
                tot = K * rng.uniform(-1.0, 1.0, (bp, bp))
                close = rng.integers(0, 4, (bp, bp)) == 0
                tot[close] = (K * (1.0 - 2.0 ** -20))[close]
                slab = np.empty((ks, bp, bp))
                slab[1:] = K[None] * rng.uniform(-1.0, 1.0, (ks - 1, bp, bp))
                slab[0] = tot - slab[1:].sum(0)
                slab += np.triu(rng.uniform(0.0, 1e-3, (bp, bp)), 1)[None]     # the upper halves differ
                yield Case(17, "b%d_d%d_ks%d" % (b, d, ks), (b, bp, d, ks, bp * bp + 6),
                           [x, inv, slab.reshape(ks, bp * bp)], [blank(bp, bp)], (JC_SF2, JC_SN2))


def _jc_device_slabs(case):
    """The slabs as gps_block_diag leaves them on the device."""
    b, bp, d, ks, _ = case.dims
    s = case.ins[2].reshape(ks, bp, bp).copy()
    s[:, b:, :] = np.nan
    s[:, :, b:] = np.nan
    for t in range(bp // 32):
        s[:, 32 * t:32 * t + 32, 32 * t + 32:] = np.nan
    return s


def check_joint_cov(case, outs):
    b, bp, d, ks, _ = case.dims
    out = view(outs[0], bp, bp)
    arg = jc_args(b, d)
    K = LD(JC_SF2) * jc_exp(b, d)
    sl = ld(case.ins[2].reshape(ks, bp, bp)[:, :b, :b])
    ref = K + LD(JC_SN2) * np.eye(b).astype(LD) - sl.sum(0)
    tol = (K * uL * ((d + 6) * np.abs(arg) + 4) + LD(SUBNORMAL)
           + (ks + 1) * uL * (K + LD(JC_SN2) * np.eye(b).astype(LD) + np.abs(sl).sum(0)))
    low = np.tril(np.ones((b, b), bool))
    want_pad = np.eye(bp)
    want_pad[:b, :b] = 0.0
    got_pad = out.copy()
    got_pad[:b, :b] = 0.0
    return {"finite": finite(out), "exact untouched": untouched(outs[0], bp, bp, bp),
            "exact symmetric": exact(out, out.T.copy()), "exact padding": exact(got_pad, want_pad),
            "out": worst_ratio(np.where(low, out[:b, :b], 0.0), np.where(low, ref, LD(0)), tol)}


def restate_joint_cov(case, defect=None):
    """float64 with the libm exp.  defect 'no_mirror': a diagonal tile's upper half from its own
    entries; 'pad_nan': the padding not overridden; 'sn2_even_only': the noise missed where
    gi == gj + 1 is the lane's second column (odd gi)."""
    b, bp, d, ks, _ = case.dims
    x, inv, _ = case.ins
    s = _jc_device_slabs(case)
    if defect == "no_mirror":            # what the kernel reads there: the diagonal tiles are whole
        raw = case.ins[2].reshape(ks, bp, bp)
        for t in range(bp // 32):
            sl = slice(32 * t, 32 * t + 32)
            s[:, sl, sl] = raw[:, sl, sl]
        s[:, b:, :] = np.nan
        s[:, :, b:] = np.nan
    xs = np.zeros((bp, d))
    xs[:b] = x * inv
    acc = np.zeros((bp, bp))
    for k in range(d):
        t = xs[:, k][:, None] - xs[:, k][None, :]
        acc = t * t + acc
    tot = s[0].copy()
    for q in range(1, ks):
        tot = tot + s[q]
    v = JC_SF2 * np.exp(-0.5 * acc)
    i = np.arange(bp)
    dg = v[i, i] + JC_SN2
    if defect == "sn2_even_only":
        dg = np.where(i % 2 == 0, dg, v[i, i])
    v[i, i] = dg
    v = v - tot
    if defect != "pad_nan":
        pad = (i[:, None] >= b) | (i[None, :] >= b)
        v[pad] = np.eye(bp)[pad]
    low = i[:, None] >= i[None, :]
    if defect == "no_mirror":
        tile = (i[:, None] // 32) == (i[None, :] // 32)
        out = np.where(low | tile, v, v.T)
    else:
        out = np.where(low, v, v.T)
    return [image(out, bp)]


# ====================================================================== 19: joint_dss
DSS_B = (1, 1023, 1024, 1025)


def cases_joint_dss():
    """out = ½b·log2π + Σ logdiag_i + ½Σ t_i²: thread i adds its ⌈b/1024⌉ terms in order, block_sum
    of 1024 (6 + 16); the squares, the halving, the constant and the two final additions four
    more: (⌈b/1024⌉ + 22 + 4)·u·(½b·log2π + Σ|logdiag| + ½Σt²)."""
    rng = np.random.default_rng(8400)
    for b in DSS_B:
        yield Case(19, "b%d" % b, (b,), [wide(rng, b, lo=-10, hi=10), wide(rng, b, lo=-10, hi=10)], [blank(1, 1)])


def check_joint_dss(case, outs):
    b = case.dims[0]
    lg, t = (ld(a) for a in case.ins)
    c0 = LD(b) * LD(LOG_2PI) / 2
    ref = c0 + lg.sum() + (t * t).sum() / 2
    tol = (-(-b // 1024) + 26) * uL * (c0 + np.abs(lg).sum() + (t * t).sum() / 2)
    return {"finite": finite(outs[0][:1]), "exact untouched": untouched(outs[0], 1, 1, 1),
            "out": worst_ratio(outs[0][:1], ref.reshape(1), tol)}


def restate_joint_dss(case, defect=None):
    """defect 'first_trip_only': the strided loop taken once; 'no_half'."""
    b = case.dims[0]
    lg, t = case.ins
    if defect == "first_trip_only":
        lg, t = lg[:1024], t[:1024]
    v0, v1 = strided_sum_f64(lg, 1024), strided_sum_f64(t * t, 1024)
    h = 1.0 if defect == "no_half" else 0.5
    return [image(0.5 * b * LOG_2PI + block_sum_f64(v0) + h * block_sum_f64(v1))]


# ====================================================================== the table
NAMES = ("fold_grad", "row_dots", "lr_fold_vec", "lr_combine", "fold_sum", "fold_logdet", "row_scale", "vec_mul",
         "blk_mdiag", "ns_init", "diag_add_const", "sym_avg", "scaled_row", "row_axpy", "ns_resid", "es_dist",
         "es_reduce", "joint_cov", "joint_resid", "joint_dss", "sign_fill", "row_add", "fitc_grad_v", "fitc_grad_y")
CASES = tuple(globals()["cases_" + n] for n in NAMES)
CHECK = tuple(globals()["check_" + n] for n in NAMES)
RESTATE = tuple(globals()["restate_" + n] for n in NAMES)
# the checks whose bound is a count of one to three roundings, which plain rounding may approach
SHARP = ("Y", "o1 dss", "g", "W")


def check(case, outs):
    need_extended()
    return CHECK[case.which](case, outs)


def restate(case, defect=None):
    with np.errstate(all="ignore"):
        return RESTATE[case.which](case, defect)


# ====================================================================== the fixture's inputs
def term_inputs():
    """What tests/golden/make_block_terms.py evaluates with mpmath: log λ of fold_logdet's pool,
    D^β of es_reduce's pool for β = 0.5 and 1.5, and exp of joint_cov's sampled arguments (as
    hi/lo pairs of the longdouble argument, which float64 cannot hold)."""
    out = {"log": logdet_lam(), "pow": es_pool()}
    for b in JC_B:
        for d in JC_D:
            i, j = jc_sample(b, d)
            a = jc_args(b, d)[i, j]
            hi = a.astype(np.float64)
            out["arg_b%d_d%d" % (b, d)] = np.stack([hi, (a - ld(hi)).astype(np.float64)])
    return out
