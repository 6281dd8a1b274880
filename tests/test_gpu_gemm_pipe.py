"""The pipelined steady-state loop of the 128-tile FP64 GEMM on the device (GemmParams::pipe,
GPS_OPT_GEMM_PIPE), one launch at a time through gps_gemm_diag with the option on,
on again, and off: C, out0 and out1 must be BITWISE equal in all three (every accumulator's MFMA
chain is the same in both loops — slices ascending, k steps ascending — only the issue order of
the loads, fragment reads and LDS stores around it differs).

Shapes: M = N = 256 (2 × 2 tiles of 128: all four wave quadrants, and tiles with a non-zero row
and column offset) at K = 16 (one slice: no steady-state iteration, the loop's tail alone), 32 and
48 (one and two iterations: the prefetched slice is stored into buffer 1, then buffer 0, and the
tail reads either), and 272 (17 slices).  Variants: the four store layouts with (alpha, beta) =
(1, 0) and (−1, 1), lower_out, the triangular clippings 1-3 at tri_off 128 (tiles of one launch
then run different slice counts, empty ranges included), the column reduction, a split into two K
slices, and live-extent hints that make three of the four tiles edge tiles — those run the edge
copy of the old loop next to the one full tile on the pipelined loop.  Wave priority: launch_gemm
raises it for exactly the launches that may take the pipelined loop; the k-scaled launch and the
row norms run at priority 0 and stay on the old loop whatever the option says (checked on the host
in tests/test_gemm_pipe_host.py) — they are launched here all the same, so that an option that
leaked into them would show.

One end-to-end case runs a full fit and predict through the production callers with the option
on, replayed, and off, asserts every output bitwise equal, and that the option is part of the
factorisation's graph-cache key (a graph of its own per value)."""
import ctypes

import numpy as np
import pytest

from gpscore import _lib

pytestmark = pytest.mark.gpu

STORE, ROWSQ, COLRED = 0, 1, 2
M = N = 256
KS = (16, 32, 48, 272)
SENT = 77777.0

# name: (lay_a, lay_b, epi, alpha, beta, lower_out, tri, tri_off, ksplit, reserved, k-scaled)
CASES = {
    "nn_store_1_0": (0, 0, STORE, 1.0, 0.0, 0, 0, 0, 1, 0, False),
    "nn_store_m1_1": (0, 0, STORE, -1.0, 1.0, 0, 0, 0, 1, 0, False),
    "nt_store_1_0": (0, 1, STORE, 1.0, 0.0, 0, 0, 0, 1, 0, False),
    "nt_store_m1_1": (0, 1, STORE, -1.0, 1.0, 0, 0, 0, 1, 0, False),
    "tn_store_1_0": (1, 0, STORE, 1.0, 0.0, 0, 0, 0, 1, 0, False),
    "tn_store_m1_1": (1, 0, STORE, -1.0, 1.0, 0, 0, 0, 1, 0, False),
    "tt_store_1_0": (1, 1, STORE, 1.0, 0.0, 0, 0, 0, 1, 0, False),
    "tt_store_m1_1": (1, 1, STORE, -1.0, 1.0, 0, 0, 0, 1, 0, False),
    "nt_lower_out": (0, 1, STORE, -1.0, 1.0, 1, 0, 0, 1, 0, False),
    "nn_tri1_off": (0, 0, STORE, -1.0, 0.0, 0, 1, 128, 1, 0, False),
    "nt_tri2_off": (0, 1, STORE, 1.0, 0.0, 0, 2, 128, 1, 0, False),
    "nn_tri3_off": (0, 0, STORE, 1.0, 0.0, 0, 3, 128, 1, 0, False),
    "nt_colred_tri1": (0, 1, COLRED, 1.0, 0.0, 0, 1, 128, 1, 0, False),
    "nt_ksplit2": (0, 1, STORE, -1.0, 1.0, 0, 0, 0, 2, 0, False),
    "nt_live_hints": (0, 1, STORE, -1.0, 1.0, 0, 0, 0, 1, 3 | 5 << 8, False),
    "nn_live_hints": (0, 0, STORE, 1.0, 0.0, 0, 0, 0, 1, 4 | 1 << 8, False),
    "nt_colred_live": (0, 1, COLRED, 1.0, 0.0, 0, 1, 128, 1, 3, False),
    "nt_kscaled": (0, 1, STORE, 1.0, 0.0, 0, 0, 0, 1, 0, True),
    "nt_row_norms": (0, 1, ROWSQ, 1.0, 0.0, 0, 2, 0, 1, 0, False),
}


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def set_pipe(ctx, value):
    ctx.call("gps_ctx_set_option", _lib.GPS_OPT_GEMM_PIPE, value)


class Launch:
    """One description with its operands; run() launches on fresh copies of C / out."""

    def __init__(self, ctx, case, K):
        la, lb, epi, alpha, beta, lower, tri, off, ksplit, reserved, kscaled = CASES[case]
        rng = np.random.default_rng([38, sorted(CASES).index(case), K])
        dm, dn = reserved & 127, reserved >> 8
        opA = rng.standard_normal((M, K))
        opB = rng.standard_normal((K, N))
        opA[M - 16 * dm:, :] = 0.0   # the live-extent promise: dead output rows are exact zeros
        opB[:, N - 16 * dn:] = 0.0   # ... and dead output columns
        self.A = np.ascontiguousarray(opA if la == 0 else opA.T)
        self.B = np.ascontiguousarray(opB if lb == 0 else opB.T)
        self.C0 = rng.standard_normal((M, N))
        self.w = rng.standard_normal(M) if epi == COLRED else None
        self.kscale = rng.uniform(0.5, 2.0, K) if kscaled else None
        self.ctx, self.epi, self.ksplit = ctx, epi, ksplit
        self.d = _lib.GemmDesc(lay_a=la, lay_b=lb, epi=epi, M=M, N=N, K=K, lda=K if la == 0 else M,
                               ldb=N if lb == 0 else K, ldc=N if epi == STORE else 0, alpha=alpha,
                               beta=beta, tri=tri, tri_off=off, lower_out=lower, mirror=0, kend=0,
                               tile=128, ksplit=ksplit, map_mode=0, use_ws=1, sk_alone=0,
                               dep_mode=0, reserved=reserved,
                               ld_out={STORE: 0, COLRED: N, ROWSQ: M}[epi], c_kslice_stride=0)

    def run(self):
        C = out0 = out1 = None
        if self.epi == STORE:
            C = self.C0.copy()
        elif self.epi == COLRED:
            out0 = np.full((M // 128, N), SENT)
            out1 = np.full((M // 128, N), SENT)
        else:
            out0 = np.full((N // 128, M), SENT)
        plan = self.ctx.gemm_diag(self.d, self.A, self.B, C, self.kscale, self.w, None, out0, out1)
        assert plan["tile"] == 128 and plan["ksplit"] == self.ksplit, plan  # the named kernel ran
        return [x for x in (C, out0, out1) if x is not None]


@pytest.mark.parametrize("case", sorted(CASES))
def test_pipelined_launch_bitwise_equals_the_old_loop(gpu_ctx, case):
    try:
        for K in KS:
            if CASES[case][8] > 1 and K < 32:
                continue  # (two K slices need two 16-deep slices)
            L = Launch(gpu_ctx, case, K)
            set_pipe(gpu_ctx, 1)
            one = L.run()
            two = L.run()  # a second launch: determinism
            set_pipe(gpu_ctx, 0)
            off = L.run()
            for x in off:
                assert np.isfinite(x).all()
            for name, a, b, r in zip(("C/out0", "out0/out1", "out1"), one, two, off):
                assert same_bits(a, r), (case, K, name, "option on differs from option off",
                                         np.argwhere(a != r)[:2])
                assert same_bits(a, b), (case, K, name, "second launch differs")
    finally:
        set_pipe(gpu_ctx, 1)


def test_store_result_is_the_product(gpu_ctx):
    """(The bitwise comparisons above would also pass if both loops were wrong alike.)"""
    try:
        for pipe in (1, 0):
            set_pipe(gpu_ctx, pipe)
            for case in ("nt_store_m1_1", "nn_store_1_0", "tn_store_1_0", "tt_store_m1_1"):
                la, lb, _, alpha, beta = CASES[case][:5]
                L = Launch(gpu_ctx, case, 272)
                opA = L.A if la == 0 else L.A.T
                opB = L.B if lb == 0 else L.B.T
                want = alpha * (opA @ opB) + beta * L.C0
                got = L.run()[0]
                # |error| <= ~K eps |A||B| elementwise; entries are O(1), sums of 272 terms
                assert np.max(np.abs(got - want)) <= 272 * 2.3e-16 * np.max(np.abs(opA) @ np.abs(opB))
    finally:
        set_pipe(gpu_ctx, 1)


# ---------------------------------------------------------------- through the production callers
# The smallest fit whose top-level W, SYRK, T, L⁻¹21 and predictive product all run the 128-tile
# kernel (tests/test_gpu_gemm_live.py derives it): n = 7960, n* = 1416.
E2E_N, E2E_NT, E2E_D = 7960, 1416, 8


def plan_tile(**kw):
    d = dict(lay_a=0, lay_b=1, epi=STORE, alpha=1.0, beta=0.0, tri=0, tri_off=0, lower_out=0,
             mirror=0, kend=0, tile=0, ksplit=1, map_mode=0, use_ws=1, sk_alone=0, dep_mode=0,
             reserved=0)
    d.update(kw)
    d.update(lda=max(d["K"], d["M"]), ldb=max(d["K"], d["N"]), ldc=d["N"], ld_out=max(d["M"], d["N"]),
             c_kslice_stride=0)
    plan = np.zeros(8, np.int32)
    items = np.zeros((1 << 15, 8), np.int32)
    lib = _lib.load()
    desc = _lib.GemmDesc(**d)
    n = lib.gps_gemm_schedule(ctypes.byref(desc), None, 0, 512, plan.ctypes.data_as(_lib._PI),
                              items.ctypes.data_as(_lib._PI), len(items))
    assert n > 0, lib.gps_last_error(None)
    assert lib.gps_gemm_pipe_resolved(ctypes.byref(desc), None, 0, 1) == 1  # ... on the new loop
    return int(plan[0])


def test_fit_and_predict_bitwise_with_option_on_and_off():
    import gpscore
    ctx = gpscore.Context(0)  # (a cache of its own: the graph counts below start from nothing)
    n, nt, d = E2E_N, E2E_NT, E2E_D
    npad, ntpad = -(-n // 128) * 128, -(-nt // 128) * 128
    n1 = (npad // 128 // 2) * 128
    n2 = npad - n1
    # the fit's launches of every layout run the 128-tile kernel (the library's own plan function)
    assert plan_tile(M=n2, N=n1, K=n1, tri=2) == 128                                  # W     (NT)
    assert plan_tile(M=n2, N=n2, K=n1, alpha=-1.0, beta=1.0, lower_out=1) == 128      # SYRK  (NT)
    assert plan_tile(M=n2, N=n1, K=n1, lay_b=0, tri=3) == 128                         # T     (NN)
    assert plan_tile(M=n2, N=n1, K=n2, lay_b=0, alpha=-1.0, tri=1) == 128             # L⁻¹21 (NN)
    assert plan_tile(M=npad, N=ntpad, K=npad, epi=COLRED, tri=1) == 128               # predictive
    rng = np.random.default_rng(38)
    X, Xt = rng.standard_normal((n, d)), rng.standard_normal((nt, d))
    wv = rng.standard_normal(d) / np.sqrt(d)
    y = np.sin(3 * X @ wv) + 0.1 * rng.standard_normal(n)
    yt = np.sin(3 * Xt @ wv) + 0.1 * rng.standard_normal(nt)
    theta = (0.0, np.log(2.0) * np.ones(d), np.log(0.05))
    gp = gpscore.GP(ctx=ctx)
    gp.set_data(X, y)
    gp.set_test(Xt, yt)

    def unit():
        res = gp.fit(theta=theta)
        mu, var, sc = gp.predict(with_scores=True)
        obj = np.array([res.objectives[k] for k in _lib.OBJ_NAMES])
        scores = np.array([sc[k] for k in _lib.SCORE_NAMES])
        return obj, res.mu_loo.copy(), res.var_loo.copy(), mu.copy(), var.copy(), scores

    names = ("objectives", "mu_loo", "var_loo", "mu*", "var*", "scores")
    try:
        set_pipe(ctx, 1)
        on = unit()
        g_on = ctx.stats()["graphs"]
        replay = unit()  # the factorisation's graph replayed
        assert ctx.stats()["graphs"] == g_on
        set_pipe(ctx, 0)
        off = unit()
        assert ctx.stats()["graphs"] == g_on + 1, "the option is not in the graph-cache key"
        off_replay = unit()
        assert ctx.stats()["graphs"] == g_on + 1
    finally:
        ctx.close()
    for x in on:
        assert np.isfinite(x).all()
    for name, a, b, c, e in zip(names, on, replay, off, off_replay):
        assert same_bits(a, b), (name, "graph replay differs from the first run")
        assert same_bits(a, c), (name, "option on differs from option off")
        assert same_bits(c, e), (name, "replay with the option off differs")
