"""The live-extent skip of the FP64 GEMM's edge tiles on the device (GemmParams::m_live / n_live,
GPS_OPT_GEMM_LIVE), one launch at a time through gps_gemm_diag, whose `reserved` field
carries the hints as dead_m16 | dead_n16 << 8 (trailing dead 16-blocks of M and N).

Shapes: M = N = 256, K = 272 (2 × 2 tiles of 128, 17 slices of 16: an odd slice count, so the
double buffer ends on either side), forced tile = 128 and again tile = 64 (4 × 4 tiles; the
extent then also lands ON a tile boundary, dead = 4, and a whole tile is dead at 5 and 7).  Dead
blocks 0, 1, 3, 4, 5, 7 on each side: 4 empties exactly one wave row / column of a 128-tile, 5 and
7 cross it.  The operands are random with the dead rows of the left operand and the dead columns
of the right operand zero, so the caller's promise holds, and every hinted launch must leave C,
out0 and out1 BITWISE what the same launch without hints leaves (the skipped accumulators stay +0,
which is what the full loop leaves there: fma(0, b, +0) = +0 for finite b).  The column reduction
runs on 128-tiles only (launch_gemm), so that case has no 64-tile twin.

That a hinted launch really skips is shown with NaN in the dead rows (columns) of an INPUT array:
with hints the output is the clean run's, without them the NaN comes through.  (A NaN in an input
array, nothing else: no fault is provoked.)

One end-to-end case runs a full fit and predict through the production callers with the switch
on, replayed, and off, and asserts every output bitwise equal."""
import ctypes
import itertools

import numpy as np
import pytest

from gpscore import _lib

pytestmark = pytest.mark.gpu

STORE, COLRED = 0, 2
M = N = 256
K = 272
DEAD = (0, 1, 3, 4, 5, 7)
SENT = 77777.0

# name: (lay_a, lay_b, epi, alpha, beta, lower_out, tri, tri_off)
CASES = {
    "nn_store_1_0": (0, 0, STORE, 1.0, 0.0, 0, 0, 0),
    "nn_store_m1_1": (0, 0, STORE, -1.0, 1.0, 0, 0, 0),
    "nt_store_1_0": (0, 1, STORE, 1.0, 0.0, 0, 0, 0),
    "nt_store_m1_1": (0, 1, STORE, -1.0, 1.0, 0, 0, 0),
    "nt_lower_out": (0, 1, STORE, -1.0, 1.0, 1, 0, 0),
    "nn_tri1_off": (0, 0, STORE, -1.0, 0.0, 0, 1, 128),
    "nt_tri2_off": (0, 1, STORE, 1.0, 0.0, 0, 2, 128),
    "nn_tri3_off": (0, 0, STORE, 1.0, 0.0, 0, 3, 128),
    "nt_colred_tri1": (0, 1, COLRED, 1.0, 0.0, 0, 1, 128),
}


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


class Launch:
    """One description with its operands; run(reserved) launches on fresh copies of C / out."""

    def __init__(self, ctx, case, tile, dm, dn, seed=0):
        la, lb, epi, alpha, beta, lower, tri, off = CASES[case]
        rng = np.random.default_rng([seed, sorted(CASES).index(case), tile, dm, dn])
        self.ctx, self.epi, self.beta = ctx, epi, beta
        self.opA = rng.standard_normal((M, K))
        self.opB = rng.standard_normal((K, N))
        self.opA[M - 16 * dm:, :] = 0.0   # the promise: dead output rows are exact zeros
        self.opB[:, N - 16 * dn:] = 0.0   # ... and dead output columns
        self.la, self.lb = la, lb
        self.C0 = rng.standard_normal((M, N))
        self.w = rng.standard_normal(M) if epi == COLRED else None
        self.dm, self.dn = dm, dn
        self.d = _lib.GemmDesc(lay_a=la, lay_b=lb, epi=epi, M=M, N=N, K=K, lda=K if la == 0 else M,
                               ldb=N if lb == 0 else K, ldc=N if epi == STORE else 0, alpha=alpha,
                               beta=beta, tri=tri, tri_off=off, lower_out=lower, mirror=0, kend=0,
                               tile=tile, ksplit=1, map_mode=0, use_ws=1, sk_alone=0, dep_mode=0,
                               reserved=0, ld_out=N if epi == COLRED else 0, c_kslice_stride=0)
        self.tile = tile

    def run(self, reserved, opA=None, opB=None):
        opA = self.opA if opA is None else opA
        opB = self.opB if opB is None else opB
        A = np.ascontiguousarray(opA if self.la == 0 else opA.T)
        B = np.ascontiguousarray(opB if self.lb == 0 else opB.T)
        self.d.reserved = reserved
        C = out0 = out1 = None
        if self.epi == STORE:
            C = self.C0.copy()
        else:
            out0 = np.full((M // 128, N), SENT)
            out1 = np.full((M // 128, N), SENT)
        plan = self.ctx.gemm_diag(self.d, A, B, C, None, self.w, None, out0, out1)
        assert plan["tile"] == self.tile and plan["ksplit"] == 1, plan  # the named kernel ran
        return [x for x in (C, out0, out1) if x is not None]


def tiles_for(case):
    return (128,) if CASES[case][2] == COLRED else (128, 64)


@pytest.mark.parametrize("case, tile", [(c, t) for c in sorted(CASES) for t in tiles_for(c)])
def test_hinted_launch_bitwise_equals_unhinted(gpu_ctx, case, tile):
    for dm, dn in itertools.product(DEAD, DEAD):
        L = Launch(gpu_ctx, case, tile, dm, dn)
        ref = L.run(0)
        for x in ref:
            assert np.isfinite(x).all()
        hint = dm | dn << 8
        one = L.run(hint)
        two = L.run(hint)  # determinism
        for name, r, a, b in zip(("C/out0", "out0/out1", "out1"), ref, one, two):
            assert same_bits(r, a), (case, tile, dm, dn, name, "hinted differs from unhinted",
                                     np.argwhere(r != a)[:2])
            assert same_bits(a, b), (case, tile, dm, dn, name, "hinted launch not deterministic")


@pytest.mark.parametrize("case", ["nn_store_1_0", "nt_store_m1_1", "nn_store_m1_1", "nt_store_1_0"])
def test_dead_rows_are_skipped(gpu_ctx, case):
    """NaN in the dead rows of A (tile 128): with the hint the live rows are the clean run's
    bitwise and the dead rows are beta·C exactly; without it the NaN is in the output."""
    for dm in DEAD[1:]:
        L = Launch(gpu_ctx, case, 128, dm, 0)
        clean = L.run(0)[0]
        bad = L.opA.copy()
        bad[M - 16 * dm:, :] = np.nan
        live = slice(0, M - 16 * dm)
        dead = slice(M - 16 * dm, M)
        got = L.run(dm, opA=bad)[0]
        assert same_bits(got[live], clean[live]), (case, dm)
        assert np.array_equal(got[dead], L.beta * L.C0[dead]), (case, dm)
        assert same_bits(got[dead], clean[dead]), (case, dm)
        unhinted = L.run(0, opA=bad)[0]
        assert np.isnan(unhinted[dead]).all() and same_bits(unhinted[live], clean[live]), (case, dm)


@pytest.mark.parametrize("case", ["nn_store_1_0", "nt_store_m1_1"])
def test_dead_columns_are_skipped(gpu_ctx, case):
    """The same for the dead columns: NaN in those columns' entries of B."""
    for dn in DEAD[1:]:
        L = Launch(gpu_ctx, case, 128, 0, dn)
        clean = L.run(0)[0]
        bad = L.opB.copy()
        bad[:, N - 16 * dn:] = np.nan
        live = slice(0, N - 16 * dn)
        dead = slice(N - 16 * dn, N)
        got = L.run(dn << 8, opB=bad)[0]
        assert same_bits(got[:, live], clean[:, live]), (case, dn)
        assert np.array_equal(got[:, dead], L.beta * L.C0[:, dead]), (case, dn)
        unhinted = L.run(0, opB=bad)[0]
        assert np.isnan(unhinted[:, dead]).all(), (case, dn)
        assert same_bits(unhinted[:, live], clean[:, live]), (case, dn)


def test_dead_rows_are_skipped_colred(gpu_ctx):
    """The column reduction over skipped rows adds zeros: NaN in A's dead rows leaves out0 / out1
    the clean run's with the hint, and reaches the last row tile's sums without it."""
    for dm in DEAD[1:]:
        L = Launch(gpu_ctx, "nt_colred_tri1", 128, dm, 0)
        clean = L.run(0)
        bad = L.opA.copy()
        bad[M - 16 * dm:, :] = np.nan
        got = L.run(dm, opA=bad)
        assert same_bits(got[0], clean[0]) and same_bits(got[1], clean[1]), dm
        unhinted = L.run(0, opA=bad)
        assert np.isnan(unhinted[0][-1]).all() and np.isnan(unhinted[1][-1]).all(), dm
        assert same_bits(unhinted[0][0], clean[0][0]), dm


# ---------------------------------------------------------------- through the production callers
# The smallest fit whose top-level W, SYRK, T, L⁻¹21 and predictive product all run the 128-tile
# kernel: gemm_plan takes 128-tiles from 512 output tiles, and the SYRK's lower half has
# t(t + 1)/2 >= 512 from t = 32 row tiles of A22, so n_pad = 63 tiles (A11 31, A22 32).  n = 7960
# rounds to 7968 = 8064 − 6·16 and n* = 1416 to 1424 = 1536 − 7·16: 6 and 7 dead 16-blocks.
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
    return int(plan[0])


def test_fit_and_predict_bitwise_with_switch_on_and_off(gpu_ctx):
    import gpscore
    n, nt, d = E2E_N, E2E_NT, E2E_D
    npad, ntpad = -(-n // 128) * 128, -(-nt // 128) * 128
    n1 = (npad // 128 // 2) * 128
    n2 = npad - n1
    assert (npad - -(-n // 16) * 16) // 16 == 6 and (ntpad - -(-nt // 16) * 16) // 16 == 7
    # the launches the hints reach run the 128-tile kernel (the library's own plan function)
    assert plan_tile(M=n2, N=n1, K=n1, tri=2) == 128                                  # W
    assert plan_tile(M=n2, N=n2, K=n1, alpha=-1.0, beta=1.0, lower_out=1) == 128      # SYRK
    assert plan_tile(M=n2, N=n1, K=n1, lay_b=0, tri=3) == 128                         # T
    assert plan_tile(M=n2, N=n1, K=n2, lay_b=0, alpha=-1.0, tri=1) == 128             # L⁻¹21
    assert plan_tile(M=npad, N=ntpad, K=npad, epi=COLRED, tri=1) == 128               # predictive
    rng = np.random.default_rng(35)
    X, Xt = rng.standard_normal((n, d)), rng.standard_normal((nt, d))
    wv = rng.standard_normal(d) / np.sqrt(d)
    y = np.sin(3 * X @ wv) + 0.1 * rng.standard_normal(n)
    yt = np.sin(3 * Xt @ wv) + 0.1 * rng.standard_normal(nt)
    theta = (0.0, np.log(2.0) * np.ones(d), np.log(0.05))
    gp = gpscore.GP(ctx=gpu_ctx)
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
        gpu_ctx.call("gps_ctx_set_option", _lib.GPS_OPT_GEMM_LIVE, 1)
        on = unit()
        replay = unit()  # the factorisation's graph replayed
        gpu_ctx.call("gps_ctx_set_option", _lib.GPS_OPT_GEMM_LIVE, 0)
        off = unit()
        off_replay = unit()
    finally:
        gpu_ctx.call("gps_ctx_set_option", _lib.GPS_OPT_GEMM_LIVE, 1)
    for x in on:
        assert np.isfinite(x).all()
    for name, a, b, c, e in zip(names, on, replay, off, off_replay):
        assert same_bits(a, b), (name, "graph replay differs from the first run")
        assert same_bits(a, c), (name, "switch on differs from switch off")
        assert same_bits(c, e), (name, "replay with the switch off differs")
