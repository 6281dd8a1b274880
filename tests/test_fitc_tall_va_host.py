"""The validated tall FITC fits on the host (no GPU): the two C-ABI entry points are
declared, bound (ABI still 900) and reject a NULL context; fitc_train_tall_validated,
fitc_blockloo_train_tall_validated and run_fitc_validated_batch refuse a bad validation set,
va_every, select and es before any library call; the argument lists position by position, va_z
NULL without select / keep_z and a pointer with either; the Z selection on hand-made rows a stub
context returns; run_fitc_validated_batch draws what run_fitc_batch / run_fitc_blockloo_batch draw
and passes the validation split."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_full_tall_host import _RecordingCtx, _ok, _sheets
from test_full_tall_va_host import _grab

VA = ("gps_fitc_train_tall_va", "gps_fitc_blockloo_train_tall_va")
NSC = 6


def _z(B=3, m=4, d=2, seed=2):
    return np.random.default_rng(seed).uniform(-1, 1, (B, m, d))


def test_header_declares_and_binding_covers_the_va_calls():
    from gpscore import _lib
    txt = open(os.path.join(ROOT, "include", "gpscore.h")).read()
    assert "#define GPS_ABI_VERSION 900" in txt
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(gps_\w+)\s*\(", code))
    lib = _lib.load()
    for s in VA:
        assert s in declared, s
        assert s in _lib.SIGNATURES, s
        assert hasattr(lib, s), s
    # the plain calls' lists with Xv, yv, nv, va_every in front of Xt and va_sc, va_z in front of info
    P, i64 = _lib._P, ctypes.c_int64
    t = _lib.SIGNATURES["gps_fitc_train_tall"][1]
    bt = _lib.SIGNATURES["gps_fitc_blockloo_train_tall"][1]
    assert _lib.SIGNATURES[VA[0]][1] == t[:14] + [P, P, i64, i64] + t[14:26] + [P, P] + t[26:]
    assert _lib.SIGNATURES[VA[1]][1] == bt[:15] + [P, P, i64, i64] + bt[15:27] + [P, P] + bt[27:]
    assert _lib.ABI_VERSION == 900 and lib.gps_version() == 900


def test_va_calls_reject_null_context():
    from gpscore import _lib
    lib = _lib.load()
    z = np.zeros(16)
    iz = np.zeros(2, np.int32)
    P = _lib.ptr
    I = iz.ctypes.data_as(_lib._PI)
    rc = lib.gps_fitc_train_tall_va(None, 1, 1, P(z), P(z), 2, 1, P(z), 1, P(z), 1, 3, 0.1, 0.1, P(z),
                                    P(z), 2, 1, None, None, 0, 0, P(z), P(z), None, None, None, None,
                                    None, None, P(z), None, I, I)
    assert rc == -1
    assert b"NULL" in lib.gps_last_error(None)
    rc = lib.gps_fitc_blockloo_train_tall_va(None, 0, 2, 1, P(z), P(z), 2, 1, P(z), 1, P(z), 1, 3,
                                             0.1, 0.1, P(z), P(z), 2, 1, None, None, 0, 0, P(z), P(z),
                                             None, None, None, None, None, None, P(z), None, I, I)
    assert rc == -1
    assert b"NULL" in lib.gps_last_error(None)


def test_validated_wrappers_refuse_before_any_call():
    import gpscore
    ctx = _RecordingCtx()
    X, y = _ok()  # B = 3, n = 10, d = 2
    Z = _z()
    th = (0.0, 0.0, -1.0)
    Xv, yv = np.zeros((3, 4, 2)), np.zeros((3, 4))
    both = (lambda *a, **k: gpscore.fitc_train_tall_validated(*a, lr=0.1, itr=2, ctx=ctx, **k),
            lambda *a, **k: gpscore.fitc_blockloo_train_tall_validated(*a, lr=0.1, itr=2, ctx=ctx,
                                                                       **k))
    for f in both:
        with pytest.raises(ValueError, match=r"Xv must be \(B, nv, d\)"):
            f(X, y, Z, th, np.zeros((3, 4, 5)), yv)  # the wrong d
        with pytest.raises(ValueError, match=r"Xv must be \(B, nv, d\)"):
            f(X, y, Z, th, np.zeros((2, 4, 2)), yv)  # the wrong B
        with pytest.raises(ValueError, match=r"Xv must be \(B, nv, d\)"):
            f(X, y, Z, th, np.zeros((3, 4)), yv)  # (B, nv) only stands for d = 1
        with pytest.raises(ValueError, match="Xv holds no rows"):
            f(X, y, Z, th, np.zeros((3, 0, 2)), np.zeros((3, 0)))
        with pytest.raises(ValueError, match="Xv must be a rectangular"):
            f(X, y, Z, th, [np.zeros((4, 2)), np.zeros((5, 2)), np.zeros((4, 2))], yv)
        with pytest.raises(ValueError, match=r"yv must be \(B, nv\)"):
            f(X, y, Z, th, Xv, np.zeros((3, 5)))
        with pytest.raises(ValueError, match=r"yv must be \(B, nv\)"):
            f(X, y, Z, th, Xv, np.zeros(4))
        with pytest.raises(ValueError, match="yv is required"):
            f(X, y, Z, th, Xv, None)
        with pytest.raises(ValueError, match="Xv is required"):
            f(X, y, Z, th, None, yv)
        for bad in (0, -3, 2.5, 1.0, True, "2"):
            with pytest.raises(ValueError, match="va_every"):
                f(X, y, Z, th, Xv, yv, va_every=bad)
        for bad in ("cover", "test_crps", "nlml", "", 0):
            with pytest.raises(ValueError, match="select"):
                f(X, y, Z, th, Xv, yv, select=bad)
        # the plain wrappers' refusals still come first
        with pytest.raises(ValueError, match="disagree"):
            f(X, y[:, :-1], Z, th, Xv, yv)
        with pytest.raises(ValueError, match=r"Z must be \(B, m, d\)"):
            f(X, y, Z[:2], th, Xv, yv)
        with pytest.raises(ValueError, match="lr_z"):
            f(X, y, Z, th, Xv, yv, lr_z=np.inf)
        with pytest.raises(ValueError, match="yt without Xt"):
            f(X, y, Z, th, Xv, yv, yt=np.zeros((3, 5)))
    with pytest.raises(ValueError, match="objective"):
        gpscore.fitc_train_tall_validated(X, y, Z, th, Xv, yv, "dss", ctx=ctx)
    with pytest.raises(ValueError, match="objective"):
        gpscore.fitc_blockloo_train_tall_validated(X, y, Z, th, Xv, yv, "loo_crps", ctx=ctx)
    with pytest.raises(ValueError, match="nfold"):
        gpscore.fitc_blockloo_train_tall_validated(X, y, Z, th, Xv, yv, "dss", nfold=11, ctx=ctx)
    assert ctx.calls == []


def test_argument_lists_position_by_position():
    import gpscore
    ctx = _RecordingCtx()
    X, y = _ok()
    Z = _z()
    rng = np.random.default_rng(1)
    Xv, yv = rng.standard_normal((3, 4, 2)), rng.standard_normal((3, 4))
    Xt, yt = rng.standard_normal((3, 5, 2)), rng.standard_normal((3, 5))
    th = rng.standard_normal((3, 4))
    res = gpscore.fitc_train_tall_validated(X, y, Z, th, Xv, yv, "loo_logs", lr=0.25, lr_z=0.5,
                                            itr=7, va_every=3, Xt=Xt, yt=yt, stale_noise=True,
                                            ctx=ctx)
    assert ctx.calls == [VA[0]]
    a = ctx.args[0]
    assert len(a) == 33
    assert a[:2] == (2, 3) and a[4:6] == (10, 2) and a[7] == 4 and a[9] == 2
    assert a[10:13] == (7, 0.25, 0.5) and a[15:17] == (4, 3)  # itr, lr, lr_z; nv, va_every
    assert a[19:21] == (5, 1)  # nt, flags
    assert np.array_equal(_grab(a[2], X.shape), X) and np.array_equal(_grab(a[3], y.shape), y)
    assert np.array_equal(_grab(a[6], Z.shape), Z) and np.array_equal(_grab(a[8], th.shape), th)
    assert np.array_equal(_grab(a[13], Xv.shape), Xv) and np.array_equal(_grab(a[14], yv.shape), yv)
    assert np.array_equal(_grab(a[17], Xt.shape), Xt) and np.array_equal(_grab(a[18], yt.shape), yt)
    assert type(res) is gpscore.FitcValidatedTrainResult
    assert isinstance(res, gpscore.ValidatedTrainResult)
    # the outputs are the result's own arrays; va_sc and va_z stand between sc and info
    assert ctypes.addressof(a[21].contents) == res.theta.ctypes.data
    assert ctypes.addressof(a[22].contents) == res.Z.ctypes.data
    assert ctypes.addressof(a[23].contents) == res.series["objective"].ctypes.data
    assert ctypes.addressof(a[24].contents) == res.series["theta"].ctypes.data
    assert ctypes.addressof(a[26].contents) == res.mu.ctypes.data
    assert ctypes.addressof(a[27].contents) == res.var.ctypes.data
    assert a[29] is not None
    assert a[30] is None and res.va_Z is None and res.Z_best is None  # no select, no keep_z
    assert ctypes.addressof(a[31].contents) == res.info.ctypes.data
    assert ctypes.addressof(a[32].contents) == res.steps_done.ctypes.data
    assert list(res.va_steps) == [0, 3, 6, 7]
    assert set(res.va_scores) == set(gpscore.SCORE_NAMES)
    assert all(v.shape == (3, 4) for v in res.va_scores.values())
    assert res.best_step is None and res.theta_best is None
    assert res.series["theta"].shape == (3, 7, 4) and res.mu.shape == (3, 5) and res.Z.shape == Z.shape

    # va_z is a pointer with keep_z or with select, the result's own (B, nva, m, d) array
    for kw in (dict(keep_z=True), dict(select="mse"), dict(select="crps", keep_z=True)):
        res = gpscore.fitc_train_tall_validated(X, y, Z, th, Xv, yv, itr=7, va_every=3, ctx=ctx, **kw)
        a = ctx.args[-1]
        assert res.va_Z.shape == (3, 4, 4, 2)
        assert ctypes.addressof(a[30].contents) == res.va_Z.ctypes.data
        assert (res.Z_best is None) == ("select" not in kw)

    # the block call: nfold behind the objective code, everything else one slot later; d = 1 from
    # (B, n) / (B, nv) / (B, m) arrays, no test rows
    n0 = len(ctx.calls)
    res = gpscore.fitc_blockloo_train_tall_validated(X[:, :, 0], y, Z[:, :, 0], (0.0, 0.0, -1.0),
                                                     Xv[:, :, 0], yv, "kc", nfold=5, lr=0.5, itr=0,
                                                     ctx=ctx)
    assert ctx.calls[n0:] == [VA[1]]
    b = ctx.args[-1]
    assert len(b) == 34
    assert b[:3] == (1, 5, 3) and b[5:7] == (10, 1) and b[8] == 4 and b[10] == 1
    assert b[11:14] == (0, 0.5, 0.5) and b[16:18] == (4, 1)  # itr, lr, lr_z = lr; nv, va_every
    assert b[18] is None and b[19] is None and b[20:22] == (0, 0)
    assert b[27] is None and b[28] is None and b[29] is None  # mu, var, sc
    assert b[30] is not None and b[31] is None and list(res.va_steps) == [0] and res.mu is None
    res = gpscore.fitc_blockloo_train_tall_validated(X, y, Z, th, Xv, yv, keep_z=True, itr=2,
                                                     ctx=ctx)
    assert ctypes.addressof(ctx.args[-1][31].contents) == res.va_Z.ctypes.data
    # the defaults are those of the plain wrappers
    gpscore.fitc_train_tall_validated(X, y, Z, (0.0, 0.0, -1.0), Xv, yv, ctx=ctx)
    gpscore.fitc_blockloo_train_tall_validated(X, y, Z, (0.0, 0.0, -1.0), Xv, yv, ctx=ctx)
    c, e = ctx.args[-2], ctx.args[-1]
    assert c[0] == 1 and c[10:13] == (400, 1.0, 1.0) and c[16] == 1 and c[20] == 0
    assert e[:2] == (0, 4) and e[11:14] == (3000, 1e-3, 1e-3) and e[17] == 1


class _FillingCtx(_RecordingCtx):
    """A recording context whose gps_fitc_train_tall_va call returns hand-made θ and Z series,
    final θ and Z and score rows."""

    def __init__(self, va_sc, thetas, theta, va_z):
        super().__init__()
        self.va_sc, self.thetas, self.theta, self.va_z = va_sc, thetas, theta, va_z

    def call(self, name, *args):
        super().call(name, *args)
        assert name == VA[0]
        _grab(args[21], self.theta.shape)[...] = self.theta
        _grab(args[22], self.va_z[:, -1].shape)[...] = self.va_z[:, -1]
        _grab(args[24], self.thetas.shape)[...] = self.thetas
        _grab(args[29], self.va_sc.shape)[...] = self.va_sc
        _grab(args[30], self.va_z.shape)[...] = self.va_z


def test_z_selection_on_hand_made_rows():
    """itr = 7, va_every = 3: rows for steps 0, 3, 6 and the final pass (7).  Six problems: the
    minimum at step 0, at an interior step, at the final row (its Z is the returned one); a tie
    (the earliest wins); NaN rows skipped; all NaN (−1 and NaN)."""
    import gpscore
    from gpscore.batch import select_best_z
    B, itr, nth, m, d = 6, 7, 4, 3, 2
    rng = np.random.default_rng(5)
    X, y = rng.standard_normal((B, 10, d)), rng.standard_normal((B, 10))
    th0 = rng.standard_normal((B, nth))
    thetas = rng.standard_normal((B, itr, nth))
    theta = thetas[:, -1] + 0.0
    va_z = rng.standard_normal((B, 4, m, d))
    Z0 = va_z[:, 0] + 0.0
    nan = np.nan
    crps = np.array([[0.1, 0.5, 0.4, 0.3],
                     [0.9, 0.5, 0.2, 0.3],
                     [0.9, 0.5, 0.4, 0.1],
                     [0.7, 0.2, 0.2, 0.2],
                     [nan, 0.6, nan, 0.8],
                     [nan, nan, nan, nan]])
    va_sc = rng.standard_normal((B, 4, NSC)) + 5.0
    va_sc[:, :, 0] = crps
    Xv, yv = np.zeros((B, 3, d)), np.zeros((B, 3))
    ctx = _FillingCtx(va_sc, thetas, theta, va_z)
    res = gpscore.fitc_train_tall_validated(X, y, Z0, th0, Xv, yv, select="crps", itr=itr,
                                            va_every=3, ctx=ctx)
    assert list(res.va_steps) == [0, 3, 6, 7]
    assert list(res.best_step) == [0, 6, 7, 3, 3, -1]
    want_th = np.stack([th0[0], thetas[1, 5], theta[2], thetas[3, 2], thetas[4, 2],
                        np.full(nth, nan)])
    assert np.array_equal(res.theta_best, want_th, equal_nan=True)
    want_z = np.stack([va_z[0, 0], va_z[1, 2], va_z[2, 3], va_z[3, 1], va_z[4, 1],
                       np.full((m, d), nan)])
    assert np.array_equal(res.Z_best, want_z, equal_nan=True)
    assert np.array_equal(res.Z_best[2], res.Z[2])  # the final row picks the returned Z
    assert np.array_equal(res.va_Z, va_z)
    # the pick itself, beside select_best
    zb = select_best_z(np.array([7, -1, 0, 3, 6, 6]), res.va_steps, va_z)
    assert np.array_equal(zb[0], va_z[0, 3]) and np.isnan(zb[1]).all()
    assert np.array_equal(zb[2], va_z[2, 0]) and np.array_equal(zb[3], va_z[3, 1])
    assert np.array_equal(zb[4], va_z[4, 2])
    # itr = 0: the one row is the final pass, its Z the returned one
    ctx0 = _FillingCtx(np.ones((B, 1, NSC)), np.zeros((B, 0, nth)), th0 + 0.0, va_z[:, :1])
    res = gpscore.fitc_train_tall_validated(X, y, Z0, th0, Xv, yv, itr=0, select="logs", ctx=ctx0)
    assert list(res.best_step) == [0] * B and np.array_equal(res.Z_best, Z0)
    assert np.array_equal(res.theta_best, th0)


def test_run_fitc_validated_batch_draws_passes_the_split_and_refuses_es():
    from gpscore import experiment as E
    sheets = _sheets()
    TT, seed, m = 3, 11, 6

    class Ctx(_RecordingCtx):
        def call(self, name, *args):
            super().call(name, *args)
            o = 1 if "blockloo" in name else 0  # nfold behind the objective code
            B, n, dd, mm = args[1 + o], args[4 + o], args[5 + o], args[7 + o]
            nth = 2 + args[9 + o]
            g = lambda p, *s: _grab(p, s).copy()  # noqa: E731
            rec = dict(code=args[0], B=B, n=n, d=dd, m=mm, itr=args[10 + o], lr=args[11 + o],
                       lr_z=args[12 + o], X=g(args[2 + o], B, n, dd), y=g(args[3 + o], B, n),
                       Z0=g(args[6 + o], B, mm, dd), th0=g(args[8 + o], B, nth))
            if name.endswith("_va"):
                nv = args[15 + o]
                rec.update(nv=nv, va_every=args[16 + o], Xv=g(args[13 + o], B, nv, dd),
                           yv=g(args[14 + o], B, nv), nt=args[19 + o], flags=args[20 + o],
                           va_z=args[30 + o])
            self.args[-1] = rec

    es = E.Method("es", 25, 0.1)  # K20 has no energy-score method; KF's step count and rate
    for bad in ({"es": es}, {"crps": E.K20_METHODS["crps"], "es": es}):
        ctx = Ctx()
        with pytest.raises(ValueError, match=r"run_fitc_validated_batch: method 'es'.*run\(kind"):
            E.run_fitc_validated_batch(sheets, TT=2, methods=bad, ctx=ctx)
        assert ctx.calls == []
    ctx = Ctx()
    for bad in (0, 2.5):
        with pytest.raises(ValueError, match="va_every"):
            E.run_fitc_validated_batch(sheets, TT=2, va_every=bad, ctx=ctx)
    with pytest.raises(ValueError, match="select"):
        E.run_fitc_validated_batch(sheets, TT=2, select="cover", ctx=ctx)
    with pytest.raises(ValueError, match="TT"):
        E.run_fitc_validated_batch(sheets, TT=0, ctx=ctx)
    with pytest.raises(ValueError, match="m must be"):
        E.run_fitc_validated_batch(sheets, TT=2, m=0, ctx=ctx)
    assert ctx.calls == []

    # the pointwise methods: run_fitc_batch's problems, plus the validation split
    ctx, ref = Ctx(), Ctx()
    out = E.run_fitc_validated_batch(sheets, TT=TT, methods={k: E.K20_METHODS[k] for k in
                                                             ("crps", "nlml", "logs")},
                                     m=m, seed=seed, va_every=50, ctx=ctx)
    E.run_fitc_batch(sheets, TT=TT, m=m, seed=seed, ctx=ref)
    assert list(out) == ["crps", "nlml", "logs"] and ctx.calls == [VA[0]] * 3
    assert ref.calls == ["gps_fitc_train_tall"] * 3
    data = [E.replicate(sheets, j, n_pool=1200) for j in range(TT)]
    for a, r, name in zip(ctx.args, ref.args, out):
        for k in ("code", "B", "n", "d", "m", "itr", "lr", "lr_z"):
            assert a[k] == r[k], (name, k)
        for k in ("X", "y", "Z0", "th0"):
            assert np.array_equal(a[k], r[k]), (name, k)
        assert (a["nv"], a["va_every"], a["nt"], a["flags"]) == (300, 50, 40, 1)
        assert a["va_z"] is None  # no select: no Z is kept
        assert np.array_equal(a["Xv"], np.stack([dd["va_x"] for dd in data])), name
        assert np.array_equal(a["yv"], np.stack([dd["va_y"] for dd in data])), name
        nva = -(-E.K20_METHODS[name].itr // 50) + 1
        assert set(out[name]) == set(E.METRICS) | {"theta", "Z", "va_scores", "va_steps"}
        assert out[name]["va_scores"]["test_crps"].shape == (TT, nva)
        assert out[name]["va_steps"][-1] == E.K20_METHODS[name].itr

    # dss and kc go through the block call and fit run_fitc_blockloo_batch's problems
    ctx, ref = Ctx(), Ctx()
    blk = {k: E.K20_METHODS[k] for k in ("dss", "kc")}
    out = E.run_fitc_validated_batch(sheets, TT=TT, methods=blk, m=m, itr=3, seed=seed, ctx=ctx,
                                     nfold=5, select="crps")
    E.run_fitc_blockloo_batch(sheets, TT=TT, m=m, itr=3, seed=seed, ctx=ref, nfold=5)
    # with select, one more fitc_train_tall(itr=0) call a method unless every best row is the final
    va_calls = [c for c in ctx.calls if c.endswith("_va")]
    assert va_calls == [VA[1]] * 2 and ref.calls == ["gps_fitc_blockloo_train_tall"] * 2
    assert set(ctx.calls) <= {VA[1], "gps_fitc_train_tall"}
    va_args = [a for c, a in zip(ctx.calls, ctx.args) if c.endswith("_va")]
    for a, r, name in zip(va_args, ref.args, blk):
        for k in ("code", "B", "n", "d", "m", "itr", "lr", "lr_z"):
            assert a[k] == r[k], (name, k)
        for k in ("X", "y", "Z0", "th0"):
            assert np.array_equal(a[k], r[k]), (name, k)
        assert a["nv"] == 300 and a["va_every"] == 1 and a["va_z"] is not None
        assert set(out[name]) == set(E.METRICS) | {"theta", "Z", "failed", "va_scores", "va_steps",
                                                   "best_step", "selected"}
        assert set(out[name]["selected"]) == set(E.METRICS)
    ctx = Ctx()
    out = E.run_fitc_validated_batch(sheets, TT=2, itr=2, m=m, ctx=ctx)
    assert list(out) == ["crps", "nlml", "logs", "dss", "kc"]
    assert ctx.calls == [VA[0]] * 3 + [VA[1]] * 2
