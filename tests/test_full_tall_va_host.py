"""The validated tall full-GP fits on the host (no GPU): the two C-ABI entry points
are declared, bound (ABI still 900) and reject a NULL context; train_tall_validated and
blockloo_train_tall_validated refuse a bad validation set, va_every and select before any library
call and hand the library the argument list position by position; va_steps; the selection on
hand-made score rows a stub context returns; run_full_validated_batch draws what run_full_batch
draws, passes the validation split and refuses es."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_full_tall_host import _RecordingCtx, _ok, _sheets

VA = ("gps_full_train_tall_va", "gps_full_blockloo_train_tall_va")
NSC = 6


def _grab(p, shape):
    k = int(np.prod(shape))
    return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_double)), (k,)).reshape(shape)


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
    # the plain calls' lists with Xv, yv, nv, va_every in front of Xt and va_sc in front of info
    P, i64 = _lib._P, ctypes.c_int64
    t = _lib.SIGNATURES["gps_full_train_tall"][1]
    bt = _lib.SIGNATURES["gps_full_blockloo_train_tall"][1]
    assert _lib.SIGNATURES[VA[0]][1] == t[:12] + [P, P, i64, i64] + t[12:23] + [P] + t[23:]
    assert _lib.SIGNATURES[VA[1]][1] == bt[:13] + [P, P, i64, i64] + bt[13:24] + [P] + bt[24:]
    assert _lib.ABI_VERSION == 900 and lib.gps_version() == 900


def test_va_calls_reject_null_context():
    from gpscore import _lib
    lib = _lib.load()
    z = np.zeros(16)
    iz = np.zeros(2, np.int32)
    P = _lib.ptr
    I = iz.ctypes.data_as(_lib._PI)
    rc = lib.gps_full_train_tall_va(None, 0, 1, 1, P(z), P(z), 2, 1, P(z), 1, 3, 0.1, P(z), P(z), 2,
                                    1, None, None, 0, 0, P(z), None, None, None, None, None, None,
                                    P(z), I, I)
    assert rc == -1
    assert b"NULL" in lib.gps_last_error(None)
    rc = lib.gps_full_blockloo_train_tall_va(None, 0, 0, 2, 1, P(z), P(z), 2, 1, P(z), 1, 3, 0.1,
                                             P(z), P(z), 2, 1, None, None, 0, 0, P(z), None, None,
                                             None, None, None, None, P(z), I, I)
    assert rc == -1
    assert b"NULL" in lib.gps_last_error(None)


def test_validated_wrappers_refuse_before_any_call():
    import gpscore
    ctx = _RecordingCtx()
    X, y = _ok()  # B = 3, n = 10, d = 2
    th = (0.0, 0.0, -1.0)
    Xv, yv = np.zeros((3, 4, 2)), np.zeros((3, 4))
    both = (lambda *a, **k: gpscore.train_tall_validated(*a, lr=0.1, itr=2, ctx=ctx, **k),
            lambda *a, **k: gpscore.blockloo_train_tall_validated(*a, lr=0.1, itr=2, ctx=ctx, **k))
    for f in both:
        with pytest.raises(ValueError, match=r"Xv must be \(B, nv, d\)"):
            f(X, y, th, np.zeros((3, 4, 5)), yv)  # the wrong d
        with pytest.raises(ValueError, match=r"Xv must be \(B, nv, d\)"):
            f(X, y, th, np.zeros((2, 4, 2)), yv)  # the wrong B
        with pytest.raises(ValueError, match=r"Xv must be \(B, nv, d\)"):
            f(X, y, th, np.zeros((3, 4)), yv)  # (B, nv) only stands for d = 1
        with pytest.raises(ValueError, match="Xv holds no rows"):
            f(X, y, th, np.zeros((3, 0, 2)), np.zeros((3, 0)))
        with pytest.raises(ValueError, match="Xv must be a rectangular"):
            f(X, y, th, [np.zeros((4, 2)), np.zeros((5, 2)), np.zeros((4, 2))], yv)
        with pytest.raises(ValueError, match=r"yv must be \(B, nv\)"):
            f(X, y, th, Xv, np.zeros((3, 5)))
        with pytest.raises(ValueError, match=r"yv must be \(B, nv\)"):
            f(X, y, th, Xv, np.zeros(4))
        with pytest.raises(ValueError, match="yv is required"):
            f(X, y, th, Xv, None)
        with pytest.raises(ValueError, match="Xv is required"):
            f(X, y, th, None, yv)
        for bad in (0, -3, 2.5, 1.0, True, "2"):
            with pytest.raises(ValueError, match="va_every"):
                f(X, y, th, Xv, yv, va_every=bad)
        for bad in ("cover", "test_crps", "nlml", "", 0):
            with pytest.raises(ValueError, match="select"):
                f(X, y, th, Xv, yv, select=bad)
        # the plain wrappers' refusals still come first
        with pytest.raises(ValueError, match="disagree"):
            f(X, y[:, :-1], th, Xv, yv)
        with pytest.raises(ValueError, match="yt without Xt"):
            f(X, y, th, Xv, yv, yt=np.zeros((3, 5)))
    with pytest.raises(ValueError, match="objective"):
        gpscore.train_tall_validated(X, y, th, Xv, yv, "dss", ctx=ctx)
    with pytest.raises(ValueError, match="objective"):
        gpscore.blockloo_train_tall_validated(X, y, th, Xv, yv, "loo_crps", ctx=ctx)
    with pytest.raises(ValueError, match="nfold"):
        gpscore.blockloo_train_tall_validated(X, y, th, Xv, yv, "dss", nfold=11, ctx=ctx)
    assert ctx.calls == []


def test_argument_lists_position_by_position():
    import gpscore
    from gpscore._lib import GPS_ARD, GPS_RBF
    ctx = _RecordingCtx()
    X, y = _ok()
    rng = np.random.default_rng(1)
    Xv, yv = rng.standard_normal((3, 4, 2)), rng.standard_normal((3, 4))
    Xt, yt = rng.standard_normal((3, 5, 2)), rng.standard_normal((3, 5))
    th = rng.standard_normal((3, 4))
    res = gpscore.train_tall_validated(X, y, th, Xv, yv, "loo_logs", lr=0.25, itr=7, va_every=3,
                                       Xt=Xt, yt=yt, rbf=True, stale_noise=True, ctx=ctx)
    assert ctx.calls == [VA[0]]
    a = ctx.args[0]
    assert len(a) == 29
    assert a[:3] == (GPS_RBF, 2, 3) and a[5:7] == (10, 2) and a[8] == 2
    assert a[9] == 7 and a[10] == 0.25 and a[13] == 4 and a[14] == 3  # itr, lr, nv, va_every
    assert a[17] == 5 and a[18] == 1  # nt, flags
    assert np.array_equal(_grab(a[3], X.shape), X) and np.array_equal(_grab(a[4], y.shape), y)
    assert np.array_equal(_grab(a[7], th.shape), th)
    assert np.array_equal(_grab(a[11], Xv.shape), Xv) and np.array_equal(_grab(a[12], yv.shape), yv)
    assert np.array_equal(_grab(a[15], Xt.shape), Xt) and np.array_equal(_grab(a[16], yt.shape), yt)
    assert type(res) is gpscore.ValidatedTrainResult and isinstance(res, gpscore.BatchTrainResult)
    # the outputs are the result's own arrays, va_sc (B, nva, 6) between sc and info
    assert ctypes.addressof(a[19].contents) == res.theta.ctypes.data
    assert ctypes.addressof(a[20].contents) == res.series["objective"].ctypes.data
    assert ctypes.addressof(a[21].contents) == res.series["theta"].ctypes.data
    assert ctypes.addressof(a[23].contents) == res.mu.ctypes.data
    assert ctypes.addressof(a[24].contents) == res.var.ctypes.data
    assert ctypes.addressof(a[27].contents) == res.info.ctypes.data
    assert ctypes.addressof(a[28].contents) == res.steps_done.ctypes.data
    assert list(res.va_steps) == [0, 3, 6, 7]
    assert set(res.va_scores) == set(gpscore.SCORE_NAMES)
    assert all(v.shape == (3, 4) for v in res.va_scores.values())
    assert res.best_step is None and res.theta_best is None
    assert res.series["theta"].shape == (3, 7, 4) and res.mu.shape == (3, 5)

    # the block call: nfold behind the objective code, everything else one slot later; d = 1 from
    # (B, n) / (B, nv) arrays, no test rows
    res = gpscore.blockloo_train_tall_validated(X[:, :, 0], y, (0.0, 0.0, -1.0), Xv[:, :, 0], yv,
                                                "kc", nfold=5, lr=0.5, itr=0, ctx=ctx)
    assert ctx.calls == list(VA)
    b = ctx.args[1]
    assert len(b) == 30
    assert b[:4] == (GPS_ARD, 1, 5, 3) and b[6:8] == (10, 1) and b[9] == 1
    assert b[10] == 0 and b[11] == 0.5 and b[14] == 4 and b[15] == 1  # itr, lr, nv, va_every
    assert b[16] is None and b[17] is None and b[18] == 0 and b[19] == 0
    assert b[24] is None and b[25] is None and b[26] is None  # mu, var, sc
    assert b[27] is not None and list(res.va_steps) == [0] and res.mu is None
    # the defaults are those of the plain wrappers
    gpscore.train_tall_validated(X, y, (0.0, 0.0, -1.0), Xv, yv, ctx=ctx)
    gpscore.blockloo_train_tall_validated(X, y, (0.0, 0.0, -1.0), Xv, yv, ctx=ctx)
    c, e = ctx.args[2], ctx.args[3]
    assert c[:2] == (GPS_ARD, 1) and c[9] == 400 and c[10] == 1.0 and c[14] == 1 and c[18] == 0
    assert e[:3] == (GPS_ARD, 0, 4) and e[10] == 150 and e[11] == 1e-3 and e[15] == 1


@pytest.mark.parametrize("itr,every,want", [(0, 1, [0]), (1, 1, [0, 1]), (10, 3, [0, 3, 6, 9, 10]),
                                            (9, 3, [0, 3, 6, 9]), (5, 7, [0, 5])])
def test_va_steps(itr, every, want):
    import gpscore
    ctx = _RecordingCtx()
    X, y = _ok()
    res = gpscore.train_tall_validated(X, y, (0.0, 0.0, -1.0), np.zeros((3, 4, 2)),
                                       np.zeros((3, 4)), itr=itr, va_every=every, ctx=ctx)
    assert list(res.va_steps) == want and res.va_steps.dtype == np.int64
    assert len(want) == -(-itr // every) + 1
    assert res.va_scores["test_crps"].shape == (3, len(want))
    a = ctx.args[0]
    assert a[9] == itr and a[14] == every


class _FillingCtx(_RecordingCtx):
    """A recording context whose gps_full_train_tall_va call returns hand-made θ series, final θ
    and score rows."""

    def __init__(self, va_sc, thetas, theta):
        super().__init__()
        self.va_sc, self.thetas, self.theta = va_sc, thetas, theta

    def call(self, name, *args):
        super().call(name, *args)
        assert name == VA[0]
        _grab(args[19], self.theta.shape)[...] = self.theta
        _grab(args[21], self.thetas.shape)[...] = self.thetas
        _grab(args[26], self.va_sc.shape)[...] = self.va_sc


def test_selection_on_hand_made_rows():
    """itr = 7, va_every = 3: rows for steps 0, 3, 6 and the final pass (7).  Six problems: the
    minimum at step 0, at an interior step, at the final row; a tie (the earliest wins); NaN rows
    skipped; all NaN."""
    import gpscore
    B, itr, nth = 6, 7, 4
    rng = np.random.default_rng(5)
    X, y = rng.standard_normal((B, 10, 2)), rng.standard_normal((B, 10))
    th0 = rng.standard_normal((B, nth))
    thetas = rng.standard_normal((B, itr, nth))
    theta = thetas[:, -1] + 0.0
    nan = np.nan
    crps = np.array([[0.1, 0.5, 0.4, 0.3],
                     [0.9, 0.5, 0.2, 0.3],
                     [0.9, 0.5, 0.4, 0.1],
                     [0.7, 0.2, 0.2, 0.2],
                     [nan, 0.6, nan, 0.8],
                     [nan, nan, nan, nan]])
    mse = crps[:, ::-1].copy()  # another metric, another choice
    va_sc = rng.standard_normal((B, 4, NSC)) + 5.0
    va_sc[:, :, 0] = crps
    va_sc[:, :, 4] = mse
    va_sc[:, :, 5] = -1.0  # cover is never what is minimised
    kw = dict(itr=itr, va_every=3)
    Xv, yv = np.zeros((B, 3, 2)), np.zeros((B, 3))
    ctx = _FillingCtx(va_sc, thetas, theta)
    res = gpscore.train_tall_validated(X, y, th0, Xv, yv, select="crps", ctx=ctx, **kw)
    assert list(res.va_steps) == [0, 3, 6, 7]
    assert np.array_equal(res.va_scores["test_crps"], crps, equal_nan=True)
    assert np.array_equal(res.va_scores["test_mse"], mse, equal_nan=True)
    assert list(res.best_step) == [0, 6, 7, 3, 3, -1] and res.best_step.shape == (B,)
    want = np.stack([th0[0], thetas[1, 5], theta[2], thetas[3, 2], thetas[4, 2],
                     np.full(nth, nan)])
    assert np.array_equal(res.theta_best, want, equal_nan=True)
    res = gpscore.train_tall_validated(X, y, th0, Xv, yv, select="mse", ctx=ctx, **kw)
    assert list(res.best_step) == [7, 3, 0, 0, 6, -1]
    want = np.stack([theta[0], thetas[1, 2], th0[2], th0[3], thetas[4, 5], np.full(nth, nan)])
    assert np.array_equal(res.theta_best, want, equal_nan=True)
    # infinities are not finite rows either; without select nothing is chosen
    va_sc[0, 0, 0] = -np.inf
    res = gpscore.train_tall_validated(X, y, th0, Xv, yv, select="crps", ctx=ctx, **kw)
    assert res.best_step[0] == 7
    res = gpscore.train_tall_validated(X, y, th0, Xv, yv, ctx=ctx, **kw)
    assert res.best_step is None and res.theta_best is None
    # itr = 0: the one row is the final pass, its θ the returned one
    ctx0 = _FillingCtx(np.ones((B, 1, NSC)), np.zeros((B, 0, nth)), th0 + 0.0)
    res = gpscore.train_tall_validated(X, y, th0, Xv, yv, itr=0, select="logs", ctx=ctx0)
    assert list(res.best_step) == [0] * B and np.array_equal(res.theta_best, th0)


def test_run_full_validated_batch_draws_passes_the_split_and_refuses_es():
    from gpscore import experiment as E
    sheets = _sheets()
    TT, d, seed = 3, 3, 11

    class Ctx(_RecordingCtx):
        def call(self, name, *args):
            super().call(name, *args)
            o = 1 if "blockloo" in name else 0  # nfold behind the objective code
            B, n, dd = args[2 + o], args[5 + o], args[6 + o]
            nth = 2 + args[8 + o]
            g = lambda p, *s: _grab(p, s).copy()  # noqa: E731
            rec = dict(code=args[1], B=B, n=n, d=dd, itr=args[9 + o], lr=args[10 + o],
                       X=g(args[3 + o], B, n, dd), y=g(args[4 + o], B, n),
                       th0=g(args[7 + o], B, nth))
            if name.endswith("_va"):
                nv = args[13 + o]
                rec.update(nv=nv, va_every=args[14 + o], Xv=g(args[11 + o], B, nv, dd),
                           yv=g(args[12 + o], B, nv), nt=args[17 + o], flags=args[18 + o])
            self.args[-1] = rec

    for bad in ({"es": E.KF_METHODS["es"]}, {"crps": E.KF_METHODS["crps"], "es": E.KF_METHODS["es"]}):
        ctx = Ctx()
        with pytest.raises(ValueError, match="run_full_es_batch"):
            E.run_full_validated_batch(sheets, TT=2, methods=bad, ctx=ctx)
        assert ctx.calls == []
    ctx = Ctx()
    for bad in (0, 2.5):
        with pytest.raises(ValueError, match="va_every"):
            E.run_full_validated_batch(sheets, TT=2, va_every=bad, ctx=ctx)
    with pytest.raises(ValueError, match="select"):
        E.run_full_validated_batch(sheets, TT=2, select="cover", ctx=ctx)
    with pytest.raises(ValueError, match="TT"):
        E.run_full_validated_batch(sheets, TT=0, ctx=ctx)
    assert ctx.calls == []

    # the pointwise methods: run_full_batch's problems, plus the validation split
    ctx, ref = Ctx(), Ctx()
    out = E.run_full_validated_batch(sheets, TT=TT, methods={k: E.KF_METHODS[k] for k in
                                                             ("crps", "nlml", "logs")},
                                     seed=seed, va_every=50, ctx=ctx)
    E.run_full_batch(sheets, TT=TT, seed=seed, ctx=ref)
    assert list(out) == ["crps", "nlml", "logs"] and ctx.calls == [VA[0]] * 3
    assert ref.calls == ["gps_full_train_tall"] * 3
    data = [E.replicate(sheets, j, n_pool=1200) for j in range(TT)]
    for a, r, name in zip(ctx.args, ref.args, out):
        for k in ("code", "B", "n", "d", "itr", "lr"):
            assert a[k] == r[k], (name, k)
        for k in ("X", "y", "th0"):
            assert np.array_equal(a[k], r[k]), (name, k)
        assert (a["nv"], a["va_every"], a["nt"], a["flags"]) == (300, 50, 40, 1)
        assert np.array_equal(a["Xv"], np.stack([dd["va_x"] for dd in data])), name
        assert np.array_equal(a["yv"], np.stack([dd["va_y"] for dd in data])), name
        nva = -(-E.KF_METHODS[name].itr // 50) + 1
        assert set(out[name]) == set(E.METRICS) | {"theta", "va_scores", "va_steps"}
        assert out[name]["va_scores"]["test_crps"].shape == (TT, nva)
        assert out[name]["va_steps"][-1] == E.KF_METHODS[name].itr

    # the default methods add dss, through the block call, and it fits run_full_blockloo_batch's
    # problems when it is the only method
    ctx, ref = Ctx(), Ctx()
    E.run_full_validated_batch(sheets, TT=TT, methods={"dss": E.KF_METHODS["dss"]}, seed=seed,
                               ctx=ctx, nfold=5)
    E.run_full_blockloo_batch(sheets, TT=TT, seed=seed, ctx=ref, nfold=5)
    assert ctx.calls == [VA[1]] and ref.calls == ["gps_full_blockloo_train_tall"]
    for k in ("X", "y", "th0"):
        assert np.array_equal(ctx.args[0][k], ref.args[0][k]), k
    assert ctx.args[0]["nv"] == 300 and ctx.args[0]["va_every"] == 1
    ctx = Ctx()
    out = E.run_full_validated_batch(sheets, TT=2, itr=2, ctx=ctx)
    assert list(out) == ["crps", "nlml", "logs", "dss"]
    assert ctx.calls == [VA[0]] * 3 + [VA[1]]
