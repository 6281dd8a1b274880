"""The tall batched full-GP energy-score path on the host (no GPU): its two C-ABI
entry points are declared, exported and bound and reject a NULL context; the Python wrappers and
experiment.run_full_es_batch refuse bad shapes, limits, fold counts, draw counts, β, draws and
draw sets before any library call; well-formed calls reach exactly the two new entry points with
the arguments in the right slots; run_full_es_batch takes its problems and draws from the generator
in run's order and turns a nonzero info into zero metrics; the older routes still refuse "es"."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_full_tall_host import _RecordingCtx, _ok, _sheets

ES_TALL = ("gps_full_es_grad_tall", "gps_full_es_train_tall")


def test_header_declares_and_binding_covers_the_es_calls():
    from gpscore import _lib
    txt = open(os.path.join(ROOT, "include", "gpscore.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(gps_\w+)\s*\(", code))
    lib = _lib.load()
    for s in ES_TALL:
        assert s in declared, s
        assert s in _lib.SIGNATURES, s
        assert hasattr(lib, s), s
    # gps_full_blockloo_*_tall's argument lists with (nfold, num_sim, beta) in the place of
    # (objective, nfold), the draws after θ (value + gradient) and draws, draw_sets after the flags
    bg = _lib.SIGNATURES["gps_full_blockloo_grad_tall"][1]
    bt = _lib.SIGNATURES["gps_full_blockloo_train_tall"][1]
    eg, et = (_lib.SIGNATURES[s][1] for s in ES_TALL)
    head = [ctypes.c_int, ctypes.c_int, ctypes.c_double]
    assert eg == bg[:2] + head + bg[4:11] + [_lib._P] + bg[11:]
    assert et == bt[:2] + head + bt[4:17] + [_lib._P, ctypes.c_int64] + bt[17:]
    assert lib.gps_version() == _lib.ABI_VERSION
    import gpscore
    assert gpscore.es_train_tall is gpscore.batch.es_train_tall
    assert gpscore.es_value_and_grad_tall is gpscore.batch.es_value_and_grad_tall


def test_es_calls_reject_null_context():
    from gpscore import _lib
    lib = _lib.load()
    z = np.zeros(64)
    iz = np.zeros(2, np.int32)
    P = _lib.ptr
    I = iz.ctypes.data_as(_lib._PI)
    rc = lib.gps_full_es_grad_tall(None, 0, 2, 2, 1.0, 1, P(z), P(z), 2, 1, P(z), 1, P(z), P(z),
                                   P(z), P(z), P(z), I)
    assert rc == -1
    assert b"NULL" in lib.gps_last_error(None)
    rc = lib.gps_full_es_train_tall(None, 0, 2, 2, 1.0, 1, P(z), P(z), 2, 1, P(z), 1, 3, 0.1, None,
                                    None, 0, 0, P(z), 1, P(z), None, None, None, None, None, None,
                                    I, I)
    assert rc == -1
    assert b"NULL" in lib.gps_last_error(None)


def test_es_wrappers_refuse_before_any_call():
    import gpscore
    ctx = _RecordingCtx()
    X, y = _ok()  # B = 3, n = 10, d = 2
    th = (0.0, 0.0, -1.0)
    kw = dict(num_sim=4, rng=0)
    both = (lambda *a, **k: gpscore.es_value_and_grad_tall(*a, ctx=ctx, **{**kw, **k}),
            lambda *a, **k: gpscore.es_train_tall(*a, lr=0.1, itr=2, ctx=ctx, **{**kw, **k}))
    for f in both:
        with pytest.raises(ValueError, match="n = 513"):
            f(np.zeros((2, 513, 1)), np.zeros((2, 513)), th)
        with pytest.raises(ValueError, match="d = 17"):
            f(np.zeros((2, 5, 17)), np.zeros((2, 5)), th)
        with pytest.raises(ValueError, match="empty"):
            f(np.zeros((0, 5, 2)), np.zeros((0, 5)), th)
        with pytest.raises(ValueError, match="log_ell"):  # n_ell = 3 with d = 2
            f(X, y, (0.0, np.zeros(3), -1.0))
        with pytest.raises(ValueError, match="disagree"):
            f(X, y[:, :-1], th)
        with pytest.raises(ValueError, match="rectangular"):  # a ragged list of problems
            f([np.zeros((4, 2)), np.zeros((5, 2))], [np.zeros(4), np.zeros(5)], th)
        for bad in (1, 0, -4, 11, 33, 2.5):  # n = 10: 2..10
            with pytest.raises(ValueError, match="nfold"):
                f(X, y, th, nfold=bad)
        with pytest.raises(ValueError, match="at most 128 rows"):  # folds of 129 rows
            f(np.zeros((1, 258, 1)), np.zeros((1, 258)), th, nfold=2)
        with pytest.raises(ValueError, match="at most 128 rows"):
            f(np.zeros((1, 512, 1)), np.zeros((1, 512)), th, nfold=3)
        for bad in (1, 513, 0, 7.5):
            with pytest.raises(ValueError, match="num_sim"):
                f(X, y, th, num_sim=bad)
        for bad in (0.0, 2.5, -1.0, np.nan):
            with pytest.raises(ValueError, match="beta"):
                f(X, y, th, beta=bad)
    V, T = gpscore.es_value_and_grad_tall, gpscore.es_train_tall
    per = 2 * 4 * 10
    with pytest.raises(ValueError, match="draws must hold"):  # one set a problem, not two
        V(X, y, th, num_sim=4, draws=np.zeros((3, 2, per)), ctx=ctx)
    with pytest.raises(ValueError, match="draws must hold"):
        V(X, y, th, num_sim=4, draws=np.zeros((3, per - 1)), ctx=ctx)
    with pytest.raises(ValueError, match="draws must hold"):  # itr = 2 sets by default
        T(X, y, th, num_sim=4, itr=2, draws=np.zeros((3, 1, per)), ctx=ctx)
    with pytest.raises(ValueError, match="draws must hold"):
        T(X, y, th, num_sim=4, itr=2, draws=np.zeros((3, 2, per)), draw_sets=1, ctx=ctx)
    with pytest.raises(ValueError, match="rectangular"):
        T(X, y, th, num_sim=4, itr=2, draws=[np.zeros(3), np.zeros(4)], ctx=ctx)
    for bad in (0, 3, -1, 1.5):  # itr = 2: 1..2
        with pytest.raises(ValueError, match="draw_sets"):
            T(X, y, th, itr=2, draw_sets=bad, ctx=ctx, **kw)
    with pytest.raises(ValueError, match="draw_sets"):  # itr = 0: one set
        T(X, y, th, itr=0, draw_sets=2, ctx=ctx, **kw)
    with pytest.raises(ValueError, match="itr"):
        T(X, y, th, itr=-1, ctx=ctx, **kw)
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="lr"):
            T(X, y, th, lr=bad, itr=2, ctx=ctx, **kw)
    with pytest.raises(ValueError, match="Xt"):
        T(X, y, th, itr=2, Xt=np.zeros((3, 4, 5)), ctx=ctx, **kw)
    with pytest.raises(ValueError, match="yt without Xt"):
        T(X, y, th, itr=2, yt=np.zeros((3, 5)), ctx=ctx, **kw)
    assert ctx.calls == []


def test_old_routes_still_refuse_es():
    import gpscore
    from gpscore import experiment as E
    ctx = _RecordingCtx()
    X, y = _ok()
    th = (0.0, 0.0, -1.0)
    with pytest.raises(ValueError, match="objective"):
        gpscore.blockloo_value_and_grad_tall(X, y, th, "es", ctx=ctx)
    with pytest.raises(ValueError, match="objective"):
        gpscore.blockloo_train_tall(X, y, th, "es", lr=0.1, itr=1, ctx=ctx)
    with pytest.raises(ValueError, match="objective"):
        gpscore.train_tall(X, y, th, "es", lr=0.1, itr=1, ctx=ctx)
    sheets = _sheets()
    with pytest.raises(ValueError, match=r"run\(kind=\"full\"\)"):
        E.run_full_blockloo_batch(sheets, TT=2, methods={"es": E.KF_METHODS["es"]}, ctx=ctx)
    with pytest.raises(ValueError, match=r"run\(kind"):
        E.run_full_batch(sheets, TT=2, methods={"es": E.KF_METHODS["es"]}, ctx=ctx)
    assert ctx.calls == []


def test_well_formed_calls_reach_exactly_the_es_entry_points():
    """kind, nfold, num_sim, β, the flags and draw_sets sit in their slots; the limits themselves
    (n = 512 with four folds of 128, num_sim = 512, β = 2) are accepted."""
    import gpscore
    from gpscore._lib import GPS_ARD, GPS_RBF
    ctx = _RecordingCtx()
    X, y = _ok()
    out = gpscore.es_value_and_grad_tall(X, y, (0.0, 0.0, -1.0), nfold=5, num_sim=6, beta=1.5,
                                         rng=1, ctx=ctx)
    res = gpscore.es_train_tall(X[:, :, 0], y, np.zeros((3, 3)), nfold=3, num_sim=7, lr=0.5, itr=0,
                                Xt=np.zeros((3, 4)), yt=np.zeros((3, 4)), rbf=True,
                                stale_noise=True, rng=1, ctx=ctx)
    assert ctx.calls == list(ES_TALL)
    vals, grads, folds, objs, info = out
    assert vals.shape == (3,) and grads.shape == (3, 3) and folds.shape == (3, 5)
    assert set(objs) == set(gpscore.OBJ_NAMES) and info.shape == (3,)
    assert type(res) is gpscore.BatchTrainResult
    assert res.theta.shape == (3, 3) and res.series["theta"].shape == (3, 0, 3)
    assert res.mu.shape == (3, 4) and set(res.scores) == set(gpscore.SCORE_NAMES)
    a, b = ctx.args
    assert a[:5] == (GPS_ARD, 5, 6, 1.5, 3) and a[7:9] == (10, 2) and a[10] == 1
    assert b[:5] == (GPS_RBF, 3, 7, 1.0, 3) and b[7:9] == (10, 1) and b[10] == 1
    assert b[11] == 0 and b[12] == 0.5 and b[15] == 4 and b[16] == 1  # itr, lr, nt, flags
    assert b[18] == 1  # itr = 0: one draw set
    big = (np.zeros((1, 512, 16)), np.zeros((1, 512)), (0.0, np.zeros(16), -1.0))
    gpscore.es_value_and_grad_tall(*big, nfold=4, num_sim=512, beta=2.0, rng=1, ctx=ctx)
    gpscore.es_train_tall(*big, nfold=4, num_sim=512, beta=2.0, lr=0.1, itr=2, draw_sets=1, rng=1,
                          ctx=ctx)
    assert ctx.calls[2:] == list(ES_TALL)
    for c in ctx.args[2:]:
        assert c[1:4] == (4, 512, 2.0) and c[7:9] == (512, 16) and c[10] == 16
    assert ctx.args[3][18] == 1
    # the defaults are the ES fit of kin40k-FULL-compare.py: 25 steps at 0.1, 300 draws, 25 sets
    gpscore.es_train_tall(X, y, (0.0, 0.0, -1.0), rng=1, ctx=ctx)
    c = ctx.args[-1]
    assert c[:4] == (GPS_ARD, 4, 300, 1.0) and c[11] == 25 and c[12] == 0.1 and c[16] == 0
    assert c[18] == 25


def test_default_draws_are_problem_major_then_set_major():
    """draws=None takes es_draws from rng once per (problem, set), problems outermost."""
    import gpscore
    from gpscore.gp import es_draws
    B, n, S, nfold, itr = 3, 10, 4, 3, 2
    per = 2 * S * n

    class Ctx(_RecordingCtx):
        def call(self, name, *args):
            super().call(name, *args)
            p = args[17]
            self.draws = np.ctypeslib.as_array(
                ctypes.cast(p, ctypes.POINTER(ctypes.c_double)), (B * itr * per,)).copy()

    ctx = Ctx()
    X, y = _ok()
    gpscore.es_train_tall(X, y, (0.0, 0.0, -1.0), nfold=nfold, num_sim=S, itr=itr,
                          rng=np.random.default_rng(5), ctx=ctx)
    rng = np.random.default_rng(5)
    want = np.concatenate([es_draws(n, nfold, S, rng) for _ in range(B * itr)])
    assert np.array_equal(ctx.draws, want)


def test_run_full_es_batch_refusals():
    from gpscore import experiment as E
    ctx = _RecordingCtx()
    sheets = _sheets()
    for name in ("crps", "nlml", "logs"):
        with pytest.raises(ValueError, match="run_full_batch"):
            E.run_full_es_batch(sheets, TT=2, methods={name: E.KF_METHODS[name]}, ctx=ctx)
    with pytest.raises(ValueError, match="run_full_blockloo_batch"):
        E.run_full_es_batch(sheets, TT=2, methods={"es": E.KF_METHODS["es"],
                                                   "dss": E.KF_METHODS["dss"]}, ctx=ctx)
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match="TT"):
            E.run_full_es_batch(sheets, TT=bad, ctx=ctx)
    with pytest.raises(ValueError, match="itr"):
        E.run_full_es_batch(sheets, TT=2, itr=-1, num_sim=4, ctx=ctx)
    assert ctx.calls == []


def test_run_full_es_batch_draws_in_runs_order_and_calls_once_per_method():
    """One gps_full_es_train_tall call for all TT replicates; θ0 and every step's draws are what
    run_method and GP.train would take from the generator: replicate-major, initial_theta first,
    then one es_draws set per step — checked against run_method's own draws in run's loop order,
    with GP.block_loo stubbed.  A nonzero info gives zero metrics and failed = True."""
    from gpscore import experiment as E
    from gpscore._lib import GPS_ARD
    from gpscore.gp import GP, es_draws
    sheets = _sheets()
    TT, d, seed, S, itr = 3, 3, 11, 5, 2
    per = 2 * S * 500

    class Ctx(_RecordingCtx):
        def call(self, name, *args):
            super().call(name, *args)
            B, n, dd = args[4], args[7], args[8]
            nth = 2 + args[10]
            grab = lambda p, k: np.ctypeslib.as_array(  # noqa: E731
                ctypes.cast(p, ctypes.POINTER(ctypes.c_double)), (k,)).copy()
            self.args[-1] = dict(kind=args[0], nfold=args[1], S=args[2], beta=args[3], B=B, n=n,
                                 d=dd, itr=args[11], lr=args[12], nt=args[15], flags=args[16],
                                 sets=args[18],
                                 X=grab(args[5], B * n * dd).reshape(B, n, dd),
                                 y=grab(args[6], B * n).reshape(B, n),
                                 th0=grab(args[9], B * nth).reshape(B, nth),
                                 draws=grab(args[17], B * args[18] * per).reshape(B, args[18], per))
            info = np.ctypeslib.as_array(args[26], (B,))
            info[1] = 7  # replicate 1 fails
            sc = np.ctypeslib.as_array(ctypes.cast(args[25], ctypes.POINTER(ctypes.c_double)),
                                       (B * 6,))
            sc[:] = 0.5

    ctx = Ctx()
    out = E.run_full_es_batch(sheets, TT=TT, seed=seed, itr=itr, num_sim=S, ctx=ctx)
    assert list(out) == ["es"] and ctx.calls == ["gps_full_es_train_tall"]
    a = ctx.args[0]
    assert (a["kind"], a["nfold"], a["S"], a["beta"]) == (GPS_ARD, 4, S, 1.0)
    assert (a["B"], a["n"], a["d"], a["nt"]) == (TT, 500, d, 40)
    assert (a["itr"], a["lr"], a["flags"], a["sets"]) == (itr, 0.1, 1, itr)
    assert set(out["es"]) == set(E.METRICS) | {"theta", "failed"}
    assert list(out["es"]["failed"]) == [False, True, False]
    for k in E.METRICS:
        assert list(out["es"][k]) == [0.5, 0.0, 0.5], k
    # KF's own step count and draw count by default
    ctx2 = _RecordingCtx()
    E.run_full_es_batch(sheets, TT=1, seed=seed, num_sim=2, ctx=ctx2)
    assert ctx2.args[0][11] == 25 and ctx2.args[0][12] == 0.1 and ctx2.args[0][18] == 25

    seen = []

    class StubGP(GP):
        def __init__(self):
            self._n = 0

        def set_data(self, X, y, kind="full", Z=None):
            self._X, self._y = np.array(X), np.array(y)
            seen.append({"X": self._X, "y": self._y, "draws": []})

        def block_loo(self, theta, objective="dss", nfold=4, grad=False, rbf=False, num_sim=300,
                      beta=1.0, draws=None, rng=None):
            assert objective == "es" and num_sim == S
            if not seen[-1]["draws"]:
                seen[-1]["th0"] = np.concatenate([[theta[0]], np.ravel(theta[1]), [theta[2]]])
            seen[-1]["draws"].append(es_draws(self._X.shape[0], nfold, num_sim, rng))
            g = np.zeros(2 + np.size(theta[1]))
            return 0.0, g, np.zeros(nfold)

        def fit(self, *a, **k):
            return None

        def predict(self, *a, **k):
            return None, None, {"test_" + m: 0.0 for m in E.METRICS}

        kind = "full"

    rng = np.random.default_rng(seed)
    meth = E.KF_METHODS["es"]
    for j in range(TT):
        data = E.replicate(sheets, j, n_pool=1200)
        E.run_method(StubGP(), data, meth, rng, itr=itr, num_sim=S)
    assert len(seen) == TT
    for j, s in enumerate(seen):
        assert np.array_equal(a["th0"][j], s["th0"]), j
        assert np.array_equal(a["X"][j], s["X"]) and np.array_equal(a["y"][j], s["y"]), j
        assert len(s["draws"]) == itr
        for i in range(itr):
            assert np.array_equal(a["draws"][j, i], s["draws"][i]), (j, i)
