"""The tall batched full-GP block-LOO path on the host (no GPU): its two C-ABI entry
points are declared, exported and bound (ABI still 900: the additions are purely additive) and
reject a NULL context; the Python wrappers and experiment.run_full_blockloo_batch refuse bad
shapes, limits, objectives, fold counts and steps before any library call; well-formed calls
reach exactly the two new entry points with the arguments in the right slots;
run_full_blockloo_batch draws its problems in run's order."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_full_tall_host import _RecordingCtx, _ok, _sheets

BLOCK_TALL = ("gps_full_blockloo_grad_tall", "gps_full_blockloo_train_tall")


def test_header_declares_and_binding_covers_the_block_calls():
    from gpscore import _lib
    txt = open(os.path.join(ROOT, "include", "gpscore.h")).read()
    assert "#define GPS_ABI_VERSION 900" in txt
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(gps_\w+)\s*\(", code))
    lib = _lib.load()
    for s in BLOCK_TALL:
        assert s in declared, s
        assert s in _lib.SIGNATURES, s
        assert hasattr(lib, s), s
    # gps_full_*_tall's argument lists with nfold after the objective, and value / fold_values
    # in front of the value + gradient call's outputs
    g, t = _lib.SIGNATURES["gps_full_grad_tall"][1], _lib.SIGNATURES["gps_full_train_tall"][1]
    bg = _lib.SIGNATURES["gps_full_blockloo_grad_tall"][1]
    bt = _lib.SIGNATURES["gps_full_blockloo_train_tall"][1]
    assert bt == t[:3] + [ctypes.c_int] + t[3:]
    assert bg == g[:3] + [ctypes.c_int] + g[3:10] + [_lib._P, _lib._P] + g[10:]
    assert _lib.ABI_VERSION == 900 and lib.gps_version() == 900
    assert re.search(r"GPS_BLOCK_DSS = 0, GPS_BLOCK_KC = 1, GPS_BLOCK_ES = 2", txt)


def test_block_calls_reject_null_context():
    from gpscore import _lib
    lib = _lib.load()
    z = np.zeros(8)
    iz = np.zeros(2, np.int32)
    P = _lib.ptr
    I = iz.ctypes.data_as(_lib._PI)
    rc = lib.gps_full_blockloo_grad_tall(None, 0, 0, 2, 1, P(z), P(z), 2, 1, P(z), 1, P(z), P(z),
                                         P(z), P(z), I)
    assert rc == -1
    assert b"NULL" in lib.gps_last_error(None)
    rc = lib.gps_full_blockloo_train_tall(None, 0, 0, 2, 1, P(z), P(z), 2, 1, P(z), 1, 3, 0.1, None,
                                          None, 0, 0, P(z), None, None, None, None, None, None, I, I)
    assert rc == -1
    assert b"NULL" in lib.gps_last_error(None)


def test_block_wrappers_refuse_before_any_call():
    import gpscore
    ctx = _RecordingCtx()
    X, y = _ok()  # B = 3, n = 10, d = 2
    th = (0.0, 0.0, -1.0)
    both = (lambda *a, **k: gpscore.blockloo_value_and_grad_tall(*a, ctx=ctx, **k),
            lambda *a, **k: gpscore.blockloo_train_tall(*a, lr=0.1, itr=2, ctx=ctx, **k))
    for f in both:
        with pytest.raises(ValueError, match="n = 513"):
            f(np.zeros((2, 513, 1)), np.zeros((2, 513)), th, "dss")
        with pytest.raises(ValueError, match="n = 0"):
            f(np.zeros((2, 0, 1)), np.zeros((2, 0)), th, "dss")
        with pytest.raises(ValueError, match="d = 17"):
            f(np.zeros((2, 5, 17)), np.zeros((2, 5)), th, "dss")
        with pytest.raises(ValueError, match="empty"):
            f(np.zeros((0, 5, 2)), np.zeros((0, 5)), th, "dss")
        with pytest.raises(ValueError, match="log_ell"):  # n_ell = 3 with d = 2
            f(X, y, (0.0, np.zeros(3), -1.0), "dss")
        with pytest.raises(ValueError, match="theta must be"):  # one row short of the batch
            f(X, y, np.zeros((2, 4)), "dss")
        with pytest.raises(ValueError, match="disagree"):
            f(X, y[:, :-1], th, "kc")
        with pytest.raises(ValueError, match="rectangular"):  # a ragged list of problems
            f([np.zeros((4, 2)), np.zeros((5, 2))], [np.zeros(4), np.zeros(5)], th, "dss")
        for obj in ("es", "nlml", "loo_crps", "loo_logs", "logdet", 0):
            with pytest.raises(ValueError, match="objective"):
                f(X, y, th, obj)
        for bad in (1, 0, -4, 11, 33, 2.5):  # n = 10: 2..10
            with pytest.raises(ValueError, match="nfold"):
                f(X, y, th, "dss", nfold=bad)
        with pytest.raises(ValueError, match="nfold"):  # n = 40: 2..32
            f(np.zeros((1, 40, 1)), np.zeros((1, 40)), th, "kc", nfold=33)
    T = gpscore.blockloo_train_tall
    with pytest.raises(ValueError, match="itr"):
        T(X, y, th, "dss", lr=0.1, itr=-1, ctx=ctx)
    with pytest.raises(ValueError, match="itr"):
        T(X, y, th, "dss", lr=0.1, itr=2.5, ctx=ctx)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="lr"):
            T(X, y, th, "dss", lr=bad, itr=2, ctx=ctx)
    with pytest.raises(ValueError, match="Xt"):
        T(X, y, th, "dss", lr=0.1, itr=2, Xt=np.zeros((3, 4, 5)), ctx=ctx)
    with pytest.raises(ValueError, match="yt"):  # mismatched Xt / yt
        T(X, y, th, "dss", lr=0.1, itr=2, Xt=np.zeros((3, 4, 2)), yt=np.zeros((3, 5)), ctx=ctx)
    with pytest.raises(ValueError, match="yt without Xt"):
        T(X, y, th, "dss", lr=0.1, itr=2, yt=np.zeros((3, 5)), ctx=ctx)
    # the pointwise wrappers keep refusing the block objectives
    for obj in ("dss", "kc"):
        with pytest.raises(ValueError, match="objective"):
            gpscore.value_and_grad_tall(X, y, th, obj, ctx=ctx)
        with pytest.raises(ValueError, match="objective"):
            gpscore.train_tall(X, y, th, obj, lr=0.1, itr=1, ctx=ctx)
    assert ctx.calls == []


def test_well_formed_calls_reach_exactly_the_block_entry_points():
    """GPS_BLOCK_DSS / GPS_BLOCK_KC, nfold, kind and the flags sit in their slots; the limits
    themselves (n = 512, d = 16, nfold = 2 and 32) are accepted."""
    import gpscore
    from gpscore._lib import GPS_ARD, GPS_RBF
    ctx = _RecordingCtx()
    X, y = _ok()
    out = gpscore.blockloo_value_and_grad_tall(X, y, (0.0, 0.0, -1.0), "kc", nfold=5, ctx=ctx)
    res = gpscore.blockloo_train_tall(X[:, :, 0], y, np.zeros((3, 3)), "dss", nfold=3, lr=0.5, itr=0,
                                      Xt=np.zeros((3, 4)), yt=np.zeros((3, 4)), rbf=True,
                                      stale_noise=True, ctx=ctx)
    assert ctx.calls == list(BLOCK_TALL)
    vals, grads, folds, objs, info = out
    assert vals.shape == (3,) and grads.shape == (3, 3) and folds.shape == (3, 5)
    assert set(objs) == set(gpscore.OBJ_NAMES) and info.shape == (3,)
    assert type(res) is gpscore.BatchTrainResult
    assert res.theta.shape == (3, 3) and res.series["theta"].shape == (3, 0, 3)
    assert res.mu.shape == (3, 4) and set(res.scores) == set(gpscore.SCORE_NAMES)
    a, b = ctx.args
    assert a[:3] == (GPS_ARD, 1, 5) and a[3] == 3 and a[6:8] == (10, 2) and a[9] == 1
    assert b[:3] == (GPS_RBF, 0, 3) and b[3] == 3 and b[6:8] == (10, 1) and b[9] == 1
    assert b[10] == 0 and b[11] == 0.5 and b[14] == 4 and b[15] == 1  # itr, lr, nt, flags
    big = (np.zeros((1, 512, 16)), np.zeros((1, 512)), (0.0, np.zeros(16), -1.0))
    for nfold in (2, 32):
        gpscore.blockloo_value_and_grad_tall(*big, "dss", nfold=nfold, ctx=ctx)
        gpscore.blockloo_train_tall(*big, "kc", nfold=nfold, lr=0.1, itr=1, ctx=ctx)
    assert ctx.calls[2:] == list(BLOCK_TALL) * 2
    for c, nfold in zip(ctx.args[2:], (2, 2, 32, 32)):
        assert c[2] == nfold and c[6:8] == (512, 16) and c[9] == 16
    # the defaults are the DSS fit of kin40k-FULL-compare.py
    gpscore.blockloo_train_tall(X, y, (0.0, 0.0, -1.0), ctx=ctx)
    c = ctx.args[-1]
    assert c[:3] == (GPS_ARD, 0, 4) and c[10] == 150 and c[11] == 1e-3 and c[15] == 0


def test_run_full_blockloo_batch_refusals():
    from gpscore import experiment as E
    ctx = _RecordingCtx()
    sheets = _sheets()
    with pytest.raises(ValueError, match=r"run\(kind=\"full\"\)"):
        E.run_full_blockloo_batch(sheets, TT=2, methods={"es": E.KF_METHODS["es"]}, ctx=ctx)
    for name in ("crps", "nlml", "logs"):
        with pytest.raises(ValueError, match="run_full_batch"):
            E.run_full_blockloo_batch(sheets, TT=2, methods={"dss": E.KF_METHODS["dss"],
                                                             name: E.KF_METHODS[name]}, ctx=ctx)
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match="TT"):
            E.run_full_blockloo_batch(sheets, TT=bad, ctx=ctx)
    with pytest.raises(ValueError, match="itr"):
        E.run_full_blockloo_batch(sheets, TT=2, itr=-1, ctx=ctx)
    assert ctx.calls == []
    with pytest.raises(ValueError, match=r"run\(kind"):  # run_full_batch itself is unchanged
        E.run_full_batch(sheets, TT=2, methods={"dss": E.KF_METHODS["dss"]}, ctx=ctx)
    assert ctx.calls == []


def test_run_full_blockloo_batch_draws_in_runs_order_and_calls_once_per_method():
    """The default method is KF's dss: one gps_full_blockloo_train_tall call for all TT replicates
    with KF's 150 steps at 1e-3 and four folds; with a kc method next to it, θ0 is the draw
    run_method would make, replicate-major, then method — checked against run_method's own draws in
    run's loop order, with GP.train stubbed."""
    from gpscore import experiment as E
    from gpscore._lib import GPS_ARD
    sheets = _sheets()
    TT, d, seed = 3, 3, 11

    class Ctx(_RecordingCtx):
        def call(self, name, *args):
            super().call(name, *args)
            B, n, dd = args[3], args[6], args[7]
            nth = 2 + args[9]
            grab = lambda p, k: np.ctypeslib.as_array(  # noqa: E731
                ctypes.cast(p, ctypes.POINTER(ctypes.c_double)), (k,)).copy()
            self.args[-1] = dict(kind=args[0], code=args[1], nfold=args[2], B=B, n=n, d=dd,
                                 itr=args[10], lr=args[11], nt=args[14], flags=args[15],
                                 X=grab(args[4], B * n * dd).reshape(B, n, dd),
                                 y=grab(args[5], B * n).reshape(B, n),
                                 th0=grab(args[8], B * nth).reshape(B, nth))

    ctx = Ctx()
    out = E.run_full_blockloo_batch(sheets, TT=TT, seed=seed, ctx=ctx)
    assert list(out) == ["dss"] and ctx.calls == ["gps_full_blockloo_train_tall"]
    a = ctx.args[0]
    assert (a["kind"], a["code"], a["nfold"]) == (GPS_ARD, 0, 4)
    assert (a["B"], a["n"], a["d"], a["nt"]) == (TT, 500, d, 40)
    assert (a["itr"], a["lr"], a["flags"]) == (150, 1e-3, 1)
    assert out["dss"]["crps"].shape == (TT,) and out["dss"]["theta"].shape == (TT, 2 + d)
    assert set(out["dss"]) == set(E.METRICS) | {"theta"}

    methods = {"dss": E.KF_METHODS["dss"], "kc": E.Method("kc", 7, 0.1, init="rand3")}
    ctx = Ctx()
    out = E.run_full_blockloo_batch(sheets, TT=TT, methods=methods, seed=seed, ctx=ctx)
    assert list(out) == ["dss", "kc"] and ctx.calls == ["gps_full_blockloo_train_tall"] * 2
    assert [c["code"] for c in ctx.args] == [0, 1]
    assert (ctx.args[1]["itr"], ctx.args[1]["lr"]) == (7, 0.1)

    seen = []

    class Stop(Exception):
        pass

    class FakeGP:
        def __init__(self, ctx=None):
            pass

        def train(self, th0, objective, lr, itr, X, y, Z0, lr_z, block_kw):
            seen.append((objective, np.concatenate([[th0[0]], np.ravel(th0[1]), [th0[2]]]),
                         np.array(X), np.array(y)))
            raise Stop

    rng = np.random.default_rng(seed)
    for j in range(TT):
        data = E.replicate(sheets, j, n_pool=1200)
        for name, meth in methods.items():
            with pytest.raises(Stop):
                E.run_method(FakeGP(), data, meth, rng)
    assert len(seen) == 2 * TT
    for q, (objective, th0, X, y) in enumerate(seen):
        j, name = q // 2, list(methods)[q % 2]
        a = ctx.args[q % 2]
        assert objective == methods[name].objective
        assert np.array_equal(a["th0"][j], th0), (j, name)
        assert np.array_equal(a["X"][j], X) and np.array_equal(a["y"][j], y), (j, name)
