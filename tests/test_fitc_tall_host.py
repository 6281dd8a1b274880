"""The tall batched FITC path on the host (no GPU): its two C-ABI entry points are declared, bound
(ABI still 900: the additions are purely additive) and reject a NULL context; the Python wrappers
and experiment.run_fitc_batch refuse bad shapes, limits, objectives and steps before any library
call; well-formed calls reach exactly the two new entry points; run_fitc_batch draws its problems
in run's order."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

FITC_TALL = ("gps_fitc_grad_tall", "gps_fitc_train_tall")


def test_header_declares_and_binding_covers_the_tall_calls():
    from gpscore import _lib
    txt = open(os.path.join(ROOT, "include", "gpscore.h")).read()
    assert "#define GPS_ABI_VERSION 900" in txt
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(gps_\w+)\s*\(", code))
    for s in FITC_TALL:
        assert s in declared, s
        assert s in _lib.SIGNATURES, s
    # the argument lists are those of the small-batch calls
    assert _lib.SIGNATURES["gps_fitc_grad_tall"] == _lib.SIGNATURES["gps_fitc_grad_batch"]
    assert _lib.SIGNATURES["gps_fitc_train_tall"] == _lib.SIGNATURES["gps_fitc_train_batch"]
    assert _lib.ABI_VERSION == 900
    assert _lib.load().gps_version() == 900
    assert _lib.BATCH_FITC_TALL_MAX_N == 2048
    assert _lib.BATCH_FITC_MAX_M == 32 and _lib.BATCH_MAX_N == 128  # the small limits stay


def test_tall_calls_reject_null_context():
    from gpscore import _lib
    lib = _lib.load()
    z = np.zeros(8)
    iz = np.zeros(2, np.int32)
    P = _lib.ptr
    I = iz.ctypes.data_as(_lib._PI)
    rc = lib.gps_fitc_grad_tall(None, 1, 1, P(z), P(z), 2, 1, P(z), 2, P(z), 1, P(z), P(z), P(z), I)
    assert rc == -1
    assert b"NULL" in lib.gps_last_error(None)
    rc = lib.gps_fitc_train_tall(None, 1, 1, P(z), P(z), 2, 1, P(z), 2, P(z), 1, 3, 0.1, 0.1, None,
                                 None, 0, 0, P(z), P(z), None, None, None, None, None, None, I, I)
    assert rc == -1
    assert b"NULL" in lib.gps_last_error(None)


class _RecordingCtx:
    """Stands in for a device context: records the C-ABI calls the wrappers would make."""

    def __init__(self):
        self.calls = []
        self.args = []

    def call(self, name, *args):
        self.calls.append(name)
        self.args.append(args)


def _ok(B=3, n=10, d=2, m=4):
    rng = np.random.default_rng(0)
    return (rng.standard_normal((B, n, d)), rng.standard_normal((B, n)),
            rng.standard_normal((B, m, d)))


def test_tall_wrappers_refuse_before_any_call():
    import gpscore
    ctx = _RecordingCtx()
    X, y, Z = _ok()
    th = (0.0, 0.0, -1.0)
    both = (lambda *a, **k: gpscore.fitc_value_and_grad_tall(*a, ctx=ctx, **k),
            lambda *a, **k: gpscore.fitc_train_tall(*a, lr=0.1, itr=2, ctx=ctx, **k))
    for f in both:
        with pytest.raises(ValueError, match="n = 2049"):
            f(np.zeros((2, 2049, 1)), np.zeros((2, 2049)), np.zeros((2, 3, 1)), th, "nlml")
        with pytest.raises(ValueError, match="n = 0"):
            f(np.zeros((2, 0, 1)), np.zeros((2, 0)), np.zeros((2, 3, 1)), th, "nlml")
        with pytest.raises(ValueError, match="m = 33"):
            f(X, y, np.zeros((3, 33, 2)), th, "nlml")
        with pytest.raises(ValueError, match="m = 0"):
            f(X, y, np.zeros((3, 0, 2)), th, "nlml")
        with pytest.raises(ValueError, match="d = 17"):
            f(np.zeros((2, 5, 17)), np.zeros((2, 5)), np.zeros((2, 3, 17)), th, "nlml")
        with pytest.raises(ValueError, match="empty"):
            f(np.zeros((0, 5, 2)), np.zeros((0, 5)), np.zeros((0, 3, 2)), th, "nlml")
        with pytest.raises(ValueError, match="Z must be"):  # wrong B
            f(X, y, Z[:2], th, "nlml")
        with pytest.raises(ValueError, match="Z must be"):  # wrong d
            f(X, y, np.zeros((3, 4, 3)), th, "nlml")
        with pytest.raises(ValueError, match="Z must be"):  # (B, m) needs d = 1
            f(X, y, np.zeros((3, 4)), th, "nlml")
        with pytest.raises(ValueError, match="Z must be"):  # ragged inducing sets
            f(X, y, [np.zeros((4, 2)), np.zeros((5, 2)), np.zeros((4, 2))], th, "nlml")
        with pytest.raises(ValueError, match="log_ell"):  # n_ell = 3 with d = 2
            f(X, y, Z, (0.0, np.zeros(3), -1.0), "nlml")
        with pytest.raises(ValueError, match="log_ell"):
            f(X, y, Z, np.zeros((3, 5)), "nlml")
        with pytest.raises(ValueError, match="disagree"):
            f(X, y[:, :-1], Z, th, "nlml")
        for obj in ("dss", "kc", "es", "logdet"):
            with pytest.raises(ValueError, match="objective"):
                f(X, y, Z, th, obj)
    T = gpscore.fitc_train_tall
    with pytest.raises(ValueError, match="itr"):
        T(X, y, Z, th, "nlml", lr=0.1, itr=-1, ctx=ctx)
    with pytest.raises(ValueError, match="itr"):
        T(X, y, Z, th, "nlml", lr=0.1, itr=2.5, ctx=ctx)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="lr"):
            T(X, y, Z, th, "nlml", lr=bad, itr=2, ctx=ctx)
        with pytest.raises(ValueError, match="lr_z"):
            T(X, y, Z, th, "nlml", lr=0.1, lr_z=bad, itr=2, ctx=ctx)
    with pytest.raises(ValueError, match="Xt"):
        T(X, y, Z, th, "nlml", lr=0.1, itr=2, Xt=np.zeros((3, 4, 5)), ctx=ctx)
    with pytest.raises(ValueError, match="yt"):
        T(X, y, Z, th, "nlml", lr=0.1, itr=2, Xt=np.zeros((3, 4, 2)), yt=np.zeros((3, 5)), ctx=ctx)
    with pytest.raises(ValueError, match="yt without Xt"):
        T(X, y, Z, th, "nlml", lr=0.1, itr=2, yt=np.zeros((3, 5)), ctx=ctx)
    assert ctx.calls == []


def test_well_formed_calls_reach_exactly_the_tall_entry_points():
    """A single θ broadcasts, (B, n) X and (B, m) Z mean d = 1, lr_z=None means lr, m > n is
    legal, and the limits themselves (n = 2048, m = 32, d = 16) are accepted."""
    import gpscore
    ctx = _RecordingCtx()
    X, y, Z = _ok()
    gpscore.fitc_value_and_grad_tall(X, y, Z, (0.0, 0.0, -1.0), "loo_logs", ctx=ctx)
    res = gpscore.fitc_train_tall(X[:, :, 0], y, np.zeros((3, 12)), np.zeros((3, 3)), "loo_crps",
                                  lr=1.0, lr_z=None, itr=0, Xt=np.zeros((3, 4)),
                                  yt=np.zeros((3, 4)), ctx=ctx)
    assert ctx.calls == list(FITC_TALL)
    assert isinstance(res, gpscore.FitcBatchTrainResult)
    assert res.Z.shape == (3, 12, 1) and res.theta.shape == (3, 3)
    assert res.mu.shape == (3, 4) and set(res.scores) == set(gpscore.SCORE_NAMES)
    lr, lr_z = ctx.args[1][11], ctx.args[1][12]
    assert lr == 1.0 and lr_z == 1.0
    gpscore.fitc_value_and_grad_tall(np.zeros((1, 2048, 16)), np.zeros((1, 2048)),
                                     np.zeros((1, 32, 16)), (0.0, np.zeros(16), -1.0), "nlml",
                                     ctx=ctx)
    assert ctx.calls[2:] == ["gps_fitc_grad_tall"]
    assert ctx.args[2][4] == 2048 and ctx.args[2][5] == 16 and ctx.args[2][7] == 32
    # the small-batch wrappers still go to their own entry points and keep their limit
    ctx2 = _RecordingCtx()
    gpscore.fitc_value_and_grad_batch(X, y, Z, (0.0, 0.0, -1.0), "nlml", ctx=ctx2)
    assert ctx2.calls == ["gps_fitc_grad_batch"]
    with pytest.raises(ValueError, match="n = 129"):
        gpscore.fitc_train_batch(np.zeros((2, 129, 1)), np.zeros((2, 129)), np.zeros((2, 3, 1)),
                                 (0.0, 0.0, -1.0), "nlml", lr=0.1, itr=1, ctx=ctx2)
    assert ctx2.calls == ["gps_fitc_grad_batch"]


def _sheets():
    from gpscore import experiment as E
    return E.synthetic_sheets(5, n_pool=1200, n_test=40, d=3)


def test_run_fitc_batch_refusals():
    from gpscore import experiment as E
    ctx = _RecordingCtx()
    sheets = _sheets()
    for name in ("dss", "kc"):
        with pytest.raises(ValueError, match=r"run\(kind"):
            E.run_fitc_batch(sheets, TT=2, methods={name: E.K20_METHODS[name]}, ctx=ctx)
    with pytest.raises(ValueError, match=r"run\(kind"):
        E.run_fitc_batch(sheets, TT=2, methods={"crps": E.K20_METHODS["crps"],
                                                "es": E.KF_METHODS["es"]}, ctx=ctx)
    with pytest.raises(ValueError, match="TT"):
        E.run_fitc_batch(sheets, TT=0, ctx=ctx)
    with pytest.raises(ValueError, match="m = 33"):
        E.run_fitc_batch(sheets, TT=2, m=33, itr=1, ctx=ctx)
    with pytest.raises(ValueError, match="m must be"):
        E.run_fitc_batch(sheets, TT=2, m=0, itr=1, ctx=ctx)
    with pytest.raises(ValueError, match="itr"):
        E.run_fitc_batch(sheets, TT=2, itr=-1, ctx=ctx)
    assert ctx.calls == []


def test_run_fitc_batch_draws_in_runs_order_and_calls_once_per_method():
    """The default methods are K20's crps, nlml, logs; each is one gps_fitc_train_tall call for
    all TT replicates with K20's steps; θ0 and Z0 are the draws run_method would make, replicate-
    major, then method, initial_theta before Z0."""
    from gpscore import experiment as E
    from gpscore._lib import OBJ_NAMES
    import ctypes
    sheets = _sheets()
    TT, m, d, seed = 3, 4, 3, 11

    class Ctx(_RecordingCtx):
        def call(self, name, *args):
            super().call(name, *args)
            B, n = args[1], args[4]
            nth = 2 + args[9]
            grab = lambda p, k: np.ctypeslib.as_array(
                ctypes.cast(p, ctypes.POINTER(ctypes.c_double)), (k,)).copy()
            self.args[-1] = dict(code=args[0], B=B, n=n, d=args[5], m=args[7], itr=args[10],
                                 lr=args[11], lr_z=args[12], nt=args[15], flags=args[16],
                                 X=grab(args[2], B * n * args[5]).reshape(B, n, args[5]),
                                 Z0=grab(args[6], B * args[7] * args[5]).reshape(B, args[7], args[5]),
                                 th0=grab(args[8], B * nth).reshape(B, nth))

    ctx = Ctx()
    out = E.run_fitc_batch(sheets, TT=TT, m=m, seed=seed, ctx=ctx)
    assert list(out) == ["crps", "nlml", "logs"]
    assert ctx.calls == ["gps_fitc_train_tall"] * 3
    rng = np.random.default_rng(seed)
    want = {k: ([], []) for k in out}
    for j in range(TT):
        for name in out:
            meth = E.K20_METHODS[name]
            k, ell, noise = E.initial_theta(meth, d, rng)
            want[name][0].append(np.concatenate([[k], np.ravel(ell), [noise]]))
            want[name][1].append(rng.random((m, d)))
    for a, name in zip(ctx.args, out):
        meth = E.K20_METHODS[name]
        assert a["code"] == OBJ_NAMES.index(meth.objective)
        assert (a["B"], a["n"], a["d"], a["m"], a["nt"]) == (TT, 500, d, m, 40)
        assert (a["itr"], a["lr"], a["lr_z"], a["flags"]) == (meth.itr, meth.lr, meth.lr_z, 1)
        assert np.array_equal(a["th0"], np.stack(want[name][0])), name
        assert np.array_equal(a["Z0"], np.stack(want[name][1])), name
        for j in range(TT):
            assert np.array_equal(a["X"][j], E.replicate(sheets, j, n_pool=1200)["train_x"])
        assert out[name]["Z"].shape == (TT, m, d) and out[name]["crps"].shape == (TT,)
        assert out[name]["theta"].shape == (TT, a["th0"].shape[1])
    assert ctx.args[2]["th0"].shape[1] == 3 and ctx.args[0]["th0"].shape[1] == 2 + d  # "ones" / rand_l
