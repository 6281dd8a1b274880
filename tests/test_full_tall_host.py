"""The tall batched full-GP path on the host (no GPU): its two C-ABI entry points are declared,
bound (ABI still 900: the additions are purely additive) and reject a NULL context; the Python
wrappers and experiment.run_full_batch refuse bad shapes, limits, objectives and steps before any
library call; well-formed calls reach exactly the two new entry points; run_full_batch draws its
problems in run's order."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

FULL_TALL = ("gps_full_grad_tall", "gps_full_train_tall")


def test_header_declares_and_binding_covers_the_tall_calls():
    from gpscore import _lib
    txt = open(os.path.join(ROOT, "include", "gpscore.h")).read()
    assert "#define GPS_ABI_VERSION 900" in txt
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(gps_\w+)\s*\(", code))
    for s in FULL_TALL:
        assert s in declared, s
        assert s in _lib.SIGNATURES, s
    # the argument lists are those of the small-batch calls
    assert _lib.SIGNATURES["gps_full_grad_tall"] == _lib.SIGNATURES["gps_full_grad_batch"]
    assert _lib.SIGNATURES["gps_full_train_tall"] == _lib.SIGNATURES["gps_full_train_batch"]
    assert _lib.ABI_VERSION == 900
    assert _lib.load().gps_version() == 900
    assert _lib.BATCH_FULL_TALL_MAX_N == 512
    assert _lib.BATCH_MAX_N == 128 and _lib.BATCH_FITC_TALL_MAX_N == 2048  # the others stay


def test_tall_calls_reject_null_context():
    from gpscore import _lib
    lib = _lib.load()
    z = np.zeros(8)
    iz = np.zeros(2, np.int32)
    P = _lib.ptr
    I = iz.ctypes.data_as(_lib._PI)
    rc = lib.gps_full_grad_tall(None, 0, 1, 1, P(z), P(z), 2, 1, P(z), 1, P(z), P(z), I)
    assert rc == -1
    assert b"NULL" in lib.gps_last_error(None)
    rc = lib.gps_full_train_tall(None, 0, 1, 1, P(z), P(z), 2, 1, P(z), 1, 3, 0.1, None, None, 0,
                                 0, P(z), None, None, None, None, None, None, I, I)
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


def _ok(B=3, n=10, d=2):
    rng = np.random.default_rng(0)
    return rng.standard_normal((B, n, d)), rng.standard_normal((B, n))


def test_tall_wrappers_refuse_before_any_call():
    import gpscore
    ctx = _RecordingCtx()
    X, y = _ok()
    th = (0.0, 0.0, -1.0)
    both = (lambda *a, **k: gpscore.value_and_grad_tall(*a, ctx=ctx, **k),
            lambda *a, **k: gpscore.train_tall(*a, lr=0.1, itr=2, ctx=ctx, **k))
    for f in both:
        with pytest.raises(ValueError, match="n = 513"):
            f(np.zeros((2, 513, 1)), np.zeros((2, 513)), th, "nlml")
        with pytest.raises(ValueError, match="n = 0"):
            f(np.zeros((2, 0, 1)), np.zeros((2, 0)), th, "nlml")
        with pytest.raises(ValueError, match="d = 17"):
            f(np.zeros((2, 5, 17)), np.zeros((2, 5)), th, "nlml")
        with pytest.raises(ValueError, match="empty"):
            f(np.zeros((0, 5, 2)), np.zeros((0, 5)), th, "nlml")
        with pytest.raises(ValueError, match="log_ell"):  # n_ell = 3 with d = 2
            f(X, y, (0.0, np.zeros(3), -1.0), "nlml")
        with pytest.raises(ValueError, match="log_ell"):  # a θ of the wrong width
            f(X, y, np.zeros((3, 5)), "nlml")
        with pytest.raises(ValueError, match="theta must be"):  # one row short of the batch
            f(X, y, np.zeros((2, 4)), "nlml")
        with pytest.raises(ValueError, match="disagree"):
            f(X, y[:, :-1], th, "nlml")
        with pytest.raises(ValueError, match="rectangular"):  # a ragged list of problems
            f([np.zeros((4, 2)), np.zeros((5, 2))], [np.zeros(4), np.zeros(5)], th, "nlml")
        for obj in ("dss", "kc", "es", "logdet"):
            with pytest.raises(ValueError, match="objective"):
                f(X, y, th, obj)
    T = gpscore.train_tall
    with pytest.raises(ValueError, match="itr"):
        T(X, y, th, "nlml", lr=0.1, itr=-1, ctx=ctx)
    with pytest.raises(ValueError, match="itr"):
        T(X, y, th, "nlml", lr=0.1, itr=2.5, ctx=ctx)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="lr"):
            T(X, y, th, "nlml", lr=bad, itr=2, ctx=ctx)
    with pytest.raises(ValueError, match="Xt"):
        T(X, y, th, "nlml", lr=0.1, itr=2, Xt=np.zeros((3, 4, 5)), ctx=ctx)
    with pytest.raises(ValueError, match="yt"):  # mismatched Xt / yt
        T(X, y, th, "nlml", lr=0.1, itr=2, Xt=np.zeros((3, 4, 2)), yt=np.zeros((3, 5)), ctx=ctx)
    with pytest.raises(ValueError, match="yt without Xt"):
        T(X, y, th, "nlml", lr=0.1, itr=2, yt=np.zeros((3, 5)), ctx=ctx)
    assert ctx.calls == []


def test_well_formed_calls_reach_exactly_the_tall_entry_points():
    """A single θ broadcasts, (B, n) X means d = 1, rbf and stale_noise reach the call, and the
    limits themselves (n = 512, d = 16) are accepted."""
    import gpscore
    from gpscore._lib import GPS_ARD, GPS_RBF
    ctx = _RecordingCtx()
    X, y = _ok()
    gpscore.value_and_grad_tall(X, y, (0.0, 0.0, -1.0), "loo_logs", ctx=ctx)
    res = gpscore.train_tall(X[:, :, 0], y, np.zeros((3, 3)), "loo_crps", lr=1.0, itr=0,
                             Xt=np.zeros((3, 4)), yt=np.zeros((3, 4)), rbf=True, stale_noise=True,
                             ctx=ctx)
    assert ctx.calls == list(FULL_TALL)
    assert type(res) is gpscore.BatchTrainResult
    assert res.theta.shape == (3, 3) and res.series["theta"].shape == (3, 0, 3)
    assert res.mu.shape == (3, 4) and set(res.scores) == set(gpscore.SCORE_NAMES)
    assert ctx.args[0][0] == GPS_ARD and ctx.args[1][0] == GPS_RBF
    assert ctx.args[1][9] == 0 and ctx.args[1][10] == 1.0 and ctx.args[1][14] == 1  # itr, lr, flags
    gpscore.value_and_grad_tall(np.zeros((1, 512, 16)), np.zeros((1, 512)),
                                (0.0, np.zeros(16), -1.0), "nlml", ctx=ctx)
    gpscore.train_tall(np.zeros((1, 512, 16)), np.zeros((1, 512)), (0.0, np.zeros(16), -1.0),
                       "nlml", lr=0.1, itr=1, ctx=ctx)
    assert ctx.calls[2:] == list(FULL_TALL)
    assert ctx.args[2][5] == 512 and ctx.args[2][6] == 16 and ctx.args[2][8] == 16
    assert ctx.args[3][5] == 512 and ctx.args[3][6] == 16
    # the small-batch wrappers still go to their own entry points and keep their limit
    ctx2 = _RecordingCtx()
    gpscore.value_and_grad_batch(X, y, (0.0, 0.0, -1.0), "nlml", ctx=ctx2)
    gpscore.train_batch(X, y, (0.0, 0.0, -1.0), "nlml", lr=0.1, itr=1, ctx=ctx2)
    assert ctx2.calls == ["gps_full_grad_batch", "gps_full_train_batch"]
    for f in (lambda *a: gpscore.value_and_grad_batch(*a, ctx=ctx2),
              lambda *a: gpscore.train_batch(*a, lr=0.1, itr=1, ctx=ctx2)):
        with pytest.raises(ValueError, match="n = 129"):
            f(np.zeros((2, 129, 1)), np.zeros((2, 129)), (0.0, 0.0, -1.0), "nlml")
    assert len(ctx2.calls) == 2


def _sheets():
    from gpscore import experiment as E
    return E.synthetic_sheets(5, n_pool=1200, n_test=40, d=3)


def test_run_full_batch_refusals():
    from gpscore import experiment as E
    ctx = _RecordingCtx()
    sheets = _sheets()
    for name in ("dss", "es"):
        with pytest.raises(ValueError, match=r"run\(kind"):
            E.run_full_batch(sheets, TT=2, methods={name: E.KF_METHODS[name]}, ctx=ctx)
    with pytest.raises(ValueError, match=r"run\(kind"):
        E.run_full_batch(sheets, TT=2, methods={"crps": E.KF_METHODS["crps"],
                                                "es": E.KF_METHODS["es"]}, ctx=ctx)
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match="TT"):
            E.run_full_batch(sheets, TT=bad, ctx=ctx)
    with pytest.raises(ValueError, match="itr"):
        E.run_full_batch(sheets, TT=2, itr=-1, ctx=ctx)
    assert ctx.calls == []


def test_run_full_batch_draws_in_runs_order_and_calls_once_per_method():
    """The default methods are KF's crps, nlml, logs; each is one gps_full_train_tall call for all
    TT replicates with KF's steps; θ0 is the draw run_method would make, replicate-major, then
    method — checked against the formula and against run_method's own draws in run's loop order,
    with GP.train stubbed."""
    from gpscore import experiment as E
    from gpscore._lib import GPS_ARD, OBJ_NAMES
    sheets = _sheets()
    TT, d, seed = 3, 3, 11

    class Ctx(_RecordingCtx):
        def call(self, name, *args):
            super().call(name, *args)
            B, n, dd = args[2], args[5], args[6]
            nth = 2 + args[8]
            grab = lambda p, k: np.ctypeslib.as_array(  # noqa: E731
                ctypes.cast(p, ctypes.POINTER(ctypes.c_double)), (k,)).copy()
            self.args[-1] = dict(kind=args[0], code=args[1], B=B, n=n, d=dd, itr=args[9],
                                 lr=args[10], nt=args[13], flags=args[14],
                                 X=grab(args[3], B * n * dd).reshape(B, n, dd),
                                 y=grab(args[4], B * n).reshape(B, n),
                                 th0=grab(args[7], B * nth).reshape(B, nth))

    ctx = Ctx()
    out = E.run_full_batch(sheets, TT=TT, seed=seed, ctx=ctx)
    assert list(out) == ["crps", "nlml", "logs"]
    assert ctx.calls == ["gps_full_train_tall"] * 3
    rng = np.random.default_rng(seed)
    want = {k: [] for k in out}
    for j in range(TT):
        for name in out:
            k, ell, noise = E.initial_theta(E.KF_METHODS[name], d, rng)
            want[name].append(np.concatenate([[k], np.ravel(ell), [noise]]))
    for a, name in zip(ctx.args, out):
        meth = E.KF_METHODS[name]
        assert a["kind"] == GPS_ARD and a["code"] == OBJ_NAMES.index(meth.objective)
        assert (a["B"], a["n"], a["d"], a["nt"]) == (TT, 500, d, 40)
        assert (a["itr"], a["lr"], a["flags"]) == (meth.itr, meth.lr, 1)
        assert np.array_equal(a["th0"], np.stack(want[name])), name
        assert out[name]["crps"].shape == (TT,) and out[name]["theta"].shape == (TT, 2 + d)
        assert set(out[name]) == set(E.METRICS) | {"theta"}

    # run's draws for the same seed and methods: GP.train is where run_method hands them over
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

    methods = {k: E.KF_METHODS[k] for k in ("crps", "nlml", "logs")}
    rng = np.random.default_rng(seed)
    seen.clear()
    for j in range(TT):
        data = E.replicate(sheets, j, n_pool=1200)
        for name, meth in methods.items():
            with pytest.raises(Stop):
                E.run_method(FakeGP(), data, meth, rng)
    assert len(seen) == 3 * TT
    for q, (objective, th0, X, y) in enumerate(seen):
        j, name = divmod(q, 3)[0], list(methods)[q % 3]
        a = ctx.args[q % 3]
        assert objective == methods[name].objective
        assert np.array_equal(a["th0"][j], th0), (j, name)
        assert np.array_equal(a["X"][j], X) and np.array_equal(a["y"][j], y), (j, name)
