"""The batched small-GP path on the host (no GPU): its two C-ABI entry points are declared, bound
(ABI 900) and reject a NULL context; the Python wrappers refuse bad shapes, limits and
objectives before any library call; the SD harness' generator and method table."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

BATCH = ("gps_full_grad_batch", "gps_full_train_batch")


def test_abi_900_declares_and_binds_the_batch_calls():
    from gpscore import _lib
    txt = open(os.path.join(ROOT, "include", "gpscore.h")).read()
    assert _lib.ABI_VERSION == 900
    assert "#define GPS_ABI_VERSION 900" in txt
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(gps_\w+)\s*\(", code))
    for s in BATCH:
        assert s in declared, s
        assert s in _lib.SIGNATURES, s
    assert _lib.load().gps_version() == 900


def test_batch_calls_reject_null_context():
    from gpscore import _lib
    lib = _lib.load()
    z = np.zeros(8)
    iz = np.zeros(2, np.int32)
    P = _lib.ptr
    I = iz.ctypes.data_as(_lib._PI)
    rc = lib.gps_full_grad_batch(None, 0, 1, 1, P(z), P(z), 2, 1, P(z), 1, P(z), P(z), I)
    assert rc == -1
    assert b"NULL" in lib.gps_last_error(None)
    rc = lib.gps_full_train_batch(None, 0, 1, 1, P(z), P(z), 2, 1, P(z), 1, 3, 0.1, None, None, 0, 0,
                                  P(z), None, None, None, None, None, None, I, I)
    assert rc == -1
    assert b"NULL" in lib.gps_last_error(None)


class _RecordingCtx:
    """Stands in for a device context: records the C-ABI calls the wrappers would make."""

    def __init__(self):
        self.calls = []

    def call(self, name, *args):
        self.calls.append(name)


def _ok(B=3, n=10, d=2):
    rng = np.random.default_rng(0)
    return rng.standard_normal((B, n, d)), rng.standard_normal((B, n))


def test_wrappers_refuse_before_any_call():
    import gpscore
    ctx = _RecordingCtx()
    X, y = _ok()
    th = (0.0, 0.0, -1.0)
    both = (lambda *a, **k: gpscore.value_and_grad_batch(*a, ctx=ctx, **k),
            lambda *a, **k: gpscore.train_batch(*a, lr=0.1, itr=2, ctx=ctx, **k))
    for f in both:
        with pytest.raises(ValueError, match="n = 129"):
            f(np.zeros((2, 129, 1)), np.zeros((2, 129)), th, "nlml")
        with pytest.raises(ValueError, match="d = 17"):
            f(np.zeros((2, 5, 17)), np.zeros((2, 5)), th, "nlml")
        with pytest.raises(ValueError, match="log_ell"):  # n_ell = 3 with d = 2
            f(X, y, (0.0, np.zeros(3), -1.0), "nlml")
        with pytest.raises(ValueError, match="log_ell"):
            f(X, y, np.zeros((3, 5)), "nlml")
        with pytest.raises(ValueError):  # ragged problems
            f([np.zeros((4, 2)), np.zeros((5, 2))], [np.zeros(4), np.zeros(5)], th, "nlml")
        with pytest.raises(ValueError, match="disagree"):
            f(X, y[:, :-1], th, "nlml")
        with pytest.raises(ValueError, match="theta"):  # one row of θ too few
            f(X, y, np.zeros((2, 3)), "nlml")
        for obj in ("dss", "kc", "es", "logdet"):
            with pytest.raises(ValueError, match="objective"):
                f(X, y, th, obj)
    with pytest.raises(ValueError, match="itr"):
        gpscore.train_batch(X, y, th, "nlml", lr=0.1, itr=-1, ctx=ctx)
    for lr in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="lr"):
            gpscore.train_batch(X, y, th, "nlml", lr=lr, itr=2, ctx=ctx)
    with pytest.raises(ValueError, match="Xt"):
        gpscore.train_batch(X, y, th, "nlml", lr=0.1, itr=2, Xt=np.zeros((3, 4, 5)), ctx=ctx)
    with pytest.raises(ValueError, match="yt"):
        gpscore.train_batch(X, y, th, "nlml", lr=0.1, itr=2, Xt=np.zeros((3, 4, 2)),
                            yt=np.zeros((3, 5)), ctx=ctx)
    assert ctx.calls == []
    # well-formed calls reach the entry points; a single θ broadcasts, (B, n) means d = 1
    gpscore.value_and_grad_batch(X, y, th, "loo_logs", ctx=ctx)
    gpscore.train_batch(X[:, :, 0], y, np.zeros((3, 3)), "loo_crps", lr=1.0, itr=0,
                        Xt=np.zeros((3, 4)), yt=np.zeros((3, 4)), ctx=ctx)
    assert ctx.calls == list(BATCH)


def test_simple_data_and_sd_methods():
    from gpscore import experiment as E
    a, b = E.simple_data(3), E.simple_data(3)
    assert a["train_x"].shape == (120, 1) and a["train_y"].shape == (120,)
    assert a["test_x"].shape == (300, 1) and a["test_y"].shape == (300,)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    c = E.simple_data(3, rng=np.random.default_rng(5))
    d = E.simple_data(7, rng=np.random.default_rng(5))
    assert np.array_equal(c["train_y"], d["train_y"])       # the rng alone decides the draws
    assert not np.array_equal(a["train_y"], c["train_y"])
    assert not np.array_equal(a["train_x"], E.simple_data(4)["train_x"])
    got = {k: (m.objective, m.itr, m.lr, m.init) for k, m in E.SD_METHODS.items()}
    assert got == {"crps": ("loo_crps", 250, 1.0, "ones"), "nlml": ("nlml", 250, 1e-3, "ones"),
                   "logs": ("loo_logs", 400, 0.05, "ones")}
