"""The batched small-FITC path on the host (no GPU): its two C-ABI entry points are declared,
bound (ABI still 900: the additions are purely additive) and reject a NULL context; the Python
wrappers refuse bad shapes, limits, objectives and steps before any library call; the SF
harness' method table, its inducing-input generator and its dataset check."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

FITC_BATCH = ("gps_fitc_grad_batch", "gps_fitc_train_batch")


def test_header_declares_and_binding_covers_the_fitc_batch_calls():
    from gpscore import _lib
    txt = open(os.path.join(ROOT, "include", "gpscore.h")).read()
    assert "#define GPS_ABI_VERSION 900" in txt
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(gps_\w+)\s*\(", code))
    for s in FITC_BATCH:
        assert s in declared, s
        assert s in _lib.SIGNATURES, s
    assert _lib.ABI_VERSION == 900
    assert _lib.load().gps_version() == 900
    assert _lib.BATCH_FITC_MAX_M == 32


def test_fitc_batch_calls_reject_null_context():
    from gpscore import _lib
    lib = _lib.load()
    z = np.zeros(8)
    iz = np.zeros(2, np.int32)
    P = _lib.ptr
    I = iz.ctypes.data_as(_lib._PI)
    rc = lib.gps_fitc_grad_batch(None, 1, 1, P(z), P(z), 2, 1, P(z), 2, P(z), 1, P(z), P(z), P(z), I)
    assert rc == -1
    assert b"NULL" in lib.gps_last_error(None)
    rc = lib.gps_fitc_train_batch(None, 1, 1, P(z), P(z), 2, 1, P(z), 2, P(z), 1, 3, 0.1, 0.1, None,
                                  None, 0, 0, P(z), P(z), None, None, None, None, None, None, I, I)
    assert rc == -1
    assert b"NULL" in lib.gps_last_error(None)


class _RecordingCtx:
    """Stands in for a device context: records the C-ABI calls the wrappers would make."""

    def __init__(self):
        self.calls = []

    def call(self, name, *args):
        self.calls.append(name)


def _ok(B=3, n=10, d=2, m=4):
    rng = np.random.default_rng(0)
    return (rng.standard_normal((B, n, d)), rng.standard_normal((B, n)),
            rng.standard_normal((B, m, d)))


def test_fitc_wrappers_refuse_before_any_call():
    import gpscore
    ctx = _RecordingCtx()
    X, y, Z = _ok()
    th = (0.0, 0.0, -1.0)
    both = (lambda *a, **k: gpscore.fitc_value_and_grad_batch(*a, ctx=ctx, **k),
            lambda *a, **k: gpscore.fitc_train_batch(*a, lr=0.1, itr=2, ctx=ctx, **k))
    for f in both:
        with pytest.raises(ValueError, match="n = 129"):
            f(np.zeros((2, 129, 1)), np.zeros((2, 129)), np.zeros((2, 3, 1)), th, "nlml")
        with pytest.raises(ValueError, match="m = 33"):
            f(X, y, np.zeros((3, 33, 2)), th, "nlml")
        with pytest.raises(ValueError, match="m = 0"):
            f(X, y, np.zeros((3, 0, 2)), th, "nlml")
        with pytest.raises(ValueError, match="d = 17"):
            f(np.zeros((2, 5, 17)), np.zeros((2, 5)), np.zeros((2, 3, 17)), th, "nlml")
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
    T = gpscore.fitc_train_batch
    with pytest.raises(ValueError, match="itr"):
        T(X, y, Z, th, "nlml", lr=0.1, itr=-1, ctx=ctx)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="lr"):
            T(X, y, Z, th, "nlml", lr=bad, itr=2, ctx=ctx)
        with pytest.raises(ValueError, match="lr_z"):
            T(X, y, Z, th, "nlml", lr=0.1, lr_z=bad, itr=2, ctx=ctx)
    with pytest.raises(ValueError, match="Xt"):
        T(X, y, Z, th, "nlml", lr=0.1, itr=2, Xt=np.zeros((3, 4, 5)), ctx=ctx)
    with pytest.raises(ValueError, match="yt"):
        T(X, y, Z, th, "nlml", lr=0.1, itr=2, Xt=np.zeros((3, 4, 2)), yt=np.zeros((3, 5)), ctx=ctx)
    assert ctx.calls == []
    # well-formed calls reach exactly the two entry points: a single θ broadcasts, (B, n) X and
    # (B, m) Z mean d = 1, lr_z=None means lr, m > n is legal
    gpscore.fitc_value_and_grad_batch(X, y, Z, th, "loo_logs", ctx=ctx)
    res = T(X[:, :, 0], y, np.zeros((3, 12)), np.zeros((3, 3)), "loo_crps", lr=1.0, lr_z=None,
            itr=0, Xt=np.zeros((3, 4)), yt=np.zeros((3, 4)), ctx=ctx)
    assert ctx.calls == list(FITC_BATCH)
    assert res.Z.shape == (3, 12, 1) and res.theta.shape == (3, 3)


def test_sf_methods_table():
    from gpscore import experiment as E
    got = {k: (m.objective, m.itr, m.lr, m.lr_z, m.init, m.ref) for k, m in E.SF_METHODS.items()}
    assert got == {"crps": ("loo_crps", 1000, 1.0, 1.0, "ones", "SF:189-237"),
                   "nlml": ("nlml", 1200, 5e-4, 5e-3, "ones", "SF:301-343"),
                   "logs": ("loo_logs", 2500, 5e-3, 5e-3, "ones", "SF:420-463")}
    assert list(E.SF_METHODS) == ["crps", "nlml", "logs"]


def test_simple_inducing():
    from gpscore import experiment as E
    a, b = E.simple_inducing(3), E.simple_inducing(3)
    assert a.shape == (5, 1) and a.dtype == np.float64
    assert np.array_equal(a, b)
    seen = set()
    for j in range(40):
        z = E.simple_inducing(j)
        assert np.array_equal(z, np.rint(z)) and z.min() >= -3 and z.max() <= 2
        seen.update(z.ravel().tolist())
    assert seen == {-3.0, -2.0, -1.0, 0.0, 1.0, 2.0}
    assert any(not np.array_equal(E.simple_inducing(j), a) for j in range(4, 10))
    c = E.simple_inducing(3, rng=np.random.default_rng(5), m=7, d=2)
    d = E.simple_inducing(9, rng=np.random.default_rng(5), m=7, d=2)
    assert c.shape == (7, 2) and np.array_equal(c, d)   # the rng alone decides the draws


def test_run_simple_fitc_checks_the_dataset_count():
    from gpscore import experiment as E
    ctx = _RecordingCtx()
    with pytest.raises(ValueError, match="datasets"):
        E.run_simple_fitc(TT=3, datasets=[E.simple_data(0), E.simple_data(1)], ctx=ctx)
    with pytest.raises(ValueError, match="Z0"):
        E.run_simple_fitc(TT=2, datasets=[E.simple_data(0), E.simple_data(1)],
                          Z0=np.zeros((3, 5, 1)), ctx=ctx)
    assert ctx.calls == []
