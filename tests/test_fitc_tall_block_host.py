"""The tall batched FITC block-LOO path on the host (no GPU): its two C-ABI entry
points are declared, exported and bound (ABI still 900: the additions are purely additive) and
reject a NULL context; the Python wrappers and experiment.run_fitc_blockloo_batch refuse bad
shapes, limits, objectives, fold counts and steps before any library call; well-formed calls
reach exactly the two new entry points with the arguments in the right slots;
run_fitc_blockloo_batch draws its problems in run's order; the kernel's LDS at the corner of its
limits fits a workgroup's 160 KB."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_full_tall_host import _RecordingCtx, _ok, _sheets

BLOCK_TALL = ("gps_fitc_blockloo_grad_tall", "gps_fitc_blockloo_train_tall")
TH = (0.0, 0.0, -1.0)


def _z(B=3, m=4, d=2):
    return np.random.default_rng(1).standard_normal((B, m, d))


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
    # gps_fitc_*_tall's argument lists with nfold after the objective, and value / fold_values
    # in front of the value + gradient call's outputs
    g, t = _lib.SIGNATURES["gps_fitc_grad_tall"][1], _lib.SIGNATURES["gps_fitc_train_tall"][1]
    bg = _lib.SIGNATURES["gps_fitc_blockloo_grad_tall"][1]
    bt = _lib.SIGNATURES["gps_fitc_blockloo_train_tall"][1]
    assert bt == t[:2] + [ctypes.c_int] + t[2:]
    assert bg == g[:2] + [ctypes.c_int] + g[2:11] + [_lib._P, _lib._P] + g[11:]
    assert _lib.ABI_VERSION == 900 and lib.gps_version() == 900
    decl = re.sub(r"\s+", " ", code)
    assert ("int gps_fitc_blockloo_grad_tall(gps_ctx* ctx, int objective, int nfold, int64_t nprob, "
            "const double* X, const double* y, int64_t n, int d, const double* Z, int m, "
            "const double* theta, int n_ell, double* value, double* fold_values, double* obj, "
            "double* grad, double* grad_z, int* info);") in decl
    assert ("int gps_fitc_blockloo_train_tall(gps_ctx* ctx, int objective, int nfold, int64_t nprob, "
            "const double* X, const double* y, int64_t n, int d, const double* Z0, int m, "
            "const double* theta0, int n_ell, int64_t itr, double lr, double lr_z, "
            "const double* Xt, const double* yt, int64_t nt, int flags, double* theta_out, "
            "double* z_out, double* values, double* thetas, double* obj, double* mu, double* var, "
            "double* sc, int* info, int* steps_done);") in decl


def test_block_calls_reject_null_context():
    from gpscore import _lib
    lib = _lib.load()
    z = np.zeros(8)
    iz = np.zeros(2, np.int32)
    P = _lib.ptr
    I = iz.ctypes.data_as(_lib._PI)
    rc = lib.gps_fitc_blockloo_grad_tall(None, 0, 2, 1, P(z), P(z), 2, 1, P(z), 2, P(z), 1, P(z),
                                         P(z), P(z), P(z), P(z), I)
    assert rc == -1
    assert b"NULL" in lib.gps_last_error(None)
    rc = lib.gps_fitc_blockloo_train_tall(None, 0, 2, 1, P(z), P(z), 2, 1, P(z), 2, P(z), 1, 3, 0.1,
                                          0.1, None, None, 0, 0, P(z), P(z), None, None, None, None,
                                          None, None, I, I)
    assert rc == -1
    assert b"NULL" in lib.gps_last_error(None)


def test_lds_and_workspace_sizes():
    """The host-callable size functions: the corner of the limits fits the 163 840 bytes a
    workgroup may have, above the pointwise tall kernel's by one m×(m|1) array and five m-vectors;
    the workspace is 4n(m|1) + (nfold + 1)·m(m|1) + 11n doubles."""
    from gpscore import _lib
    lib = _lib.load()
    lds = lib["_ZN3gps31batch_fitc_tall_block_lds_bytesEiii"]
    lds.restype, lds.argtypes = ctypes.c_size_t, [ctypes.c_int] * 3
    old = lib["_ZN3gps25batch_fitc_tall_lds_bytesEiii"]
    old.restype, old.argtypes = ctypes.c_size_t, [ctypes.c_int] * 3
    ws = lib["_ZN3gps32batch_fitc_tall_block_ws_doublesElii"]
    ws.restype, ws.argtypes = ctypes.c_int64, [ctypes.c_int64, ctypes.c_int, ctypes.c_int]
    corner = lds(2048, 32, 16)
    assert corner <= 163840, corner
    assert corner == old(2048, 32, 16) + 8 * (32 * 33 + 5 * 32)
    for n, m, d in ((1, 1, 1), (500, 20, 8), (127, 32, 16), (2048, 1, 1)):
        assert lds(n, m, d) <= corner and lds(n, m, d) > old(n, m, d)
    for n, m, nfold in ((500, 20, 4), (2048, 32, 32), (5, 1, 2)):
        ld = m | 1
        assert ws(n, m, nfold) == 4 * n * ld + (nfold + 1) * m * ld + 11 * n


def test_block_wrappers_refuse_before_any_call():
    import gpscore
    ctx = _RecordingCtx()
    X, y = _ok()  # B = 3, n = 10, d = 2
    Z = _z()
    both = (lambda *a, **k: gpscore.fitc_blockloo_value_and_grad_tall(*a, ctx=ctx, **k),
            lambda *a, **k: gpscore.fitc_blockloo_train_tall(*a, lr=0.1, itr=2, ctx=ctx, **k))
    for f in both:
        with pytest.raises(ValueError, match="n = 2049"):
            f(np.zeros((2, 2049, 1)), np.zeros((2, 2049)), np.zeros((2, 3, 1)), TH, "dss")
        with pytest.raises(ValueError, match="n = 0"):
            f(np.zeros((2, 0, 1)), np.zeros((2, 0)), np.zeros((2, 3, 1)), TH, "dss")
        with pytest.raises(ValueError, match="d = 17"):
            f(np.zeros((2, 5, 17)), np.zeros((2, 5)), np.zeros((2, 3, 17)), TH, "dss")
        with pytest.raises(ValueError, match="empty"):
            f(np.zeros((0, 5, 2)), np.zeros((0, 5)), np.zeros((0, 3, 2)), TH, "dss")
        with pytest.raises(ValueError, match="m = 33"):
            f(X, y, np.zeros((3, 33, 2)), TH, "dss")
        with pytest.raises(ValueError, match="m = 0"):
            f(X, y, np.zeros((3, 0, 2)), TH, "dss")
        with pytest.raises(ValueError, match="Z must be"):  # another batch size, another d
            f(X, y, np.zeros((2, 4, 2)), TH, "dss")
        with pytest.raises(ValueError, match="Z must be"):
            f(X, y, np.zeros((3, 4, 3)), TH, "kc")
        with pytest.raises(ValueError, match="log_ell"):  # n_ell = 3 with d = 2
            f(X, y, Z, (0.0, np.zeros(3), -1.0), "dss")
        with pytest.raises(ValueError, match="theta must be"):  # one row short of the batch
            f(X, y, Z, np.zeros((2, 4)), "dss")
        with pytest.raises(ValueError, match="disagree"):
            f(X, y[:, :-1], Z, TH, "kc")
        with pytest.raises(ValueError, match="rectangular"):  # a ragged list of problems
            f([np.zeros((4, 2)), np.zeros((5, 2))], [np.zeros(4), np.zeros(5)], Z, TH, "dss")
        for obj in ("es", "nlml", "loo_crps", "loo_logs", "logdet", 0):
            with pytest.raises(ValueError, match="objective"):
                f(X, y, Z, TH, obj)
        for bad in (1, 0, -4, 11, 33, 2.5, True):  # n = 10: 2..10
            with pytest.raises(ValueError, match="nfold"):
                f(X, y, Z, TH, "dss", nfold=bad)
        with pytest.raises(ValueError, match="nfold"):  # n = 40: 2..32
            f(np.zeros((1, 40, 1)), np.zeros((1, 40)), np.zeros((1, 3, 1)), TH, "kc", nfold=33)
    T = gpscore.fitc_blockloo_train_tall
    with pytest.raises(ValueError, match="itr"):
        T(X, y, Z, TH, "dss", lr=0.1, itr=-1, ctx=ctx)
    with pytest.raises(ValueError, match="itr"):
        T(X, y, Z, TH, "dss", lr=0.1, itr=2.5, ctx=ctx)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="lr"):
            T(X, y, Z, TH, "dss", lr=bad, itr=2, ctx=ctx)
        with pytest.raises(ValueError, match="lr_z"):
            T(X, y, Z, TH, "dss", lr=0.1, lr_z=bad, itr=2, ctx=ctx)
    with pytest.raises(ValueError, match="Xt"):
        T(X, y, Z, TH, "dss", lr=0.1, itr=2, Xt=np.zeros((3, 4, 5)), ctx=ctx)
    with pytest.raises(ValueError, match="yt"):  # mismatched Xt / yt
        T(X, y, Z, TH, "dss", lr=0.1, itr=2, Xt=np.zeros((3, 4, 2)), yt=np.zeros((3, 5)), ctx=ctx)
    with pytest.raises(ValueError, match="yt without Xt"):
        T(X, y, Z, TH, "dss", lr=0.1, itr=2, yt=np.zeros((3, 5)), ctx=ctx)
    # the pointwise tall wrappers keep refusing the block objectives
    for obj in ("dss", "kc"):
        with pytest.raises(ValueError, match="objective"):
            gpscore.fitc_value_and_grad_tall(X, y, Z, TH, obj, ctx=ctx)
        with pytest.raises(ValueError, match="objective"):
            gpscore.fitc_train_tall(X, y, Z, TH, obj, lr=0.1, itr=1, ctx=ctx)
    assert ctx.calls == []


def test_well_formed_calls_reach_exactly_the_block_entry_points():
    """GPS_BLOCK_DSS / GPS_BLOCK_KC, nfold, m and the flags sit in their slots; the limits
    themselves (n = 2048, m = 32, d = 16, nfold = 2 and 32) are accepted."""
    import gpscore
    ctx = _RecordingCtx()
    X, y = _ok()
    Z = _z()
    out = gpscore.fitc_blockloo_value_and_grad_tall(X, y, Z, TH, "kc", nfold=5, ctx=ctx)
    res = gpscore.fitc_blockloo_train_tall(X[:, :, 0], y, Z[:, :, 0], np.zeros((3, 3)), "dss",
                                           nfold=3, lr=0.5, lr_z=0.25, itr=0, Xt=np.zeros((3, 4)),
                                           yt=np.zeros((3, 4)), stale_noise=True, ctx=ctx)
    assert ctx.calls == list(BLOCK_TALL)
    vals, grads, gz, folds, objs, info = out
    assert vals.shape == (3,) and grads.shape == (3, 3) and gz.shape == (3, 4, 2)
    assert folds.shape == (3, 5)
    assert set(objs) == set(gpscore.OBJ_NAMES) and info.shape == (3,)
    assert type(res) is gpscore.FitcBatchTrainResult
    assert res.theta.shape == (3, 3) and res.series["theta"].shape == (3, 0, 3)
    assert res.Z.shape == (3, 4, 1)
    assert res.mu.shape == (3, 4) and set(res.scores) == set(gpscore.SCORE_NAMES)
    a, b = ctx.args
    # objective, nfold, nprob | n, d | m | n_ell
    assert a[:3] == (1, 5, 3) and a[5:7] == (10, 2) and a[8] == 4 and a[10] == 1
    assert b[:3] == (0, 3, 3) and b[5:7] == (10, 1) and b[8] == 4 and b[10] == 1
    assert b[11:14] == (0, 0.5, 0.25) and b[16] == 4 and b[17] == 1  # itr, lr, lr_z, nt, flags
    big = (np.zeros((1, 2048, 16)), np.zeros((1, 2048)), np.zeros((1, 32, 16)),
           (0.0, np.zeros(16), -1.0))
    for nfold in (2, 32):
        gpscore.fitc_blockloo_value_and_grad_tall(*big, "dss", nfold=nfold, ctx=ctx)
        gpscore.fitc_blockloo_train_tall(*big, "kc", nfold=nfold, lr=0.1, itr=1, ctx=ctx)
    assert ctx.calls[2:] == list(BLOCK_TALL) * 2
    for c, nfold in zip(ctx.args[2:], (2, 2, 32, 32)):
        assert c[1] == nfold and c[5:7] == (2048, 16) and c[8] == 32 and c[10] == 16
    # the defaults are K20's DSS fit; lr_z defaults to lr
    gpscore.fitc_blockloo_train_tall(X, y, Z, TH, ctx=ctx)
    c = ctx.args[-1]
    assert c[:2] == (0, 4) and c[11:14] == (3000, 1e-3, 1e-3) and c[17] == 0


def test_run_fitc_blockloo_batch_refusals():
    from gpscore import experiment as E
    ctx = _RecordingCtx()
    sheets = _sheets()
    es = E.Method("es", 25, 0.1)
    with pytest.raises(ValueError, match=r"run\(kind=\"fitc\"\)"):
        E.run_fitc_blockloo_batch(sheets, TT=2, methods={"es": es}, ctx=ctx)
    for name in ("crps", "nlml", "logs"):
        with pytest.raises(ValueError, match="run_fitc_batch"):
            E.run_fitc_blockloo_batch(sheets, TT=2, methods={"dss": E.K20_METHODS["dss"],
                                                             name: E.K20_METHODS[name]}, ctx=ctx)
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match="TT"):
            E.run_fitc_blockloo_batch(sheets, TT=bad, ctx=ctx)
        with pytest.raises(ValueError, match="m must be"):
            E.run_fitc_blockloo_batch(sheets, TT=2, m=bad, ctx=ctx)
    with pytest.raises(ValueError, match="m = 33"):
        E.run_fitc_blockloo_batch(sheets, TT=2, m=33, ctx=ctx)
    with pytest.raises(ValueError, match="itr"):
        E.run_fitc_blockloo_batch(sheets, TT=2, itr=-1, ctx=ctx)
    with pytest.raises(ValueError, match="nfold"):
        E.run_fitc_blockloo_batch(sheets, TT=2, nfold=1, ctx=ctx)
    assert ctx.calls == []
    for name in ("dss", "kc"):  # run_fitc_batch itself is unchanged
        with pytest.raises(ValueError, match=r"run\(kind"):
            E.run_fitc_batch(sheets, TT=2, methods={name: E.K20_METHODS[name]}, ctx=ctx)
    assert ctx.calls == []


def test_run_fitc_blockloo_batch_draws_in_runs_order_and_calls_once_per_method():
    """The default methods are K20's dss and kc: one gps_fitc_blockloo_train_tall call each for all
    TT replicates, with K20's steps, rates and four folds; θ0 and Z0 are the draws run_method would
    make, replicate-major, then method, θ0 first and Z0 second, N(0,1) for dss and U(0,1) for kc —
    checked against run_method's own draws in run's loop order, with GP.train stubbed."""
    from gpscore import experiment as E
    sheets = _sheets()
    TT, d, m, seed = 3, 3, 6, 11

    class Ctx(_RecordingCtx):
        def call(self, name, *args):
            super().call(name, *args)
            B, n, dd, mm = args[2], args[5], args[6], args[8]
            nth = 2 + args[10]
            grab = lambda p, k: np.ctypeslib.as_array(  # noqa: E731
                ctypes.cast(p, ctypes.POINTER(ctypes.c_double)), (k,)).copy()
            self.args[-1] = dict(code=args[0], nfold=args[1], B=B, n=n, d=dd, m=mm, itr=args[11],
                                 lr=args[12], lr_z=args[13], nt=args[16], flags=args[17],
                                 X=grab(args[3], B * n * dd).reshape(B, n, dd),
                                 y=grab(args[4], B * n).reshape(B, n),
                                 Z0=grab(args[7], B * mm * dd).reshape(B, mm, dd),
                                 th0=grab(args[9], B * nth).reshape(B, nth))
            # the call's outputs stay uninitialised: make every replicate a success
            ctypes.memset(args[26], 0, 4 * B)

    ctx = Ctx()
    out = E.run_fitc_blockloo_batch(sheets, TT=TT, m=m, seed=seed, ctx=ctx)
    assert list(out) == ["dss", "kc"] and ctx.calls == ["gps_fitc_blockloo_train_tall"] * 2
    a, b = ctx.args
    assert (a["code"], a["nfold"], b["code"], b["nfold"]) == (0, 4, 1, 4)
    for c in (a, b):
        assert (c["B"], c["n"], c["d"], c["m"], c["nt"], c["flags"]) == (TT, 500, d, m, 40, 1)
    assert (a["itr"], a["lr"], a["lr_z"]) == (3000, 1e-3, 1e-3)
    assert (b["itr"], b["lr"], b["lr_z"]) == (3000, 0.1, 0.1)
    for name in ("dss", "kc"):
        assert out[name]["crps"].shape == (TT,) and out[name]["theta"].shape == (TT, 2 + d)
        assert out[name]["Z"].shape == (TT, m, d) and out[name]["failed"].shape == (TT,)
        assert set(out[name]) == set(E.METRICS) | {"theta", "Z", "failed"}
    assert np.abs(a["Z0"]).max() > 1.0 and b["Z0"].min() >= 0.0 and b["Z0"].max() < 1.0

    methods = {k: E.K20_METHODS[k] for k in ("dss", "kc")}
    seen = []

    class Stop(Exception):
        pass

    class FakeGP:
        def __init__(self, ctx=None):
            pass

        def train(self, th0, objective, lr, itr, X, y, Z0, lr_z, block_kw):
            seen.append((objective, np.concatenate([[th0[0]], np.ravel(th0[1]), [th0[2]]]),
                         np.array(Z0), np.array(X), np.array(y)))
            raise Stop

    rng = np.random.default_rng(seed)
    for j in range(TT):
        data = E.replicate(sheets, j, n_pool=1200)
        for name, meth in methods.items():
            with pytest.raises(Stop):
                E.run_method(FakeGP(), data, meth, rng, kind="fitc", m=m)
    assert len(seen) == 2 * TT
    for q, (objective, th0, Z0, X, y) in enumerate(seen):
        j, name = q // 2, list(methods)[q % 2]
        c = ctx.args[q % 2]
        assert objective == methods[name].objective
        assert np.array_equal(c["th0"][j], th0), (j, name)
        assert np.array_equal(c["Z0"][j], Z0), (j, name)
        assert np.array_equal(c["X"][j], X) and np.array_equal(c["y"][j], y), (j, name)


def test_a_failed_kc_replicate_gives_zero_metrics_and_a_failed_dss_replicate_raises():
    from gpscore import NotPositiveDefinite
    from gpscore import experiment as E
    sheets = _sheets()

    class Ctx(_RecordingCtx):
        def call(self, name, *args):
            super().call(name, *args)
            B = args[2]
            info = np.ctypeslib.as_array(ctypes.cast(args[26], ctypes.POINTER(ctypes.c_int32)), (B,))
            info[:] = 0
            info[1] = 7  # replicate 1 failed
            sc = np.ctypeslib.as_array(ctypes.cast(args[25], ctypes.POINTER(ctypes.c_double)),
                                       (B, 6))
            sc[:] = 2.0
            sc[1] = np.nan

    out = E.run_fitc_blockloo_batch(sheets, TT=3, m=4, itr=1, seed=0, ctx=Ctx(),
                                    methods={"kc": E.K20_METHODS["kc"]})
    assert list(out["kc"]["failed"]) == [False, True, False]
    for k in E.METRICS:
        assert list(out["kc"][k]) == [2.0, 0.0, 2.0], k
    with pytest.raises(NotPositiveDefinite, match="replicate 1"):
        E.run_fitc_blockloo_batch(sheets, TT=3, m=4, itr=1, seed=0, ctx=Ctx(),
                                  methods={"dss": E.K20_METHODS["dss"]})
