"""Batches of small full GPs and small FITC GPs, one workgroup per problem in one launch
(DESIGN §19, §20), and their siblings for taller problems (§22, §24; the block-LOO DSS / KC
objectives §26 for the full GP, §27 for FITC; the block-LOO energy score §32; a validation set
scored inside the tall full-GP fits §34 and the tall FITC fits §37).

    vals, grads, objs, info = gpscore.value_and_grad_batch(X, y, theta, "loo_crps")
    res = gpscore.train_batch(X, y, (1.0, 1.0, 1.0), "loo_crps", lr=1.0, itr=250, Xt=Xt, yt=yt)
    vals, grads, gZ, objs, info = gpscore.fitc_value_and_grad_batch(X, y, Z, theta, "loo_crps")
    res = gpscore.fitc_train_batch(X, y, Z0, (1.0, 1.0, 1.0), "loo_crps", lr=1.0, lr_z=1.0,
                                   itr=1000, Xt=Xt, yt=yt)
    res = gpscore.train_tall(X, y, theta0, "loo_crps", lr=1.0, itr=400, Xt=Xt, yt=yt)  # n <= 512
    res = gpscore.blockloo_train_tall(X, y, theta0, "dss", nfold=4, lr=1e-3, itr=150, Xt=Xt, yt=yt)
    res = gpscore.es_train_tall(X, y, theta0, nfold=4, num_sim=300, lr=0.1, itr=25, Xt=Xt, yt=yt)
    res = gpscore.train_tall_validated(X, y, theta0, Xv, yv, "loo_crps", itr=400, select="crps")  # §34
    res = gpscore.fitc_blockloo_train_tall(X, y, Z0, theta0, "kc", nfold=4, lr=0.1, itr=3000,
                                           Xt=Xt, yt=yt)                                # n <= 2048
    res = gpscore.fitc_train_tall_validated(X, y, Z0, theta0, Xv, yv, "loo_crps", itr=2000,
                                            va_every=10, select="crps")                 # §37

The replicate loops of "SIMPLE-DATA FULL-comapre.py" (TT = 100 data sets of n = 120, three SGD
fits each: SD:192-231, 277-301, 372-396) and contour-plot.R's n = 20 problems are many tiny,
independent, sequential fits; here B of them of one shape (n <= 128, d <= 16) run side by side,
each with its own data and θ.  ``X`` is (B, n, d) or (B, n); ``theta`` is one (log_sf2, log_ell,
log_sn2) for every problem (log_ell a scalar or length d), or a (B, 2 + n_ell) array with one
row [log_sf2, log_ell..., log_sn2] per problem.  A problem whose matrix is not positive
definite does not raise: its ``info`` is the order of the failing leading minor and its outputs
are NaN; the others are untouched.  Every number comes from libgpscore.so on the GPU.

The FITC calls do the same for the replicate loops of "SIMPLE-FITC--comapre.py" (TT = 100 data
sets of n = 120 with m = 5 inducing inputs, three SGD fits each that move the inducing inputs
too: SF:189-237, 301-343, 420-463): ``Z`` is (B, m, d), or (B, m) when d = 1, with m <= 32 (m > n
is legal); the ARD kernel with the 1e-3 jitter inside K(Z,Z) as the resident FITC path.  There
``info`` is k in 1..m when the leading minor of order k of K(Z,Z) + 1e-3·I fails and m + k when
that of B = K(Z,Z) + 1e-3·I + KᵀΛ⁻¹K does.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

from . import _lib
from ._lib import (BATCH_BLOCK_MAX_FOLDS, BATCH_ES_MAX_FOLD, BATCH_ES_MAX_SIM, BATCH_FITC_MAX_M,
                   BATCH_FITC_TALL_MAX_N, BATCH_FULL_TALL_MAX_N, BATCH_MAX_D, BATCH_MAX_N, GPS_ARD,
                   GPS_BATCH_STALE_NOISE, GPS_RBF, OBJ_NAMES, SCORE_NAMES, f64, ptr)

BATCH_OBJS = OBJ_NAMES[:3]  # nlml, loo_crps, loo_logs
BLOCK_BATCH_OBJS = ["dss", "kc"]  # GPS_BLOCK_DSS, GPS_BLOCK_KC
_PI = ctypes.POINTER(ctypes.c_int32)


def _iptr(a):
    return a.ctypes.data_as(_PI)


def _problems(X, y, max_n=BATCH_MAX_N):
    """(X (B, n, d), y (B, n)) checked against the kernel's limits."""
    try:
        X, y = f64(X), f64(y)
    except (ValueError, TypeError) as e:  # a ragged list of problems
        raise ValueError(f"X and y must be rectangular arrays, one shape per batch: {e}") from None
    if X.ndim == 2:
        X = X[:, :, None]
    if X.ndim != 3 or y.ndim != 2:
        raise ValueError(f"X must be (B, n, d) or (B, n) and y (B, n), got {X.shape} and {y.shape}")
    B, n, d = X.shape
    if y.shape != (B, n):
        raise ValueError(f"X {X.shape} and y {y.shape} disagree on (B, n)")
    if B < 1:
        raise ValueError("the batch is empty")
    if not 1 <= n <= max_n:
        raise ValueError(f"n = {n}: a batched problem holds 1..{max_n} training points")
    if not 1 <= d <= BATCH_MAX_D:
        raise ValueError(f"d = {d}: a batched problem has 1..{BATCH_MAX_D} input dimensions")
    return np.ascontiguousarray(X), np.ascontiguousarray(y)


def _thetas(theta, B, d):
    """(B, 2 + n_ell) array and n_ell from one (k, ell, noise) or a per-problem array."""
    if isinstance(theta, (tuple, list)) and len(theta) == 3 and np.ndim(theta[0]) == 0 \
            and np.ndim(theta[2]) == 0:
        ell = np.atleast_1d(np.asarray(theta[1], dtype=np.float64)).ravel()
        row = np.concatenate([[float(theta[0])], ell, [float(theta[2])]])
        th = np.tile(row, (B, 1))
    else:
        try:
            th = f64(theta)
        except (ValueError, TypeError) as e:
            raise ValueError(f"theta must be (k, ell, noise) or a (B, 2 + n_ell) array: {e}") from None
        if th.ndim == 1:
            th = np.tile(th, (B, 1))
        if th.ndim != 2 or th.shape[0] != B:
            raise ValueError(f"theta must be (k, ell, noise) or a (B, 2 + n_ell) array with B = {B}, "
                             f"got shape {th.shape}")
    n_ell = th.shape[1] - 2
    if n_ell not in (1, d):
        raise ValueError(f"log_ell has {n_ell} entries, expected 1 or d={d}")
    return np.ascontiguousarray(th), n_ell


def _objective(objective):
    if objective not in BATCH_OBJS:
        raise ValueError(f"objective must be one of {BATCH_OBJS} (the block-LOO objectives have "
                         f"no batched path), got {objective!r}")
    return OBJ_NAMES.index(objective)


def _block_objective(objective):
    if objective not in BLOCK_BATCH_OBJS:
        raise ValueError(f"objective must be one of {BLOCK_BATCH_OBJS} (the pointwise objectives go "
                         f"through train_tall, the energy score through GP.block_loo), got "
                         f"{objective!r}")
    return BLOCK_BATCH_OBJS.index(objective)


def _nfold(nfold, n):
    hi = min(n, BATCH_BLOCK_MAX_FOLDS)
    if isinstance(nfold, bool) or int(nfold) != nfold or not 2 <= nfold <= hi:
        raise ValueError(f"nfold = {nfold!r}: a batched block-LOO problem of n = {n} rows has "
                         f"2..{hi} folds")
    return int(nfold)


def _es_args(nfold, n, num_sim, beta):
    nfold = _nfold(nfold, n)
    if -(-n // nfold) > BATCH_ES_MAX_FOLD:
        raise ValueError(f"n = {n} rows in {nfold} folds: a batched energy-score fold holds at most "
                         f"{BATCH_ES_MAX_FOLD} rows (its square-root work has to fit one launch), "
                         f"use more folds")
    if isinstance(num_sim, bool) or int(num_sim) != num_sim or not 2 <= num_sim <= BATCH_ES_MAX_SIM:
        raise ValueError(f"num_sim = {num_sim!r}: a batched energy score takes 2..{BATCH_ES_MAX_SIM} "
                         f"draws a fold")
    beta = float(beta)
    if not 0.0 < beta <= 2.0:
        raise ValueError(f"beta must be in (0, 2], got {beta!r}")
    return nfold, int(num_sim), beta


def _es_draws(draws, B, sets, n, nfold, num_sim, rng):
    """(B, sets, 2·num_sim·n) draws: the caller's, or es_draws from rng problem-major then
    set-major."""
    from .gp import es_draws
    per = 2 * num_sim * n
    if draws is None:
        rng = np.random.default_rng(rng)
        return np.stack([np.stack([es_draws(n, nfold, num_sim, rng) for _ in range(sets)])
                         for _ in range(B)])
    try:
        draws = f64(draws)
    except (ValueError, TypeError) as e:
        raise ValueError(f"draws must be a rectangular array: {e}") from None
    if draws.size != B * sets * per:
        raise ValueError(f"draws must hold B·draw_sets·2·num_sim·n = {B}·{sets}·{per} values "
                         f"(es_draws' layout per set), got {draws.size}")
    return np.ascontiguousarray(draws).reshape(B, sets, per)


def _inducing(Z, B, d):
    """Z (B, m, d) checked against the batch and the kernel's limit."""
    try:
        Z = f64(Z)
    except (ValueError, TypeError) as e:  # a ragged list of inducing sets
        raise ValueError(f"Z must be a rectangular array, one m per batch: {e}") from None
    if Z.ndim == 2 and d == 1:
        Z = Z[:, :, None]
    if Z.ndim != 3 or Z.shape[0] != B or Z.shape[2] != d:
        raise ValueError(f"Z must be (B, m, d) = ({B}, m, {d}) (or (B, m) when d = 1), got {Z.shape}")
    m = Z.shape[1]
    if not 1 <= m <= BATCH_FITC_MAX_M:
        raise ValueError(f"m = {m}: a batched FITC problem holds 1..{BATCH_FITC_MAX_M} inducing "
                         f"inputs")
    return np.ascontiguousarray(Z), m


@dataclass
class BatchTrainResult:
    """train_batch's outputs, problem-major.  ``theta`` (B, 2 + n_ell) final parameters;
    ``series`` {"objective": (B, itr) value before each step, "theta": (B, itr, 2 + n_ell)
    parameters after it} as GP.train; ``objectives`` {name: (B,)} of the final pass; ``mu`` /
    ``var`` (B, nt) and ``scores`` {name: (B,)} of the test predictive (None without Xt / yt);
    ``info`` (B,) 0 or the failing leading minor; ``steps_done`` (B,)."""
    theta: np.ndarray
    series: dict
    objectives: dict
    mu: np.ndarray | None
    var: np.ndarray | None
    scores: dict | None
    info: np.ndarray
    steps_done: np.ndarray


def _steps(itr, lr):
    if int(itr) != itr or itr < 0:
        raise ValueError(f"itr must be a non-negative integer, got {itr!r}")
    lr = float(lr)
    if not np.isfinite(lr):
        raise ValueError(f"lr must be finite, got {lr!r}")
    return int(itr), lr


def _tests(Xt, yt, B, d):
    """(Xt (B, nt, d) or None, yt (B, nt) or None, nt) checked against the batch."""
    nt = 0
    if Xt is not None:
        try:
            Xt = f64(Xt)
        except (ValueError, TypeError) as e:
            raise ValueError(f"Xt must be a rectangular array: {e}") from None
        if Xt.ndim == 2 and d == 1:
            Xt = Xt[:, :, None]
        if Xt.ndim != 3 or Xt.shape[0] != B or Xt.shape[2] != d:
            raise ValueError(f"Xt must be (B, nt, d) = ({B}, nt, {d}), got {Xt.shape}")
        Xt = np.ascontiguousarray(Xt)
        nt = Xt.shape[1]
        if nt < 1:
            raise ValueError("Xt holds no rows")
    if yt is not None:
        if Xt is None:
            raise ValueError("yt without Xt")
        yt = f64(yt)
        if yt.shape != (B, nt):
            raise ValueError(f"yt must be (B, nt) = ({B}, {nt}), got {yt.shape}")
    return Xt, yt, nt


@dataclass
class FitcBatchTrainResult(BatchTrainResult):
    """fitc_train_batch's outputs: BatchTrainResult's fields and ``Z`` (B, m, d), the final
    inducing inputs.  ``info`` is 0, k in 1..m (K(Z,Z) + 1e-3·I's leading minor) or m + k (B's)."""
    Z: np.ndarray = None


@dataclass(frozen=True)
class _Path:
    """One batch path, as api_batch.hip's Path<P>: its two entry points, its limit on n, whether
    the model is FITC (Z and m in the call, no kernel kind) and its objective rule — "point": one
    of BATCH_OBJS; "block": one of BLOCK_BATCH_OBJS over nfold folds; "es": the energy score over
    nfold folds with num_sim draws and β."""
    grad: str
    train: str
    max_n: int
    fitc: bool = False
    rule: str = "point"
    va: bool = False  # the training entry takes a validation set and returns its score rows (§34)


_FULL =_Path("gps_full_grad_batch", "gps_full_train_batch", BATCH_MAX_N)
_FULL_TALL = _Path("gps_full_grad_tall", "gps_full_train_tall", BATCH_FULL_TALL_MAX_N)
_FULL_BLOCK = _Path("gps_full_blockloo_grad_tall", "gps_full_blockloo_train_tall",
                    BATCH_FULL_TALL_MAX_N, rule="block")
_FULL_ES = _Path("gps_full_es_grad_tall", "gps_full_es_train_tall", BATCH_FULL_TALL_MAX_N,
                 rule="es")
_FULL_TALL_VA = _Path("gps_full_grad_tall", "gps_full_train_tall_va", BATCH_FULL_TALL_MAX_N, va=True)
_FULL_BLOCK_VA = _Path("gps_full_blockloo_grad_tall", "gps_full_blockloo_train_tall_va",
                       BATCH_FULL_TALL_MAX_N, rule="block", va=True)
_FITC = _Path("gps_fitc_grad_batch","gps_fitc_train_batch", BATCH_MAX_N, fitc=True)
_FITC_TALL = _Path("gps_fitc_grad_tall", "gps_fitc_train_tall", BATCH_FITC_TALL_MAX_N, fitc=True)
_FITC_BLOCK = _Path("gps_fitc_blockloo_grad_tall", "gps_fitc_blockloo_train_tall",
                    BATCH_FITC_TALL_MAX_N, fitc=True, rule="block")
_FITC_TALL_VA = _Path("gps_fitc_grad_tall", "gps_fitc_train_tall_va", BATCH_FITC_TALL_MAX_N,
                      fitc=True, va=True)
_FITC_BLOCK_VA = _Path("gps_fitc_blockloo_grad_tall", "gps_fitc_blockloo_train_tall_va",
                       BATCH_FITC_TALL_MAX_N, fitc=True, rule="block", va=True)


def _front(path, X, y, Z, theta, objective, nfold, num_sim, beta, rbf):
    """The checks every call starts with, in their order — problems, Z, θ, the objective or the ES
    triple, nfold — and ``lead``, the call's arguments up to n_ell (the pointers in it keep their
    arrays alive)."""
    X, y = _problems(X, y, path.max_n)
    B, n, d = X.shape
    m = 0
    if path.fitc:
        Z, m = _inducing(Z, B, d)
    th, n_ell = _thetas(theta, B, d)
    if path.rule == "es":
        nfold, num_sim, beta = head = _es_args(nfold, n, num_sim, beta)
    elif path.rule == "block":
        code = _block_objective(objective)
        nfold = _nfold(nfold, n)
        head = (code, nfold)
    else:
        head = (_objective(objective),)
    lead = (() if path.fitc else (GPS_RBF if rbf else GPS_ARD,)) + head \
        + (B, ptr(X), ptr(y), n, d) + ((ptr(Z), m) if path.fitc else ()) + (ptr(th), n_ell)
    return SimpleNamespace(lead=lead, B=B, n=n, d=d, m=m, n_ell=n_ell, nfold=nfold,
                           num_sim=num_sim, th=th)


def _objectives(obj):
    return {k: obj[:, q].copy() for q, k in enumerate(OBJ_NAMES)}


def _grad(path, X, y, Z, theta, objective=None, nfold=None, num_sim=None, beta=None, draws=None,
          rng=None, rbf=False, ctx=None):
    """A path's value + gradient call: (values, grads[, grad_Z][, fold_values], objectives, info);
    ``values`` is the call's own output on the block and ES paths, objectives[objective] else."""
    f = _front(path, X, y, Z, theta, objective, nfold, num_sim, beta, rbf)
    B, es, folds = f.B, path.rule == "es", path.rule != "point"
    if es:
        draws = _es_draws(draws, B, 1, f.n, f.nfold, f.num_sim, rng)
    ctx = ctx or _lib.default_context()
    vals, fold = (np.empty(B), np.empty((B, f.nfold))) if folds else (None, None)
    obj = np.empty((B, len(OBJ_NAMES)))
    grad = np.empty((B, 2 + f.n_ell))
    gz = np.empty((B, f.m, f.d)) if path.fitc else None
    info = np.zeros(B, np.int32)
    ctx.call(path.grad, *f.lead, *((ptr(draws),) if es else ()),
             *((ptr(vals), ptr(fold)) if folds else ()), ptr(obj), ptr(grad),
             *((ptr(gz),) if path.fitc else ()), _iptr(info))
    objs = _objectives(obj)
    return (vals if folds else objs[objective], grad) + ((gz,) if path.fitc else ()) \
        + ((fold,) if folds else ()) + (objs, info)


SELECT_METRICS = ("crps", "logs", "msll", "smse", "mse")  # validation scores a fit can be selected on


@dataclass
class ValidatedTrainResult(BatchTrainResult):
    """train_tall_validated's outputs: BatchTrainResult's fields, ``va_steps`` (nva,) the step index
    of each validation row — 0, va_every, 2·va_every, ... below itr, then itr for the final pass —
    and ``va_scores`` {name: (B, nva)} over SCORE_NAMES, the validation set's score bundle at the
    parameters of that step's forward (θ before the step; the last row at the final pass's).  With
    ``select``: ``best_step`` (B,) the va_steps entry of the smallest finite score (the earliest
    wins a tie; −1 when no row is finite) and ``theta_best`` (B, 2 + n_ell) the θ that row was
    evaluated at (NaN where best_step is −1); None without."""
    va_steps: np.ndarray = None
    va_scores: dict = None
    best_step: np.ndarray | None = None
    theta_best: np.ndarray | None = None


@dataclass
class FitcValidatedTrainResult(ValidatedTrainResult):
    """fitc_train_tall_validated's outputs: ValidatedTrainResult's fields, ``Z`` (B, m, d) the final
    inducing inputs, and ``va_Z`` (B, nva, m, d) the inducing inputs each validation row was scored
    at (the SGD steps move Z, so θ alone does not name a row's model; the last row is ``Z``) — filled
    when ``select`` is given or ``keep_z`` is true, else None.  With ``select``, ``Z_best`` (B, m, d)
    stands beside ``best_step`` / ``theta_best``: the Z of the selected row, NaN where best_step is
    −1."""
    Z: np.ndarray = None
    va_Z: np.ndarray | None = None
    Z_best: np.ndarray | None = None


def select_best_z(best_step, va_steps, va_Z):
    """The Z pick beside select_best: ``best_step`` (B,) → Z_best (B, m, d), row r of ``va_Z`` (B,
    nva, m, d) where va_steps[r] == best_step (the final pass's row for best_step == itr, which holds
    the returned Z), NaN where best_step is −1."""
    B = va_Z.shape[0]
    zb = np.full((B,) + va_Z.shape[2:], np.nan)
    row = {int(st): r for r, st in enumerate(va_steps)}
    for q in range(B):
        if best_step[q] >= 0:
            zb[q] = va_Z[q, row[int(best_step[q])]]
    return zb


def _va_every(va_every):
    if isinstance(va_every, bool) or not isinstance(va_every, (int, np.integer)) or va_every < 1:
        raise ValueError(f"va_every must be a positive integer, got {va_every!r}")
    return int(va_every)


def _select_metric(select):
    if select is not None and select not in SELECT_METRICS:
        raise ValueError(f"select must be None or one of {SELECT_METRICS} (all lower-is-better; "
                         f"'cover' is a calibration figure, not a score to minimise), got "
                         f"{select!r}")
    return select


def _valids(Xv, yv, B, d):
    """(Xv (B, nv, d), yv (B, nv), nv) checked against the batch as _tests checks Xt / yt; both are
    mandatory."""
    if Xv is None:
        raise ValueError("Xv is required: the validation rows, (B, nv, d)")
    if yv is None:
        raise ValueError("yv is required: a validation set is scored against its targets")
    try:
        Xv = f64(Xv)
    except (ValueError, TypeError) as e:
        raise ValueError(f"Xv must be a rectangular array: {e}") from None
    if Xv.ndim == 2 and d == 1:
        Xv = Xv[:, :, None]
    if Xv.ndim != 3 or Xv.shape[0] != B or Xv.shape[2] != d:
        raise ValueError(f"Xv must be (B, nv, d) = ({B}, nv, {d}), got {Xv.shape}")
    Xv = np.ascontiguousarray(Xv)
    nv = Xv.shape[1]
    if nv < 1:
        raise ValueError("Xv holds no rows")
    try:
        yv = f64(yv)
    except (ValueError, TypeError) as e:
        raise ValueError(f"yv must be a rectangular array: {e}") from None
    if yv.shape != (B, nv):
        raise ValueError(f"yv must be (B, nv) = ({B}, {nv}), got {yv.shape}")
    return Xv, np.ascontiguousarray(yv), nv


def va_steps_of(itr, va_every):
    """The step index of each validation row of a fit of ``itr`` steps: the checkpoints 0, va_every,
    ... below itr, then itr (the final pass): ceil(itr / va_every) + 1 rows."""
    return np.concatenate([np.arange(0, itr, va_every), [itr]]).astype(np.int64)


def select_best(va_row, va_steps, theta0, thetas, theta):
    """Host arithmetic of ``select``: ``va_row`` (B, nva) one lower-is-better score per validation
    row → (best_step (B,), theta_best (B, nth)).  The smallest finite entry wins, the earliest on a
    tie; the θ of row r is theta0 for step 0, thetas[:, i − 1] for checkpoint step i and ``theta``
    for the last row (the final pass).  No finite row: −1 and NaN."""
    va_row = np.asarray(va_row, dtype=np.float64)
    B, nva = va_row.shape
    best = np.full(B, -1, np.int64)
    th = np.full((B, theta0.shape[1]), np.nan)
    for q in range(B):
        ok = np.isfinite(va_row[q])
        if not ok.any():
            continue
        r = int(np.argmin(np.where(ok, va_row[q], np.inf)))  # argmin: the first of equal minima
        best[q] = va_steps[r]
        th[q] = theta[q] if r == nva - 1 else theta0[q] if va_steps[r] == 0 \
            else thetas[q, va_steps[r] - 1]
    return best, th


def _train(path, X, y, Z0, theta0, objective=None, nfold=None, num_sim=None, beta=None, lr=1.0,
           lr_z=None, itr=400, draws=None, draw_sets=None, rng=None, Xt=None, yt=None, rbf=False,
           stale_noise=False, ctx=None, Xv=None, yv=None, va_every=1, select=None, keep_z=False):
    """A path's training call: BatchTrainResult, FitcBatchTrainResult on a FITC path, or
    ValidatedTrainResult on a path with a validation set (path.va: Xv, yv, va_every, select;
    FitcValidatedTrainResult and keep_z where the path is FITC too)."""
    f = _front(path, X, y, Z0, theta0, objective, nfold, num_sim, beta, rbf)
    B, es = f.B, path.rule == "es"
    itr, lr = _steps(itr, lr)
    if path.fitc:
        lr_z = lr if lr_z is None else float(lr_z)
        if not np.isfinite(lr_z):
            raise ValueError(f"lr_z must be finite, got {lr_z!r}")
    if es:
        sets = max(itr, 1) if draw_sets is None else draw_sets
        if isinstance(sets, bool) or int(sets) != sets or not 1 <= sets <= max(itr, 1):
            raise ValueError(f"draw_sets = {draw_sets!r}: a fit of {itr} steps takes 1..{max(itr, 1)} "
                             f"draw sets")
        sets = int(sets)
    Xt, yt, nt = _tests(Xt, yt, B, f.d)
    if path.va:
        Xv, yv, nv = _valids(Xv, yv, B, f.d)
        va_every = _va_every(va_every)
        select = _select_metric(select)
        va_steps = va_steps_of(itr, va_every)
        va_sc = np.empty((B, len(va_steps), len(SCORE_NAMES)))
        va_Z = np.empty((B, len(va_steps), f.m, f.d)) \
            if path.fitc and (select is not None or keep_z) else None
    if es:
        draws = _es_draws(draws, B, sets, f.n, f.nfold, f.num_sim, rng)
    ctx = ctx or _lib.default_context()
    nth = 2 + f.n_ell
    theta = np.empty((B, nth))
    Z = np.empty((B, f.m, f.d)) if path.fitc else None
    values, thetas = np.empty((B, itr)), np.empty((B, itr, nth))
    obj = np.empty((B, len(OBJ_NAMES)))
    mu = np.empty((B, nt)) if nt else None
    var = np.empty((B, nt)) if nt else None
    sc = np.empty((B, len(SCORE_NAMES))) if yt is not None else None
    info, steps = np.zeros(B, np.int32), np.zeros(B, np.int32)
    ctx.call(path.train, *f.lead, itr, lr, *((lr_z,) if path.fitc else ()),
             *((ptr(Xv), ptr(yv), nv, va_every) if path.va else ()), ptr(Xt), ptr(yt), nt,
             GPS_BATCH_STALE_NOISE if stale_noise else 0, *((ptr(draws), sets) if es else ()),
             ptr(theta), *((ptr(Z),) if path.fitc else ()), ptr(values), ptr(thetas), ptr(obj),
             ptr(mu), ptr(var), ptr(sc), *((ptr(va_sc),) if path.va else ()),
             *((ptr(va_Z),) if path.va and path.fitc else ()), _iptr(info),
             _iptr(steps))
    res = dict(theta=theta, series={"objective": values, "theta": thetas},
               objectives=_objectives(obj), mu=mu, var=var,
               scores=None if sc is None else {k: sc[:, q].copy()
                                               for q, k in enumerate(SCORE_NAMES)},
               info=info, steps_done=steps)
    if path.va:
        va_scores = {k: va_sc[:, :, q].copy() for q, k in enumerate(SCORE_NAMES)}
        best, th_best = (None, None) if select is None else select_best(
            va_scores["test_" + select], va_steps, f.th, thetas, theta)
        if path.fitc:
            return FitcValidatedTrainResult(
                va_steps=va_steps, va_scores=va_scores, best_step=best, theta_best=th_best, Z=Z,
                va_Z=va_Z, Z_best=None if select is None else select_best_z(best, va_steps, va_Z),
                **res)
        return ValidatedTrainResult(va_steps=va_steps, va_scores=va_scores, best_step=best,
                                    theta_best=th_best, **res)
    return FitcBatchTrainResult(Z=Z, **res) if path.fitc else BatchTrainResult(**res)


def value_and_grad_batch(X, y, theta, objective="loo_crps", rbf=False, ctx=None):
    """Objective value and analytic gradient of B small full GPs at their own θ (one
    gps_full_grad_batch call; per problem what GP.value_and_grad returns).  Returns
    (values (B,), grads (B, 2 + n_ell), objectives {name: (B,)}, info (B,))."""
    return _grad(_FULL, X, y, None, theta, objective, rbf=rbf, ctx=ctx)


def train_batch(X, y, theta0, objective="loo_crps", lr=1.0, itr=400, Xt=None, yt=None, rbf=False,
                stale_noise=False, ctx=None):
    """The reference's SGD fit loop (`itr` steps θ -= lr·grad, KF:236-260) for B small full GPs
    at once on the device, then one forward at the final kernel parameters with the test
    predictive at ``Xt`` ((B, nt, d) or (B, nt)) and its score bundle against ``yt`` (B, nt).
    ``stale_noise``: the final pass uses the noise variance of the last step's forward (θ0's
    with itr = 0), the scripts' module-global sigma_noise_sq (experiment.run_method)."""
    return _train(_FULL, X, y, None, theta0, objective, lr=lr, itr=itr, Xt=Xt, yt=yt, rbf=rbf,
                  stale_noise=stale_noise, ctx=ctx)


def value_and_grad_tall(X, y, theta, objective="loo_crps", rbf=False, ctx=None):
    """value_and_grad_batch for problems of 1 <= n <= 512 training points (one gps_full_grad_tall
    call, DESIGN §24: one workgroup per problem with the n×n arrays in a device workspace
    instead of LDS and the O(n³) work on the FP64 matrix instruction).  Same arguments, returns,
    refusals and ``info``; for n <= 128 the small-batch call is the faster route."""
    return _grad(_FULL_TALL, X, y, None, theta, objective, rbf=rbf, ctx=ctx)


def train_tall(X, y, theta0, objective="loo_crps", lr=1.0, itr=400, Xt=None, yt=None, rbf=False,
               stale_noise=False, ctx=None):
    """train_batch for problems of 1 <= n <= 512 training points (one gps_full_train_tall call):
    the replicate loop of "kin40k-FULL-compare.py" (n = 500, d = 8) for B problems at once.  Same
    arguments, refusals and BatchTrainResult."""
    return _train(_FULL_TALL, X, y, None, theta0, objective, lr=lr, itr=itr, Xt=Xt, yt=yt, rbf=rbf,
                  stale_noise=stale_noise, ctx=ctx)


def blockloo_value_and_grad_tall(X, y, theta, objective="dss", nfold=4, rbf=False, ctx=None):
    """Block-LOO objective ("dss" or "kc", GP.block_loo's, over the scripts' nfold folds
    [int(f·n/nfold), int((f+1)·n/nfold))) and its analytic gradient for B full GPs of 1 <= n <=
    512 training points at their own θ (one gps_full_blockloo_grad_tall call).
    Arguments, refusals and ``info`` as value_and_grad_tall; ``info`` n + k reports an internal
    error at global row k of its fold's block.  Returns (values (B,), grads (B, 2 + n_ell),
    fold_values (B, nfold), objectives {name: (B,)}, info (B,))."""
    return _grad(_FULL_BLOCK, X, y, None, theta, objective, nfold, rbf=rbf, ctx=ctx)


def blockloo_train_tall(X, y, theta0, objective="dss", nfold=4, lr=1e-3, itr=150, Xt=None, yt=None,
                        rbf=False, stale_noise=False, ctx=None):
    """train_tall on a block-LOO objective (one gps_full_blockloo_train_tall call): the 4-fold DSS
    fit of "kin40k-FULL-compare.py" (KF:487-601: 150 steps at lr 1e-3, the defaults here) or its
    CRPS sibling "kc" (K20:655-720) for B problems at once.  ``series["objective"]`` is the block
    objective before each step; everything else as train_tall: arguments, refusals and
    BatchTrainResult."""
    return _train(_FULL_BLOCK, X, y, None, theta0, objective, nfold, lr=lr, itr=itr, Xt=Xt, yt=yt,
                  rbf=rbf, stale_noise=stale_noise, ctx=ctx)


def train_tall_validated(X, y, theta0, Xv, yv, objective="loo_crps", lr=1.0, itr=400, va_every=1,
                         select=None, Xt=None, yt=None, rbf=False, stale_noise=False, ctx=None):
    """train_tall with a validation set scored inside the fit (one gps_full_train_tall_va call,
    DESIGN §34): the per-iteration validation series "kin40k-FULL-compare.py" carries commented out
    (KF:441-449), from the factorisation each step has in hand.  ``Xv`` (B, nv, d) or (B, nv), ``yv``
    (B, nv), both mandatory; every step i with i % ``va_every`` == 0 scores them at that step's
    forward (θ before the step, its own σ²: the model ``series["objective"][:, i]`` describes), and
    the final pass adds one more row at its own parameters.  Under ``stale_noise`` that last row's
    noise is the stale one — the σ² of the last step's forward, so with itr = k it is the scripts'
    va_series[k − 1] — while ``theta_best`` for it is the final θ as returned.  ``select``: one of
    "crps", "logs", "msll", "smse", "mse" (lower is better) picks each problem's best row on the
    host.  The fit is bitwise train_tall's; everything else as there.  Returns
    ValidatedTrainResult."""
    return _train(_FULL_TALL_VA, X, y, None, theta0, objective, lr=lr, itr=itr, Xt=Xt, yt=yt,
                  rbf=rbf, stale_noise=stale_noise, ctx=ctx, Xv=Xv, yv=yv, va_every=va_every,
                  select=select)


def blockloo_train_tall_validated(X, y, theta0, Xv, yv, objective="dss", nfold=4, lr=1e-3, itr=150,
                                  va_every=1, select=None, Xt=None, yt=None, rbf=False,
                                  stale_noise=False, ctx=None):
    """blockloo_train_tall with a validation set scored inside the fit (one
    gps_full_blockloo_train_tall_va call; the series KF:557-563 carries commented out,
    its pointwise scores).  Validation arguments, ``select`` and ValidatedTrainResult as
    train_tall_validated; the fit is bitwise blockloo_train_tall's."""
    return _train(_FULL_BLOCK_VA, X, y, None, theta0, objective, nfold, lr=lr, itr=itr, Xt=Xt,
                  yt=yt, rbf=rbf, stale_noise=stale_noise, ctx=ctx, Xv=Xv, yv=yv,
                  va_every=va_every, select=select)


def es_value_and_grad_tall(X, y, theta, nfold=4, num_sim=300, beta=1.0, draws=None, rng=None,
                           rbf=False, ctx=None):
    """The block-LOO energy score (GP.block_loo's "es", KF:607-663) and its analytic gradient for B
    full GPs of 1 <= n <= 512 training points at their own θ (one gps_full_es_grad_tall call,
    DESIGN §32: the fold work runs on one workgroup per (problem, fold)).  ``draws``: (B,
    2·num_sim·n) standard-normal draws, one es_draws set a problem (None: drawn from ``rng``,
    problem-major).  A fold holds at most 128 rows (ceil(n / nfold) <= 128), 2 <= num_sim <= 512, 0 <
    beta <= 2; other arguments and refusals as blockloo_value_and_grad_tall.  ``info`` n + k as
    there, 2n + 1 + f: fold f's square root would need more than 40 Newton–Schulz steps.
    Returns (values (B,), grads (B, 2 + n_ell), fold_values (B, nfold), objectives {name: (B,)},
    info (B,))."""
    return _grad(_FULL_ES, X, y, None, theta, None, nfold, num_sim, beta, draws=draws, rng=rng,
                 rbf=rbf, ctx=ctx)


def es_train_tall(X, y, theta0, nfold=4, num_sim=300, beta=1.0, lr=0.1, itr=25, draws=None,
                  draw_sets=None, rng=None, Xt=None, yt=None, rbf=False, stale_noise=False,
                  ctx=None):
    """train_tall on the block-LOO energy score (one gps_full_es_train_tall call): the 4-fold ES fit
    of "kin40k-FULL-compare.py" (KF:607-732: 25 steps at lr 0.1 with 300 draws a fold, the defaults
    here) for B problems at once.  Step i uses draw set i mod ``draw_sets``: ``draw_sets`` = itr (the
    default) is the scripts' fresh draws every step, 1 is common random numbers; 1 <= draw_sets <=
    max(itr, 1).  ``draws``: (B, draw_sets, 2·num_sim·n), every set in es_draws' layout (None: drawn
    from ``rng``, problem-major then set-major).  The draws count towards the 8 GiB a call may
    take: B = 30 with 25 sets of 300 at n = 500 is 1.8 GB and fits, B = 256 does not — fewer
    ``draw_sets`` is the way out.  ``series["objective"]`` is the energy score before each step;
    limits as es_value_and_grad_tall, everything else as train_tall: arguments, refusals and
    BatchTrainResult."""
    return _train(_FULL_ES, X, y, None, theta0, None, nfold, num_sim, beta, lr=lr, itr=itr,
                  draws=draws, draw_sets=draw_sets, rng=rng, Xt=Xt, yt=yt, rbf=rbf,
                  stale_noise=stale_noise, ctx=ctx)


def fitc_value_and_grad_batch(X, y, Z, theta, objective="loo_crps", ctx=None):
    """Objective value and analytic gradient of B small FITC GPs at their own (θ, Z) (one
    gps_fitc_grad_batch call; per problem what GP.value_and_grad(..., Z=Z) returns).  Returns
    (values (B,), grads (B, 2 + n_ell), grad_Z (B, m, d), objectives {name: (B,)}, info (B,))."""
    return _grad(_FITC, X, y, Z, theta, objective, ctx=ctx)


def fitc_train_batch(X, y, Z0, theta0, objective="loo_crps", lr=1.0, lr_z=None, itr=400, Xt=None,
                     yt=None, stale_noise=False, ctx=None):
    """The SGD fit loop of the FITC scripts (`itr` steps θ -= lr·grad, Z -= lr_z·grad_Z,
    SF:229-233; lr_z defaults to lr) for B small FITC GPs at once on the device, then one forward
    at the final θ and Z with the test predictive at ``Xt`` ((B, nt, d) or (B, nt)) and its score
    bundle against ``yt`` (B, nt).  ``stale_noise`` as train_batch."""
    return _train(_FITC, X, y, Z0, theta0, objective, lr=lr, lr_z=lr_z, itr=itr, Xt=Xt, yt=yt,
                  stale_noise=stale_noise, ctx=ctx)


def fitc_value_and_grad_tall(X, y, Z, theta, objective="loo_crps", ctx=None):
    """fitc_value_and_grad_batch for tall problems, 1 <= n <= 2048 (one gps_fitc_grad_tall call,
    DESIGN §22: one workgroup per problem with the n-sized arrays in a device workspace instead
    of LDS).  Same arguments, returns, refusals and ``info``; for n <= 128 the small-batch call
    is the faster route."""
    return _grad(_FITC_TALL, X, y, Z, theta, objective, ctx=ctx)


def fitc_train_tall(X, y, Z0, theta0, objective="loo_crps", lr=1.0, lr_z=None, itr=400, Xt=None,
                    yt=None, stale_noise=False, ctx=None):
    """fitc_train_batch for tall problems, 1 <= n <= 2048 (one gps_fitc_train_tall call): the
    replicate loops of "KIN40K-COMPARE-ALL-FITC-20" (n = 500, d = 8, m = 20) for B problems at
    once.  Same arguments, refusals and FitcBatchTrainResult."""
    return _train(_FITC_TALL, X, y, Z0, theta0, objective, lr=lr, lr_z=lr_z, itr=itr, Xt=Xt, yt=yt,
                  stale_noise=stale_noise, ctx=ctx)


def fitc_blockloo_value_and_grad_tall(X, y, Z, theta, objective="dss", nfold=4, ctx=None):
    """Block-LOO objective ("dss" or "kc", GP.block_loo's, over the scripts' nfold folds
    [int(f·n/nfold), int((f+1)·n/nfold))) and its analytic gradients for B FITC GPs of 1 <= n <=
    2048 training points at their own (θ, Z) (one gps_fitc_blockloo_grad_tall call).
    Arguments, refusals and ``info`` as fitc_value_and_grad_tall; ``info`` (2 + f)·m + k reports an
    internal error in fold f's factorisation.  Returns (values (B,), grads (B, 2 + n_ell), grad_Z
    (B, m, d), fold_values (B, nfold), objectives {name: (B,)}, info (B,))."""
    return _grad(_FITC_BLOCK, X, y, Z, theta, objective, nfold, ctx=ctx)


def fitc_blockloo_train_tall(X, y, Z0, theta0, objective="dss", nfold=4, lr=1e-3, lr_z=None,
                             itr=3000, Xt=None, yt=None, stale_noise=False, ctx=None):
    """fitc_train_tall on a block-LOO objective (one gps_fitc_blockloo_train_tall call): the 4-fold
    DSS fit of "KIN40K-COMPARE-ALL-FITC-20" (K20:523-593: 3000 steps at lr = lr_z = 1e-3, the
    defaults here) or its CRPS sibling "kc" (K20:655-726, lr = lr_z = 0.1) for B problems at once.
    ``series["objective"]`` is the block objective before each step; everything else as
    fitc_train_tall: arguments, refusals and FitcBatchTrainResult."""
    return _train(_FITC_BLOCK, X, y, Z0, theta0, objective, nfold, lr=lr, lr_z=lr_z, itr=itr, Xt=Xt,
                  yt=yt, stale_noise=stale_noise, ctx=ctx)


def fitc_train_tall_validated(X, y, Z0, theta0, Xv, yv, objective="loo_crps", lr=1.0, lr_z=None,
                              itr=400, va_every=1, select=None, keep_z=False, Xt=None, yt=None,
                              stale_noise=False, ctx=None):
    """fitc_train_tall with a validation set scored inside the fit (one gps_fitc_train_tall_va call,
    DESIGN §37): the per-iteration validation series "KIN40K-COMPARE-ALL-FITC-20" carries commented
    out (K20:258-264, 469-476), from Lm⁻¹, Lb⁻¹ and c as each step's forward leaves them.  Validation
    arguments, ``va_every`` and ``select`` as train_tall_validated; a row's model is θ AND Z before
    its step, so ``select`` (or ``keep_z``) also brings back ``va_Z``, every row's inducing inputs,
    and ``select`` adds ``Z_best``.  The fit is bitwise fitc_train_tall's.  Returns
    FitcValidatedTrainResult."""
    return _train(_FITC_TALL_VA, X, y, Z0, theta0, objective, lr=lr, lr_z=lr_z, itr=itr, Xt=Xt,
                  yt=yt, stale_noise=stale_noise, ctx=ctx, Xv=Xv, yv=yv, va_every=va_every,
                  select=select, keep_z=keep_z)


def fitc_blockloo_train_tall_validated(X, y, Z0, theta0, Xv, yv, objective="dss", nfold=4, lr=1e-3,
                                       lr_z=None, itr=3000, va_every=1, select=None, keep_z=False,
                                       Xt=None, yt=None, stale_noise=False, ctx=None):
    """fitc_blockloo_train_tall with a validation set scored inside the fit (one
    gps_fitc_blockloo_train_tall_va call; the series K20:737-743 carries commented out,
    its pointwise scores).  Validation arguments, ``select``, ``keep_z`` and
    FitcValidatedTrainResult as fitc_train_tall_validated; the fit is bitwise
    fitc_blockloo_train_tall's."""
    return _train(_FITC_BLOCK_VA, X, y, Z0, theta0, objective, nfold, lr=lr, lr_z=lr_z, itr=itr,
                  Xt=Xt, yt=yt, stale_noise=stale_noise, ctx=ctx, Xv=Xv, yv=yv, va_every=va_every,
                  select=select, keep_z=keep_z)
