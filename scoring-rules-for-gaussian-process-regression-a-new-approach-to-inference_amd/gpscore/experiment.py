"""Data ingest and the replicate harness of the reference scripts, on top of the device hot
path.

kin40k-FULL-compare.py (KF) loops over TT replicates (KF:149-190): 800 of the 10 000
training rows drawn with Python's `random` seeded 100·j (KF:194-196), 300 of them held out
for validation (KF:203-209), the first 500 test rows (KF:199-200); then five fits of the
full GP from a random start, each scored on the test set (MSE, SMSE, LogS, CRPS, MSLL and
the ±2σ coverage, e.g. KF:267-299).  KIN40K-COMPARE-ALL-FITC-20.py (K20) does the same with
a 20-point FITC model whose inducing inputs are trained too, drawing rows without
reseeding (K20:184-192).

"SIMPLE-DATA FULL-comapre.py" (SD) draws TT = 100 one-dimensional data sets of 120 training
and 300 test points (SD:158-181) and makes three fits of each from (1, 1, 1) (SD:192-231,
277-301, 372-396): run_simple sends all replicates of a method through one train_batch call.
"SIMPLE-FITC--comapre.py" (SF) fits the same data sets with a FITC model of m = 5 inducing inputs
that are trained too (SF:189-237, 301-343, 420-463): run_simple_fitc, one fitc_train_batch call
per method.  K20's own LOO-CRPS / NLML / LOO-LogS fits (n = 500, m = 20) go the same way through
run_fitc_batch, one fitc_train_tall call per method; its block-LOO DSS and KC fits through
run_fitc_blockloo_batch, one fitc_blockloo_train_tall call per method.  KF's
LOO-CRPS / NLML / LOO-LogS fits (full GP, n = 500) have a batch route as well: run_full_batch, one
train_tall call per method for all replicates; its block-LOO DSS fit goes through
run_full_blockloo_batch, one blockloo_train_tall call for all replicates, and its ES fit through
run_full_es_batch, one es_train_tall call: all five KF methods have a one-call-per-method route.
run_full_validated_batch is run_full_batch / run_full_blockloo_batch with every replicate's
validation split (KF:203-209) scored inside the fits, step by step (KF:441-449, commented out there).

Every number here comes from gpscore.GP (libgpscore.so): the SGD loops are GP.train, the
predictive and its scores GP.predict (run_simple: gpscore.batch.train_batch).  The workbook is not shipped (the scripts open it from
a Windows drive), so load_sheets reads the .xlsx when pandas has an Excel engine, or the
same four sheets from an .npz or a directory of <sheet>.csv files.
"""
from __future__ import annotations

import os
import random
from dataclasses import dataclass

import numpy as np

from ._lib import NotPositiveDefinite
from .batch import (BATCH_OBJS, BLOCK_BATCH_OBJS, blockloo_train_tall, es_train_tall,
                    fitc_blockloo_train_tall, fitc_train_batch, fitc_train_tall, train_batch,
                    train_tall)
from .gp import GP

SHEETS = ("trainx", "trainy", "testx", "testy")
METRICS = ("mse", "smse", "logs", "crps", "msll", "cover")


def _as2d(a):
    a = np.asarray(a, dtype=np.float64)
    return a.reshape(a.shape[0], -1) if a.ndim == 1 else a


def load_sheets(path):
    """{trainx, trainy, testx, testy} as 2-D float64 arrays from kin40k.xlsx (sheet names and
    header=None as KF:197-200), an .npz holding those keys, or a directory of <sheet>.csv."""
    if os.path.isdir(path):
        return {s: _as2d(np.loadtxt(os.path.join(path, s + ".csv"), delimiter=",", ndmin=2))
                for s in SHEETS}
    if str(path).endswith(".npz"):
        with np.load(path, allow_pickle=False) as z:
            return {s: _as2d(z[s]) for s in SHEETS}
    import pandas as pd  # an Excel engine (openpyxl / xlrd) must be installed for .xlsx
    return {s: _as2d(pd.read_excel(path, sheet_name=s, header=None).values) for s in SHEETS}


def synthetic_sheets(rng=None, n_pool=10000, n_test=500, d=8):
    """Stand-in sheets of kin40k's shapes (d = 8 inputs, one target) from the SURVEY.md §8d
    generator, for running the harness without the workbook."""
    rng = np.random.default_rng(rng)
    w = rng.standard_normal(d) / np.sqrt(d)
    X, Xt = rng.standard_normal((n_pool, d)), rng.standard_normal((n_test, d))
    y = np.sin(3 * X @ w) + 0.1 * rng.standard_normal(n_pool)
    yt = np.sin(3 * Xt @ w) + 0.1 * rng.standard_normal(n_test)
    return {"trainx": X, "trainy": y[:, None], "testx": Xt, "testy": yt[:, None]}


def replicate_indices(j=None, n_pool=10000, n_train=500, num_va=300, rs=None):
    """Row draws of replicate j as the scripts make them with the global `random`:
    random.seed(100·j) (KF:194; K20 never reseeds: pass j=None and one `rs` for all
    replicates), sam = random.sample(range(0, n_pool), n_train + num_va) (KF:196),
    va = random.sample(range(0, n_train + num_va), num_va) (KF:203)."""
    if rs is None:
        rs = random.Random()
    if j is not None:
        rs.seed(j * 100)
    sam = np.array(rs.sample(range(0, n_pool), n_train + num_va))
    va = np.array(rs.sample(range(0, n_train + num_va), num_va))
    return sam, va


def replicate(sheets, j=None, n_train=500, num_va=300, n_test=500, n_pool=10000, rs=None):
    """Train / validation / test arrays of replicate j (KF:194-211): full = trainx[sam], the va
    rows held out (np.delete, KF:208-209), test = the first n_test rows (KF:199-200)."""
    sam, va = replicate_indices(j, n_pool, n_train, num_va, rs)
    full_x, full_y = sheets["trainx"][sam], sheets["trainy"][sam]
    return {"train_x": np.delete(full_x, va, axis=0),
            "train_y": np.delete(full_y, va, axis=0).ravel(),
            "va_x": full_x[va], "va_y": full_y[va].ravel(),
            "test_x": sheets["testx"][:n_test], "test_y": sheets["testy"][:n_test].ravel()}


@dataclass(frozen=True)
class Method:
    """One fit of the scripts: objective (GP.train name), SGD length and step, starting point,
    the lines it restates."""
    objective: str
    itr: int
    lr: float
    lr_z: float | None = None  # FITC inducing-input step (None: lr)
    init: str = "rand_l"       # rand3: para_l ~ U(0,1)^d, para_k, para_noise ~ U(0,1) (KF:226-233)
                               # rand_l: para_l ~ U(0,1)^d, para_k = para_noise = 1 (KF:321-324)
                               # ones: scalar para_l = para_k = para_noise = 1 (K20:422-424)
    z_init: str = "rand"       # FITC inducing_x start: U(0,1) (K20:215) or N(0,1) (K20:531)
    ref: str = ""


KF_METHODS = {
    "crps": Method("loo_crps", 400, 1.0, init="rand3", ref="KF:220-299"),
    "nlml": Method("nlml", 400, 5e-4, ref="KF:312-399"),   # the scripts' "gp" series
    "logs": Method("loo_logs", 500, 0.05, ref="KF:405-482"),
    "dss": Method("dss", 150, 1e-3, ref="KF:487-601"),
    "es": Method("es", 25, 0.1, ref="KF:607-732"),
}
K20_METHODS = {
    "crps": Method("loo_crps", 2000, 1.0, 1.0, ref="K20:207-247"),
    "nlml": Method("nlml", 3000, 1e-4, 1e-3, ref="K20:315-350"),
    "logs": Method("loo_logs", 3000, 0.2, 0.2, init="ones", ref="K20:417-458"),
    "dss": Method("dss", 3000, 1e-3, 1e-3, z_init="randn", ref="K20:523-593"),
    "kc": Method("kc", 3000, 0.1, 0.1, ref="K20:655-726"),
}
# "SIMPLE-DATA FULL-comapre.py": scalar para_l = para_k = para_noise = 1 (SD:203-205), ARD kernel
SD_METHODS = {
    "crps": Method("loo_crps", 250, 1.0, init="ones", ref="SD:192-231"),
    "nlml": Method("nlml", 250, 1e-3, init="ones", ref="SD:277-301"),   # the script's "gp" series
    "logs": Method("loo_logs", 400, 0.05, init="ones", ref="SD:372-396"),
}
# "SIMPLE-FITC--comapre.py": the same start, m = 5 inducing inputs with their own step lr_z
SF_METHODS = {
    "crps": Method("loo_crps", 1000, 1.0, 1.0, init="ones", ref="SF:189-237"),
    "nlml": Method("nlml", 1200, 5e-4, 5e-3, init="ones", ref="SF:301-343"),   # the "gp" series
    "logs": Method("loo_logs", 2500, 5e-3, 5e-3, init="ones", ref="SF:420-463"),
}


def initial_theta(method, d, rng):
    """(para_k, para_l, para_noise) at the method's start (torch.rand there, numpy here)."""
    if method.init == "rand3":
        return (float(rng.random()), rng.random(d), float(rng.random()))
    if method.init == "ones":
        return (1.0, np.array([1.0]), 1.0)
    return (1.0, rng.random(d), 1.0)


def run_method(gp, data, method, rng, kind="full", m=20, itr=None, stale_noise=True,
               num_sim=300, joint=()):
    """One fit (the method's SGD loop, GP.train) + test predictive + score bundle.
    Returns {mse, smse, logs, crps, msll, cover, theta, Z, failed}.  The predictive uses the
    final kernel parameters and, with stale_noise, the noise variance of the last iteration's
    forward pass: the scripts' module-global sigma_noise_sq is set before the last update and
    read by cal_mean_and_cov / spgp_cal_mean_and_cov.  The ES and KC fits turn
    a non-PD factorisation into zero metrics (KF:726-732, K20:784-790); others raise.
    ``joint``: names from ("dss", "es") — also report the multivariate score of the test targets
    under the JOINT test predictive (GP.joint_score, one block: the calls the scripts carry
    commented out at KF:556-563 and KF:677-684); off by default, so the series are unchanged."""
    joint = tuple(joint)
    d = data["train_x"].shape[1]
    th0 = initial_theta(method, d, rng)
    itr = method.itr if itr is None else int(itr)
    block_kw = {"num_sim": num_sim, "rng": rng} if method.objective == "es" else None
    Z0 = None
    if kind == "fitc":
        Z0 = rng.random((m, d)) if method.z_init == "rand" else rng.standard_normal((m, d))
    try:
        theta, series = gp.train(th0, method.objective, lr=method.lr, itr=itr,
                                 X=data["train_x"], y=data["train_y"], Z0=Z0, lr_z=method.lr_z,
                                 block_kw=block_kw)
        noise = theta[2]
        if stale_noise:
            noise = float(series["theta"][itr - 2][-1]) if itr >= 2 else float(th0[2])
        gp.fit(theta=(theta[0], theta[1], noise), return_loo=False)
        _, _, sc = gp.predict(data["test_x"], data["test_y"], with_scores=True)
        js = {k: gp.joint_score(k, num_sim=num_sim, rng=rng) for k in joint}
    except NotPositiveDefinite:
        if method.objective not in ("es", "kc"):
            raise
        return dict({k: 0.0 for k in METRICS + joint}, theta=None, Z=None, failed=True)
    return {**js, "mse": sc["test_mse"], "smse": sc["test_smse"], "logs": sc["test_logs"],
            "crps": sc["test_crps"], "msll": sc["test_msll"], "cover": sc["test_cover"],
            "theta": theta, "Z": series.get("Z"), "failed": False}


def run(sheets, TT=30, methods=None, kind="full", itr=None, seed=None, ctx=None, reseed=True,
        **kw):
    """TT replicates → {method: {metric: array(TT)}}, the scripts' <metric>_<method>_series
    (KF:149-184, K20:145-180).  reseed: KF's random.seed(100·j); False: one unseeded stream
    (K20).  `seed` drives the random starting points (torch.rand in the scripts)."""
    methods = methods or (KF_METHODS if kind == "full" else K20_METHODS)
    gp = GP(ctx=ctx)
    rng = np.random.default_rng(seed)
    rs = None if reseed else random.Random()
    keys = METRICS + tuple(kw.get("joint", ()))
    out = {name: {k: np.zeros(TT) for k in keys} for name in methods}
    n_pool = sheets["trainx"].shape[0]  # 10 000 in kin40k, the scripts' range(0, 10000)
    for j in range(TT):
        data = replicate(sheets, j if reseed else None, n_pool=n_pool, rs=rs)
        for name, meth in methods.items():
            r = run_method(gp, data, meth, rng, kind=kind, itr=itr, **kw)
            for k in keys:
                out[name][k][j] = r[k]
    return out


def simple_data(j, rng=None, num_train=120, num_test=300, num_va=30):
    """Replicate j of SD's generator (SD:158-181): x = 2·N(0, 1) for num_train + num_test +
    num_va = 450 points, y one draw of N(0, K + 0.3²I) with K the unit-scale, unit-length
    squared-exponential kernel, split in that order into train / test / validation.  The
    script seeds torch with 100·j and draws in float32; here the draws are numpy's, in float64,
    from ``rng`` (a Generator or a seed; default seed 100·j) — NOT torch's: the same law, other
    numbers.  The script's own j = 0, 1 data sets are the tests' sd_j* golden files."""
    rng = np.random.default_rng(100 * j if rng is None else rng)
    tot = num_train + num_test + num_va
    x = 2.0 * rng.standard_normal(tot)
    K = np.exp(-0.5 * (x[:, None] - x[None, :]) ** 2) + 0.3 ** 2 * np.eye(tot)
    y = np.linalg.cholesky(K) @ rng.standard_normal(tot)
    a, b = num_train, num_train + num_test
    return {"train_x": x[:a, None], "train_y": y[:a], "test_x": x[a:b, None], "test_y": y[a:b],
            "va_x": x[b:, None], "va_y": y[b:]}


def run_simple(TT=100, methods=None, datasets=None, itr=None, stale_noise=True, ctx=None):
    """SD's replicate loop → {method: {metric: array(TT)}} as run: every method's TT fits (its
    SGD loop, the test predictive and the score bundle) are ONE train_batch call, one
    workgroup per replicate.  ``datasets``: TT dicts with train_x / train_y / test_x / test_y of
    one shape (default simple_data(j), j < TT); ``itr`` overrides the methods' step counts;
    stale_noise as run_method.  A replicate whose factorisation fails raises
    NotPositiveDefinite, as run_method does for these objectives."""
    methods = SD_METHODS if methods is None else methods
    if datasets is None:
        datasets = [simple_data(j) for j in range(TT)]
    datasets = list(datasets)
    if len(datasets) != TT:
        raise ValueError(f"{len(datasets)} datasets for TT = {TT} replicates")
    X = np.stack([_as2d(dd["train_x"]) for dd in datasets])
    y = np.stack([np.asarray(dd["train_y"], np.float64).ravel() for dd in datasets])
    Xt = np.stack([_as2d(dd["test_x"]) for dd in datasets])
    yt = np.stack([np.asarray(dd["test_y"], np.float64).ravel() for dd in datasets])
    d = X.shape[2]
    out = {}
    for name, meth in methods.items():
        th0 = initial_theta(meth, d, None)
        res = train_batch(X, y, th0, meth.objective, lr=meth.lr,
                          itr=meth.itr if itr is None else int(itr), Xt=Xt, yt=yt,
                          stale_noise=stale_noise, ctx=ctx)
        bad = np.flatnonzero(res.info)
        if bad.size:
            q = int(bad[0])
            raise NotPositiveDefinite(int(res.info[q]), f"run_simple: method {name!r}, replicate "
                                      f"{q}: the leading minor of order {int(res.info[q])} is not "
                                      f"positive definite after {int(res.steps_done[q])} steps")
        out[name] = {k: res.scores["test_" + k].copy() for k in METRICS}
    return out


def simple_inducing(j, rng=None, m=5, d=1):
    """Replicate j's starting inducing inputs as SF:200 draws them, torch.randint(-3, 3, (m, d)):
    integers uniform in {-3, ..., 2}, as float64.  The draws are numpy's from ``rng`` (a Generator
    or a seed; default seed 100·j + 1), NOT torch's — the same caveat as simple_data.  Duplicates
    are expected and legal: the 1e-3 jitter keeps K(Z,Z) + 1e-3·I positive definite."""
    rng = np.random.default_rng(100 * j + 1 if rng is None else rng)
    return rng.integers(-3, 3, size=(m, d)).astype(np.float64)


def run_simple_fitc(TT=100, methods=None, datasets=None, Z0=None, itr=None, stale_noise=True,
                    ctx=None):
    """SF's replicate loop → {method: {metric: array(TT), "Z": array(TT, m, d)}}: every method's
    TT FITC fits (its SGD loop over θ and the inducing inputs, the test predictive and the score
    bundle) are ONE fitc_train_batch call, one workgroup per replicate.  ``datasets`` as
    run_simple; ``Z0``: (TT, m, d) starting inducing inputs (default simple_inducing(j), j < TT),
    the same for every method; ``itr`` overrides the methods' step counts; stale_noise as
    run_method.  A replicate whose factorisation fails raises NotPositiveDefinite."""
    methods = SF_METHODS if methods is None else methods
    if datasets is None:
        datasets = [simple_data(j) for j in range(TT)]
    datasets = list(datasets)
    if len(datasets) != TT:
        raise ValueError(f"{len(datasets)} datasets for TT = {TT} replicates")
    X = np.stack([_as2d(dd["train_x"]) for dd in datasets])
    y = np.stack([np.asarray(dd["train_y"], np.float64).ravel() for dd in datasets])
    Xt = np.stack([_as2d(dd["test_x"]) for dd in datasets])
    yt = np.stack([np.asarray(dd["test_y"], np.float64).ravel() for dd in datasets])
    d = X.shape[2]
    if Z0 is None:
        Z0 = np.stack([simple_inducing(j, d=d) for j in range(TT)])
    Z0 = np.asarray(Z0, np.float64)
    if Z0.shape[0] != TT:
        raise ValueError(f"Z0 holds {Z0.shape[0]} inducing sets for TT = {TT} replicates")
    out = {}
    for name, meth in methods.items():
        th0 = initial_theta(meth, d, None)
        res = fitc_train_batch(X, y, Z0, th0, meth.objective, lr=meth.lr, lr_z=meth.lr_z,
                               itr=meth.itr if itr is None else int(itr), Xt=Xt, yt=yt,
                               stale_noise=stale_noise, ctx=ctx)
        bad = np.flatnonzero(res.info)
        if bad.size:
            q = int(bad[0])
            raise NotPositiveDefinite(int(res.info[q]), f"run_simple_fitc: method {name!r}, "
                                      f"replicate {q}: info = {int(res.info[q])} (k: the leading "
                                      f"minor of order k of K(Z,Z) + 1e-3 I, m + k: of B) after "
                                      f"{int(res.steps_done[q])} steps")
        out[name] = {k: res.scores["test_" + k].copy() for k in METRICS}
        out[name]["Z"] = res.Z.copy()
    return out


BATCH_OBJECTIVES = BATCH_OBJS  # what the batched pointwise kernels can fit


def _run_batch(who, sheets, TT, methods, accepts, why, route, train, what, m=None, es=None,
               zero_for=(), itr=None, seed=None, reseed=True, stale_noise=True, ctx=None,
               post=None):
    """The replicate runner behind the run_*_batch functions (``who``: the caller's name in its
    messages).  Every method's objective must be in ``accepts``, else ValueError "<why>; use
    <route(objective)> for it".  Data replicates and starting points are drawn as run draws them:
    replicate-major, then method by method initial_theta, then Z0 (m given: FITC, U(0,1) or N(0,1)
    by the method's z_init) or one es_draws set per step (es = (nfold, num_sim)).  Then one call a
    method, ``train(X, y, th0, Z0 or draws or None, method, lr=, itr=, Xt=, yt=, stale_noise=,
    ctx=)``.  A failed replicate of a method whose objective is in ``zero_for`` gets zero metrics
    (run_method's rule); of any other raises NotPositiveDefinite "...: <what> after k steps".
    Returns {method: {metric: array(TT), "theta"[, "Z" with m][, "failed" with zero_for]}}.
    ``post`` (run_full_validated_batch, run_fitc_validated_batch): ``train`` also gets Xv= / yv=, the replicates' validation
    rows, and post(entry, res, method, X, y, Xt, yt) adds to a method's entry."""
    from .gp import es_draws
    for name, meth in methods.items():
        if meth.objective not in accepts:
            raise ValueError(f"{who}: method {name!r} has objective {meth.objective!r}, {why}; use "
                             f"{route(meth.objective)} for it")
    if int(TT) != TT or TT < 1:
        raise ValueError(f"TT must be a positive integer, got {TT!r}")
    if m is not None and (int(m) != m or m < 1):
        raise ValueError(f"m must be a positive integer, got {m!r}")
    TT = int(TT)
    rng = np.random.default_rng(seed)
    rs = None if reseed else random.Random()
    n_pool = sheets["trainx"].shape[0]
    steps = {name: meth.itr if itr is None else int(itr) for name, meth in methods.items()}
    data, th0, start = [], {name: [] for name in methods}, {name: [] for name in methods}
    for j in range(TT):
        dd = replicate(sheets, j if reseed else None, n_pool=n_pool, rs=rs)
        data.append(dd)
        n, d = dd["train_x"].shape
        for name, meth in methods.items():
            k, ell, noise = initial_theta(meth, d, rng)
            th0[name].append(np.concatenate([[k], np.ravel(ell), [noise]]))
            if m is not None:
                start[name].append(rng.random((int(m), d)) if meth.z_init == "rand"
                                   else rng.standard_normal((int(m), d)))
            elif es is not None:
                start[name].append(np.stack([es_draws(n, *es, rng)
                                             for _ in range(max(steps[name], 1))]))
    X = np.stack([dd["train_x"] for dd in data])
    y = np.stack([dd["train_y"] for dd in data])
    Xt = np.stack([dd["test_x"] for dd in data])
    yt = np.stack([dd["test_y"] for dd in data])
    out = {}
    va = {} if post is None else {"Xv": np.stack([dd["va_x"] for dd in data]),
                                  "yv": np.stack([dd["va_y"] for dd in data])}
    for name, meth in methods.items():
        res = train(X, y, np.stack(th0[name]), np.stack(start[name]) if start[name] else None,
                    meth, lr=meth.lr, itr=steps[name], Xt=Xt, yt=yt, stale_noise=stale_noise,
                    ctx=ctx, **va)
        failed = np.asarray(res.info) != 0
        if failed.any() and meth.objective not in zero_for:
            q = int(np.flatnonzero(failed)[0])
            raise NotPositiveDefinite(int(res.info[q]), f"{who}: method {name!r}, replicate {q}: "
                                      + what.format(info=int(res.info[q]))
                                      + f" after {int(res.steps_done[q])} steps")
        out[name] = {k: np.where(failed, 0.0, res.scores["test_" + k]) for k in METRICS}
        if m is not None:
            out[name]["Z"] = res.Z.copy()
        out[name]["theta"] = res.theta.copy()
        if zero_for:
            out[name]["failed"] = failed
        if post is not None:
            post(out[name], res, meth, X, y, Xt, yt)
    return out


_FITC_INFO = "info = {info} (k: the leading minor of order k of K(Z,Z) + 1e-3 I, m + k: of B"


def run_fitc_batch(sheets, TT=10, methods=None, m=20, itr=None, seed=None, reseed=True,
                   stale_noise=True, ctx=None):
    """K20's replicate loop for its batchable methods → {method: {metric: array(TT), "Z":
    array(TT, m, d), "theta": array(TT, 2 + n_ell)}}: every method's TT FITC fits (n = 500, m
    inducing inputs trained too, the test predictive and the score bundle) are ONE
    fitc_train_tall call, one workgroup per replicate.  ``methods`` defaults to the
    crps / nlml / logs entries of K20_METHODS; a method whose objective is dss, kc or es has no
    batched path and raises ValueError (use run(kind="fitc")).  Data replicates and starting
    points are drawn in run's order — replicate-major, then method, initial_theta first and Z0
    second as run_method — so with the same ``seed``, ``reseed=True`` and the same method subset
    run(kind="fitc", methods=subset) and this fit the same problems.  ``itr`` overrides the
    methods' step counts; stale_noise as run_method.  A replicate whose factorisation fails
    raises NotPositiveDefinite."""
    if methods is None:
        methods = {k: K20_METHODS[k] for k in ("crps", "nlml", "logs")}
    return _run_batch(
        "run_fitc_batch", sheets, TT, methods, BATCH_OBJECTIVES,
        f"which has no batched path (only {BATCH_OBJECTIVES})", lambda o: "run(kind=\"fitc\")",
        lambda X, y, th0, Z0, meth, **kw: fitc_train_tall(X, y, Z0, th0, meth.objective,
                                                          lr_z=meth.lr_z, **kw),
        _FITC_INFO + ")", m=m, itr=itr, seed=seed, reseed=reseed, stale_noise=stale_noise, ctx=ctx)


def run_full_batch(sheets, TT=30, methods=None, itr=None, seed=None, reseed=True,
                   stale_noise=True, ctx=None):
    """KF's replicate loop for its batchable methods → {method: {metric: array(TT), "theta":
    array(TT, 2 + n_ell)}}: every method's TT full-GP fits (n = 500, the test predictive and the
    score bundle) are ONE train_tall call, one workgroup per replicate.  ``methods``
    defaults to the crps / nlml / logs entries of KF_METHODS; a method whose objective is dss or es
    (block-LOO) raises ValueError here (dss and kc: run_full_blockloo_batch; es: run_full_es_batch).
    Data replicates
    and starting points are drawn in run's order — replicate-major, then method, initial_theta per
    method — so with the same ``seed``, ``reseed=True`` and the same method subset
    run(kind="full", methods=subset) and this fit the same problems.  ``itr`` overrides the
    methods' step counts; stale_noise as run_method.  A replicate whose factorisation fails
    raises NotPositiveDefinite."""
    if methods is None:
        methods = {k: KF_METHODS[k] for k in ("crps", "nlml", "logs")}
    return _run_batch(
        "run_full_batch", sheets, TT, methods, BATCH_OBJECTIVES,
        f"which has no batched path (only {BATCH_OBJECTIVES})", lambda o: "run(kind=\"full\")",
        lambda X, y, th0, _, meth, **kw: train_tall(X, y, th0, meth.objective, **kw),
        "the leading minor of order {info} is not positive definite", itr=itr, seed=seed,
        reseed=reseed, stale_noise=stale_noise, ctx=ctx)


def run_full_blockloo_batch(sheets, TT=30, methods=None, itr=None, seed=None, reseed=True,
                            stale_noise=True, ctx=None, nfold=4):
    """run_full_batch for KF's block-LOO fits → the same {method: {metric: array(TT), "theta":
    array(TT, 2 + n_ell)}}: every method's TT full-GP fits on the nfold-fold block-LOO DSS (or KC)
    objective, the test predictive and the score bundle are ONE blockloo_train_tall call, one
    workgroup per replicate.  ``methods`` defaults to KF_METHODS' dss entry (KF:487-601,
    150 steps at lr 1e-3); a method whose objective is es raises ValueError (its batch route is
    run_full_es_batch), one whose objective is pointwise raises too (use run_full_batch).  Data replicates and starting
    points are drawn in run's order — replicate-major, then method, initial_theta per method — so
    with the same ``seed``, ``reseed=True`` and the same method subset run(kind="full",
    methods=subset) and this fit the same problems.  ``itr`` overrides the methods' step counts;
    stale_noise as run_method.  A replicate whose factorisation fails raises
    NotPositiveDefinite."""
    if methods is None:
        methods = {"dss": KF_METHODS["dss"]}
    return _run_batch(
        "run_full_blockloo_batch", sheets, TT, methods, BLOCK_BATCH_OBJS,
        f"not one of {BLOCK_BATCH_OBJS}",
        lambda o: "run(kind=\"full\")" if o == "es" else "run_full_batch",
        lambda X, y, th0, _, meth, **kw: blockloo_train_tall(X, y, th0, meth.objective,
                                                             nfold=nfold, **kw),
        "info {info} (the failing leading minor, or n + the fold block's row)", itr=itr, seed=seed,
        reseed=reseed, stale_noise=stale_noise, ctx=ctx)


def run_full_validated_batch(sheets, TT=30, methods=None, itr=None, seed=None, reseed=True,
                             stale_noise=True, va_every=1, select=None, ctx=None, nfold=4):
    """run_full_batch / run_full_blockloo_batch with every replicate's validation split (va_x /
    va_y, the 300 rows KF:203-209 holds out) scored inside the fits, step by step: the
    series the scripts carry commented out and chose their step counts by.  Pointwise methods go
    through ONE train_tall_validated call each, dss / kc through ONE blockloo_train_tall_validated
    call; ``methods`` defaults to KF_METHODS' crps, nlml, logs and dss entries.  A method whose
    objective is es raises ValueError: its route is run_full_es_batch, which has no validation.
    Data replicates and starting points are drawn in run's order, so with the same ``seed`` this
    fits the problems run_full_batch / run_full_blockloo_batch fit, and the standard entries —
    {metric: array(TT), "theta"} — are theirs.  Added per method: "va_scores" {name: array(TT,
    nva)} over SCORE_NAMES, "va_steps" (nva,), and with ``select`` (a metric of
    batch.SELECT_METRICS) "best_step" array(TT) and "selected" {metric: array(TT)}: the test
    metrics at each replicate's theta_best, from one more train_tall(itr=0, theta0=theta_best)
    call for the batch; a replicate whose best row is the final one keeps the first call's
    metrics (under stale_noise that row's noise is the stale one).  ``itr``, stale_noise and
    failures as run_full_batch."""
    from .batch import (_select_metric, _va_every, blockloo_train_tall_validated,
                        train_tall_validated)
    if methods is None:
        methods = {k: KF_METHODS[k] for k in ("crps", "nlml", "logs", "dss")}
    va_every, select = _va_every(va_every), _select_metric(select)

    def train(X, y, th0, _, meth, **kw):
        if meth.objective in BLOCK_BATCH_OBJS:
            return blockloo_train_tall_validated(X, y, th0, objective=meth.objective, nfold=nfold,
                                                 va_every=va_every, select=select, **kw)
        return train_tall_validated(X, y, th0, objective=meth.objective, va_every=va_every,
                                    select=select, **kw)

    def post(entry, res, meth, X, y, Xt, yt):
        entry["va_scores"] = {k: v.copy() for k, v in res.va_scores.items()}
        entry["va_steps"] = res.va_steps.copy()
        if select is None:
            return
        entry["best_step"] = res.best_step.copy()
        sel = {k: np.array(entry[k], dtype=np.float64) for k in METRICS}
        redo = np.flatnonzero(res.best_step != res.va_steps[-1])  # not the final row
        if redo.size:
            r2 = train_tall(X[redo], y[redo], res.theta_best[redo], itr=0, Xt=Xt[redo],
                            yt=yt[redo], ctx=ctx)
            for k in METRICS:
                sel[k][redo] = r2.scores["test_" + k]
        entry["selected"] = sel

    return _run_batch(
        "run_full_validated_batch", sheets, TT, methods, tuple(BATCH_OBJS) + tuple(BLOCK_BATCH_OBJS),
        "which has no validated batch path (the energy-score route has no validation)",
        lambda o: "run_full_es_batch" if o == "es" else "run(kind=\"full\")", train,
        "info {info} (the failing leading minor, or n + the fold block's row)", itr=itr, seed=seed,
        reseed=reseed, stale_noise=stale_noise, ctx=ctx, post=post)


def run_full_es_batch(sheets, TT=30, methods=None, itr=None, seed=None, reseed=True,
                      stale_noise=True, num_sim=300, ctx=None, nfold=4):
    """run_full_batch for KF's energy-score fit → {method: {metric: array(TT), "theta": array(TT,
    2 + n_ell), "failed": array(TT, bool)}}: every method's TT full-GP fits on the nfold-fold
    block-LOO energy score with ``num_sim`` draws a fold redrawn every step, the test predictive and
    the score bundle are ONE es_train_tall call.  ``methods`` defaults to KF_METHODS' es
    entry (KF:607-732, 25 steps at lr 0.1); any other objective raises ValueError (use
    run_full_batch or run_full_blockloo_batch).  Data replicates, starting points and draws are
    taken from the generator in run's order — replicate-major, then method: initial_theta, then
    one es_draws set per step — so with the same ``seed``, ``reseed=True`` and the same es-only
    method subset run(kind="full", methods=subset) and this fit the same problems with the same
    draws.  ``itr`` overrides the methods' step counts; stale_noise as run_method.  A replicate
    whose factorisation fails gets zero metrics as in run_method (KF:726-732)."""
    if methods is None:
        methods = {"es": KF_METHODS["es"]}
    return _run_batch(
        "run_full_es_batch", sheets, TT, methods, ("es",), "not 'es'",
        lambda o: "run_full_blockloo_batch" if o in BLOCK_BATCH_OBJS else "run_full_batch",
        lambda X, y, th0, draws, meth, **kw: es_train_tall(
            X, y, th0, nfold=nfold, num_sim=num_sim, draws=draws, draw_sets=draws.shape[1], **kw),
        "", es=(nfold, num_sim), zero_for=("es",), itr=itr, seed=seed, reseed=reseed,
        stale_noise=stale_noise, ctx=ctx)


def run_fitc_blockloo_batch(sheets, TT=10, methods=None, m=20, itr=None, seed=None, reseed=True,
                            stale_noise=True, ctx=None, nfold=4):
    """run_fitc_batch for K20's block-LOO fits → {method: {metric: array(TT), "Z": array(TT, m, d),
    "theta": array(TT, 2 + n_ell), "failed": array(TT, bool)}}: every method's TT FITC fits on the
    nfold-fold block-LOO DSS or KC objective (n = 500, m inducing inputs trained too), the test
    predictive and the score bundle are ONE fitc_blockloo_train_tall call, one workgroup per
    replicate.  ``methods`` defaults to the dss and kc entries of K20_METHODS
    (K20:523-593, K20:655-726: 3000 steps each); a method whose objective is pointwise raises
    ValueError (use run_fitc_batch), one whose objective is es raises too (use run(kind="fitc")).
    Data replicates and starting points are drawn in run's order — replicate-major, then method,
    initial_theta first and Z0 second, U(0,1) or N(0,1) by the method's z_init — so with the same
    ``seed``, ``reseed=True`` and the same method subset run(kind="fitc", methods=subset) and this
    fit the same problems.  ``itr`` overrides the methods' step counts; stale_noise as run_method.
    A kc replicate whose factorisation fails gets zero metrics as in run_method (K20:784-790); a
    dss replicate that fails raises NotPositiveDefinite."""
    if methods is None:
        methods = {k: K20_METHODS[k] for k in ("dss", "kc")}
    return _run_batch(
        "run_fitc_blockloo_batch", sheets, TT, methods, BLOCK_BATCH_OBJS,
        f"not one of {BLOCK_BATCH_OBJS}",
        lambda o: "run(kind=\"fitc\")" if o == "es" else "run_fitc_batch",
        lambda X, y, th0, Z0, meth, **kw: fitc_blockloo_train_tall(
            X, y, Z0, th0, meth.objective, nfold=nfold, lr_z=meth.lr_z, **kw),
        _FITC_INFO + ", (2 + f) m + k: of fold f's B)", m=m, zero_for=("kc",), itr=itr, seed=seed,
        reseed=reseed, stale_noise=stale_noise, ctx=ctx)


def run_fitc_validated_batch(sheets, TT=10, methods=None, m=20, itr=None, seed=None, reseed=True,
                             stale_noise=True, va_every=1, select=None, ctx=None, nfold=4):
    """run_fitc_batch / run_fitc_blockloo_batch with every replicate's validation split (va_x /
    va_y) scored inside the fits, step by step: the series K20 carries commented out
    (K20:258-264, 469-476, 737-743).  Pointwise methods go through ONE fitc_train_tall_validated
    call each, dss / kc through ONE fitc_blockloo_train_tall_validated call; ``methods`` defaults to
    K20_METHODS' crps, nlml, logs, dss and kc entries.  A method whose objective is es raises
    ValueError: FITC has no energy-score batch path.  Data replicates, θ0 and Z0 are drawn in run's
    order, so with the same ``seed`` this fits the problems run_fitc_batch /
    run_fitc_blockloo_batch fit, and the standard entries — {metric: array(TT), "Z", "theta"} and,
    for dss / kc, "failed" — are theirs: a failed kc replicate gets zero metrics, a failed dss or
    pointwise replicate raises NotPositiveDefinite.  Added per method: "va_scores" {name: array(TT,
    nva)} over SCORE_NAMES, "va_steps" (nva,), and with ``select`` (a metric of
    batch.SELECT_METRICS) "best_step" array(TT) and "selected" {metric: array(TT)}: the test metrics
    at each replicate's (theta_best, Z_best), from one more fitc_train_tall(itr=0) call for the
    replicates whose best row is not the final one; the others (and a replicate with no finite row)
    keep the first call's metrics."""
    from .batch import (_select_metric, _va_every, fitc_blockloo_train_tall_validated,
                        fitc_train_tall_validated)
    if methods is None:
        methods = {k: K20_METHODS[k] for k in ("crps", "nlml", "logs", "dss", "kc")}
    va_every, select = _va_every(va_every), _select_metric(select)

    def train(X, y, th0, Z0, meth, **kw):
        if meth.objective in BLOCK_BATCH_OBJS:
            return fitc_blockloo_train_tall_validated(
                X, y, Z0, th0, objective=meth.objective, nfold=nfold, lr_z=meth.lr_z,
                va_every=va_every, select=select, **kw)
        return fitc_train_tall_validated(X, y, Z0, th0, objective=meth.objective, lr_z=meth.lr_z,
                                         va_every=va_every, select=select, **kw)

    def post(entry, res, meth, X, y, Xt, yt):
        if meth.objective not in BLOCK_BATCH_OBJS:
            entry.pop("failed", None)  # run_fitc_batch's entries carry none
        entry["va_scores"] = {k: v.copy() for k, v in res.va_scores.items()}
        entry["va_steps"] = res.va_steps.copy()
        if select is None:
            return
        entry["best_step"] = res.best_step.copy()
        sel = {k: np.array(entry[k], dtype=np.float64) for k in METRICS}
        redo = np.flatnonzero((res.best_step >= 0) & (res.best_step != res.va_steps[-1]))
        if redo.size:
            r2 = fitc_train_tall(X[redo], y[redo], res.Z_best[redo], res.theta_best[redo], itr=0,
                                 Xt=Xt[redo], yt=yt[redo], ctx=ctx)
            for k in METRICS:
                sel[k][redo] = r2.scores["test_" + k]
        entry["selected"] = sel

    return _run_batch(
        "run_fitc_validated_batch", sheets, TT, methods,
        tuple(BATCH_OBJS) + tuple(BLOCK_BATCH_OBJS),
        "which has no validated batch path (FITC has no energy-score batch path)",
        lambda o: "run(kind=\"fitc\")", train,
        _FITC_INFO + ", (2 + f) m + k: of fold f's B)", m=m, zero_for=("kc",), itr=itr, seed=seed,
        reseed=reseed, stale_noise=stale_noise, ctx=ctx, post=post)
