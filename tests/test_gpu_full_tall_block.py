"""Batches of full GPs of up to 512 rows on the block-LOO DSS / KC objectives
(gps_full_blockloo_grad_tall / gps_full_blockloo_train_tall) against the reference's
autograd goldens, the oracle at the fold and tile edges, the pointwise tall kernel at degenerate
folds, the resident path (GP.block_loo, GP.train, GP.fit + GP.predict), and their own invariants:
the launch split, the batch size and a problem's position change no bit, a failed problem touches
no other, the rest of the context is left alone.  Follows tests/test_gpu_full_tall.py and reuses
its helpers.  Runs on the GPU box.

Tolerances: 1e-9 (close / nrel) on values and gradients, 1e-8 on the predictive and its scores, as
the issue sets them; at the edges max(1e-9, 30 × the case's conditioning floor), the floor being
the oracle on X perturbed by 1e-15 relative, with the cap 30 × floor <= 5e-9 asserted on the oracle
alone.  The paths sum in different orders, so they are compared at those tolerances, never bitwise.
The info code n + k (a fold block's pivot) cannot be reached with honest inputs and is not tested."""
import functools

import numpy as np
import pytest

import gp_oracle as O
from conftest import load_golden, nrel, theta_of
from test_gpu_batch import (OBJ5, SCORES, TOL, close, edge_problems, result_fields, row_of,
                            same_bits, tup_of)
from test_gpu_full_tall import TOL8, problems

pytestmark = pytest.mark.gpu

BOBJS = ("dss", "kc")
LR = {"dss": 1e-3, "kc": 0.1}  # the scripts' steps (KF:487-601, K20:655-720)


@pytest.fixture(scope="module")
def gp(gpu_ctx):
    import gpscore
    return gpscore.GP(ctx=gpu_ctx)


def oracle(X, y, row, obj, kind="ARD", nfold=4):
    return O.fast_full_blockloo(X, y, *tup_of(row), obj, kind=kind, nfold=nfold, want_grad=True)


# ------------------------------------------------------------ 1. the reference's autograd
@pytest.mark.parametrize("name", ["block_full_n500", "block_full_n64"])
def test_block_vs_autograd_golden(gpu_ctx, name):
    import gpscore
    g = load_golden(name)
    th, kern = theta_of(g)
    assert kern != "rbf"
    row = row_of(th)
    X, y = np.stack([g["X"]] * 3), np.stack([g["y"]] * 3)
    rows = np.stack([row - 0.05, row, row + 0.05])
    for obj in BOBJS:
        vals, grads, folds, objs, info = gpscore.blockloo_value_and_grad_tall(
            X, y, rows, obj, nfold=4, ctx=gpu_ctx)
        assert not info.any(), info
        assert close(vals[1], float(g["value_" + obj])), (obj, vals[1], float(g["value_" + obj]))
        assert nrel(grads[1], g["grad_" + obj]) <= TOL, (obj, grads[1], g["grad_" + obj])
        assert folds.shape == (3, 4)
        assert np.all(np.abs(folds.sum(1) - vals) <= 1e-12 * np.abs(vals)), (obj, folds, vals)
        for q in range(3):
            if q != 1:  # the neighbours against the oracle
                ov, og = oracle(X[q], y[q], rows[q], obj)
                assert close(vals[q], ov), (obj, q, vals[q], ov)
                assert nrel(grads[q], og) <= TOL, (obj, q, grads[q], og)
            fit = O.fast_full_fit(X[q], y[q], *tup_of(rows[q]), "ARD")
            for k in OBJ5:
                assert close(objs[k][q], fit[k]), (obj, q, k, objs[k][q], fit[k])


# ------------------------------------------------- 2. the oracle at the fold and tile edges
EDGE_N = (4, 5, 63, 64, 65, 127, 129, 130, 255, 256, 257, 260, 385, 500, 509, 512)
EDGE_CASES = [(n, d, vec, rbf) for n in EDGE_N
              for d, vec, rbf in ((1, False, False), (1, False, True), (8, True, False),
                                  (16, True, False))]
NQ = 3


def nfolds_of(d):
    return (4, 2, 3) if d == 8 else (4,)


@functools.lru_cache(maxsize=None)
def edge_oracle(n, d, vec, rbf, obj, nfold):
    """Per problem (value, grad, tol): the oracle and the case's tolerance from its conditioning
    floor (the oracle on X perturbed by 1e-15 relative, same metrics)."""
    X, y, th = (a[:NQ] for a in edge_problems(n, d, vec))
    kind = "rbf" if rbf else "ARD"
    out = []
    for q in range(NQ):
        ov, og = oracle(X[q], y[q], th[q], obj, kind, nfold)
        r = np.random.default_rng(1)
        Xp = X[q] * (1 + 1e-15 * r.standard_normal(X[q].shape))
        pv, pg = oracle(Xp, y[q], th[q], obj, kind, nfold)
        floor = max(abs(pv - ov) / max(1.0, abs(ov)), nrel(pg, og))
        assert 30 * floor <= 5e-9, (n, d, vec, rbf, obj, nfold, q, floor)  # the hard cap
        out.append((ov, og, max(TOL, 30 * floor)))
    return out


@pytest.mark.parametrize("n,d,vec,rbf", EDGE_CASES)
def test_block_vs_oracle_edges(gpu_ctx, n, d, vec, rbf):
    import gpscore
    X, y, th = (a[:NQ] for a in edge_problems(n, d, vec))
    worst = 0.0
    for nfold in nfolds_of(d):
        for obj in BOBJS:
            refs = edge_oracle(n, d, vec, rbf, obj, nfold)  # asserts the cap first
            vals, grads, folds, objs, info = gpscore.blockloo_value_and_grad_tall(
                X, y, th, obj, nfold=nfold, rbf=rbf, ctx=gpu_ctx)
            assert not info.any(), (obj, nfold, info)
            for q, (ov, og, tol) in enumerate(refs):
                ev, eg = abs(vals[q] - ov) / max(1.0, abs(ov)), nrel(grads[q], og)
                worst = max(worst, ev, eg)
                assert ev <= tol, (obj, nfold, q, "value", vals[q], ov, tol)
                assert eg <= tol, (obj, nfold, q, "grad", grads[q], og, tol)
    print("block edge", n, d, vec, rbf, "worst error %.3g" % worst)


# ------------------------------------- 3. degenerate folds are the pointwise objectives
@pytest.mark.parametrize("n", [7, 32])
@pytest.mark.parametrize("d", [1, 8])
def test_one_row_folds_equal_the_pointwise_objectives(gpu_ctx, n, d):
    """nfold = n: every fold is one row, DSS is n × LOO-LogS and KC n × LOO-CRPS, values and
    gradients, against the pointwise tall kernel without the oracle in between."""
    import gpscore
    X, y, th = (a[:NQ] for a in edge_problems(n, d, d > 1))
    for obj, point in (("dss", "loo_logs"), ("kc", "loo_crps")):
        vals, grads, folds, objs, info = gpscore.blockloo_value_and_grad_tall(
            X, y, th, obj, nfold=n, ctx=gpu_ctx)
        pv, pg, po, pi = gpscore.value_and_grad_tall(X, y, th, point, ctx=gpu_ctx)
        assert not info.any() and not pi.any()
        for q in range(NQ):
            assert close(vals[q], n * pv[q]), (obj, q, vals[q], n * pv[q])
            assert nrel(grads[q], n * pg[q]) <= TOL, (obj, q, grads[q], n * pg[q])


# ----------------------------------------------------------------- 4. the resident path
@pytest.mark.parametrize("n", [129, 500])
def test_block_vs_resident_path(gp, gpu_ctx, n):
    import gpscore
    X, y, _, _, th = problems(2, n)
    for obj in BOBJS:
        vals, grads, folds, objs, info = gpscore.blockloo_value_and_grad_tall(
            X, y, th, obj, nfold=4, ctx=gpu_ctx)
        assert not info.any()
        for q in range(2):
            gp.set_data(X[q], y[q], kind="full")
            v1, g1, f1 = gp.block_loo(tup_of(th[q]), obj, 4, grad=True)
            assert close(vals[q], v1), (obj, q, vals[q], v1)
            assert nrel(grads[q], g1) <= TOL, (obj, q, grads[q], g1)
            assert nrel(folds[q], f1) <= TOL, (obj, q, folds[q], f1)


# ----------------------------------------------------------------------------- 5. training
@pytest.mark.parametrize("obj", BOBJS)
def test_block_train_matches_oracle_and_gp_train(gp, gpu_ctx, obj):
    """Five SGD steps at the scripts' lr from two starts at n = 200, d = 8, against the oracle loop
    and against GP.train."""
    import gpscore
    lr = LR[obj]
    X, y, _, _, th = problems(2, 200)
    th[1, 1:-1] += 0.3
    res = gpscore.blockloo_train_tall(X, y, th, obj, nfold=4, lr=lr, itr=5, ctx=gpu_ctx)
    assert not res.info.any() and list(res.steps_done) == [5, 5]
    for q in range(2):
        t = th[q].copy()
        for i in range(5):
            v, gr = oracle(X[q], y[q], t, obj)
            assert close(res.series["objective"][q, i], v), (q, i, res.series["objective"][q, i], v)
            t = t - lr * gr
            assert nrel(res.series["theta"][q, i], t) <= TOL, (q, i)
        assert nrel(res.theta[q], t) <= TOL
        assert same_bits(res.theta[q], res.series["theta"][q, -1])
        theta, series = gp.train(tup_of(th[q]), obj, lr=lr, itr=5, X=X[q], y=y[q])
        for i in range(5):
            assert close(res.series["objective"][q, i], series["objective"][i]), (q, i)
            assert nrel(res.series["theta"][q, i], series["theta"][i]) <= TOL, (q, i)
        assert nrel(res.theta[q], row_of(theta)) <= TOL


# ------------------------------------------------------------ 6. the launch split is invisible
@pytest.mark.parametrize("obj", BOBJS)
def test_block_launch_split_changes_no_bit(gpu_ctx, obj):
    """At n = 130 (three blocks: 37 steps a launch) itr = a + b beyond one launch equals, bitwise
    in every field, itr = a continued by itr = b: the split points 37 | 13, 30 | 20 and 10 | 40
    differ."""
    import gpscore
    X, y, Xt, yt, th = problems(3, 130, d=3, nt=9)
    kw = dict(nfold=4, lr=LR[obj], Xt=Xt, yt=yt, ctx=gpu_ctx)
    whole = gpscore.blockloo_train_tall(X, y, th, obj, itr=50, **kw)
    assert not whole.info.any() and list(whole.steps_done) == [50] * 3
    for a, b in ((30, 20), (10, 40)):
        first = gpscore.blockloo_train_tall(X, y, th, obj, itr=a, **kw)
        second = gpscore.blockloo_train_tall(X, y, first.theta, obj, itr=b, **kw)
        assert same_bits(whole.theta, second.theta)
        for k in ("objective", "theta"):
            joined = np.concatenate([first.series[k], second.series[k]], axis=1)
            assert same_bits(whole.series[k], joined), (a, k)
        fw, fs = result_fields(whole), result_fields(second)
        for k in fw:
            if k not in ("values", "thetas", "steps_done"):
                assert same_bits(fw[k], fs[k]), (a, k)
    assert not same_bits(whole.series["theta"][:, 0], whole.series["theta"][:, -1])  # it did move


# ----------------------------------------------------------------------------- 7. final pass
@pytest.mark.parametrize("stale", [True, False])
@pytest.mark.parametrize("nt", [1, 65, 300])
def test_block_final_pass_vs_fit_predict(gp, gpu_ctx, nt, stale):
    """After two steps the predictive's σ² is, with stale_noise, the one the second step's forward
    used (θ after step 1), without it the final θ's; GP.fit + GP.predict at that θ."""
    import gpscore
    X, y, Xt, yt, th = problems(2, 200, nt=nt)
    res = gpscore.blockloo_train_tall(X, y, th, "kc", nfold=4, lr=0.1, itr=2, Xt=Xt, yt=yt,
                                      stale_noise=stale, ctx=gpu_ctx)
    assert not res.info.any() and res.mu.shape == (2, nt)
    for q in range(2):
        k, ell, noise = tup_of(res.theta[q])
        if stale:
            noise = float(res.series["theta"][q, 0, -1])
        assert noise != res.series["theta"][q, 1 if stale else 0, -1]
        fit = gp.fit(X[q], y[q], (k, ell, noise))
        mu, var, sc1 = gp.predict(Xt[q], yt[q], with_scores=True)
        assert nrel(res.mu[q], mu) <= TOL8 and nrel(res.var[q], var) <= TOL8
        for s in SCORES:
            assert close(res.scores[s][q], sc1[s], TOL8), (s, q, res.scores[s][q], sc1[s])
        for o in OBJ5:
            assert close(res.objectives[o][q], fit[o]), (q, o)


# ---------------------------------------------------------------------- 8. failure isolation
def test_block_failed_problems_touch_no_other(gpu_ctx):
    """Problem 1: a NaN feature in row 0 (info = 1); problem 2: one in row 70, a pivot of the
    second diagonal block (info = 71); problem 3: a NaN in θ (info = 1).  All end with NaN outputs
    and no step done; the call succeeds; problems 0 and 4 keep every bit."""
    import gpscore
    X, y, Xt, yt, th = problems(5, 130, d=3, nt=9)
    X[1, 0, 1] = np.nan
    X[2, 70, 0] = np.nan
    th[3, 1] = np.nan
    good, bad = [0, 4], [1, 2, 3]
    for obj in BOBJS:
        kw = dict(nfold=4, lr=LR[obj], itr=3, ctx=gpu_ctx)
        res = gpscore.blockloo_train_tall(X, y, th, obj, Xt=Xt, yt=yt, **kw)
        ref = gpscore.blockloo_train_tall(X[good], y[good], th[good], obj, Xt=Xt[good],
                                          yt=yt[good], **kw)
        assert list(res.info) == [0, 1, 71, 1, 0], res.info
        assert list(res.steps_done) == [3, 0, 0, 0, 3]
        fr, fref = result_fields(res), result_fields(ref)
        for k, v in fr.items():
            assert same_bits(v[good], fref[k]), k
            if k not in ("info", "steps_done", "theta"):
                assert np.isnan(v[bad]).all(), k
        assert not np.isnan(fref["mu"]).any() and not np.isnan(fref["thetas"]).any()
        assert same_bits(res.theta[1], th[1]) and same_bits(res.theta[2], th[2])
        vals, grads, folds, objs, info = gpscore.blockloo_value_and_grad_tall(
            X, y, th, obj, nfold=4, ctx=gpu_ctx)
        v0, g0, f0, o0, i0 = gpscore.blockloo_value_and_grad_tall(
            X[good], y[good], th[good], obj, nfold=4, ctx=gpu_ctx)
        assert list(info) == [0, 1, 71, 1, 0] and not i0.any()
        assert same_bits(vals[good], v0) and same_bits(grads[good], g0)
        assert same_bits(folds[good], f0)
        assert np.isnan(vals[bad]).all() and np.isnan(grads[bad]).all()
        assert np.isnan(folds[bad]).all()
        for k in OBJ5:
            assert same_bits(objs[k][good], o0[k]) and np.isnan(objs[k][bad]).all(), k


def test_block_failure_in_a_later_step(gpu_ctx):
    """A step of 1e6 throws θ far outside the representable kernels after the first update, and a
    forward within the next two steps meets a pivot of A that is not > 0 (info in 1..n).  The
    problem stops there, as in the pointwise kernel: steps_done counts the completed steps,
    theta_out is the θ the failing forward was at, the rest of its series and its final outputs
    are NaN."""
    import gpscore
    n = 130
    X, y, Xt, yt, th = problems(2, n, d=3, nt=9)
    res = gpscore.blockloo_train_tall(X, y, th, "dss", nfold=4, lr=1e6, itr=5, Xt=Xt, yt=yt,
                                      ctx=gpu_ctx)
    assert res.info.all() and (res.info <= n).all(), res.info
    for q in range(2):
        done = int(res.steps_done[q])
        assert 1 <= done <= 3, done  # the first forward is at a sane θ
        assert same_bits(res.theta[q], res.series["theta"][q, done - 1])
        assert not np.isnan(res.series["objective"][q, 0])
        assert np.isnan(res.series["objective"][q, done:]).all()
        assert np.isnan(res.series["theta"][q, done:]).all()
        assert np.isnan(res.mu[q]).all() and np.isnan(res.var[q]).all()
        assert np.isnan(res.objectives["nlml"][q])
        for k in SCORES:
            assert np.isnan(res.scores[k][q]), k


# ------------------------------------------------- 9. batch size and position change no bit
def test_block_batch_size_and_position_change_no_bit(gpu_ctx):
    import gpscore
    B = 300  # more workgroups than the chip has compute units: two rounds
    X, y, Xt, yt, th = problems(B, 130, d=3, nt=9)
    for a in (X, y, Xt, yt, th):
        a[B - 1] = a[0]
    kw = dict(nfold=4, lr=0.1, itr=2, ctx=gpu_ctx)
    alone = gpscore.blockloo_train_tall(X[:1], y[:1], th[:1], "kc", Xt=Xt[:1], yt=yt[:1], **kw)
    full = gpscore.blockloo_train_tall(X, y, th, "kc", Xt=Xt, yt=yt, **kw)
    assert not full.info.any() and list(full.steps_done) == [2] * B
    fa, ff = result_fields(alone), result_fields(full)
    for k in fa:
        assert same_bits(fa[k][0], ff[k][0]), k
        assert same_bits(fa[k][0], ff[k][B - 1]), k
    assert not same_bits(ff["theta"][0], ff["theta"][1])  # the problems are distinct
    v1 = gpscore.blockloo_value_and_grad_tall(X[:1], y[:1], th[:1], "dss", ctx=gpu_ctx)
    vB = gpscore.blockloo_value_and_grad_tall(X, y, th, "dss", ctx=gpu_ctx)
    for a, b in zip(v1[:3], vB[:3]):
        assert same_bits(a[0], b[0]) and same_bits(a[0], b[B - 1])
    for k in OBJ5:
        assert same_bits(v1[3][k][0], vB[3][k][B - 1]), k


def test_block_position_changes_no_bit_at_n500(gpu_ctx):
    import gpscore
    X, y, Xt, yt, th = problems(3, 500, nt=70)
    for obj in BOBJS:
        for one in (slice(0, 1), slice(2, 3)):
            v1 = gpscore.blockloo_value_and_grad_tall(X[one], y[one], th[one], obj, ctx=gpu_ctx)
            v3 = gpscore.blockloo_value_and_grad_tall(X, y, th, obj, ctx=gpu_ctx)
            assert not v3[4].any()
            for a, b in zip(v1[:3], v3[:3]):
                assert same_bits(a[0], b[one][0]), obj
    one = slice(2, 3)
    kw = dict(nfold=4, lr=1e-3, itr=2, ctx=gpu_ctx)
    r1 = gpscore.blockloo_train_tall(X[one], y[one], th[one], "dss", Xt=Xt[one], yt=yt[one], **kw)
    r3 = gpscore.blockloo_train_tall(X, y, th, "dss", Xt=Xt, yt=yt, **kw)
    f1, f3 = result_fields(r1), result_fields(r3)
    for k in f1:
        assert same_bits(f1[k][0], f3[k][2]), k


# ------------------------------------------------------ 10. the rest of the context is untouched
def test_block_leaves_resident_fit_and_tall_calls_alone(gp, gpu_ctx):
    import gpscore
    g = load_golden("full_n64_d8")
    gp.fit(g["X"], g["y"], theta_of(g)[0])
    before = gp.predict(g["Xt"], g["yt"], with_scores=True)
    X, y, Xt, yt, th = problems(3, 200, nt=70)
    tb = gpscore.value_and_grad_tall(X, y, th, "loo_crps", ctx=gpu_ctx)
    gpscore.blockloo_train_tall(X, y, th, "dss", lr=1e-3, itr=2, Xt=Xt, yt=yt, ctx=gpu_ctx)
    gpscore.blockloo_value_and_grad_tall(X, y, th, "kc", ctx=gpu_ctx)
    after = gp.predict(with_scores=True)
    assert same_bits(before[0], after[0]) and same_bits(before[1], after[1])
    assert before[2] == after[2]
    ta = gpscore.value_and_grad_tall(X, y, th, "loo_crps", ctx=gpu_ctx)
    assert same_bits(tb[0], ta[0]) and same_bits(tb[1], ta[1]) and same_bits(tb[3], ta[3])
    for k in OBJ5:
        assert same_bits(tb[2][k], ta[2][k]), k


# ------------------------------------------------------------------------ 11. profiling tags
def test_block_launches_have_their_own_profiling_tags(gpu_ctx):
    import gpscore
    X, y, _, _, th = problems(2, 130, d=3)
    gpu_ctx.prof(True)
    gpscore.blockloo_train_tall(X, y, th, "dss", lr=1e-3, itr=40, ctx=gpu_ctx)  # two launches
    gpscore.blockloo_value_and_grad_tall(X, y, th, "dss", ctx=gpu_ctx)
    rep = gpu_ctx.prof_collect()
    gpu_ctx.prof(False)
    assert rep["batch_full_tall_block_train"]["count"] == 1, rep
    assert rep["batch_full_tall_block_grad"]["count"] == 1, rep
    assert rep["batch_full_tall_block_train"]["ms"] > 0
    assert "batch_full_tall_train" not in rep and "batch_full_tall_grad" not in rep


# ------------------------------------------------------------------------ 12. C-ABI refusals
B_, N_, D_, NT_, ITR_ = 2, 4, 2, 3, 2
ENTRIES = {"gps_full_blockloo_grad_tall": False, "gps_full_blockloo_train_tall": True}
NULL_ARG = "NULL argument"
NFOLD = "batch: nfold must be in 2..32 and at most n"
CASES = [("X", None, NULL_ARG, "all"),
         ("theta", None, NULL_ARG, "all"),
         ("value", None, NULL_ARG, "grad"),
         ("grad", None, NULL_ARG, "grad"),
         ("theta_out", None, NULL_ARG, "train"),
         ("kind", 7, "kind must be GPS_ARD or GPS_RBF", "all"),
         ("objective", 2, "objective must be GPS_BLOCK_DSS or GPS_BLOCK_KC", "all"),
         ("nfold", 1, NFOLD, "all"),
         ("nfold", 33, NFOLD, "all"),
         ("nfold", N_ + 1, NFOLD, "all"),
         ("nprob", 0, "batch: nprob must be in 1..2^20", "all"),
         ("n", 513, "batch: n must be in 1..512", "all"),
         ("d", 17, "batch: d must be in 1..16", "all"),
         ("n_ell", 3, "n_ell must be 1 or d", "all"),
         ("itr", -1, "batch: itr must be in 0..2^20", "train"),
         ("lr", float("inf"), "batch: lr must be finite", "train"),
         ("nt", -1, "batch: nt must be in 0..2^24", "train"),
         ("flags", 2, "unknown batch flag", "train")]
PARAMS = [pytest.param(entry, arg, bad, msg, id=f"{entry}-{arg}={bad}")
          for entry, train in ENTRIES.items()
          for arg, bad, msg, where in CASES
          if where == "all" or (where == "train") == train]


def arguments(train):
    """The entry's arguments by name, in the order of include/gpscore.h, all valid."""
    rng = np.random.default_rng(7)
    X = rng.normal(size=(B_, N_, D_))
    a = dict(kind=0, objective=1, nfold=2, nprob=B_, X=X, y=np.sin(X.sum(axis=2)), n=N_, d=D_,
             theta=np.tile([0.0, 0.1, -0.1, -2.0], (B_, 1)), n_ell=D_)
    if train:
        Xt = rng.normal(size=(B_, NT_, D_))
        a.update(itr=ITR_, lr=0.01, Xt=Xt, yt=np.sin(Xt.sum(axis=2)), nt=NT_, flags=0,
                 theta_out=np.zeros((B_, 2 + D_)), values=np.zeros((B_, ITR_)),
                 thetas=np.zeros((B_, ITR_, 2 + D_)), obj=np.zeros((B_, 5)),
                 mu=np.zeros((B_, NT_)), var=np.zeros((B_, NT_)), sc=np.zeros((B_, 6)),
                 info=np.full(B_, -1, np.int32), steps_done=np.full(B_, -1, np.int32))
    else:
        a.update(value=np.zeros(B_), fold_values=np.zeros((B_, 2)), obj=np.zeros((B_, 5)),
                 grad=np.zeros((B_, 2 + D_)), info=np.full(B_, -1, np.int32))
    return a


@pytest.mark.parametrize("entry,arg,bad,msg", PARAMS)
def test_block_refusal_and_recovery(gpu_ctx, entry, arg, bad, msg):
    from gpscore import GpsError
    from test_gpu_batch_refusals import positional
    train = ENTRIES[entry]
    a = arguments(train)
    assert arg in a
    a[arg] = bad
    with pytest.raises(GpsError) as e:
        gpu_ctx.call(entry, *positional(a))
    assert str(e.value) == f"{entry} failed (-1): {msg}"
    ok = arguments(train)  # the same context runs a valid call straight away
    gpu_ctx.call(entry, *positional(ok))
    assert (ok["info"] == 0).all()
    assert np.isfinite(ok["obj"]).all() and (ok["obj"] != 0).any()
    if train:
        assert (ok["steps_done"] == ITR_).all()
        assert np.isfinite(ok["theta_out"]).all() and np.isfinite(ok["sc"]).all()
    else:
        assert np.isfinite(ok["grad"]).all() and (ok["grad"] != 0).any()
        assert np.isfinite(ok["value"]).all() and np.isfinite(ok["fold_values"]).all()


def test_block_optional_outputs_may_be_null(gpu_ctx):
    """fold_values and obj may be NULL; the rest comes out the same."""
    from test_gpu_batch_refusals import positional
    full, part = arguments(False), arguments(False)
    part["fold_values"] = None
    part["obj"] = None
    gpu_ctx.call("gps_full_blockloo_grad_tall", *positional(full))
    gpu_ctx.call("gps_full_blockloo_grad_tall", *positional(part))
    assert same_bits(full["value"], part["value"]) and same_bits(full["grad"], part["grad"])
    assert (part["info"] == 0).all()


# --------------------------------------------------------------------------- 13. the harness
def test_run_full_blockloo_batch_matches_run(gpu_ctx):
    """run_full_blockloo_batch against run(kind="full") on synthetic sheets: TT = 2, three DSS
    steps, the same seed: the same problems, metrics at 1e-8."""
    from gpscore import experiment as E
    sheets = E.synthetic_sheets(5, n_pool=2000, n_test=500)
    methods = {"dss": E.KF_METHODS["dss"]}
    out = E.run_full_blockloo_batch(sheets, TT=2, itr=3, seed=7, ctx=gpu_ctx)
    ref = E.run(sheets, TT=2, methods=methods, kind="full", itr=3, seed=7, ctx=gpu_ctx)
    assert list(out) == ["dss"]
    assert out["dss"]["theta"].shape == (2, 10)
    for k in E.METRICS:
        for j in range(2):
            assert close(out["dss"][k][j], ref["dss"][k][j], TOL8), (k, j, out["dss"][k][j],
                                                                     ref["dss"][k][j])
