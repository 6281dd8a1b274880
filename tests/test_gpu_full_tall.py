"""Batches of full GPs of up to 512 rows (gps_full_grad_tall / gps_full_train_tall)
against the reference's autograd goldens, the oracle at the tile edges, the other implementations
(GP.value_and_grad, GP.train, GP.fit + GP.predict, the small-batch calls), and their own
invariants: the launch split, the batch size and a problem's position change no bit, a failed
problem touches no other, the rest of the context is left alone.  Follows tests/test_gpu_batch.py
and reuses its helpers.  Runs on the GPU box.

Tolerances: 1e-9 (close / nrel) on values, gradients and objectives, 1e-8 on the predictive and
its scores, as the issue sets them; at the tile edges max(1e-9, 30 × the case's conditioning
floor), the floor being the oracle on X perturbed by 1e-15 relative, with the cap 30 × floor <=
5e-9 asserted on the oracle alone.  The tall path, the small-batch path and the resident path sum
in different orders, so they are compared at those tolerances, never bitwise."""
import functools

import numpy as np
import pytest

import gp_oracle as O
from conftest import load_golden, nrel, theta_of
from test_gpu_batch import (OBJ5, OBJS, SCORES, TOL, close, edge_problems, result_fields, row_of,
                            same_bits, tup_of)

pytestmark = pytest.mark.gpu

T = 64       # kBatchFullTallTile
TOL8 = 1e-8  # the predictive and its scores


@pytest.fixture(scope="module")
def gp(gpu_ctx):
    import gpscore
    return gpscore.GP(ctx=gpu_ctx)


def problems(B, n, d=8, nt=0, seed=3):
    """B problems of one shape by test_gpu_batch.small_problems' recipe, one ℓ per dimension."""
    rng = np.random.default_rng(seed + n)
    X, Xt = rng.standard_normal((B, n, d)), rng.standard_normal((B, max(nt, 1), d))
    w = rng.standard_normal(d) / np.sqrt(d)
    y = np.sin(X @ w) + 0.1 * rng.standard_normal((B, n))
    yt = np.sin(Xt @ w) + 0.1 * rng.standard_normal((B, max(nt, 1)))
    th = np.stack([np.concatenate([[0.1 + 0.01 * (q % 7)],
                                   np.log(np.linspace(1.2, 2.4, d)) + 0.02 * (q % 5),
                                   [np.log(0.05) + 0.03 * (q % 3)]]) for q in range(B)])
    return X, y, Xt, yt, th


# ------------------------------------------------------------ 1. the reference's autograd
def golden_batch(name):
    """The golden as problem 1 of three; its neighbours are the same data at θ ∓ 0.05."""
    g = load_golden(name)
    th, kern = theta_of(g)
    row = row_of(th)
    X, y = np.stack([g["X"]] * 3), np.stack([g["y"]] * 3)
    return g, kern == "rbf", X, y, np.stack([row - 0.05, row, row + 0.05])


@pytest.mark.parametrize("name", ["full_n500_d8", "full_n64_d8", "full_n64_d8_iso", "sd_j0_init",
                                  "sd_j0_rbf"])
def test_tall_vs_autograd_golden(gpu_ctx, name):
    import gpscore
    g, rbf, X, y, th = golden_batch(name)
    kind = "rbf" if rbf else "ARD"
    for obj in OBJS:
        vals, grads, objs, info = gpscore.value_and_grad_tall(X, y, th, obj, rbf=rbf, ctx=gpu_ctx)
        assert not info.any(), info
        assert close(vals[1], float(g[obj])), (obj, vals[1], float(g[obj]))
        assert nrel(grads[1], g["grad_" + obj]) <= TOL, (obj, grads[1], g["grad_" + obj])
        for k in OBJ5:
            assert close(objs[k][1], float(g[k])), (obj, k, objs[k][1], float(g[k]))
        for q in (0, 2):  # the neighbours against the oracle
            ov, og = O.fast_full_grad(X[q], y[q], *tup_of(th[q]), obj, kind=kind)
            assert close(vals[q], ov), (obj, q, vals[q], ov)
            assert nrel(grads[q], og) <= TOL, (obj, q, grads[q], og)
    Xt, yt = np.stack([g["Xt"]] * 3), np.stack([g["yt"]] * 3)
    res = gpscore.train_tall(X, y, th, "loo_crps", lr=1.0, itr=0, Xt=Xt, yt=yt, rbf=rbf,
                             ctx=gpu_ctx)
    assert not res.info.any() and not res.steps_done.any() and same_bits(res.theta, th)
    assert nrel(res.mu[1], g["pred_mu"]) <= TOL8, nrel(res.mu[1], g["pred_mu"])
    assert nrel(res.var[1], g["pred_var"]) <= TOL8, nrel(res.var[1], g["pred_var"])
    for k in SCORES:
        assert close(res.scores[k][1], float(g[k]), TOL8), (k, res.scores[k][1], float(g[k]))
    for k in OBJ5:
        assert close(res.objectives[k][1], float(g[k])), (k, res.objectives[k][1], float(g[k]))


# ------------------------------------------------------------ 2. the oracle at the tile edges
EDGE_N = (1, 2, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T - 1, 3 * T, 3 * T + 1, 500,
          511, 512)
EDGE_CASES = [(n, d, vec, rbf) for n in EDGE_N
              for d, vec, rbf in ((1, False, False), (1, False, True), (8, True, False),
                                  (16, True, False))]
NQ = 3


@functools.lru_cache(maxsize=None)
def edge_oracle(n, d, vec, rbf, obj):
    """Per problem (value, grad, tol): the oracle and the case's tolerance from its conditioning
    floor (the oracle on X perturbed by 1e-15 relative, same metrics)."""
    X, y, th = (a[:NQ] for a in edge_problems(n, d, vec))
    kind = "rbf" if rbf else "ARD"
    out = []
    for q in range(NQ):
        ov, og = O.fast_full_grad(X[q], y[q], *tup_of(th[q]), obj, kind=kind)
        r = np.random.default_rng(1)
        Xp = X[q] * (1 + 1e-15 * r.standard_normal(X[q].shape))
        pv, pg = O.fast_full_grad(Xp, y[q], *tup_of(th[q]), obj, kind=kind)
        floor = max(abs(pv - ov) / max(1.0, abs(ov)), nrel(pg, og))
        assert 30 * floor <= 5e-9, (n, d, vec, rbf, obj, q, floor)  # the hard cap, on the reference
        out.append((ov, og, max(TOL, 30 * floor)))
    return out


@pytest.mark.parametrize("n,d,vec,rbf", EDGE_CASES)
def test_tall_vs_oracle_edges(gpu_ctx, n, d, vec, rbf):
    import gpscore
    X, y, th = (a[:NQ] for a in edge_problems(n, d, vec))
    worst = 0.0
    for obj in OBJS:
        refs = edge_oracle(n, d, vec, rbf, obj)  # asserts the cap before the GPU is looked at
        vals, grads, objs, info = gpscore.value_and_grad_tall(X, y, th, obj, rbf=rbf, ctx=gpu_ctx)
        assert not info.any(), (obj, info)
        for q, (ov, og, tol) in enumerate(refs):
            ev, eg = abs(vals[q] - ov) / max(1.0, abs(ov)), nrel(grads[q], og)
            worst = max(worst, ev, eg)
            assert ev <= tol, (obj, q, "value", vals[q], ov, tol)
            assert eg <= tol, (obj, q, "grad", grads[q], og, tol)
    print("edge", n, d, vec, rbf, "worst error %.3g" % worst)


# ------------------------------------------------------------ 3. the other implementations
@pytest.mark.parametrize("n", [129, 500])
def test_tall_vs_resident_path(gp, gpu_ctx, n):
    import gpscore
    X, y, _, _, th = problems(2, n)
    for obj in OBJS:
        vals, grads, objs, info = gpscore.value_and_grad_tall(X, y, th, obj, ctx=gpu_ctx)
        assert not info.any()
        for q in range(2):
            v1, g1, o1 = gp.value_and_grad(tup_of(th[q]), obj, X=X[q], y=y[q])
            assert close(vals[q], v1), (obj, q, vals[q], v1)
            assert nrel(grads[q], g1) <= TOL, (obj, q, grads[q], g1)
            for k in OBJ5:
                assert close(objs[k][q], o1[k]), (obj, q, k, objs[k][q], o1[k])


@pytest.mark.parametrize("n", [64, 128])
def test_tall_vs_small_batch(gpu_ctx, n):
    import gpscore
    X, y, Xt, yt, th = problems(3, n, nt=70)
    for obj in OBJS:
        a = gpscore.value_and_grad_tall(X, y, th, obj, ctx=gpu_ctx)
        b = gpscore.value_and_grad_batch(X, y, th, obj, ctx=gpu_ctx)
        assert not a[3].any() and not b[3].any()
        for q in range(3):
            assert close(a[0][q], b[0][q]), (obj, q)
            assert nrel(a[1][q], b[1][q]) <= TOL, (obj, q)
            for k in OBJ5:
                assert close(a[2][k][q], b[2][k][q]), (obj, q, k)
    kw = dict(lr=0.05, itr=2, Xt=Xt, yt=yt, stale_noise=True, ctx=gpu_ctx)
    ra, rb = gpscore.train_tall(X, y, th, "loo_logs", **kw), gpscore.train_batch(X, y, th, "loo_logs", **kw)
    assert nrel(ra.theta, rb.theta) <= TOL and nrel(ra.mu, rb.mu) <= TOL8 and nrel(ra.var, rb.var) <= TOL8
    for k in SCORES:
        for q in range(3):
            assert close(ra.scores[k][q], rb.scores[k][q], TOL8), (k, q)


# ----------------------------------------------------------------------------- 4. training
@pytest.mark.parametrize("obj,lr", [("loo_crps", 1.0), ("nlml", 5e-4), ("loo_logs", 0.05)])
def test_tall_train_matches_oracle_and_gp_train(gp, gpu_ctx, obj, lr):
    """Five SGD steps at the KF method's lr from two starts at n = 200, d = 8, against the oracle
    loop and against GP.train."""
    import gpscore
    X, y, _, _, th = problems(2, 200)
    th[1, 1:-1] += 0.3
    res = gpscore.train_tall(X, y, th, obj, lr=lr, itr=5, ctx=gpu_ctx)
    assert not res.info.any() and list(res.steps_done) == [5, 5]
    for q in range(2):
        t = th[q].copy()
        for i in range(5):
            v, gr = O.fast_full_grad(X[q], y[q], t[0], t[1:-1], t[-1], obj)
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


# ------------------------------------------------------------ 5. the launch split is invisible
def test_launch_split_changes_no_bit(gpu_ctx):
    """At n = 130 (three blocks: 37 steps a launch) itr = a + b beyond one launch equals, bitwise
    in every field, itr = a continued by itr = b: the split points 37 | 13 and 30 | 20 differ."""
    import gpscore
    a, b = 30, 20
    X, y, Xt, yt, th = problems(3, 130, d=3, nt=9)
    kw = dict(lr=0.05, Xt=Xt, yt=yt, ctx=gpu_ctx)
    whole = gpscore.train_tall(X, y, th, "loo_logs", itr=a + b, **kw)
    first = gpscore.train_tall(X, y, th, "loo_logs", itr=a, **kw)
    second = gpscore.train_tall(X, y, first.theta, "loo_logs", itr=b, **kw)
    assert not whole.info.any() and list(whole.steps_done) == [a + b] * 3
    assert same_bits(whole.theta, second.theta)
    for k in ("objective", "theta"):
        joined = np.concatenate([first.series[k], second.series[k]], axis=1)
        assert same_bits(whole.series[k], joined), k
    fw, fs = result_fields(whole), result_fields(second)
    for k in fw:
        if k not in ("values", "thetas", "steps_done"):
            assert same_bits(fw[k], fs[k]), k
    assert not same_bits(whole.series["theta"][:, 0], whole.series["theta"][:, -1])  # it did move


# ----------------------------------------------------------------------------- 6. final pass
@pytest.mark.parametrize("stale", [True, False])
@pytest.mark.parametrize("nt", [1, 63, 65, 300])
def test_final_pass_vs_fit_predict(gp, gpu_ctx, nt, stale):
    """After three steps the predictive's σ² is, with stale_noise, the one the third step's
    forward used (θ after step 2), without it the final θ's; GP.fit + GP.predict at that θ."""
    import gpscore
    X, y, Xt, yt, th = problems(2, 200, nt=nt)
    res = gpscore.train_tall(X, y, th, "loo_crps", lr=1.0, itr=3, Xt=Xt, yt=yt, stale_noise=stale,
                             ctx=gpu_ctx)
    assert not res.info.any() and res.mu.shape == (2, nt)
    for q in range(2):
        k, ell, noise = tup_of(res.theta[q])
        if stale:
            noise = float(res.series["theta"][q, 1, -1])
        assert noise != res.series["theta"][q, 2 if stale else 1, -1]
        fit = gp.fit(X[q], y[q], (k, ell, noise))
        mu, var, sc1 = gp.predict(Xt[q], yt[q], with_scores=True)
        assert nrel(res.mu[q], mu) <= TOL8 and nrel(res.var[q], var) <= TOL8
        for s in SCORES:
            assert close(res.scores[s][q], sc1[s], TOL8), (s, q, res.scores[s][q], sc1[s])
        for o in OBJ5:
            assert close(res.objectives[o][q], fit[o]), (q, o)


# ---------------------------------------------------------------------- 7. failure isolation
def test_failed_problems_touch_no_other(gpu_ctx):
    """Problem 1: a NaN feature in row 0 (info = 1); problem 2: one in row 70, a pivot of the
    second diagonal block (info = 71); problem 3: a NaN in θ.  All end with NaN outputs and no
    step done; the call succeeds; problems 0 and 4 keep every bit."""
    import gpscore
    X, y, Xt, yt, th = problems(5, 130, d=3, nt=9)
    X[1, 0, 1] = np.nan
    X[2, 70, 0] = np.nan
    th[3, 1] = np.nan
    good, bad = [0, 4], [1, 2, 3]
    kw = dict(lr=0.05, itr=3, ctx=gpu_ctx)
    res = gpscore.train_tall(X, y, th, "loo_crps", Xt=Xt, yt=yt, **kw)
    ref = gpscore.train_tall(X[good], y[good], th[good], "loo_crps", Xt=Xt[good], yt=yt[good], **kw)
    assert res.info[1] == 1 and res.info[2] == 71 and res.info[3] > 0 and not res.info[good].any()
    assert list(res.steps_done) == [3, 0, 0, 0, 3]
    fr, fref = result_fields(res), result_fields(ref)
    for k, v in fr.items():
        assert same_bits(v[good], fref[k]), k
        if k not in ("info", "steps_done", "theta"):
            assert np.isnan(v[bad]).all(), k
    assert not np.isnan(fref["mu"]).any() and not np.isnan(fref["thetas"]).any()
    assert same_bits(res.theta[1], th[1]) and same_bits(res.theta[2], th[2])
    for obj in OBJS:
        vals, grads, objs, info = gpscore.value_and_grad_tall(X, y, th, obj, ctx=gpu_ctx)
        v0, g0, o0, i0 = gpscore.value_and_grad_tall(X[good], y[good], th[good], obj, ctx=gpu_ctx)
        assert list(info[:3]) == [0, 1, 71] and info[3] > 0 and info[4] == 0 and not i0.any()
        assert same_bits(vals[good], v0) and same_bits(grads[good], g0)
        assert np.isnan(vals[bad]).all() and np.isnan(grads[bad]).all()
        for k in OBJ5:
            assert same_bits(objs[k][good], o0[k]) and np.isnan(objs[k][bad]).all(), k


def test_failure_in_a_later_step(gpu_ctx):
    """A step of 1e6 throws θ far outside the representable kernels after the first update: sf²
    and σ² underflow to 0 or overflow, and a forward within the next two steps meets a pivot that
    is not > 0.  The problem stops there: steps_done counts the completed steps (kernels_batch's
    definition), theta_out is the θ the failing forward was at — the last series entry written —
    and the rest of its series and its final outputs are NaN."""
    import gpscore
    X, y, Xt, yt, th = problems(2, 130, d=3, nt=9)
    res = gpscore.train_tall(X, y, th, "nlml", lr=1e6, itr=5, Xt=Xt, yt=yt, ctx=gpu_ctx)
    assert res.info.all(), res.info
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


# ------------------------------------------------- 8. batch size and position change no bit
def test_batch_size_and_position_change_no_bit(gpu_ctx):
    import gpscore
    B = 300  # more workgroups than the chip has compute units: two rounds
    X, y, Xt, yt, th = problems(B, 130, d=3, nt=9)
    for a in (X, y, Xt, yt, th):
        a[B - 1] = a[0]
    kw = dict(lr=0.05, itr=2, ctx=gpu_ctx)
    alone = gpscore.train_tall(X[:1], y[:1], th[:1], "loo_crps", Xt=Xt[:1], yt=yt[:1], **kw)
    full = gpscore.train_tall(X, y, th, "loo_crps", Xt=Xt, yt=yt, **kw)
    assert not full.info.any() and list(full.steps_done) == [2] * B
    fa, ff = result_fields(alone), result_fields(full)
    for k in fa:
        assert same_bits(fa[k][0], ff[k][0]), k
        assert same_bits(fa[k][0], ff[k][B - 1]), k
    assert not same_bits(ff["theta"][0], ff["theta"][1])  # the problems are distinct
    v1 = gpscore.value_and_grad_tall(X[:1], y[:1], th[:1], "loo_logs", ctx=gpu_ctx)
    vB = gpscore.value_and_grad_tall(X, y, th, "loo_logs", ctx=gpu_ctx)
    assert same_bits(v1[1][0], vB[1][0]) and same_bits(v1[1][0], vB[1][B - 1])
    assert same_bits(v1[0][0], vB[0][B - 1])
    for k in OBJ5:
        assert same_bits(v1[2][k][0], vB[2][k][B - 1]), k


def test_position_changes_no_bit_at_n500(gpu_ctx):
    import gpscore
    X, y, Xt, yt, th = problems(3, 500, nt=70)
    one = slice(2, 3)
    for obj in OBJS:
        v1 = gpscore.value_and_grad_tall(X[one], y[one], th[one], obj, ctx=gpu_ctx)
        v3 = gpscore.value_and_grad_tall(X, y, th, obj, ctx=gpu_ctx)
        assert not v3[3].any()
        assert same_bits(v1[0][0], v3[0][2]) and same_bits(v1[1][0], v3[1][2]), obj
    kw = dict(lr=1.0, itr=2, ctx=gpu_ctx)
    r1 = gpscore.train_tall(X[one], y[one], th[one], "loo_crps", Xt=Xt[one], yt=yt[one], **kw)
    r3 = gpscore.train_tall(X, y, th, "loo_crps", Xt=Xt, yt=yt, **kw)
    f1, f3 = result_fields(r1), result_fields(r3)
    for k in f1:
        assert same_bits(f1[k][0], f3[k][2]), k


# ------------------------------------------------------- 9. the rest of the context is untouched
def test_tall_leaves_resident_fit_and_small_batch_alone(gp, gpu_ctx):
    import gpscore
    g = load_golden("full_n64_d8")
    gp.fit(g["X"], g["y"], theta_of(g)[0])
    before = gp.predict(g["Xt"], g["yt"], with_scores=True)
    Xs, ys, Xts, yts, ths = problems(4, 40, d=3, nt=9)
    kws = dict(lr=0.05, itr=3, Xt=Xts, yt=yts, ctx=gpu_ctx)
    sb = gpscore.train_batch(Xs, ys, ths, "loo_crps", **kws)
    X, y, Xt, yt, th = problems(3, 200, nt=70)
    gpscore.train_tall(X, y, th, "nlml", lr=1e-3, itr=2, Xt=Xt, yt=yt, ctx=gpu_ctx)
    gpscore.value_and_grad_tall(X, y, th, "loo_crps", ctx=gpu_ctx)
    after = gp.predict(with_scores=True)
    assert same_bits(before[0], after[0]) and same_bits(before[1], after[1])
    assert before[2] == after[2]
    sa = gpscore.train_batch(Xs, ys, ths, "loo_crps", **kws)
    fb, fa = result_fields(sb), result_fields(sa)
    for k in fb:
        assert same_bits(fb[k], fa[k]), k


def test_tall_launches_have_their_own_profiling_tags(gpu_ctx):
    import gpscore
    X, y, _, _, th = problems(2, 130, d=3)
    gpu_ctx.prof(True)
    gpscore.train_tall(X, y, th, "nlml", lr=1e-3, itr=40, ctx=gpu_ctx)  # two launches, one tag
    gpscore.value_and_grad_tall(X, y, th, "nlml", ctx=gpu_ctx)
    rep = gpu_ctx.prof_collect()
    gpu_ctx.prof(False)
    assert rep["batch_full_tall_train"]["count"] == 1, rep
    assert rep["batch_full_tall_grad"]["count"] == 1, rep
    assert rep["batch_full_tall_train"]["ms"] > 0


# --------------------------------------------------------------------------- 10. the harness
def test_run_full_batch_matches_run(gpu_ctx):
    """run_full_batch against run(kind="full") on synthetic sheets: TT = 2, three steps a method,
    the same seed: the same problems, metrics at 1e-8."""
    from gpscore import experiment as E
    sheets = E.synthetic_sheets(5, n_pool=2000, n_test=500)
    methods = {k: E.KF_METHODS[k] for k in ("crps", "nlml", "logs")}
    out = E.run_full_batch(sheets, TT=2, itr=3, seed=7, ctx=gpu_ctx)
    ref = E.run(sheets, TT=2, methods=methods, kind="full", itr=3, seed=7, ctx=gpu_ctx)
    assert list(out) == list(methods)
    for name in methods:
        assert out[name]["theta"].shape == (2, 10)
        for k in E.METRICS:
            for j in range(2):
                assert close(out[name][k][j], ref[name][k][j], TOL8), (name, k, j, out[name][k][j],
                                                                      ref[name][k][j])
