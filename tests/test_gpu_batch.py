"""Batches of small full GPs in one launch (gps_full_grad_batch / gps_full_train_batch, DESIGN
§19) against the reference's autograd goldens, the oracle at the size edges, the existing
one-problem path (GP.value_and_grad / GP.train / GP.fit + GP.predict), and their own invariants:
the launch split, the batch size and a problem's position change no bit, a failed problem
touches no other, the rest of the context is left alone.  Runs on the GPU box.

Tolerances are the project's for the same quantities: 1e-9 normwise on gradients and vectors,
1e-9·max(1, |v|) on values and scores (tests/test_gpu_grad.py, tests/test_gpu_parity.py's sd_*
goldens).  The batched and the one-problem paths sum in different orders, so they are compared
at that tolerance, never bitwise."""
import numpy as np
import pytest

import gp_oracle as O
from conftest import load_golden, nrel, theta_of

pytestmark = pytest.mark.gpu

OBJS = ("nlml", "loo_crps", "loo_logs")
OBJ5 = ("nlml", "loo_crps", "loo_logs", "logdet", "quad")
SCORES = ("test_crps", "test_logs", "test_msll", "test_smse", "test_mse", "test_cover")
TOL = 1e-9
CUS = 256  # compute units of the MI355X (as tests/test_gemm_schedule.py's SLOTS)


@pytest.fixture(scope="module")
def gp(gpu_ctx):
    import gpscore
    return gpscore.GP(ctx=gpu_ctx)


def close(a, b, tol=TOL):
    return abs(a - b) <= tol * max(1.0, abs(b))


def row_of(th):
    return np.concatenate([[th[0]], np.atleast_1d(th[1]).ravel(), [th[2]]])


def tup_of(row):
    return (float(row[0]), np.array(row[1:-1]), float(row[-1]))


def same_bits(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def result_fields(r):
    """Every array of a BatchTrainResult, flat."""
    out = {"theta": r.theta, "values": r.series["objective"], "thetas": r.series["theta"],
           "info": r.info, "steps_done": r.steps_done}
    out.update({"obj_" + k: v for k, v in r.objectives.items()})
    if r.mu is not None:
        out.update(mu=r.mu, var=r.var)
    if r.scores is not None:
        out.update(r.scores)
    return out


# ------------------------------------------------------------ 1. the reference's autograd
GOLDEN_BATCHES = {"sd_ard": ["sd_j0_init", "sd_j1_init", "sd_j0_fit", "sd_j1_fit"],
                  "sd_rbf": ["sd_j0_rbf", "sd_j1_rbf"], "full_n64_d8": ["full_n64_d8"]}


@pytest.mark.parametrize("batch", sorted(GOLDEN_BATCHES))
@pytest.mark.parametrize("obj", OBJS)
def test_batch_grad_vs_autograd_golden(gpu_ctx, batch, obj):
    import gpscore
    gs = [load_golden(nm) for nm in GOLDEN_BATCHES[batch]]
    kerns = {theta_of(g)[1] for g in gs}
    assert len(kerns) == 1
    X = np.stack([g["X"] for g in gs])
    y = np.stack([g["y"] for g in gs])
    th = np.stack([row_of(theta_of(g)[0]) for g in gs])
    vals, grads, objs, info = gpscore.value_and_grad_batch(X, y, th, obj, rbf=kerns == {"rbf"},
                                                           ctx=gpu_ctx)
    assert not info.any()
    for q, g in enumerate(gs):
        assert close(vals[q], float(g[obj])), (q, vals[q], float(g[obj]))
        assert nrel(grads[q], g["grad_" + obj]) <= TOL, (q, grads[q], g["grad_" + obj])
        for k in OBJ5:
            assert close(objs[k][q], float(g[k])), (q, k, objs[k][q], float(g[k]))


# ------------------------------------------------- 2, 3. the oracle and the existing path
B_EDGE = 5
EDGE_N = (1, 2, 17, 63, 64, 65, 127, 128)
EDGE_D = [(1, False), (3, False), (3, True), (16, False), (16, True)]  # (d, one ℓ per dimension)
_edge_cache = {}


def edge_problems(n, d, vec):
    """B_EDGE problems by the data recipe of test_grad_vs_oracle_shapes, each with its own θ."""
    rng = np.random.default_rng(n + d)
    X = rng.standard_normal((B_EDGE, n, d))
    y = np.sin(X.sum(2)) + 0.1 * rng.standard_normal((B_EDGE, n))
    ell = np.log(np.linspace(0.8, 2.5, d)) if vec else np.array([np.log(1.3)])
    th = np.stack([np.concatenate([[0.1 + 0.05 * q], ell + 0.03 * q, [np.log(0.03) + 0.1 * q]])
                   for q in range(B_EDGE)])
    return X, y, th


def edge_batch(ctx, n, d, vec, rbf, obj):
    import gpscore
    key = (n, d, vec, rbf, obj)
    if key not in _edge_cache:
        X, y, th = edge_problems(n, d, vec)
        _edge_cache[key] = gpscore.value_and_grad_batch(X, y, th, obj, rbf=rbf, ctx=ctx)
    return _edge_cache[key]


@pytest.mark.parametrize("rbf", [False, True])
@pytest.mark.parametrize("d,vec", EDGE_D)
@pytest.mark.parametrize("n", EDGE_N)
def test_batch_grad_vs_oracle_edges(gpu_ctx, n, d, vec, rbf):
    X, y, th = edge_problems(n, d, vec)
    for obj in OBJS:
        vals, grads, objs, info = edge_batch(gpu_ctx, n, d, vec, rbf, obj)
        assert not info.any(), info
        for q in range(B_EDGE):
            ov, og = O.fast_full_grad(X[q], y[q], *tup_of(th[q]), obj, kind="rbf" if rbf else "ARD")
            assert close(vals[q], ov), (obj, q, vals[q], ov)
            assert nrel(grads[q], og) <= TOL, (obj, q, grads[q], og)


@pytest.mark.parametrize("rbf", [False, True])
@pytest.mark.parametrize("d,vec", EDGE_D)
@pytest.mark.parametrize("n", [n for n in EDGE_N if n > 1])  # gps_full_set_data needs n > 1
def test_batch_grad_vs_single_path(gp, gpu_ctx, n, d, vec, rbf):
    """The same problems through GP.value_and_grad: 1e-9, not bitwise (another summation order)."""
    X, y, th = edge_problems(n, d, vec)
    for obj in OBJS:
        vals, grads, objs, info = edge_batch(gpu_ctx, n, d, vec, rbf, obj)
        for q in range(B_EDGE):
            v1, g1, o1 = gp.value_and_grad(tup_of(th[q]), obj, X=X[q], y=y[q], rbf=rbf)
            assert close(vals[q], v1), (obj, q, vals[q], v1)
            assert nrel(grads[q], g1) <= TOL, (obj, q, grads[q], g1)
            for k in OBJ5:
                assert close(objs[k][q], o1[k]), (obj, q, k, objs[k][q], o1[k])


# ----------------------------------------------------------------------------- 4. training
@pytest.mark.parametrize("obj,lr", [("loo_crps", 1.0), ("nlml", 1e-3)])
def test_batch_train_matches_oracle_and_gp_train(gp, gpu_ctx, obj, lr):
    """Five SGD steps from (1, 1, 1) on both SD data sets (SD:192-231, 277-301), checked as
    test_sgd_train_matches_oracle checks GP.train, and against GP.train itself."""
    import gpscore
    gs = [load_golden("sd_j0_init"), load_golden("sd_j1_init")]
    X, y = np.stack([g["X"] for g in gs]), np.stack([g["y"] for g in gs])
    res = gpscore.train_batch(X, y, (1.0, 1.0, 1.0), obj, lr=lr, itr=5, ctx=gpu_ctx)
    assert not res.info.any() and list(res.steps_done) == [5, 5]
    for q, g in enumerate(gs):
        t = np.array([1.0, 1.0, 1.0])
        for i in range(5):
            v, gr = O.fast_full_grad(g["X"], g["y"], t[0], t[1:-1], t[-1], obj)
            assert abs(v - res.series["objective"][q, i]) <= TOL * abs(v), (q, i)
            t = t - lr * gr
            assert nrel(res.series["theta"][q, i], t) <= TOL, (q, i)
        assert nrel(res.theta[q], t) <= TOL
        assert same_bits(res.theta[q], res.series["theta"][q, -1])
        theta, series = gp.train((1.0, 1.0, 1.0), obj, lr=lr, itr=5, X=g["X"], y=g["y"])
        for i in range(5):
            assert abs(series["objective"][i] - res.series["objective"][q, i]) \
                <= TOL * abs(series["objective"][i]), (q, i)
            assert nrel(res.series["theta"][q, i], series["theta"][i]) <= TOL, (q, i)
        assert nrel(res.theta[q], row_of(theta)) <= TOL


# ------------------------------------------------------------ 5. the launch split is invisible
def small_problems(B, n=32, d=3, nt=9, seed=11):
    rng = np.random.default_rng(seed)
    X, Xt = rng.standard_normal((B, n, d)), rng.standard_normal((B, nt, d))
    y = np.sin(X.sum(2)) + 0.1 * rng.standard_normal((B, n))
    yt = np.sin(Xt.sum(2)) + 0.1 * rng.standard_normal((B, nt))
    th = np.stack([[0.1 + 0.01 * (q % 7), np.log(1.3) + 0.02 * (q % 5), np.log(0.05) + 0.03 * (q % 3)]
                   for q in range(B)])
    return X, y, Xt, yt, th


def test_launch_split_changes_no_bit(gpu_ctx):
    """itr = a + b beyond the steps one launch runs (64) equals, bitwise, itr = a continued by
    itr = b from the returned θ: the split points 64 | 6 and 40 | 30 differ, the bits do not."""
    import gpscore
    a, b = 40, 30
    X, y, Xt, yt, th = small_problems(3)
    kw = dict(lr=0.05, Xt=Xt, yt=yt, ctx=gpu_ctx)
    whole = gpscore.train_batch(X, y, th, "loo_logs", itr=a + b, **kw)
    first = gpscore.train_batch(X, y, th, "loo_logs", itr=a, **kw)
    second = gpscore.train_batch(X, y, first.theta, "loo_logs", itr=b, **kw)
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
def check_predictive(mu, var, sc, ref_mu, ref_var, ref_sc):
    assert nrel(mu, ref_mu) <= TOL, nrel(mu, ref_mu)
    assert nrel(var, ref_var) <= TOL, nrel(var, ref_var)
    for k in SCORES:
        assert close(sc[k], float(ref_sc[k])), (k, sc[k], float(ref_sc[k]))


def test_final_pass_itr0_vs_golden_and_predict(gp, gpu_ctx):
    import gpscore
    gs = [load_golden("sd_j0_fit"), load_golden("sd_j1_fit")]
    stack = lambda k: np.stack([g[k] for g in gs])  # noqa: E731
    th = np.stack([row_of(theta_of(g)[0]) for g in gs])
    res = gpscore.train_batch(stack("X"), stack("y"), th, "loo_crps", lr=1.0, itr=0,
                              Xt=stack("Xt"), yt=stack("yt"), ctx=gpu_ctx)
    assert not res.info.any() and not res.steps_done.any()
    assert same_bits(res.theta, th) and res.series["objective"].shape == (2, 0)
    for q, g in enumerate(gs):
        sc = {k: res.scores[k][q] for k in SCORES}
        check_predictive(res.mu[q], res.var[q], sc, g["pred_mu"], g["pred_var"], g)
        for k in OBJ5:
            assert close(res.objectives[k][q], float(g[k])), (q, k)
        fit = gp.fit(g["X"], g["y"], theta_of(g)[0])
        mu, var, sc1 = gp.predict(g["Xt"], g["yt"], with_scores=True)
        check_predictive(res.mu[q], res.var[q], sc, mu, var, sc1)
        for k in OBJ5:
            assert close(res.objectives[k][q], fit[k]), (q, k)


@pytest.mark.parametrize("stale", [True, False])
def test_final_pass_noise_after_three_steps(gp, gpu_ctx, stale):
    """stale_noise: the predictive's σ² is the one the last (third) step's forward used, θ after
    step 2 — the scripts' module-global sigma_noise_sq; without it the final θ's."""
    import gpscore
    gs = [load_golden("sd_j0_init"), load_golden("sd_j1_init")]
    stack = lambda k: np.stack([g[k] for g in gs])  # noqa: E731
    res = gpscore.train_batch(stack("X"), stack("y"), (1.0, 1.0, 1.0), "loo_crps", lr=1.0, itr=3,
                              Xt=stack("Xt"), yt=stack("yt"), stale_noise=stale, ctx=gpu_ctx)
    assert not res.info.any()
    for q, g in enumerate(gs):
        k, ell, noise = tup_of(res.theta[q])
        if stale:
            noise = float(res.series["theta"][q, 1, -1])
        assert noise != res.series["theta"][q, 2 if stale else 1, -1]
        fit = gp.fit(g["X"], g["y"], (k, ell, noise))
        mu, var, sc1 = gp.predict(g["Xt"], g["yt"], with_scores=True)
        check_predictive(res.mu[q], res.var[q], {s: res.scores[s][q] for s in SCORES}, mu, var, sc1)
        for o in OBJ5:
            assert close(res.objectives[o][q], fit[o]), (q, o)


# ---------------------------------------------------------------------- 7. failure isolation
def test_failed_problems_touch_no_other(gpu_ctx):
    """Problem 1: rows 0 and 1 identical, log sf² = 0, log σ² = −800 (σ² underflows to 0), so its
    second pivot is exactly 0; problem 2: a NaN in θ.  Both end with info > 0, NaN outputs and
    no step done; the call succeeds; problems 0 and 3 keep every bit."""
    import gpscore
    X, y, Xt, yt, th = small_problems(4, n=16, d=2)
    X[1, 1] = X[1, 0]
    th[1] = [0.0, 0.2, -800.0]
    th[2, 1] = np.nan
    good = [0, 3]
    kw = dict(lr=0.05, itr=3, ctx=gpu_ctx)
    res = gpscore.train_batch(X, y, th, "loo_crps", Xt=Xt, yt=yt, **kw)
    ref = gpscore.train_batch(X[good], y[good], th[good], "loo_crps", Xt=Xt[good], yt=yt[good], **kw)
    assert res.info[1] == 2 and res.info[2] > 0 and not res.info[good].any()
    assert list(res.steps_done) == [3, 0, 0, 3]
    fr, fref = result_fields(res), result_fields(ref)
    for k, v in fr.items():
        assert same_bits(v[good], fref[k]), k
        if k not in ("info", "steps_done", "theta"):
            assert np.isnan(v[1]).all() and np.isnan(v[2]).all(), k
    assert not np.isnan(fref["mu"]).any() and not np.isnan(fref["thetas"]).any()
    assert same_bits(res.theta[1], th[1])  # a failed problem keeps the θ it stopped at
    for obj in OBJS:
        vals, grads, objs, info = gpscore.value_and_grad_batch(X, y, th, obj, ctx=gpu_ctx)
        v0, g0, o0, i0 = gpscore.value_and_grad_batch(X[good], y[good], th[good], obj, ctx=gpu_ctx)
        assert info[1] == 2 and info[2] > 0 and not info[good].any() and not i0.any()
        assert same_bits(vals[good], v0) and same_bits(grads[good], g0)
        assert np.isnan(vals[[1, 2]]).all() and np.isnan(grads[[1, 2]]).all()
        for k in OBJ5:
            assert same_bits(objs[k][good], o0[k]) and np.isnan(objs[k][[1, 2]]).all(), k


# ------------------------------------------------- 8. batch size and position change no bit
def test_batch_size_and_position_change_no_bit(gpu_ctx):
    import gpscore
    B = 2 * CUS + 3  # more workgroups than the chip holds at once (one per CU: the LDS)
    X, y, Xt, yt, th = small_problems(B)
    for a in (X, y, Xt, yt, th):
        a[B - 1] = a[0]
    kw = dict(lr=0.05, itr=3, ctx=gpu_ctx)
    alone = gpscore.train_batch(X[:1], y[:1], th[:1], "loo_crps", Xt=Xt[:1], yt=yt[:1], **kw)
    full = gpscore.train_batch(X, y, th, "loo_crps", Xt=Xt, yt=yt, **kw)
    again = gpscore.train_batch(X, y, th, "loo_crps", Xt=Xt, yt=yt, **kw)
    assert not full.info.any() and list(full.steps_done) == [3] * B
    fa, ff, fg = result_fields(alone), result_fields(full), result_fields(again)
    for k in fa:
        assert same_bits(fa[k][0], ff[k][0]), k
        assert same_bits(fa[k][0], ff[k][B - 1]), k
        assert same_bits(ff[k], fg[k]), k
    assert not same_bits(ff["theta"][0], ff["theta"][1])  # the problems are distinct
    v1 = gpscore.value_and_grad_batch(X[:1], y[:1], th[:1], "loo_logs", ctx=gpu_ctx)
    vB = gpscore.value_and_grad_batch(X, y, th, "loo_logs", ctx=gpu_ctx)
    assert same_bits(v1[1][0], vB[1][0]) and same_bits(v1[1][0], vB[1][B - 1])
    assert same_bits(v1[0][0], vB[0][B - 1])


# ------------------------------------------------------- 9. the rest of the context is untouched
def test_batch_leaves_resident_fit_alone(gp, gpu_ctx):
    import gpscore
    g = load_golden("full_n64_d8")
    gp.fit(g["X"], g["y"], theta_of(g)[0])
    before = gp.predict(g["Xt"], g["yt"], with_scores=True)
    X, y, Xt, yt, th = small_problems(6)
    gpscore.train_batch(X, y, th, "nlml", lr=1e-3, itr=2, Xt=Xt, yt=yt, ctx=gpu_ctx)
    gpscore.value_and_grad_batch(X, y, th, "loo_crps", ctx=gpu_ctx)
    after = gp.predict(with_scores=True)
    assert same_bits(before[0], after[0]) and same_bits(before[1], after[1])
    assert before[2] == after[2]


def test_batch_launches_have_their_own_profiling_tags(gpu_ctx):
    import gpscore
    X, y, Xt, yt, th = small_problems(2)
    gpu_ctx.prof(True)
    gpscore.train_batch(X, y, th, "nlml", lr=1e-3, itr=70, ctx=gpu_ctx)  # two launches, one tag
    gpscore.value_and_grad_batch(X, y, th, "nlml", ctx=gpu_ctx)
    rep = gpu_ctx.prof_collect()
    gpu_ctx.prof(False)
    assert rep["batch_train"]["count"] == 1 and rep["batch_grad"]["count"] == 1, rep
    assert rep["batch_train"]["ms"] > 0


# --------------------------------------------------------------------------- 10. the harness
def test_run_simple_matches_run_method(gp, gpu_ctx):
    """run_simple on the two torch-drawn SD data sets, five steps a method: the metrics of
    GP.train + GP.predict (experiment.run_method, stale noise included) for each."""
    from gpscore import experiment as E
    gs = [load_golden("sd_j0_init"), load_golden("sd_j1_init")]
    data = [{"train_x": g["X"], "train_y": g["y"], "test_x": g["Xt"], "test_y": g["yt"]} for g in gs]
    out = E.run_simple(TT=2, datasets=data, itr=5, ctx=gpu_ctx)
    assert set(out) == set(E.SD_METHODS)
    for name, meth in E.SD_METHODS.items():
        for j, dd in enumerate(data):
            r = E.run_method(gp, dd, meth, None, itr=5)
            assert not r["failed"]
            for k in E.METRICS:
                assert out[name][k].shape == (2,)
                assert close(out[name][k][j], r[k]), (name, j, k, out[name][k][j], r[k])
