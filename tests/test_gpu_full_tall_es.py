"""Batches of full GPs of up to 512 rows on the block-LOO energy score (gps_full_es_grad_tall /
gps_full_es_train_tall) against the reference's autograd goldens, the oracle at the
fold, tile and draw-padding edges, the resident path (GP.block_loo, GP.train, GP.fit + GP.predict)
and their own invariants: how itr is split, the batch size and a problem's position change no bit,
a failed problem touches no other, the rest of the context is left alone.  Follows
tests/test_gpu_full_tall_block.py and reuses its helpers.  Runs on the GPU box.

Tolerances: 1e-9·max(1, |ref|) on values and nrel <= 1e-8 on gradients, what tests/test_gpu_blockloo.py
holds the resident ES path to; at the edges max(those, 30 × the oracle's own floor under a 1e-15
relative perturbation of X and y), with 30 × floor <= the tolerance asserted on the oracle alone;
1e-8 on the predictive and its scores.  The paths sum in different orders, so they are compared at
those tolerances, never bitwise.  The info codes n + k and 2n + 1 + f cannot be reached with honest
inputs and are not tested."""
import functools

import numpy as np
import pytest

import gp_oracle as O
from conftest import load_golden, nrel, theta_of
from test_gpu_batch import OBJ5, SCORES, close, result_fields, row_of, same_bits, tup_of
from test_gpu_full_tall import TOL8, problems

pytestmark = pytest.mark.gpu

VTOL, GTOL = 1e-9, 1e-8


@pytest.fixture(scope="module")
def gp(gpu_ctx):
    import gpscore
    return gpscore.GP(ctx=gpu_ctx)


def draws_for(B, sets, n, nfold, S, seed):
    from gpscore.gp import es_draws
    rng = np.random.default_rng(seed)
    return np.stack([np.stack([es_draws(n, nfold, S, rng) for _ in range(sets)]) for _ in range(B)])


def oracle(X, y, row, draws, S, nfold=4, beta=1.0, kind="ARD"):
    es = {"draws": draws, "S": S, "beta": beta}
    return O.fast_full_blockloo(X, y, *tup_of(row), "es", kind=kind, nfold=nfold, want_grad=True,
                                es=es)


# ------------------------------------------------------------ 1. the reference's autograd
@pytest.mark.parametrize("name", ["blockes_full_n64", "blockes_full_n200"])
def test_es_vs_autograd_golden(gpu_ctx, name):
    import gpscore
    g = load_golden(name)
    th, kern = theta_of(g)
    assert kern != "rbf"
    S, row, n = int(g["num_sim"]), row_of(th), g["X"].shape[0]
    X, y = np.stack([g["X"]] * 3), np.stack([g["y"]] * 3)
    rows = np.stack([row - 0.05, row, row + 0.05])
    draws = draws_for(3, 1, n, 4, S, 11)[:, 0]
    draws[1] = np.ravel(g["draws_es"])
    vals, grads, folds, objs, info = gpscore.es_value_and_grad_tall(
        X, y, rows, nfold=4, num_sim=S, draws=draws, ctx=gpu_ctx)
    assert not info.any(), info
    ref = float(g["value_es"])
    print(name, "value err %.3g grad nrel %.3g" % (abs(vals[1] - ref) / max(1.0, abs(ref)),
                                                  nrel(grads[1], g["grad_es"])))
    assert abs(vals[1] - ref) <= VTOL * max(1.0, abs(ref)), (vals[1], ref)
    assert nrel(grads[1], g["grad_es"]) <= GTOL, (grads[1], g["grad_es"])
    assert folds.shape == (3, 4)
    assert np.all(np.abs(folds.sum(1) - vals) <= 1e-12 * np.maximum(1.0, np.abs(vals)))
    for q in (0, 2):  # the neighbours against the oracle
        ov, og = oracle(X[q], y[q], rows[q], draws[q], S)
        assert close(vals[q], ov, VTOL), (q, vals[q], ov)
        assert nrel(grads[q], og) <= GTOL, (q, grads[q], og)
    for q in range(3):
        fit = O.fast_full_fit(X[q], y[q], *tup_of(rows[q]), "ARD")
        for k in OBJ5:
            assert close(objs[k][q], fit[k]), (q, k, objs[k][q], fit[k])


# ------------------------------- 2. the oracle at the fold, tile and draw-padding edges
EDGES = [(5, 1, 4, 2), (4, 2, 4, 3), (65, 3, 2, 17), (129, 8, 2, 16), (130, 2, 3, 63),
         (257, 8, 4, 64), (509, 8, 4, 15), (512, 16, 4, 65), (500, 8, 4, 300)]
EDGE_CASES = [(n, d, k, S, 1.0, False) for n, d, k, S in EDGES] + [(130, 2, 3, 63, 1.5, False),
                                                                  (129, 8, 2, 16, 1.0, True)]


def edge_problem(n, d, nfold, S, rbf):
    """Data and θ as tests/test_gpu_blockloo.py::test_es_vs_oracle builds them; two problems, the
    second at a shifted θ with its own draws."""
    from gpscore.gp import es_draws
    rng = np.random.default_rng(n + S)
    X = rng.standard_normal((n, d))
    y = np.sin(X.sum(1)) + 0.1 * rng.standard_normal(n)
    ell = np.array([np.log(1.3)]) if rbf else np.log(np.linspace(0.8, 2.0, d))
    row = np.concatenate([[0.1], ell, [np.log(0.05)]])
    draws = np.stack([es_draws(n, nfold, S, rng) for _ in range(2)])
    return np.stack([X, X]), np.stack([y, y]), np.stack([row, row + 0.03]), draws


@functools.lru_cache(maxsize=None)
def edge_oracle(n, d, nfold, S, beta, rbf):
    """Per problem (value, grad) and the case's (value, gradient) tolerances from the oracle's own
    floor: the oracle on X and y perturbed by 1e-15 relative."""
    X, y, th, draws = edge_problem(n, d, nfold, S, rbf)
    kind = "rbf" if rbf else "ARD"
    refs = [oracle(X[q], y[q], th[q], draws[q], S, nfold, beta, kind) for q in range(2)]
    r = np.random.default_rng(1)
    Xp = X[0] * (1 + 1e-15 * r.standard_normal(X[0].shape))
    yp = y[0] * (1 + 1e-15 * r.standard_normal(y[0].shape))
    pv, pg = oracle(Xp, yp, th[0], draws[0], S, nfold, beta, kind)
    fv, fg = abs(pv - refs[0][0]) / max(1.0, abs(refs[0][0])), nrel(pg, refs[0][1])
    assert 30 * fv <= VTOL and 30 * fg <= GTOL, (n, d, nfold, S, beta, rbf, fv, fg)  # the cap
    return refs, max(VTOL, 30 * fv), max(GTOL, 30 * fg)


@pytest.mark.parametrize("n,d,nfold,S,beta,rbf", EDGE_CASES)
def test_es_vs_oracle_edges(gpu_ctx, n, d, nfold, S, beta, rbf):
    import gpscore
    X, y, th, draws = edge_problem(n, d, nfold, S, rbf)
    refs, vtol, gtol = edge_oracle(n, d, nfold, S, beta, rbf)  # asserts the cap first
    vals, grads, folds, objs, info = gpscore.es_value_and_grad_tall(
        X, y, th, nfold=nfold, num_sim=S, beta=beta, draws=draws, rbf=rbf, ctx=gpu_ctx)
    assert not info.any(), info
    for q, (ov, og) in enumerate(refs):
        ev, eg = abs(vals[q] - ov) / max(1.0, abs(ov)), nrel(grads[q], og)
        print("es edge", n, d, nfold, S, beta, rbf, q, "value %.3g grad %.3g" % (ev, eg))
        assert ev <= vtol, (q, "value", vals[q], ov, vtol)
        assert eg <= gtol, (q, "grad", grads[q], og, gtol)
    assert np.all(np.abs(folds.sum(1) - vals) <= 1e-12 * np.maximum(1.0, np.abs(vals)))


# ----------------------------------------------------------------- 3. the resident path
@pytest.mark.parametrize("n", [129, 500])
def test_es_vs_resident_path(gp, gpu_ctx, n):
    import gpscore
    S = 32
    X, y, _, _, th = problems(2, n)
    draws = draws_for(2, 1, n, 4, S, n)[:, 0]
    vals, grads, folds, objs, info = gpscore.es_value_and_grad_tall(
        X, y, th, nfold=4, num_sim=S, draws=draws, ctx=gpu_ctx)
    assert not info.any()
    for q in range(2):
        gp.set_data(X[q], y[q], kind="full")
        v1, g1, f1 = gp.block_loo(tup_of(th[q]), "es", 4, grad=True, num_sim=S, draws=draws[q])
        assert close(vals[q], v1, VTOL), (q, vals[q], v1)
        assert nrel(grads[q], g1) <= GTOL, (q, grads[q], g1)
        assert nrel(folds[q], f1) <= GTOL, (q, folds[q], f1)


# ----------------------------------------------------------------------------- 4. training
def test_es_train_matches_oracle_and_gp_train(gp, gpu_ctx):
    """Three SGD steps with S = 32 at the scripts' lr on the n = 64 golden's data from two starts,
    against the oracle loop replaying the draws and against GP.train fed the same generator."""
    import gpscore
    from gpscore.gp import es_draws
    g = load_golden("blockes_full_n64")
    row = row_of(theta_of(g)[0])
    n, lr, S, itr = g["X"].shape[0], 0.1, 32, 3
    X, y = np.stack([g["X"]] * 2), np.stack([g["y"]] * 2)
    th = np.stack([row, row + 0.1])
    res = gpscore.es_train_tall(X, y, th, nfold=4, num_sim=S, lr=lr, itr=itr,
                                rng=np.random.default_rng(3), ctx=gpu_ctx)
    assert not res.info.any() and list(res.steps_done) == [itr, itr]
    rng, rng2 = np.random.default_rng(3), np.random.default_rng(3)
    for q in range(2):
        t = th[q].copy()
        for i in range(itr):
            v, gr = oracle(X[q], y[q], t, es_draws(n, 4, S, rng), S)
            assert close(res.series["objective"][q, i], v, VTOL), (q, i)
            t = t - lr * gr
            assert nrel(res.series["theta"][q, i], t) <= GTOL, (q, i)
        assert same_bits(res.theta[q], res.series["theta"][q, -1])
        theta, series = gp.train(tup_of(th[q]), "es", lr=lr, itr=itr, X=X[q], y=y[q],
                                 block_kw={"num_sim": S, "rng": rng2})
        for i in range(itr):
            assert close(res.series["objective"][q, i], series["objective"][i], VTOL), (q, i)
            assert nrel(res.series["theta"][q, i], series["theta"][i]) <= GTOL, (q, i)


def test_es_draw_sets(gpu_ctx):
    """draw_sets = 1: step i's value is es_value_and_grad_tall at the θ after step i − 1 with that
    one set, to the last bit; draw_sets = 2 cycles: steps 0 and 2 read set 0, step 1 set 1."""
    import gpscore
    S, n = 16, 130
    X, y, _, _, th = problems(2, n, d=3)
    kw = dict(nfold=3, num_sim=S, ctx=gpu_ctx)
    d2 = draws_for(2, 2, n, 3, S, 5)
    one = gpscore.es_train_tall(X, y, th, lr=0.1, itr=3, draws=d2[:, :1], draw_sets=1, **kw)
    two = gpscore.es_train_tall(X, y, th, lr=0.1, itr=3, draws=d2, draw_sets=2, **kw)
    assert not one.info.any() and not two.info.any()
    for res, sets in ((one, (0, 0, 0)), (two, (0, 1, 0))):
        at = th
        for i, k in enumerate(sets):
            vals = gpscore.es_value_and_grad_tall(X, y, at, draws=d2[:, k], **kw)[0]
            assert same_bits(res.series["objective"][:, i], vals), (sets, i)
            at = res.series["theta"][:, i]
    assert same_bits(one.series["theta"][:, 0], two.series["theta"][:, 0])
    assert not same_bits(one.series["theta"][:, 1], two.series["theta"][:, 1])


def test_es_split_of_itr_changes_no_bit(gpu_ctx):
    """One step runs per launch sequence, so there is one split of itr inside a call; itr = 3
    equals, bitwise, three itr = 1 calls chained through θ with the same sets."""
    import gpscore
    S, n = 16, 130
    X, y, Xt, yt, th = problems(3, n, d=3, nt=9)
    dr = draws_for(3, 3, n, 4, S, 9)
    kw = dict(nfold=4, num_sim=S, lr=0.1, Xt=Xt, yt=yt, ctx=gpu_ctx)
    whole = gpscore.es_train_tall(X, y, th, itr=3, draws=dr, **kw)
    assert not whole.info.any() and list(whole.steps_done) == [3] * 3
    at, last = th, None
    for i in range(3):
        last = gpscore.es_train_tall(X, y, at, itr=1, draws=dr[:, i:i + 1], **kw)
        assert same_bits(whole.series["objective"][:, i], last.series["objective"][:, 0]), i
        assert same_bits(whole.series["theta"][:, i], last.series["theta"][:, 0]), i
        at = last.theta
    assert same_bits(whole.theta, last.theta)
    # (without stale_noise the final pass is a function of the final θ alone)
    fw, fl = result_fields(whole), result_fields(last)
    for k in fw:
        if k not in ("values", "thetas", "steps_done"):
            assert same_bits(fw[k], fl[k]), k
    assert not same_bits(whole.series["theta"][:, 0], whole.series["theta"][:, -1])


# ------------------------------------------------- 5. batch size and position change no bit
def test_es_batch_size_and_position_change_no_bit(gpu_ctx):
    import gpscore
    B, n, S = 300, 500, 16  # more fold workgroups than the chip has compute units
    X1, y1, Xt1, yt1, th1 = problems(3, n, nt=9)
    idx = np.arange(B) % 3
    idx[B - 1] = 0
    X, y, Xt, yt, th = X1[idx], y1[idx], Xt1[idx], yt1[idx], th1[idx]
    d3 = draws_for(3, 2, n, 4, S, 13)
    dr = d3[idx]
    kw = dict(nfold=4, num_sim=S, lr=0.1, itr=2, ctx=gpu_ctx)
    alone = gpscore.es_train_tall(X[:1], y[:1], th[:1], draws=dr[:1], Xt=Xt[:1], yt=yt[:1], **kw)
    full = gpscore.es_train_tall(X, y, th, draws=dr, Xt=Xt, yt=yt, **kw)
    assert not full.info.any() and list(full.steps_done) == [2] * B
    fa, ff = result_fields(alone), result_fields(full)
    for k in fa:
        assert same_bits(fa[k][0], ff[k][0]), k
        assert same_bits(fa[k][0], ff[k][B - 1]), k
        assert same_bits(ff[k][1], ff[k][B - 2]), k  # (B − 2) mod 3 = 1
    assert not same_bits(ff["theta"][0], ff["theta"][1])  # the problems are distinct
    v1 = gpscore.es_value_and_grad_tall(X[:1], y[:1], th[:1], nfold=4, num_sim=S,
                                        draws=dr[:1, 0], ctx=gpu_ctx)
    vB = gpscore.es_value_and_grad_tall(X, y, th, nfold=4, num_sim=S, draws=dr[:, 0], ctx=gpu_ctx)
    for a, b in zip(v1[:3], vB[:3]):
        assert same_bits(a[0], b[0]) and same_bits(a[0], b[B - 1])


# ----------------------------------------------------------------------------- 6. final pass
@pytest.mark.parametrize("stale", [True, False])
def test_es_final_pass_vs_fit_predict(gp, gpu_ctx, stale):
    import gpscore
    nt = 65
    X, y, Xt, yt, th = problems(2, 200, nt=nt)
    res = gpscore.es_train_tall(X, y, th, nfold=4, num_sim=16, lr=0.1, itr=2, Xt=Xt, yt=yt,
                                rng=np.random.default_rng(1), stale_noise=stale, ctx=gpu_ctx)
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


# ---------------------------------------------------------------------- 7. failure isolation
def duplicate_rows(X, y, th, q):
    """Problem q gets two equal leading rows, sf² = e⁰ = 1 and a noise of e⁻⁸⁰: A's first 2×2 minor
    is [[1, 1], [1, 1]] exactly, so the second pivot is 1 − 1·1 = 0, which is not > 0."""
    X[q, 1] = X[q, 0]
    th[q, 0] = 0.0
    th[q, -1] = -80.0


def test_es_failed_problem_touches_no_other(gpu_ctx):
    import gpscore
    n, S = 130, 16
    X, y, Xt, yt, th = problems(4, n, d=3, nt=9)
    duplicate_rows(X, y, th, 1)
    good = [0, 2, 3]
    dr = draws_for(4, 2, n, 4, S, 17)
    kw = dict(nfold=4, num_sim=S, lr=0.1, itr=2, ctx=gpu_ctx)
    res = gpscore.es_train_tall(X, y, th, draws=dr, Xt=Xt, yt=yt, **kw)
    ref = gpscore.es_train_tall(X[good], y[good], th[good], draws=dr[good], Xt=Xt[good],
                                yt=yt[good], **kw)
    assert 1 <= res.info[1] <= n and not res.info[good].any(), res.info
    assert list(res.steps_done) == [2, 0, 2, 2]
    fr, fref = result_fields(res), result_fields(ref)
    for k, v in fr.items():
        assert same_bits(v[good], fref[k]), k
        if k not in ("info", "steps_done", "theta"):
            assert np.isnan(v[1]).all(), k
    assert same_bits(res.theta[1], th[1])
    vals, grads, folds, objs, info = gpscore.es_value_and_grad_tall(
        X, y, th, nfold=4, num_sim=S, draws=dr[:, 0], ctx=gpu_ctx)
    v0, g0, f0, o0, i0 = gpscore.es_value_and_grad_tall(
        X[good], y[good], th[good], nfold=4, num_sim=S, draws=dr[good, 0], ctx=gpu_ctx)
    assert 1 <= info[1] <= n and not info[good].any() and not i0.any()
    assert same_bits(vals[good], v0) and same_bits(grads[good], g0) and same_bits(folds[good], f0)
    assert np.isnan(vals[1]) and np.isnan(grads[1]).all() and np.isnan(folds[1]).all()
    for k in OBJ5:
        assert same_bits(objs[k][good], o0[k]) and np.isnan(objs[k][1]), k


def test_es_failure_in_a_later_step(gpu_ctx):
    """Problem 1 has two equal rows; a step of 1e6 throws θ far outside the representable kernels
    after the first update, and a forward within the next two steps meets a pivot of A that is not
    > 0 (info in 1..n), as in tests/test_gpu_full_tall_block.py.  The problem stops there:
    steps_done counts the completed steps, theta_out is the θ the failing forward was at, the rest
    of its series and its final outputs are NaN."""
    import gpscore
    n, S = 130, 16
    X, y, Xt, yt, th = problems(2, n, d=3, nt=9)
    X[1, 7] = X[1, 3]
    dr = draws_for(2, 5, n, 4, S, 19)
    kw = dict(nfold=4, num_sim=S, itr=5, ctx=gpu_ctx)
    res = gpscore.es_train_tall(X, y, th, lr=1e6, draws=dr, Xt=Xt, yt=yt, **kw)
    print("later-step failure: info", res.info, "steps_done", res.steps_done)
    assert res.info.all() and (res.info <= n).all(), res.info
    for q in range(2):
        done = int(res.steps_done[q])
        assert 1 <= done <= 3, done  # the first forward is at a sane θ
        assert same_bits(res.theta[q], res.series["theta"][q, done - 1])
        assert not np.isnan(res.series["objective"][q, 0])
        assert np.isnan(res.series["objective"][q, done:]).all()
        assert np.isnan(res.series["theta"][q, done:]).all()
        assert np.isnan(res.mu[q]).all() and np.isnan(res.objectives["nlml"][q])
        for k in SCORES:
            assert np.isnan(res.scores[k][q]), k


# ------------------------------------------------------ 8. the rest of the context is untouched
def test_es_leaves_resident_fit_alone(gp, gpu_ctx):
    import gpscore
    g = load_golden("full_n64_d8")
    gp.fit(g["X"], g["y"], theta_of(g)[0])
    before = gp.predict(g["Xt"], g["yt"], with_scores=True)
    X, y, Xt, yt, th = problems(3, 200, nt=70)
    gpscore.es_train_tall(X, y, th, num_sim=16, itr=2, Xt=Xt, yt=yt, rng=np.random.default_rng(2),
                          ctx=gpu_ctx)
    gpscore.es_value_and_grad_tall(X, y, th, num_sim=16, rng=np.random.default_rng(2), ctx=gpu_ctx)
    after = gp.predict(with_scores=True)
    assert same_bits(before[0], after[0]) and same_bits(before[1], after[1])
    assert before[2] == after[2]


# ------------------------------------------------------------------------ 9. profiling tags
def test_es_launches_have_their_own_profiling_tags(gpu_ctx):
    import gpscore
    X, y, _, _, th = problems(2, 130, d=3)
    gpu_ctx.prof(True)
    gpscore.es_train_tall(X, y, th, num_sim=16, itr=2, rng=np.random.default_rng(2), ctx=gpu_ctx)
    gpscore.es_value_and_grad_tall(X, y, th, num_sim=16, rng=np.random.default_rng(2), ctx=gpu_ctx)
    rep = gpu_ctx.prof_collect()
    gpu_ctx.prof(False)
    assert rep["batch_full_tall_es_train"]["count"] == 1, rep
    assert rep["batch_full_tall_es_grad"]["count"] == 1, rep
    assert rep["batch_full_tall_es_train"]["ms"] > 0
    assert "batch_full_tall_block_train" not in rep and "batch_full_tall_train" not in rep


# ------------------------------------------------------------------------ 10. C-ABI refusals
B_, N_, D_, NT_, ITR_, S_ = 2, 4, 2, 3, 2, 3
ENTRIES = {"gps_full_es_grad_tall": False, "gps_full_es_train_tall": True}
NULL_ARG = "NULL argument"
NFOLD = "batch: nfold must be in 2..32 and at most n"
NSIM = "batch: num_sim must be in 2..512"
BETA = "beta must be in (0, 2]"
FOLD = ("batch: an energy-score fold holds at most 128 rows (ceil(n / nfold) <= 128: a fold's "
        "O(b^3) square-root work has to fit one launch of ~20 ms), use more folds")
CASES = [("X", None, NULL_ARG, "all"),
         ("theta", None, NULL_ARG, "all"),
         ("draws", None, NULL_ARG, "all"),
         ("value", None, NULL_ARG, "grad"),
         ("grad", None, NULL_ARG, "grad"),
         ("theta_out", None, NULL_ARG, "train"),
         ("kind", 7, "kind must be GPS_ARD or GPS_RBF", "all"),
         ("nfold", 1, NFOLD, "all"),
         ("nfold", 33, NFOLD, "all"),
         ("nfold", N_ + 1, NFOLD, "all"),
         ("num_sim", 1, NSIM, "all"),
         ("num_sim", 513, NSIM, "all"),
         ("beta", 0.0, BETA, "all"),
         ("beta", 2.5, BETA, "all"),
         ("nprob", 0, "batch: nprob must be in 1..2^20", "all"),
         ("n", 513, "batch: n must be in 1..512", "all"),
         ("n", 300, FOLD, "all"),
         ("d", 17, "batch: d must be in 1..16", "all"),
         ("n_ell", 3, "n_ell must be 1 or d", "all"),
         ("itr", -1, "batch: itr must be in 0..2^20", "train"),
         ("lr", float("inf"), "batch: lr must be finite", "train"),
         ("nt", -1, "batch: nt must be in 0..2^24", "train"),
         ("flags", 2, "unknown batch flag", "train"),
         ("draw_sets", 0, "batch: draw_sets must be at least 1", "train"),
         ("draw_sets", ITR_ + 1, "batch: draw_sets must be at most max(itr, 1)", "train")]
PARAMS = [pytest.param(entry, arg, bad, msg, id=f"{entry}-{arg}={bad}")
          for entry, train in ENTRIES.items()
          for arg, bad, msg, where in CASES
          if where == "all" or (where == "train") == train]


def arguments(train):
    """The entry's arguments by name, in the order of include/gpscore.h, all valid."""
    rng = np.random.default_rng(7)
    X = rng.normal(size=(B_, N_, D_))
    a = dict(kind=0, nfold=2, num_sim=S_, beta=1.0, nprob=B_, X=X, y=np.sin(X.sum(axis=2)), n=N_,
             d=D_, theta=np.tile([0.0, 0.1, -0.1, -2.0], (B_, 1)), n_ell=D_)
    if train:
        Xt = rng.normal(size=(B_, NT_, D_))
        a.update(itr=ITR_, lr=0.01, Xt=Xt, yt=np.sin(Xt.sum(axis=2)), nt=NT_, flags=0,
                 draws=rng.normal(size=(B_, ITR_, 2 * S_ * N_)), draw_sets=ITR_,
                 theta_out=np.zeros((B_, 2 + D_)), values=np.zeros((B_, ITR_)),
                 thetas=np.zeros((B_, ITR_, 2 + D_)), obj=np.zeros((B_, 5)),
                 mu=np.zeros((B_, NT_)), var=np.zeros((B_, NT_)), sc=np.zeros((B_, 6)),
                 info=np.full(B_, -1, np.int32), steps_done=np.full(B_, -1, np.int32))
    else:
        a.update(draws=rng.normal(size=(B_, 2 * S_ * N_)), value=np.zeros(B_),
                 fold_values=np.zeros((B_, 2)), obj=np.zeros((B_, 5)),
                 grad=np.zeros((B_, 2 + D_)), info=np.full(B_, -1, np.int32))
    return a


@pytest.mark.parametrize("entry,arg,bad,msg", PARAMS)
def test_es_refusal_and_recovery(gpu_ctx, entry, arg, bad, msg):
    """Every refusal comes before anything is read, so the arrays may be too small for the bad
    size; the same context runs a valid call straight away."""
    from gpscore import GpsError
    from test_gpu_batch_refusals import positional
    train = ENTRIES[entry]
    a = arguments(train)
    assert arg in a
    a[arg] = bad
    with pytest.raises(GpsError) as e:
        gpu_ctx.call(entry, *positional(a))
    assert str(e.value) == f"{entry} failed (-1): {msg}"
    ok = arguments(train)
    gpu_ctx.call(entry, *positional(ok))
    assert (ok["info"] == 0).all()
    assert np.isfinite(ok["obj"]).all() and (ok["obj"] != 0).any()
    if train:
        assert (ok["steps_done"] == ITR_).all()
        assert np.isfinite(ok["theta_out"]).all() and np.isfinite(ok["sc"]).all()
    else:
        assert np.isfinite(ok["grad"]).all() and (ok["grad"] != 0).any()
        assert np.isfinite(ok["value"]).all() and np.isfinite(ok["fold_values"]).all()


def test_es_too_many_draws_are_refused(gpu_ctx):
    """B = 256 with 25 sets of 300 draws at n = 500 is over the 8 GiB a call may take: refused with
    the batch calls' message before anything is read (the arrays here are tiny)."""
    from gpscore import GpsError
    from test_gpu_batch_refusals import positional
    a = arguments(True)
    a.update(nprob=256, n=500, nfold=4, num_sim=300, itr=25, draw_sets=25, d=D_)
    with pytest.raises(GpsError) as e:
        gpu_ctx.call("gps_full_es_train_tall", *positional(a))
    assert str(e.value) == ("gps_full_es_train_tall failed (-1): batch: more than 8 GiB of inputs or "
                            "outputs, split the batch")


# --------------------------------------------------------------------------- 11. the harness
def test_run_full_es_batch_matches_run(gpu_ctx):
    """run_full_es_batch against run(kind="full") on synthetic sheets: TT = 2, three ES steps with
    16 draws a fold, the same seed: the same problems and draws, metrics at 1e-8."""
    from gpscore import experiment as E
    sheets = E.synthetic_sheets(5, n_pool=2000, n_test=500)
    methods = {"es": E.KF_METHODS["es"]}
    out = E.run_full_es_batch(sheets, TT=2, itr=3, seed=7, num_sim=16, ctx=gpu_ctx)
    ref = E.run(sheets, TT=2, methods=methods, kind="full", itr=3, seed=7, num_sim=16, ctx=gpu_ctx)
    assert list(out) == ["es"] and not out["es"]["failed"].any()
    assert out["es"]["theta"].shape == (2, 10)
    for k in E.METRICS:
        for j in range(2):
            assert close(out["es"][k][j], ref["es"][k][j], TOL8), (k, j, out["es"][k][j],
                                                                   ref["es"][k][j])
