"""Batches of tall FITC GPs on the block-LOO DSS / KC objectives on the GPU
(gps_fitc_blockloo_grad_tall / gps_fitc_blockloo_train_tall): one workgroup per
problem, n up to 2048, the folds in low rank — K20's dss and kc fits (n = 500, d = 8, m = 20, four
folds).  The plan of test_gpu_fitc_tall.py, whose generators and helpers are reused:

 1. the reference's autograd gradients (block_fitc_n500_m20, block_fitc_n64_m6), each as problem 1
    of three whose neighbours (θ ± 0.05) are oracle-checked; fold values; the five objectives;
 2. the oracle (fast_fitc_blockloo) at the fold and chunk edges: fold boundaries inside and on a
    chunk, folds shorter than a chunk, of one row, of unequal length, spanning eight chunks, m
    larger than a fold; m = 1 / 5 / 20 / 32; d = 1 / 8 / 16;
 3. nfold = n against the pointwise tall kernel: DSS = n·LOO-LogS, KC = n·LOO-CRPS;
 4. the resident path GP.block_loo, never required to be bitwise;
 5. five SGD steps at K20's DSS and KC rates against the oracle loop and GP.train, two starts;
 6. the launch split is invisible bitwise;
 7. the final pass against GP.fit + GP.predict; itr = 0;
 8. a failed problem leaves its neighbours bitwise alone;
 9. results do not depend on the batch size or a problem's position, bitwise;
10. the context's resident fit and the pointwise tall path are left alone;
11. profiling tags;
12. the C-ABI's refusals, message by message, with a valid call after each;
13. experiment.run_fitc_blockloo_batch against experiment.run(kind="fitc").

Tolerances (fp64).  Against the autograd goldens test_gpu_blockloo.py's rule: value 1e-9 relative,
gradients 1e-9 normwise, 1e-6 where cond(K̃mm) >= 1e3.  Against the oracle on the edge grid tol =
max(1e-9, 30 × the case's conditioning floor) in the joint floor-at-1 metric (the oracle on X, Z
perturbed by 1e-15 relative), the hard cap 30 × floor <= 5e-9 asserted on the oracle alone before
the GPU is compared; measured on the CPU the worst floor of the grid is 3.5e-11 (n = 2048, nfold =
2, m = 32, d = 1, KC), so the cap never binds on the reference."""
import functools
import os
import re

import numpy as np
import pytest

import gp_oracle as O
from conftest import load_golden, nrel, theta_of
from test_gpu_fitc_batch import (FIVE, SCORES, close, edge_problem, joint_err, result_fields,
                                 row_of, same_bits, small_problems, th_of)

pytestmark = pytest.mark.gpu

OBJS = ("dss", "kc")
POINTWISE = {"dss": "loo_logs", "kc": "loo_crps"}
GOLDENS = ("block_fitc_n500_m20", "block_fitc_n64_m6")
CHUNK = 128  # kBatchFitcTallChunk


def steps_per_launch(n):
    """batch_fitc_tall_block_steps: max(1, 64 / kBatchFitcTallBlockDiv / ceil(n / 128))."""
    import gpscore
    src = os.path.join(os.path.dirname(os.path.dirname(gpscore.__file__)), "csrc", "gps_internal.h")
    div = int(re.search(r"kBatchFitcTallBlockDiv = (\d+);", open(src, encoding="utf-8").read())[1])
    return max(1, 64 // div // -(-n // CHUNK))


@pytest.fixture(scope="module")
def gp(gpu_ctx):
    import gpscore
    return gpscore.GP(ctx=gpu_ctx)


# --------------------------------------------------------------------- 1. autograd goldens
@functools.lru_cache(maxsize=None)
def golden_batch(name):
    g = load_golden(name)
    th, _ = theta_of(g)
    row = row_of(th)
    X, y, Z = (np.stack([g[k]] * 3) for k in ("X", "y", "Z"))
    rows = np.stack([row - 0.05, row, row + 0.05])
    return g, X, y, Z, rows


def oracle_fold_values(X, y, Z, th, obj, nfold):
    """block_loo on each single fold of fitc_fold_cov."""
    Kmm, Lm_inv, _ = O.fitc_shared(Z, *th[:2])
    part = O.fitc_partials(X, y, Z, Lm_inv, *th)
    K, lam = part["_Knm"], part["_lam"]
    _, _, c = O.fitc_finish_shared(Kmm, part["B"], part["b"])
    alpha = (y - K @ c) / lam
    folds = O.block_folds(y.size, nfold)
    cov = O.fitc_fold_cov(K, lam, Kmm, folds)
    return np.array([O.block_loo(lambda a, b: cov[(a, b)], alpha, y, [f], obj, cform=True)
                     for f in folds])


@pytest.mark.parametrize("name", GOLDENS)
@pytest.mark.parametrize("obj", OBJS)
def test_block_vs_autograd_golden(gpu_ctx, name, obj):
    import gpscore
    g, X, y, Z, rows = golden_batch(name)
    vals, grads, gz, fold, objs, info = gpscore.fitc_blockloo_value_and_grad_tall(
        X, y, Z, rows, obj, nfold=4, ctx=gpu_ctx)
    assert not info.any(), info
    assert fold.shape == (3, 4)
    Kmm, _, _ = O.fitc_shared(g["Z"], *th_of(rows[1])[:2])
    tol = 1e-9 if np.linalg.cond(Kmm) < 1e3 else 1e-6
    ref = float(g["value_" + obj])
    print(name, obj, "value", abs(vals[1] - ref) / max(1.0, abs(ref)), "grad",
          nrel(grads[1], g["grad_" + obj]), "gradZ", nrel(gz[1], g["gradZ_" + obj]), "tol", tol)
    assert abs(vals[1] - ref) <= 1e-9 * max(1.0, abs(ref)), (vals[1], ref)
    assert nrel(grads[1], g["grad_" + obj]) <= tol, (grads[1], g["grad_" + obj])
    assert nrel(gz[1], g["gradZ_" + obj]) <= tol
    for q in (0, 2):  # the neighbours, against the oracle
        ov, og, oz = O.fast_fitc_blockloo(g["X"], g["y"], g["Z"], *th_of(rows[q]), obj, 4, True)
        assert abs(vals[q] - ov) <= 1e-9 * max(1.0, abs(ov)), (q, vals[q], ov)
        assert nrel(grads[q], og) <= tol and nrel(gz[q], oz) <= tol, q
    for q in range(3):
        assert abs(fold[q].sum() - vals[q]) <= 1e-12 * max(1.0, abs(vals[q])), q
        fv = oracle_fold_values(g["X"], g["y"], g["Z"], th_of(rows[q]), obj, 4)
        assert nrel(fold[q], fv) <= 1e-9, (q, fold[q], fv)
        five = O.fast_fitc(g["X"], g["y"], g["X"][:2], g["y"][:2], g["Z"], *th_of(rows[q]))
        for k in FIVE:
            assert close(objs[k][q], five[k]), (q, k, objs[k][q], five[k])


# --------------------------------------------------------------------------- 2. oracle edges
FOLD_CASES = ((5, 4), (5, 5), (31, 31), (127, 4), (128, 4), (129, 4), (129, 3), (130, 2), (257, 4),
              (385, 3), (500, 4), (512, 4), (509, 32), (2048, 2), (2048, 4))
EDGE_M = (1, 5, 20, 32)
EDGE_D = ((1, False), (8, True), (16, True))
EDGE_CASES = [(n, nf, m, d, per) for n, nf in FOLD_CASES for m in EDGE_M for d, per in EDGE_D]


def nq_of(n):
    return 2 if n == 2048 else 5


@functools.lru_cache(maxsize=None)
def edge_batch(n, m, d, per):
    ps = [edge_problem(n, m, d, per, q) for q in range(nq_of(n))]
    return tuple(np.stack([p[k] for p in ps]) for k in range(4))


@functools.lru_cache(maxsize=None)
def edge_oracle(n, nfold, m, d, per, obj):
    """Per problem (value, grad, grad_Z, tol): the oracle and the case's tolerance from its
    conditioning floor (the oracle on inputs perturbed by 1e-15 relative, same metric)."""
    X, y, Z, rows = edge_batch(n, m, d, per)
    out = []
    for q in range(nq_of(n)):
        th = th_of(rows[q])
        ov, og, oz = O.fast_fitc_blockloo(X[q], y[q], Z[q], *th, obj, nfold, True)
        assert np.isfinite(ov) and np.isfinite(og).all() and np.isfinite(oz).all()
        r = np.random.default_rng(1)
        Xp = X[q] * (1 + 1e-15 * r.standard_normal(X[q].shape))
        Zp = Z[q] * (1 + 1e-15 * r.standard_normal(Z[q].shape))
        pv, pg, pz = O.fast_fitc_blockloo(Xp, y[q], Zp, *th, obj, nfold, True)
        floor = max(abs(pv - ov) / max(1.0, abs(ov)), joint_err(pg, pz, og, oz))
        assert 30 * floor <= 5e-9, (n, nfold, m, d, per, obj, q, floor)  # the cap, on the reference
        out.append((ov, og, oz, max(1e-9, 30 * floor)))
    return out


_edge_gpu = {}


def edge_gpu(ctx, n, nfold, m, d, per, obj):
    import gpscore
    key = (n, nfold, m, d, per, obj)
    if key not in _edge_gpu:
        X, y, Z, rows = edge_batch(n, m, d, per)
        _edge_gpu[key] = gpscore.fitc_blockloo_value_and_grad_tall(X, y, Z, rows, obj, nfold=nfold,
                                                                   ctx=ctx)
    return _edge_gpu[key]


@pytest.mark.parametrize("n,nfold,m,d,per", EDGE_CASES)
def test_block_vs_oracle_edges(gpu_ctx, n, nfold, m, d, per):
    worst = 0.0
    for obj in OBJS:
        refs = edge_oracle(n, nfold, m, d, per, obj)  # asserts the cap before the GPU is looked at
        vals, grads, gz, fold, objs, info = edge_gpu(gpu_ctx, n, nfold, m, d, per, obj)
        assert not info.any(), (obj, info)
        for q, (ov, og, oz, tol) in enumerate(refs):
            ev = abs(vals[q] - ov) / max(1.0, abs(ov))
            eg = joint_err(grads[q], gz[q], og, oz)
            worst = max(worst, ev / tol, eg / tol)
            assert ev <= tol, (obj, q, "value", vals[q], ov, tol)
            assert eg <= tol, (obj, q, "grad", eg, tol)
            assert abs(fold[q].sum() - vals[q]) <= 1e-12 * max(1.0, abs(vals[q])), (obj, q)
    print("edge", n, nfold, m, d, per, "worst error / tolerance %.3g" % worst)


# ---------------------------------------------------- 3. nfold = n against the pointwise kernel
@pytest.mark.parametrize("n,m,d", ((31, 5, 8), (32, 32, 1), (7, 20, 16)))
def test_one_row_folds_are_the_pointwise_objectives(gpu_ctx, n, m, d):
    import gpscore
    per = d > 1
    X, y, Z, rows = edge_batch(n, m, d, per)
    for obj in OBJS:
        tols = [o[3] for o in edge_oracle(n, n, m, d, per, obj)]
        vals, grads, gz, fold, objs, info = gpscore.fitc_blockloo_value_and_grad_tall(
            X, y, Z, rows, obj, nfold=n, ctx=gpu_ctx)
        pv, pg, pz, pobjs, pinfo = gpscore.fitc_value_and_grad_tall(X, y, Z, rows, POINTWISE[obj],
                                                                    ctx=gpu_ctx)
        assert not info.any() and not pinfo.any()
        for q in range(nq_of(n)):
            ev = abs(vals[q] - n * pv[q]) / max(1.0, abs(n * pv[q]))
            eg = joint_err(grads[q], gz[q], n * pg[q], n * pz[q])
            print("nfold = n", n, m, d, obj, q, "value", ev, "grad", eg, "tol", tols[q])
            assert ev <= tols[q], (obj, q, vals[q], n * pv[q])
            assert eg <= tols[q], (obj, q, eg, tols[q])


# ------------------------------------------------------------------ 4. against the resident path
@pytest.mark.parametrize("n,m", ((500, 20), (129, 5)))
def test_block_vs_resident_path(gp, gpu_ctx, n, m):
    d, per, nfold = 8, True, 4
    X, y, Z, rows = edge_batch(n, m, d, per)
    for obj in OBJS:
        vals, grads, gz, fold, objs, info = edge_gpu(gpu_ctx, n, nfold, m, d, per, obj)
        tols = [o[3] for o in edge_oracle(n, nfold, m, d, per, obj)]
        for q in range(nq_of(n)):
            gp.set_data(X[q], y[q], kind="fitc", Z=Z[q])
            rv, rg, rf, rz = gp.block_loo(th_of(rows[q]), obj, nfold=nfold, grad=True)
            ev = abs(vals[q] - rv) / max(1.0, abs(rv))
            eg = joint_err(grads[q], gz[q], rg, rz)
            assert ev <= tols[q], (obj, q, vals[q], rv)
            assert eg <= tols[q], (obj, q, eg, tols[q])
            assert nrel(fold[q], rf) <= max(1e-9, tols[q]), (obj, q, fold[q], rf)


# ------------------------------------------------------------------------------------ 5. SGD
K20_BLOCK_STEPS = (("dss", 1e-3, 1e-3), ("kc", 0.1, 0.1))
SGD_N = 300


def sgd_start(start):
    """(X, y, Z0, θ0 as a row): the first SGD_N rows of the K20-shaped golden with the golden's own
    θ and Z ("golden"), or scalar ℓ = noise = sf² = 1 in the scripts' parametrisation with N(0,1)
    inducing inputs, K20's DSS start ("ones").  Chosen on the CPU: the oracle loop stays positive
    definite for both methods from both."""
    g = load_golden("block_fitc_n500_m20")
    X, y = g["X"][:SGD_N], g["y"][:SGD_N]
    if start == "golden":
        return X, y, g["Z"], row_of(theta_of(g)[0])
    return X, y, np.random.default_rng(20).standard_normal((20, X.shape[1])), np.ones(3)


@pytest.mark.parametrize("obj,lr,lr_z", K20_BLOCK_STEPS)
@pytest.mark.parametrize("start", ("golden", "ones"))
def test_sgd_matches_oracle_and_gp_train(gp, gpu_ctx, obj, lr, lr_z, start):
    import gpscore
    X, y, Z0, t0 = sgd_start(start)
    res = gpscore.fitc_blockloo_train_tall(X[None], y[None], Z0[None], t0[None], obj, nfold=4,
                                           lr=lr, lr_z=lr_z, itr=5, ctx=gpu_ctx)
    assert res.info[0] == 0 and res.steps_done[0] == 5
    t, Z = t0.copy(), Z0.copy()
    for i in range(5):
        v, gr, gzo = O.fast_fitc_blockloo(X, y, Z, t[0], t[1:-1], t[-1], obj, 4, True)
        assert close(res.series["objective"][0, i], v), (i, res.series["objective"][0, i], v)
        t = t - lr * gr
        Z = Z - lr_z * gzo
        assert nrel(res.series["theta"][0, i], t) <= 1e-9, (i, res.series["theta"][0, i], t)
    assert nrel(res.Z[0], Z) <= 1e-9, (res.Z[0], Z)
    assert nrel(res.theta[0], t) <= 1e-9
    theta, series = gp.train(th_of(t0), obj, lr=lr, itr=5, X=X, y=y, Z0=Z0, lr_z=lr_z)
    for i in range(5):
        assert close(res.series["objective"][0, i], series["objective"][i]), i
    assert nrel(res.series["theta"][0], series["theta"]) <= 1e-9
    assert nrel(res.Z[0], series["Z"]) <= 1e-9


# ---------------------------------------------------------------------------- 6. launch split
@pytest.mark.parametrize("stale", (False, True))
def test_launch_split_is_invisible(gpu_ctx, stale):
    """n = 150 is two chunks.  s + 6 steps in one call (launches of s and 6, s the rule's steps
    per launch) against 13 steps and a second call for the other s − 7 from the first's θ and Z:
    the concatenated series and every final output, bitwise."""
    import gpscore
    s = steps_per_launch(150)
    assert s >= 8
    X, y, Z, th, Xt, yt = small_problems(3, n=150)
    kw = dict(nfold=4, lr=0.02, lr_z=0.01, Xt=Xt, yt=yt, stale_noise=stale, ctx=gpu_ctx)
    one = gpscore.fitc_blockloo_train_tall(X, y, Z, th, "kc", itr=s + 6, **kw)
    a = gpscore.fitc_blockloo_train_tall(X, y, Z, th, "kc", itr=13, **kw)
    b = gpscore.fitc_blockloo_train_tall(X, y, a.Z, a.theta, "kc", itr=s - 7, **kw)
    assert not one.info.any() and (one.steps_done == s + 6).all()
    assert (a.steps_done == 13).all() and (b.steps_done == s - 7).all()
    for k in ("objective", "theta"):
        assert same_bits(one.series[k], np.concatenate([a.series[k], b.series[k]], axis=1)), k
    fo, fb = result_fields(one), result_fields(b)
    for k in fo:
        assert same_bits(fo[k], fb[k]), k
    assert not same_bits(one.theta, th) and not same_bits(one.Z, Z)


# ------------------------------------------------------------------------------ 7. final pass
@pytest.mark.parametrize("stale", (False, True))
def test_final_pass_vs_fit_and_predict(gp, gpu_ctx, stale):
    import gpscore
    X, y, Z, th, Xt, yt = small_problems(3, n=293, m=6, d=3, nt=11)
    res = gpscore.fitc_blockloo_train_tall(X, y, Z, th, "dss", nfold=3, lr=1e-3, lr_z=1e-3, itr=4,
                                           Xt=Xt, yt=yt, stale_noise=stale, ctx=gpu_ctx)
    assert not res.info.any()
    for q in range(3):
        noise = res.series["theta"][q, 2, -1] if stale else res.theta[q, -1]
        t = th_of(res.theta[q])
        fr = gp.fit(X[q], y[q], (t[0], t[1], float(noise)), kind="fitc", Z=res.Z[q])
        mu, var, sc = gp.predict(Xt[q], yt[q], with_scores=True)
        assert nrel(res.mu[q], mu) <= 1e-8 and nrel(res.var[q], var) <= 1e-8, q
        for k in SCORES:
            assert close(res.scores[k][q], sc[k], 1e-8), (q, k, res.scores[k][q], sc[k])
        for k in FIVE:
            assert close(res.objectives[k][q], fr.objectives[k], 1e-8), (q, k)


def test_no_steps_returns_the_start(gpu_ctx):
    import gpscore
    X, y, Z, th, Xt, yt = small_problems(3, n=140)
    res = gpscore.fitc_blockloo_train_tall(X, y, Z, th, "kc", itr=0, Xt=Xt, yt=yt, ctx=gpu_ctx)
    assert not res.info.any() and not res.steps_done.any()
    assert same_bits(res.theta, th) and same_bits(res.Z, Z)
    assert res.series["objective"].shape == (3, 0)
    ref = gpscore.fitc_train_tall(X, y, Z, th, "nlml", itr=0, Xt=Xt, yt=yt, ctx=gpu_ctx)
    assert nrel(res.mu, ref.mu) <= 1e-8 and nrel(res.var, ref.var) <= 1e-8


# ----------------------------------------------------------------------- 8. failure isolation
def test_failed_problems_leave_the_others_alone(gpu_ctx):
    """test_gpu_fitc_tall.py's construction at n = 140 (two chunks).  Problem 1 has a NaN inducing
    coordinate (K̃mm fails: info in 1..m), problem 3 a NaN training row in the second chunk (B
    fails: info in m+1..2m), problem 4's targets are scaled by 1e150, so its first DSS step is
    out of range and it fails at a later one.  The call returns 0 and problems 0, 2, 5 are bitwise
    what they are without the bad ones."""
    import gpscore
    X, y, Z, th, Xt, yt = small_problems(6, n=140)
    m, itr = Z.shape[1], 6
    Z[1, 2, 1] = np.nan
    X[3, 133, :] = np.nan  # in the second chunk
    y[4] *= 1e150
    kw = dict(nfold=4, lr=1e-3, lr_z=1e-3, itr=itr, Xt=Xt, yt=yt, ctx=gpu_ctx)
    res = gpscore.fitc_blockloo_train_tall(X, y, Z, th, "dss", **kw)
    good = [0, 2, 5]
    ref = gpscore.fitc_blockloo_train_tall(X[good], y[good], Z[good], th[good], "dss",
                                           **{**kw, "Xt": Xt[good], "yt": yt[good]})
    print("info", res.info, "steps_done", res.steps_done, "theta[4]", res.theta[4])
    assert 1 <= res.info[1] <= m and res.steps_done[1] == 0
    assert m + 1 <= res.info[3] <= 2 * m and res.steps_done[3] == 0
    assert res.info[4] > 0 and 0 < res.steps_done[4] < itr
    for q in (1, 3, 4):
        sd = res.steps_done[q]
        assert np.isnan(res.series["objective"][q, sd:]).all()
        assert np.isnan(res.series["theta"][q, sd:]).all()
        assert np.isnan(res.mu[q]).all() and np.isnan(res.var[q]).all()
        assert all(np.isnan(v[q]) for v in res.objectives.values())
        assert all(np.isnan(v[q]) for v in res.scores.values())
    assert same_bits(res.theta[1], th[1]) and same_bits(res.theta[3], th[3])  # where they stopped
    assert same_bits(res.Z[3], Z[3])
    assert same_bits(res.theta[4], res.series["theta"][4, res.steps_done[4] - 1])
    assert not res.info[good].any() and (res.steps_done[good] == itr).all()
    fa, fb = result_fields(res), result_fields(ref)
    for k in fa:
        assert same_bits(fa[k][good], fb[k]), k
    for k in ("objective", "theta"):
        assert same_bits(res.series[k][good], ref.series[k]), k
    # gradient mode: the same isolation
    vals, grads, gz, fold, objs, info = gpscore.fitc_blockloo_value_and_grad_tall(
        X, y, Z, th, "kc", ctx=gpu_ctx)
    v2, g2, z2, f2, o2, i2 = gpscore.fitc_blockloo_value_and_grad_tall(
        X[good], y[good], Z[good], th[good], "kc", ctx=gpu_ctx)
    assert 1 <= info[1] <= m and m + 1 <= info[3] <= 2 * m and not info[good].any()
    assert np.isnan(grads[1]).all() and np.isnan(gz[3]).all() and np.isnan(vals[1])
    assert np.isnan(fold[1]).all() and np.isnan(fold[3]).all()
    assert same_bits(vals[good], v2) and same_bits(grads[good], g2) and same_bits(gz[good], z2)
    assert same_bits(fold[good], f2)


# ---------------------------------------------------------------- 9. batch size and position
def test_results_do_not_depend_on_batch_size_or_position(gpu_ctx):
    """300 distinct problems at K20's n = 500, m = 20, four folds (two rounds of workgroups on 256
    CUs), 2 steps: the batch reversed gives every problem's bits back, and so does each of a
    handful (the first, the last, both sides of the 256th) run alone."""
    import gpscore
    B = 300
    X, y, Z, th, Xt, yt = small_problems(B, n=500, m=20, nt=5)
    kw = dict(nfold=4, lr=0.02, lr_z=0.02, itr=2, ctx=gpu_ctx)
    full = gpscore.fitc_blockloo_train_tall(X, y, Z, th, "kc", Xt=Xt, yt=yt, **kw)
    assert not full.info.any()
    rev = gpscore.fitc_blockloo_train_tall(X[::-1], y[::-1], Z[::-1], th[::-1], "kc",
                                           Xt=Xt[::-1], yt=yt[::-1], **kw)
    ff, fr = result_fields(full), result_fields(rev)
    for k in ff:
        assert same_bits(ff[k], fr[k][::-1]), k
    for k in ("objective", "theta"):
        assert same_bits(full.series[k], rev.series[k][::-1]), k
    assert len({full.theta[q].tobytes() for q in range(B)}) == B  # the problems are distinct
    for q in (0, 1, 137, 255, 256, 299):
        one = gpscore.fitc_blockloo_train_tall(X[q:q + 1], y[q:q + 1], Z[q:q + 1], th[q:q + 1],
                                               "kc", Xt=Xt[q:q + 1], yt=yt[q:q + 1], **kw)
        fo = result_fields(one)
        for k in ff:
            assert same_bits(ff[k][q:q + 1], fo[k]), (q, k)
        assert same_bits(full.series["theta"][q:q + 1], one.series["theta"]), q
        assert same_bits(full.series["objective"][q:q + 1], one.series["objective"]), q


# ---------------------------------------------------------------------- 10. context left alone
def test_resident_fit_and_pointwise_tall_are_left_alone(gp, gpu_ctx):
    import gpscore
    g = load_golden("fitc_n64_m5_d8_iso")
    gp.fit(g["X"], g["y"], theta_of(g)[0], kind="fitc", Z=g["Z"])
    before = gp.predict(g["Xt"], g["yt"], with_scores=True)
    X, y, Z, th, Xt, yt = small_problems(6, n=140)
    tall = gpscore.fitc_train_tall(X, y, Z, th, "nlml", lr=1e-3, itr=2, Xt=Xt, yt=yt, ctx=gpu_ctx)
    kept = {k: np.copy(v) for k, v in result_fields(tall).items()}
    gpscore.fitc_blockloo_train_tall(X, y, Z, th, "dss", lr=1e-3, itr=2, Xt=Xt, yt=yt, ctx=gpu_ctx)
    gpscore.fitc_blockloo_value_and_grad_tall(X, y, Z, th, "kc", ctx=gpu_ctx)
    after = gp.predict(with_scores=True)
    assert same_bits(before[0], after[0]) and same_bits(before[1], after[1])
    assert before[2] == after[2]
    again = gpscore.fitc_train_tall(X, y, Z, th, "nlml", lr=1e-3, itr=2, Xt=Xt, yt=yt, ctx=gpu_ctx)
    for k, v in result_fields(again).items():
        assert same_bits(v, kept[k]), k


# ------------------------------------------------------------------------- 11. profiling tags
def test_block_launches_have_their_own_profiling_tags(gpu_ctx):
    import gpscore
    s = steps_per_launch(150)
    X, y, Z, th, Xt, yt = small_problems(2, n=150)
    gpu_ctx.prof(True)
    gpscore.fitc_blockloo_train_tall(X, y, Z, th, "dss", lr=1e-3, itr=s + 3, ctx=gpu_ctx)  # two launches
    gpscore.fitc_blockloo_value_and_grad_tall(X, y, Z, th, "dss", ctx=gpu_ctx)
    rep = gpu_ctx.prof_collect()
    gpu_ctx.prof(False)
    assert rep["batch_fitc_tall_block_train"]["count"] == 1, rep
    assert rep["batch_fitc_tall_block_grad"]["count"] == 1, rep
    assert rep["batch_fitc_tall_block_train"]["ms"] > 0
    assert "batch_fitc_tall_train" not in rep and "batch_fitc_tall_grad" not in rep


# ------------------------------------------------------------------------ 12. C-ABI refusals
B_, N_, D_, M_, NT_, ITR_ = 2, 6, 2, 3, 3, 2
ENTRIES = {"gps_fitc_blockloo_grad_tall": False, "gps_fitc_blockloo_train_tall": True}
NULL_ARG = "NULL argument"
NFOLD = "batch: nfold must be in 2..32 and at most n"
CASES = [("X", None, NULL_ARG, "all"),
         ("Z", None, NULL_ARG, "all"),
         ("theta", None, NULL_ARG, "all"),
         ("value", None, NULL_ARG, "grad"),
         ("grad", None, NULL_ARG, "grad"),
         ("grad_z", None, NULL_ARG, "grad"),
         ("theta_out", None, NULL_ARG, "train"),
         ("z_out", None, NULL_ARG, "train"),
         ("objective", 2, "objective must be GPS_BLOCK_DSS or GPS_BLOCK_KC", "all"),
         ("objective", -1, "objective must be GPS_BLOCK_DSS or GPS_BLOCK_KC", "all"),
         ("nfold", 1, NFOLD, "all"),
         ("nfold", 33, NFOLD, "all"),
         ("nfold", N_ + 1, NFOLD, "all"),
         ("nprob", 0, "batch: nprob must be in 1..2^20", "all"),
         ("n", 2049, "batch: n must be in 1..2048", "all"),
         ("m", 33, "batch: m must be in 1..32", "all"),
         ("d", 17, "batch: d must be in 1..16", "all"),
         ("n_ell", 3, "n_ell must be 1 or d", "all"),
         ("itr", -1, "batch: itr must be in 0..2^20", "train"),
         ("lr", float("inf"), "batch: lr must be finite", "train"),
         ("lr_z", float("nan"), "batch: lr_z must be finite", "train"),
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
    a = dict(objective=1, nfold=2, nprob=B_, X=X, y=np.sin(X.sum(axis=2)), n=N_, d=D_,
             Z=rng.uniform(-1, 1, (B_, M_, D_)), m=M_,
             theta=np.tile([0.0, 0.1, -0.1, -2.0], (B_, 1)), n_ell=D_)
    if train:
        Xt = rng.normal(size=(B_, NT_, D_))
        a.update(itr=ITR_, lr=0.01, lr_z=0.01, Xt=Xt, yt=np.sin(Xt.sum(axis=2)), nt=NT_, flags=0,
                 theta_out=np.zeros((B_, 2 + D_)), z_out=np.zeros((B_, M_, D_)),
                 values=np.zeros((B_, ITR_)), thetas=np.zeros((B_, ITR_, 2 + D_)),
                 obj=np.zeros((B_, 5)), mu=np.zeros((B_, NT_)), var=np.zeros((B_, NT_)),
                 sc=np.zeros((B_, 6)), info=np.full(B_, -1, np.int32),
                 steps_done=np.full(B_, -1, np.int32))
    else:
        a.update(value=np.zeros(B_), fold_values=np.zeros((B_, 2)), obj=np.zeros((B_, 5)),
                 grad=np.zeros((B_, 2 + D_)), grad_z=np.zeros((B_, M_, D_)),
                 info=np.full(B_, -1, np.int32))
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
        assert np.isfinite(ok["z_out"]).all() and (ok["z_out"] != 0).any()
    else:
        assert np.isfinite(ok["grad"]).all() and (ok["grad"] != 0).any()
        assert np.isfinite(ok["grad_z"]).all() and (ok["grad_z"] != 0).any()
        assert np.isfinite(ok["value"]).all() and np.isfinite(ok["fold_values"]).all()


def test_block_optional_outputs_may_be_null(gpu_ctx):
    """fold_values and obj may be NULL; the rest comes out the same."""
    from test_gpu_batch_refusals import positional
    full, part = arguments(False), arguments(False)
    part["fold_values"] = None
    part["obj"] = None
    gpu_ctx.call("gps_fitc_blockloo_grad_tall", *positional(full))
    gpu_ctx.call("gps_fitc_blockloo_grad_tall", *positional(part))
    assert same_bits(full["value"], part["value"]) and same_bits(full["grad"], part["grad"])
    assert same_bits(full["grad_z"], part["grad_z"])
    assert (part["info"] == 0).all()


# --------------------------------------------------------------------------- 13. the harness
def test_run_fitc_blockloo_batch_matches_run(gpu_ctx):
    """run_fitc_blockloo_batch against run(kind="fitc", methods=subset) on synthetic sheets: TT =
    2, five steps, the same seed: the same problems, metrics at 1e-8."""
    from gpscore import experiment as E
    sheets = E.synthetic_sheets(5, n_pool=2000, n_test=500)
    subset = {k: E.K20_METHODS[k] for k in ("dss", "kc")}
    out = E.run_fitc_blockloo_batch(sheets, TT=2, itr=5, seed=7, ctx=gpu_ctx)
    ref = E.run(sheets, TT=2, methods=subset, kind="fitc", itr=5, seed=7, ctx=gpu_ctx)
    assert list(out) == ["dss", "kc"]
    for name in subset:
        assert out[name]["theta"].shape == (2, 10) and out[name]["Z"].shape == (2, 20, 8)
        for k in E.METRICS:
            for j in range(2):
                assert close(out[name][k][j], ref[name][k][j], 1e-8), (name, k, j, out[name][k][j],
                                                                       ref[name][k][j])
