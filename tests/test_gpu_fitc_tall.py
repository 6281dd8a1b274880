"""Batches of tall FITC GPs on the GPU (gps_fitc_grad_tall / gps_fitc_train_tall): one
workgroup per problem with the n-sized arrays in a device workspace, n up to 2048 — the shape of
"KIN40K-COMPARE-ALL-FITC-20" (n = 500, d = 8, m = 20).  The plan of test_gpu_fitc_batch.py, whose
problem generators and helpers are reused:

 1. the reference's own autograd gradients at exactly K20's shape (fitc_n500_m20_rows, _uniform),
    each as problem 1 of a batch of 3 whose neighbours (θ ± 0.05) are oracle-checked; value,
    gradients, Z gradients, the five objectives and, through fitc_train_tall(itr=0), the
    predictive and the six scores;
 2. the oracle at the edges of the kernel's paths: n at, one below and one above each multiple
    of the chunk height (128) up to three chunks, plus 500 and 2048; m = 1 / 5 / 20 / 32; d = 1 /
    8 / 16, scalar and per-dimension ℓ;
 3. the same numbers from the other implementations, never bitwise: the resident FITC path
    (GP.value_and_grad) at n = 500, m = 20 and the small batch kernel at n = 64 and 128;
 4. five SGD steps at each K20 method's steps against the oracle loop and GP.train, two starts;
 5. the launch split (32 steps a launch at n = 150) is invisible bitwise;
 6. the final pass against GP.fit + GP.predict, stale and fresh σ²;
 7. a failed problem leaves its neighbours bitwise alone;
 8. results do not depend on the batch size or a problem's position, bitwise (B = 300: two rounds);
 9. the context's resident fit and the small-batch path are left alone; profiling tags;
10. experiment.run_fitc_batch against experiment.run(kind="fitc").

Tolerances (fp64) are those of test_gpu_fitc_batch.py.  Against the autograd goldens 1e-9
normwise, 1e-6 where cond(K̃mm) >= 1e3; predictive and scores 1e-8.  Against the oracle on the
edge grid tol = max(1e-9, 30 × the case's conditioning floor) in the joint floor-at-1 metric, the
hard cap of 5e-9 asserted on the oracle alone before the GPU is compared; measured on the CPU
the worst floor of this grid (and of the n = 64 / 128 cases of part 3) is 1.5e-11 (n = 384, m =
20, d = 1, NLML), so the cap never binds on the reference.  Worst measured error on the MI355X:
3.8 % of the tolerance (n = 385, m = 20, d = 1)."""
import functools

import numpy as np
import pytest

import gp_oracle as O
from conftest import load_golden, nrel, theta_of
from test_gpu_fitc_batch import (FIVE, NQ, OBJS, SCORES, close, edge_problem, joint_err,
                                 result_fields, row_of, same_bits, small_problems, th_of)

pytestmark = pytest.mark.gpu

GOLDENS = ("fitc_n500_m20_rows", "fitc_n500_m20_uniform")
CHUNK = 128  # kBatchFitcTallChunk


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


@pytest.mark.parametrize("name", GOLDENS)
@pytest.mark.parametrize("obj", OBJS)
def test_tall_vs_autograd_golden(gpu_ctx, name, obj):
    import gpscore
    g, X, y, Z, rows = golden_batch(name)
    vals, grads, gz, objs, info = gpscore.fitc_value_and_grad_tall(X, y, Z, rows, obj, ctx=gpu_ctx)
    assert not info.any(), info
    Kmm, _, _ = O.fitc_shared(g["Z"], *th_of(rows[1])[:2])
    tol = 1e-9 if np.linalg.cond(Kmm) < 1e3 else 1e-6
    ref = float(g["value_" + obj])
    print(name, obj, "value", abs(vals[1] - ref), "grad", nrel(grads[1], g["grad_" + obj]),
          "gradZ", nrel(gz[1], g["gradZ_" + obj]), "tol", tol)
    assert abs(vals[1] - ref) <= 1e-9 * max(1.0, abs(ref))
    assert nrel(grads[1], g["grad_" + obj]) <= tol, (grads[1], g["grad_" + obj])
    assert nrel(gz[1], g["gradZ_" + obj]) <= tol
    for k in FIVE:
        assert close(objs[k][1], float(g[k])), (k, objs[k][1], float(g[k]))
    for q in (0, 2):  # the neighbours, against the oracle
        ov, og, oz = O.fast_fitc_grad(g["X"], g["y"], g["Z"], *th_of(rows[q]), obj)
        assert close(vals[q], ov), (q, vals[q], ov)
        assert nrel(grads[q], og) <= tol and nrel(gz[q], oz) <= tol, q


@pytest.mark.parametrize("name", GOLDENS)
def test_final_pass_vs_golden(gpu_ctx, name):
    import gpscore
    g, X, y, Z, rows = golden_batch(name)
    Xt, yt = np.stack([g["Xt"]] * 3), np.stack([g["yt"]] * 3)
    res = gpscore.fitc_train_tall(X, y, Z, rows, "loo_crps", itr=0, Xt=Xt, yt=yt, ctx=gpu_ctx)
    assert not res.info.any() and not res.steps_done.any()
    assert same_bits(res.theta, rows) and same_bits(res.Z, Z)
    assert nrel(res.mu[1], g["pred_mu"]) <= 1e-8 and nrel(res.var[1], g["pred_var"]) <= 1e-8
    for k in FIVE:
        assert close(res.objectives[k][1], float(g[k]), 1e-8), k
    for k in SCORES:
        assert close(res.scores[k][1], float(g[k]), 1e-8), (k, res.scores[k][1], float(g[k]))
    for q in (0, 2):
        ref = O.fast_fitc(g["X"], g["y"], g["Xt"], g["yt"], g["Z"], *th_of(rows[q]))
        assert nrel(res.mu[q], ref["pred_mu"]) <= 1e-8 and nrel(res.var[q], ref["pred_var"]) <= 1e-8
        for k in SCORES:
            assert close(res.scores[k][q], ref[k], 1e-8), (q, k)


# --------------------------------------------------------------------------- 2. oracle edges
EDGE_N = tuple(k * CHUNK + o for k in (1, 2, 3) for o in (-1, 0, 1)) + (500, 2048)  # 129 is 128 + 1
EDGE_M = (1, 5, 20, 32)
EDGE_D = ((1, False), (8, True), (16, True))
EDGE_CASES = [(n, m, d, per) for n in EDGE_N for m in EDGE_M for d, per in EDGE_D]


@functools.lru_cache(maxsize=None)
def edge_batch(n, m, d, per):
    ps = [edge_problem(n, m, d, per, q) for q in range(NQ)]
    return tuple(np.stack([p[k] for p in ps]) for k in range(4))


@functools.lru_cache(maxsize=None)
def edge_oracle(n, m, d, per, obj):
    """Per problem (value, grad, grad_Z, tol): the oracle and the case's tolerance from its
    conditioning floor (the oracle on inputs perturbed by 1e-15 relative, same metric)."""
    X, y, Z, rows = edge_batch(n, m, d, per)
    out = []
    for q in range(NQ):
        th = th_of(rows[q])
        ov, og, oz = O.fast_fitc_grad(X[q], y[q], Z[q], *th, obj)
        r = np.random.default_rng(1)
        Xp = X[q] * (1 + 1e-15 * r.standard_normal(X[q].shape))
        Zp = Z[q] * (1 + 1e-15 * r.standard_normal(Z[q].shape))
        pv, pg, pz = O.fast_fitc_grad(Xp, y[q], Zp, *th, obj)
        floor = max(abs(pv - ov) / max(1.0, abs(ov)), joint_err(pg, pz, og, oz))
        assert 30 * floor <= 5e-9, (n, m, d, per, obj, q, floor)  # the hard cap, on the reference
        out.append((ov, og, oz, max(1e-9, 30 * floor)))
    return out


_edge_gpu = {}


def edge_gpu(ctx, n, m, d, per, obj):
    import gpscore
    key = (n, m, d, per, obj)
    if key not in _edge_gpu:
        X, y, Z, rows = edge_batch(n, m, d, per)
        _edge_gpu[key] = gpscore.fitc_value_and_grad_tall(X, y, Z, rows, obj, ctx=ctx)
    return _edge_gpu[key]


@pytest.mark.parametrize("n,m,d,per", EDGE_CASES)
def test_tall_vs_oracle_edges(gpu_ctx, n, m, d, per):
    worst = 0.0
    for obj in OBJS:
        refs = edge_oracle(n, m, d, per, obj)  # asserts the cap before the GPU is looked at
        vals, grads, gz, objs, info = edge_gpu(gpu_ctx, n, m, d, per, obj)
        assert not info.any(), (obj, info)
        for q, (ov, og, oz, tol) in enumerate(refs):
            ev = abs(vals[q] - ov) / max(1.0, abs(ov))
            eg = joint_err(grads[q], gz[q], og, oz)
            worst = max(worst, ev / tol, eg / tol)
            assert ev <= tol, (obj, q, "value", vals[q], ov, tol)
            assert eg <= tol, (obj, q, "grad", eg, tol)
    print("edge", n, m, d, per, "worst error / tolerance %.3g" % worst)


# -------------------------------------------------------- 3. against the other implementations
def test_tall_vs_resident_path_at_k20_shape(gp, gpu_ctx):
    n, m, d, per = 500, 20, 8, True
    X, y, Z, rows = edge_batch(n, m, d, per)
    for obj in OBJS:
        vals, grads, gz, objs, info = edge_gpu(gpu_ctx, n, m, d, per, obj)
        tols = [o[3] for o in edge_oracle(n, m, d, per, obj)]
        for q in range(NQ):
            rv, rg, robjs = gp.value_and_grad(th_of(rows[q]), obj, X=X[q], y=y[q], Z=Z[q])
            assert close(vals[q], rv), (obj, q, vals[q], rv)
            for k in FIVE:
                assert close(objs[k][q], robjs[k]), (obj, q, k, objs[k][q], robjs[k])
            eg = joint_err(grads[q], gz[q], rg, robjs["grad_Z"])
            assert eg <= tols[q], (obj, q, eg, tols[q])
            assert not same_bits(grads[q], rg)  # another summation order: never bitwise


@pytest.mark.parametrize("n", (64, 128))
@pytest.mark.parametrize("m,d,per", ((5, 1, False), (20, 8, True), (32, 16, True)))
def test_tall_vs_small_batch_kernel(gpu_ctx, n, m, d, per):
    import gpscore
    X, y, Z, rows = edge_batch(n, m, d, per)
    for obj in OBJS:
        tols = [o[3] for o in edge_oracle(n, m, d, per, obj)]
        tv, tg, tz, tobjs, ti = gpscore.fitc_value_and_grad_tall(X, y, Z, rows, obj, ctx=gpu_ctx)
        sv, sg, sz, sobjs, si = gpscore.fitc_value_and_grad_batch(X, y, Z, rows, obj, ctx=gpu_ctx)
        assert not ti.any() and not si.any()
        for q in range(NQ):
            assert close(tv[q], sv[q]), (obj, q, tv[q], sv[q])
            for k in FIVE:
                assert close(tobjs[k][q], sobjs[k][q]), (obj, q, k)
            eg = joint_err(tg[q], tz[q], sg[q], sz[q])
            assert eg <= tols[q], (obj, q, eg, tols[q])


# ------------------------------------------------------------------------------------ 4. SGD
K20_STEPS = (("loo_crps", 1.0, 1.0), ("nlml", 1e-4, 1e-3), ("loo_logs", 0.2, 0.2))
SGD_N = 2 * CHUNK + 44  # two chunks and a bit


def sgd_start(start):
    """(X, y, Z0, θ0 as a row) for the SGD test: the first SGD_N rows of the K20-shaped golden
    with the golden's own θ and Z ("golden"), or K20's LOO-LogS start, scalar ℓ = noise = sf² = 1
    in the scripts' parametrisation, with U(0,1) inducing inputs ("ones").  Chosen on the CPU: the
    oracle loop stays positive definite for all three methods from both."""
    g = load_golden("fitc_n500_m20_rows")
    X, y = g["X"][:SGD_N], g["y"][:SGD_N]
    if start == "golden":
        return X, y, g["Z"], row_of(theta_of(g)[0])
    return X, y, np.random.default_rng(20).random((20, X.shape[1])), np.ones(3)


@pytest.mark.parametrize("obj,lr,lr_z", K20_STEPS)
@pytest.mark.parametrize("start", ("golden", "ones"))
def test_sgd_matches_oracle_and_gp_train(gp, gpu_ctx, obj, lr, lr_z, start):
    import gpscore
    X, y, Z0, t0 = sgd_start(start)
    res = gpscore.fitc_train_tall(X[None], y[None], Z0[None], t0[None], obj, lr=lr, lr_z=lr_z,
                                  itr=5, ctx=gpu_ctx)
    assert res.info[0] == 0 and res.steps_done[0] == 5
    t, Z = t0.copy(), Z0.copy()
    for i in range(5):
        v, gr, gzo = O.fast_fitc_grad(X, y, Z, t[0], t[1:-1], t[-1], obj)
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


# ---------------------------------------------------------------------------- 5. launch split
@pytest.mark.parametrize("stale", (False, True))
def test_launch_split_is_invisible(gpu_ctx, stale):
    """n = 150 is two chunks, so a launch runs 32 steps: 70 steps in one call (launches of 32, 32
    and 6) against 40 steps (32 and 8) and a second call for 30 (one launch) from the first's θ
    and Z: the concatenated series and every final output, bitwise."""
    import gpscore
    X, y, Z, th, Xt, yt = small_problems(3, n=150)
    kw = dict(lr=0.05, lr_z=0.02, Xt=Xt, yt=yt, stale_noise=stale, ctx=gpu_ctx)
    one = gpscore.fitc_train_tall(X, y, Z, th, "loo_crps", itr=70, **kw)
    a = gpscore.fitc_train_tall(X, y, Z, th, "loo_crps", itr=40, **kw)
    b = gpscore.fitc_train_tall(X, y, a.Z, a.theta, "loo_crps", itr=30, **kw)
    assert not one.info.any() and (one.steps_done == 70).all()
    assert (a.steps_done == 40).all() and (b.steps_done == 30).all()
    for k in ("objective", "theta"):
        assert same_bits(one.series[k], np.concatenate([a.series[k], b.series[k]], axis=1)), k
    fo, fb = result_fields(one), result_fields(b)
    for k in fo:
        assert same_bits(fo[k], fb[k]), k
    assert not same_bits(one.theta, th) and not same_bits(one.Z, Z)


# ------------------------------------------------------------------------------ 6. final pass
@pytest.mark.parametrize("stale", (False, True))
def test_final_pass_vs_fit_and_predict(gp, gpu_ctx, stale):
    import gpscore
    X, y, Z, th, Xt, yt = small_problems(3, n=293, m=6, d=3, nt=11)
    res = gpscore.fitc_train_tall(X, y, Z, th, "loo_crps", lr=0.3, lr_z=0.1, itr=4, Xt=Xt, yt=yt,
                                  stale_noise=stale, ctx=gpu_ctx)
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


# ----------------------------------------------------------------------- 7. failure isolation
def test_failed_problems_leave_the_others_alone(gpu_ctx):
    """test_gpu_fitc_batch.py's construction at n = 140 (two chunks).  Problem 1 has a NaN
    inducing coordinate (K̃mm fails: info in 1..m), problem 3 a NaN training row (B fails: info in
    m+1..2m), problem 4's targets are scaled by 1e150 under NLML, so its first step is of the
    order of 1e297 and it fails at a later one.  The call returns 0 and problems 0, 2, 5 are
    bitwise what they are without the bad ones."""
    import gpscore
    X, y, Z, th, Xt, yt = small_problems(6, n=140)
    m, itr = Z.shape[1], 6
    Z[1, 2, 1] = np.nan
    X[3, 133, :] = np.nan  # in the second chunk
    y[4] *= 1e150
    kw = dict(lr=1e-3, lr_z=1e-3, itr=itr, Xt=Xt, yt=yt, ctx=gpu_ctx)
    res = gpscore.fitc_train_tall(X, y, Z, th, "nlml", **kw)
    good = [0, 2, 5]
    ref = gpscore.fitc_train_tall(X[good], y[good], Z[good], th[good], "nlml",
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
    vals, grads, gz, objs, info = gpscore.fitc_value_and_grad_tall(X, y, Z, th, "loo_crps",
                                                                   ctx=gpu_ctx)
    v2, g2, z2, o2, i2 = gpscore.fitc_value_and_grad_tall(X[good], y[good], Z[good], th[good],
                                                          "loo_crps", ctx=gpu_ctx)
    assert 1 <= info[1] <= m and m + 1 <= info[3] <= 2 * m and not info[good].any()
    assert np.isnan(grads[1]).all() and np.isnan(gz[3]).all() and np.isnan(vals[1])
    assert same_bits(vals[good], v2) and same_bits(grads[good], g2) and same_bits(gz[good], z2)


# ---------------------------------------------------------------- 8. batch size and position
def test_results_do_not_depend_on_batch_size_or_position(gpu_ctx):
    """300 distinct problems of n = 130 (two chunks; two rounds of workgroups on 256 CUs), 2
    steps: each is bitwise itself run alone and in the reversed batch."""
    import gpscore
    B = 300
    X, y, Z, th, Xt, yt = small_problems(B, n=130, nt=5)
    kw = dict(lr=0.05, lr_z=0.05, itr=2, ctx=gpu_ctx)
    full = gpscore.fitc_train_tall(X, y, Z, th, "loo_crps", Xt=Xt, yt=yt, **kw)
    assert not full.info.any()
    rev = gpscore.fitc_train_tall(X[::-1], y[::-1], Z[::-1], th[::-1], "loo_crps", Xt=Xt[::-1],
                                  yt=yt[::-1], **kw)
    ff, fr = result_fields(full), result_fields(rev)
    for k in ff:
        assert same_bits(ff[k], fr[k][::-1]), k
    for k in ("objective", "theta"):
        assert same_bits(full.series[k], rev.series[k][::-1]), k
    assert len({full.theta[q].tobytes() for q in range(B)}) == B  # the problems are distinct
    for q in range(B):
        one = gpscore.fitc_train_tall(X[q:q + 1], y[q:q + 1], Z[q:q + 1], th[q:q + 1], "loo_crps",
                                      Xt=Xt[q:q + 1], yt=yt[q:q + 1], **kw)
        fo = result_fields(one)
        for k in ff:
            assert same_bits(ff[k][q:q + 1], fo[k]), (q, k)
        assert same_bits(full.series["theta"][q:q + 1], one.series["theta"]), q


# ----------------------------------------------------------------------- 9. context left alone
def test_resident_fit_and_small_batch_are_left_alone(gp, gpu_ctx):
    import gpscore
    g = load_golden("fitc_n64_m5_d8_iso")
    gp.fit(g["X"], g["y"], theta_of(g)[0], kind="fitc", Z=g["Z"])
    before = gp.predict(g["Xt"], g["yt"], with_scores=True)
    Xs, ys, Zs, ths, Xts, yts = small_problems(4)
    small = gpscore.fitc_train_batch(Xs, ys, Zs, ths, "nlml", lr=1e-3, itr=2, Xt=Xts, yt=yts,
                                     ctx=gpu_ctx)
    kept = {k: np.copy(v) for k, v in result_fields(small).items()}
    X, y, Z, th, Xt, yt = small_problems(6, n=140)
    gpscore.fitc_train_tall(X, y, Z, th, "nlml", lr=1e-3, itr=2, Xt=Xt, yt=yt, ctx=gpu_ctx)
    gpscore.fitc_value_and_grad_tall(X, y, Z, th, "loo_crps", ctx=gpu_ctx)
    after = gp.predict(with_scores=True)
    assert same_bits(before[0], after[0]) and same_bits(before[1], after[1])
    assert before[2] == after[2]
    again = gpscore.fitc_train_batch(Xs, ys, Zs, ths, "nlml", lr=1e-3, itr=2, Xt=Xts, yt=yts,
                                     ctx=gpu_ctx)
    for k, v in result_fields(small).items():
        assert same_bits(v, kept[k]) and same_bits(v, result_fields(again)[k]), k


def test_tall_launches_have_their_own_profiling_tags(gpu_ctx):
    import gpscore
    X, y, Z, th, Xt, yt = small_problems(2, n=150)
    gpu_ctx.prof(True)
    gpscore.fitc_train_tall(X, y, Z, th, "nlml", lr=1e-3, itr=40, ctx=gpu_ctx)  # two launches
    gpscore.fitc_value_and_grad_tall(X, y, Z, th, "nlml", ctx=gpu_ctx)
    rep = gpu_ctx.prof_collect()
    gpu_ctx.prof(False)
    assert rep["batch_fitc_tall_train"]["count"] == 1, rep
    assert rep["batch_fitc_tall_grad"]["count"] == 1, rep
    assert rep["batch_fitc_tall_train"]["ms"] > 0
    assert "batch_fitc_train" not in rep and "batch_fitc_grad" not in rep


# --------------------------------------------------------------------------- 10. the harness
HARNESS_SEED = 3  # chosen on the CPU: the oracle loops of all nine fits stay positive definite


def test_run_fitc_batch_matches_run(gp, gpu_ctx):
    """run_fitc_batch(TT=3, itr=3, seed=s) against run(kind="fitc", methods=subset, TT=3, itr=3,
    seed=s, reseed=True) on synthetic sheets of kin40k's shape: every metric series within 1e-8;
    run does not return the inducing inputs, so Z is compared with run_method's, called in run's
    order (which also shows the draws are the same)."""
    from gpscore import experiment as E
    TT, itr = 3, 3
    sheets = E.synthetic_sheets(0)
    subset = {k: E.K20_METHODS[k] for k in ("crps", "nlml", "logs")}
    out = E.run_fitc_batch(sheets, TT=TT, itr=itr, seed=HARNESS_SEED, ctx=gpu_ctx)
    ref = E.run(sheets, TT=TT, methods=subset, kind="fitc", itr=itr, seed=HARNESS_SEED,
                ctx=gpu_ctx, reseed=True)
    assert list(out) == list(subset)
    for name in subset:
        for k in E.METRICS:
            assert out[name][k].shape == (TT,)
            for j in range(TT):
                assert close(out[name][k][j], ref[name][k][j], 1e-8), (name, k, j)
    rng = np.random.default_rng(HARNESS_SEED)
    for j in range(TT):
        data = E.replicate(sheets, j, n_pool=sheets["trainx"].shape[0])
        for name, meth in subset.items():
            r = E.run_method(gp, data, meth, rng, kind="fitc", itr=itr)
            assert out[name]["Z"].shape == (TT, 20, 8)
            assert nrel(out[name]["Z"][j], r["Z"]) <= 1e-8, (name, j)
            assert nrel(out[name]["theta"][j], row_of(r["theta"])) <= 1e-8, (name, j)
