"""Batches of small FITC GPs on the GPU (gps_fitc_grad_batch / gps_fitc_train_batch):
one workgroup per problem, value + gradient (θ and the inducing inputs) and the SGD fit loop of
"SIMPLE-FITC--comapre.py" with the final predictive and scores.

 1. the reference's own autograd gradients (the fitc_* goldens that carry them), each as problem
    1 of a batch of 3 whose neighbours (the same data, θ shifted by ±0.05) are oracle-checked;
 2. the oracle at the edges of the kernel's paths: n around the wave / half-block boundaries and
    the limit, m from 1 to the limit (m > n included), d = 1 / 3 / 16, scalar and per-dimension ℓ;
 3. the same problems through the resident FITC path (GP.value_and_grad), never bitwise;
 4. five SGD steps at each SF method's steps against the oracle loop and GP.train;
 5. the launch split (64 steps a launch) is invisible bitwise;
 6. the final pass against GP.fit + GP.predict, stale and fresh σ²;
 7. a failed problem leaves its neighbours bitwise alone;
 8. results do not depend on the batch size or a problem's position, bitwise;
 9. the context's resident fit is left alone; profiling tags;
10. experiment.run_simple_fitc against sequential GP.train fits.

Tolerances (fp64).  Against the autograd goldens: the rule of test_gpu_fitc_grad.py, 1e-9
normwise, 1e-6 where cond(K̃mm) >= 1e3 (the dense reference's LU solves limit agreement there).
Against the oracle on the edge grid: tol = max(1e-9, 30 × the case's conditioning floor) with a
hard cap of 5e-9, the floor being the oracle re-run on X, Z perturbed by 1e-15 relative, in the
same metric; measured on the CPU the worst floor of the grid is 4.5e-11 (n = 63, m =
32, d = 1, NLML) and 1.6e-13 on the tiny-n part, so the cap never binds on the reference alone
(tiny n with m >= 16 is left out: its floor reaches 6e-10).  The metric is joint over [g; g_Z]
with a floor of 1 on the reference's norm: at n = 1 the Z-gradient is analytically zero.
Predictive and scores: the project's FITC tolerance, 1e-8 normwise."""
import functools

import numpy as np
import pytest

import gp_oracle as O
from conftest import load_golden, nrel, theta_of

pytestmark = pytest.mark.gpu

OBJS = ("nlml", "loo_crps", "loo_logs")
FIVE = ("nlml", "loo_crps", "loo_logs", "logdet", "quad")
SCORES = ("test_crps", "test_logs", "test_msll", "test_smse", "test_mse", "test_cover")
GOLDENS = ("fitc_n120_m5_d1_iso", "fitc_n64_m5_d8_iso", "fitc_n64_m5_rows")


@pytest.fixture(scope="module")
def gp(gpu_ctx):
    import gpscore
    return gpscore.GP(ctx=gpu_ctx)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def close(a, b, tol=1e-9):
    return abs(a - b) <= tol * max(1.0, abs(b))


def row_of(th):
    return np.concatenate([[th[0]], np.atleast_1d(th[1]).ravel(), [th[2]]])


def th_of(row):
    return (float(row[0]), np.asarray(row[1:-1]), float(row[-1]))


def joint_err(g, gz, og, oz):
    a = np.concatenate([np.ravel(g), np.ravel(gz)])
    b = np.concatenate([np.ravel(og), np.ravel(oz)])
    return float(np.linalg.norm(a - b) / max(1.0, np.linalg.norm(b)))


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
def test_batch_vs_autograd_golden(gpu_ctx, name, obj):
    import gpscore
    g, X, y, Z, rows = golden_batch(name)
    vals, grads, gz, objs, info = gpscore.fitc_value_and_grad_batch(X, y, Z, rows, obj, ctx=gpu_ctx)
    assert not info.any(), info
    Kmm, _, _ = O.fitc_shared(g["Z"], *th_of(rows[1])[:2])
    tol = 1e-9 if np.linalg.cond(Kmm) < 1e3 else 1e-6
    ref = float(g["value_" + obj])
    print(name, obj, "value", abs(vals[1] - ref), "grad", nrel(grads[1], g["grad_" + obj]),
          "gradZ", nrel(gz[1], g["gradZ_" + obj]))
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
    res = gpscore.fitc_train_batch(X, y, Z, rows, "loo_crps", itr=0, Xt=Xt, yt=yt, ctx=gpu_ctx)
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
EDGE_N = (17, 63, 64, 65, 127, 128)
EDGE_M = (1, 2, 5, 16, 31, 32)
EDGE_D = ((1, False), (3, False), (3, True), (16, False), (16, True))
EDGE_CASES = ([(n, m, d, per) for n in EDGE_N for m in EDGE_M for d, per in EDGE_D] +
              [(n, m, d, per) for n in (1, 2, 3) for m in (1, 2, 5) for d, per in EDGE_D])
NQ = 5


def edge_problem(n, m, d, per, q):
    rng = np.random.default_rng(1000 * n + 10 * m + d + 100000 * q)
    X = rng.standard_normal((n, d))
    y = np.sin(X.sum(1)) + 0.1 * rng.standard_normal(n)
    if d > 1:
        Z = rng.uniform(-2, 2, (m, d))
    else:
        Z = (np.linspace(-2.5, 2.5, m) + 0.1 * rng.standard_normal(m))[:, None]
    if d == 1:
        ell = np.array([np.log(min(0.8, 2.5 / m))])
    elif per:
        ell = np.log(np.linspace(0.5, 1.2, d) * np.sqrt(d) / 2)
    else:
        ell = np.array([np.log(0.45 * np.sqrt(d))])
    row = np.concatenate([[0.1 + 0.05 * q], ell + 0.03 * q, [np.log(0.05) + 0.1 * q]])
    return X, y, Z, row


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
        _edge_gpu[key] = gpscore.fitc_value_and_grad_batch(X, y, Z, rows, obj, ctx=ctx)
    return _edge_gpu[key]


@pytest.mark.parametrize("n,m,d,per", EDGE_CASES)
def test_batch_vs_oracle_edges(gpu_ctx, n, m, d, per):
    worst = 0.0
    for obj in OBJS:
        vals, grads, gz, objs, info = edge_gpu(gpu_ctx, n, m, d, per, obj)
        assert not info.any(), (obj, info)
        for q, (ov, og, oz, tol) in enumerate(edge_oracle(n, m, d, per, obj)):
            ev = abs(vals[q] - ov) / max(1.0, abs(ov))
            eg = joint_err(grads[q], gz[q], og, oz)
            worst = max(worst, ev / tol, eg / tol)
            assert ev <= tol, (obj, q, "value", vals[q], ov, tol)
            assert eg <= tol, (obj, q, "grad", eg, tol)
    print("edge", n, m, d, per, "worst error / tolerance %.3g" % worst)


# --------------------------------------------------------------- 3. against the resident path
@pytest.mark.parametrize("n,m,d,per", [c for c in EDGE_CASES if c[0] >= 17])
def test_batch_vs_resident_path(gp, gpu_ctx, n, m, d, per):
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


# ------------------------------------------------------------------------------------ 4. SGD
SF_STEPS = (("loo_crps", 1.0, 1.0), ("nlml", 5e-4, 5e-3), ("loo_logs", 5e-3, 5e-3))
DUP_Z0 = np.array([-3.0, 2.0, 0.0, 0.0, -1.0])[:, None]


@pytest.mark.parametrize("obj,lr,lr_z", SF_STEPS)
@pytest.mark.parametrize("start", ("golden", "duplicate"))
def test_sgd_matches_oracle_and_gp_train(gp, gpu_ctx, obj, lr, lr_z, start):
    import gpscore
    g = load_golden("fitc_n120_m5_d1_iso")
    Z0 = g["Z"] if start == "golden" else DUP_Z0
    X, y = g["X"], g["y"]
    res = gpscore.fitc_train_batch(X[None], y[None], Z0[None], (1.0, 1.0, 1.0), obj, lr=lr,
                                   lr_z=lr_z, itr=5, ctx=gpu_ctx)
    assert res.info[0] == 0 and res.steps_done[0] == 5
    t, Z = np.ones(3), Z0.copy()
    for i in range(5):
        v, gr, gzo = O.fast_fitc_grad(X, y, Z, t[0], t[1:-1], t[-1], obj)
        assert close(res.series["objective"][0, i], v), (i, res.series["objective"][0, i], v)
        t = t - lr * gr
        Z = Z - lr_z * gzo
        assert nrel(res.series["theta"][0, i], t) <= 1e-9, (i, res.series["theta"][0, i], t)
    assert nrel(res.Z[0], Z) <= 1e-9, (res.Z[0], Z)
    assert nrel(res.theta[0], t) <= 1e-9
    theta, series = gp.train((1.0, np.array([1.0]), 1.0), obj, lr=lr, itr=5, X=X, y=y, Z0=Z0,
                             lr_z=lr_z)
    for i in range(5):
        assert close(res.series["objective"][0, i], series["objective"][i]), i
    assert nrel(res.series["theta"][0], series["theta"]) <= 1e-9
    assert nrel(res.Z[0], series["Z"]) <= 1e-9


# --------------------------------------------------------------------------- small problems
def small_problems(B, n=20, m=5, d=2, nt=7, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((B, n, d))
    y = np.sin(X.sum(2)) + 0.1 * rng.standard_normal((B, n))
    Xt = rng.standard_normal((B, nt, d))
    yt = np.sin(Xt.sum(2)) + 0.1 * rng.standard_normal((B, nt))
    Z = rng.uniform(-2, 2, (B, m, d))
    th = np.column_stack([0.1 + 0.2 * rng.random(B), np.log(0.9) + 0.2 * rng.random(B),
                          np.log(0.05) + 0.2 * rng.random(B)])
    return X, y, Z, th, Xt, yt


def result_fields(res):
    out = {"theta": res.theta, "Z": res.Z, "mu": res.mu, "var": res.var}
    out.update({"obj_" + k: v for k, v in res.objectives.items()})
    out.update(res.scores)
    return out


# ---------------------------------------------------------------------------- 5. launch split
@pytest.mark.parametrize("stale", (False, True))
def test_launch_split_is_invisible(gpu_ctx, stale):
    """70 steps in one call (launches of 64 and 6) against 40 steps and a second call for 30 from
    the first's θ and Z: the concatenated series and every final output, bitwise."""
    import gpscore
    X, y, Z, th, Xt, yt = small_problems(3)
    kw = dict(lr=0.05, lr_z=0.02, Xt=Xt, yt=yt, stale_noise=stale, ctx=gpu_ctx)
    one = gpscore.fitc_train_batch(X, y, Z, th, "loo_crps", itr=70, **kw)
    a = gpscore.fitc_train_batch(X, y, Z, th, "loo_crps", itr=40, **kw)
    b = gpscore.fitc_train_batch(X, y, a.Z, a.theta, "loo_crps", itr=30, **kw)
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
    X, y, Z, th, Xt, yt = small_problems(3, n=37, m=6, d=3, nt=11)
    res = gpscore.fitc_train_batch(X, y, Z, th, "loo_crps", lr=0.3, lr_z=0.1, itr=4, Xt=Xt, yt=yt,
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
    """Problem 1 has a NaN inducing coordinate (K̃mm fails: info in 1..m), problem 3 a NaN training
    row (B fails: info in m+1..2m).  Problem 4 takes steps of the order of 1e300: the step lr is
    one number per call, so its targets are scaled by 1e150 instead — the NLML gradient is
    quadratic in them — and its θ overflows; it fails at a later step.  The call returns 0 and
    problems 0, 2, 5 are bitwise what they are without the bad ones."""
    import gpscore
    X, y, Z, th, Xt, yt = small_problems(6)
    m, itr = Z.shape[1], 6
    Z[1, 2, 1] = np.nan
    X[3, 7, :] = np.nan
    y[4] *= 1e150
    kw = dict(lr=1e-3, lr_z=1e-3, itr=itr, Xt=Xt, yt=yt, ctx=gpu_ctx)
    res = gpscore.fitc_train_batch(X, y, Z, th, "nlml", **kw)
    good = [0, 2, 5]
    ref = gpscore.fitc_train_batch(X[good], y[good], Z[good], th[good], "nlml",
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
    assert same_bits(res.theta[4], res.series["theta"][4, res.steps_done[4] - 1])
    assert not res.info[good].any() and (res.steps_done[good] == itr).all()
    fa, fb = result_fields(res), result_fields(ref)
    for k in fa:
        assert same_bits(fa[k][good], fb[k]), k
    for k in ("objective", "theta"):
        assert same_bits(res.series[k][good], ref.series[k]), k
    # gradient mode: the same isolation
    vals, grads, gz, objs, info = gpscore.fitc_value_and_grad_batch(X, y, Z, th, "loo_crps",
                                                                    ctx=gpu_ctx)
    v2, g2, z2, o2, i2 = gpscore.fitc_value_and_grad_batch(X[good], y[good], Z[good], th[good],
                                                           "loo_crps", ctx=gpu_ctx)
    assert 1 <= info[1] <= m and m + 1 <= info[3] <= 2 * m and not info[good].any()
    assert np.isnan(grads[1]).all() and np.isnan(gz[3]).all() and np.isnan(vals[1])
    assert same_bits(vals[good], v2) and same_bits(grads[good], g2) and same_bits(gz[good], z2)


def test_a_step_of_1e300_overflows_and_stops(gpu_ctx):
    """lr = 1e300 itself, for a whole call (lr is per call): after the first LOO-CRPS step θ is of
    the order of ±1e300, so sf², σ² and 1/ℓ are each 0 or inf and either a factorisation fails
    at the next forward or the value is NaN and the one after fails.  Every problem stops with
    info > 0 before itr, NaN from there on, theta_out the θ it stopped at; the call returns 0."""
    import gpscore
    X, y, Z, th, Xt, yt = small_problems(3)
    itr = 6
    res = gpscore.fitc_train_batch(X, y, Z, th, "loo_crps", lr=1e300, lr_z=1.0, itr=itr, Xt=Xt,
                                   yt=yt, ctx=gpu_ctx)
    print("info", res.info, "steps_done", res.steps_done, "theta", res.theta)
    for q in range(3):
        sd = res.steps_done[q]
        assert res.info[q] > 0 and 0 < sd < itr, (q, res.info[q], sd)
        assert np.isnan(res.series["objective"][q, sd:]).all()
        assert np.isnan(res.series["theta"][q, sd:]).all()
        assert same_bits(res.theta[q], res.series["theta"][q, sd - 1])
        assert np.isfinite(res.series["objective"][q, 0])
        assert np.isnan(res.mu[q]).all() and all(np.isnan(v[q]) for v in res.scores.values())


# ---------------------------------------------------------------- 8. batch size and position
def test_results_do_not_depend_on_batch_size_or_position(gpu_ctx):
    """515 distinct problems (two rounds of workgroups and a bit on 256 CUs), 3 steps: each is
    bitwise itself run alone and in the reversed batch."""
    import gpscore
    B = 515
    X, y, Z, th, Xt, yt = small_problems(B, nt=5)
    kw = dict(lr=0.05, lr_z=0.05, itr=3, ctx=gpu_ctx)
    full = gpscore.fitc_train_batch(X, y, Z, th, "loo_crps", Xt=Xt, yt=yt, **kw)
    assert not full.info.any()
    rev = gpscore.fitc_train_batch(X[::-1], y[::-1], Z[::-1], th[::-1], "loo_crps", Xt=Xt[::-1],
                                   yt=yt[::-1], **kw)
    ff, fr = result_fields(full), result_fields(rev)
    for k in ff:
        assert same_bits(ff[k], fr[k][::-1]), k
    for k in ("objective", "theta"):
        assert same_bits(full.series[k], rev.series[k][::-1]), k
    assert len({full.theta[q].tobytes() for q in range(B)}) == B  # the problems are distinct
    for q in range(B):
        one = gpscore.fitc_train_batch(X[q:q + 1], y[q:q + 1], Z[q:q + 1], th[q:q + 1], "loo_crps",
                                       Xt=Xt[q:q + 1], yt=yt[q:q + 1], **kw)
        fo = result_fields(one)
        for k in ff:
            assert same_bits(ff[k][q:q + 1], fo[k]), (q, k)
        assert same_bits(full.series["theta"][q:q + 1], one.series["theta"]), q


# ----------------------------------------------------------------------- 9. context left alone
def test_resident_fitc_fit_is_left_alone(gp, gpu_ctx):
    import gpscore
    g = load_golden("fitc_n64_m5_d8_iso")
    gp.fit(g["X"], g["y"], theta_of(g)[0], kind="fitc", Z=g["Z"])
    before = gp.predict(g["Xt"], g["yt"], with_scores=True)
    X, y, Z, th, Xt, yt = small_problems(6)
    gpscore.fitc_train_batch(X, y, Z, th, "nlml", lr=1e-3, itr=2, Xt=Xt, yt=yt, ctx=gpu_ctx)
    gpscore.fitc_value_and_grad_batch(X, y, Z, th, "loo_crps", ctx=gpu_ctx)
    after = gp.predict(with_scores=True)
    assert same_bits(before[0], after[0]) and same_bits(before[1], after[1])
    assert before[2] == after[2]


def test_fitc_batch_launches_have_their_own_profiling_tags(gpu_ctx):
    import gpscore
    X, y, Z, th, Xt, yt = small_problems(2)
    gpu_ctx.prof(True)
    gpscore.fitc_train_batch(X, y, Z, th, "nlml", lr=1e-3, itr=70, ctx=gpu_ctx)  # two launches
    gpscore.fitc_value_and_grad_batch(X, y, Z, th, "nlml", ctx=gpu_ctx)
    rep = gpu_ctx.prof_collect()
    gpu_ctx.prof(False)
    assert rep["batch_fitc_train"]["count"] == 1 and rep["batch_fitc_grad"]["count"] == 1, rep
    assert rep["batch_fitc_train"]["ms"] > 0


# --------------------------------------------------------------------------- 10. the harness
def test_run_simple_fitc_matches_sequential_fits(gp, gpu_ctx):
    """run_simple_fitc(TT=4, itr=3) against four sequential fits per method from the same data
    and Z0: GP.train with the method's steps, the stale noise of run_method, GP.fit, GP.predict."""
    from gpscore import experiment as E
    TT, itr = 4, 3
    data = [E.simple_data(j) for j in range(TT)]
    Z0 = np.stack([E.simple_inducing(j) for j in range(TT)])
    out = E.run_simple_fitc(TT=TT, datasets=data, Z0=Z0, itr=itr, ctx=gpu_ctx)
    assert set(out) == set(E.SF_METHODS)
    for name, meth in E.SF_METHODS.items():
        assert out[name]["Z"].shape == (TT, 5, 1)
        for j, dd in enumerate(data):
            th0 = E.initial_theta(meth, 1, None)
            theta, series = gp.train(th0, meth.objective, lr=meth.lr, itr=itr, X=dd["train_x"],
                                     y=dd["train_y"], Z0=Z0[j], lr_z=meth.lr_z)
            noise = float(series["theta"][itr - 2][-1])
            gp.fit(theta=(theta[0], theta[1], noise), return_loo=False)
            _, _, sc = gp.predict(dd["test_x"], dd["test_y"], with_scores=True)
            for k in E.METRICS:
                assert out[name][k].shape == (TT,)
                assert close(out[name][k][j], sc["test_" + k], 1e-8), (name, j, k)
            assert nrel(out[name]["Z"][j], series["Z"]) <= 1e-8, (name, j)
