"""The joint test predictive on the GPU (gps_*_predict_cov / _predict_joint / _predict_draws):
the full predictive covariance of cal_mean_and_cov (KF:121-126) and spgp_cal_mean_and_cov
(K20:76-83), the multivariate scores of held-out data on it (dss KF:103-108 as called at
KF:556-563, ES KF:70-101 as called at KF:677-684) and joint draws, against the oracle's dense
forms on the SURVEY §8(d) data (seeded sin(3Xw), θ = (0, log 2, log 0.01), Z a subset of X).
Tolerances (fp64): covariance 1e-9 normwise (test_gpu_parity's compat predictives), FITC
max(1e-9, 10× the oracle's own change under 1e-15 input perturbations) as test_gpu_blockloo;
scores 1e-9·max(1, |ref|) per block and in sum; draws 1e-9 normwise."""
import functools

import numpy as np
import pytest

import gp_oracle as O
from conftest import nrel

pytestmark = pytest.mark.gpu

FULL = [(64, 1, 8), (200, 37, 1), (300, 128, 8), (700, 129, 3), (700, 300, 16), (1500, 520, 8)]
FITC = [(300, 5, 37, 1), (500, 20, 137, 8), (900, 200, 300, 8)]


@pytest.fixture(scope="module")
def gp(gpu_ctx):
    import gpscore
    return gpscore.GP(ctx=gpu_ctx)


@functools.lru_cache(maxsize=None)
def case(n, nt, d, m=0, kind="ARD"):
    """Data and the oracle's predictive (mu, cov), computed once per shape and left unchanged."""
    rng = np.random.default_rng(1000 * n + 10 * nt + d + m)
    X, Xt = rng.standard_normal((n, d)), rng.standard_normal((nt, d))
    w = rng.standard_normal(d) / np.sqrt(d)
    y = np.sin(3 * X @ w) + 0.1 * rng.standard_normal(n)
    yt = np.sin(3 * Xt @ w) + 0.1 * rng.standard_normal(nt)
    ell = np.log(2.0) * np.ones(d)
    th = (0.0, 2 * ell if kind == "rbf" else ell, np.log(0.01))  # rbf: b = log ℓ²
    Z = X[rng.choice(n, m, replace=False)] if m else None
    mu, cov = oracle_cov(X, y, Xt, Z, th, kind)
    for a in (X, y, Xt, yt, mu, cov):
        a.setflags(write=False)
    return {"X": X, "y": y, "Xt": Xt, "yt": yt, "Z": Z, "th": th, "mu": mu, "cov": cov}


def oracle_cov(X, y, Xt, Z, th, kind="ARD"):
    sn2, nt = np.exp(th[2]), Xt.shape[0]
    if Z is None:
        A = O.fast_gram(X, X, *th[:2], kind=kind, diag_add=sn2)
        Ks = O.fast_gram(Xt, X, *th[:2], kind=kind)
        mu = Ks @ O.ref_chol_solve(y.reshape(-1, 1), A)
        return mu.ravel(), (sn2 * np.eye(nt) + O.fast_gram(Xt, Xt, *th[:2], kind=kind)
                            - Ks @ O.ref_chol_solve(Ks.T, A))
    n = X.shape[0]
    k_ff, Q_ff = O.ref_ard(X, X, *th[:2]), O.ref_Q(X, Z, X, *th[:2])
    big_Q = Q_ff + np.diag(np.diag(k_ff - Q_ff + sn2 * np.eye(n)))
    Q_sf = O.ref_Q(Xt, Z, X, *th[:2])
    mu = Q_sf @ O.ref_chol_solve(y.reshape(-1, 1), big_Q)
    return mu.ravel(), (sn2 * np.eye(nt) + O.ref_ard(Xt, Xt, *th[:2])
                        - Q_sf @ O.ref_chol_solve(Q_sf.T, big_Q))


def fit(gp, c, rbf=False):
    if c["Z"] is None:
        gp.fit(c["X"], c["y"], c["th"], rbf=rbf, return_loo=False)
    else:
        gp.fit(c["X"], c["y"], c["th"], kind="fitc", Z=c["Z"], return_loo=False)
    gp.set_test(c["Xt"], c["yt"])


def check_cov(gp, c, tol):
    mu0, var0 = gp.predict()
    mu, cov = gp.predict_cov()
    e = {"cov": nrel(cov, c["cov"]), "diag": nrel(np.diag(cov), var0), "mu": nrel(mu, mu0),
         "mu_oracle": nrel(mu, c["mu"])}
    print(e)
    assert e["cov"] <= tol, e
    assert np.array_equal(cov, cov.T)
    assert e["diag"] <= 1e-9 and e["mu"] <= 1e-10, e
    assert e["mu_oracle"] <= (1e-9 if c["Z"] is None else 1e-8), e  # test_gpu_parity.py:669, 681
    mu1, var1 = gp.predict()
    assert np.array_equal(mu1, mu0) and np.array_equal(var1, var0)
    return cov


@pytest.mark.parametrize("n,nt,d", FULL)
def test_full_cov(gp, n, nt, d):
    c = case(n, nt, d, 0)
    fit(gp, c)
    check_cov(gp, c, 1e-9)


def test_full_cov_rbf(gp):
    c = case(300, 128, 8, 0, "rbf")
    fit(gp, c, rbf=True)
    check_cov(gp, c, 1e-9)


@pytest.mark.parametrize("n,nt,d,m", [(700, 300, 16, 0), (500, 137, 8, 20)])
def test_row_windows(gp, n, nt, d, m):
    """A window is formed from its own cross Gram (pad rows zero), not a slice of the resident
    one: unaligned starts, a single row, the last row."""
    c = case(n, nt, d, m)
    fit(gp, c)
    _, whole = gp.predict_cov()
    scale = np.max(np.abs(whole))
    for r0, r1 in ((0, nt), (0, 1), (5, 133), (nt - 1, nt)):
        mu, cov = gp.predict_cov((r0, r1))
        assert cov.shape == (r1 - r0, r1 - r0)
        err = np.max(np.abs(cov - whole[r0:r1, r0:r1])) / scale
        print((r0, r1), err)
        assert err <= 1e-11, ((r0, r1), err)
        assert np.array_equal(cov, cov.T)
        assert nrel(mu, c["mu"][r0:r1]) <= 1e-8


@pytest.mark.parametrize("n,m,nt,d", FITC)
def test_fitc_cov(gp, n, m, nt, d):
    c = case(n, nt, d, m)
    r = np.random.default_rng(1)
    _, pc = oracle_cov(c["X"] * (1 + 1e-15 * r.standard_normal(c["X"].shape)), c["y"], c["Xt"],
                       c["Z"] * (1 + 1e-15 * r.standard_normal(c["Z"].shape)), c["th"])
    tol = max(1e-9, 10 * nrel(pc, c["cov"]))
    print("floor", tol)
    assert tol < 1e-6
    fit(gp, c)
    check_cov(gp, c, tol)


def ref_scores(c, obj, nblock, draws, S, beta=1.0):
    nt = c["yt"].size
    folds = O.block_folds(nt, nblock)
    xs = O.split_draws(draws, folds, S) if obj == "es" else None
    out = []
    for f, (a, b) in enumerate(folds):
        m, C, y = c["mu"][a:b], c["cov"][a:b, a:b], c["yt"][a:b]
        if obj == "es":
            out.append(O.es_value(m, C, y, xs[f][0], xs[f][1], beta))
        else:  # compat.dss (KF:103-108)
            r = (y - m).reshape(-1, 1)
            out.append(0.5 * (b - a) * O.LOG2PI + O.ref_half_logdet(C)
                       + 0.5 * (r.T @ O.ref_chol_solve(r, C)).item())
    return np.array(out)


@pytest.mark.parametrize("nblock", [1, 3])
@pytest.mark.parametrize("obj", ["dss", "es"])
@pytest.mark.parametrize("n,nt,d,m", [(300, 128, 8, 0), (700, 129, 3, 0), (500, 137, 8, 20)])
def test_joint_scores(gp, n, nt, d, m, obj, nblock):
    from gpscore.gp import es_draws
    c = case(n, nt, d, m)
    S = 50
    draws = es_draws(nt, nblock, S, 7) if obj == "es" else None
    ref = ref_scores(c, obj, nblock, draws, S)
    fit(gp, c)
    val, blocks = gp.joint_score(obj, nblock=nblock, num_sim=S, draws=draws, return_blocks=True)
    print(val, ref.sum(), blocks - ref)
    assert abs(val - ref.sum()) <= 1e-9 * max(1.0, abs(ref.sum())), (val, ref.sum())
    for v, rv in zip(blocks, ref):
        assert abs(v - rv) <= 1e-9 * max(1.0, abs(rv)), (blocks, ref)
    assert abs(blocks.sum() - val) <= 1e-12 * max(1.0, abs(val))


def test_not_positive_definite_then_valid(gp):
    """Identical test rows under σ² = e⁻⁴⁰: Sigma is a·11ᵀ to the last bit, its Cholesky hits a
    non-positive pivot; the context stays usable."""
    import gpscore
    rng = np.random.default_rng(3)
    X = rng.standard_normal((20, 8))
    y = rng.standard_normal(20)
    Xt = np.repeat(rng.standard_normal((1, 8)), 70, axis=0)
    yt = rng.standard_normal(70)
    gp.fit(X, y, (0.0, np.zeros(8), -40.0), return_loo=False)
    gp.set_test(Xt, yt)
    with pytest.raises(gpscore.NotPositiveDefinite):
        gp.joint_score("dss")
    with pytest.raises(gpscore.NotPositiveDefinite):
        gp.sample(2, rng=0)
    gp.fit(theta=(0.0, np.zeros(8), np.log(0.01)), return_loo=False)
    v = gp.joint_score("dss")
    mu, cov = gp.predict_cov()
    r = (yt - mu).reshape(-1, 1)
    ref = 0.5 * 70 * O.LOG2PI + O.ref_half_logdet(cov) + 0.5 * (r.T @ O.ref_chol_solve(r, cov)).item()
    assert abs(v - ref) <= 1e-9 * max(1.0, abs(ref)), (v, ref)


@pytest.mark.parametrize("nsamp", [1, 7])
@pytest.mark.parametrize("n,nt,d,m", [(700, 129, 3, 0), (500, 137, 8, 20)])
def test_draws(gp, n, nt, d, m, nsamp):
    c = case(n, nt, d, m)
    fit(gp, c)
    xi = np.random.default_rng(nsamp).standard_normal((nsamp, nt))
    mu, _ = gp.predict_cov()
    out = gp.sample(nsamp, xi=xi)
    ref = xi @ np.linalg.cholesky(c["cov"]).T
    print(nrel(out - mu, ref))
    assert nrel(out - mu, ref) <= 1e-9
    sub = gp.sample(nsamp, rows=(1, nt), xi=xi[:, 1:])  # an unaligned window's own factor
    assert nrel(sub - mu[1:], xi[:, 1:] @ np.linalg.cholesky(c["cov"][1:, 1:]).T) <= 1e-9


def test_communicator_refused(gp):
    """A context with a communicator refuses the joint calls (sharded joint scores are out of
    scope) and says so; a plain context is unaffected."""
    import gpscore
    c = case(300, 128, 8, 0)
    ctx = gpscore.Context(0)
    try:
        ctx.call("gps_comm_init_local", 1, 0, 990017)
        g1 = gpscore.GP(ctx=ctx)
        fit(g1, c)
        for call in (lambda: g1.predict_cov(), lambda: g1.joint_score("dss"),
                     lambda: g1.sample(1, rng=0)):
            with pytest.raises(gpscore.GpsError, match="communicator"):
                call()
        g1.predict()
        ctx.call("gps_comm_destroy")
    finally:
        ctx.close()
    fit(gp, c)
    assert nrel(gp.predict_cov()[1], c["cov"]) <= 1e-6


def test_experiment_joint_metric(gpu_ctx):
    """run_method(joint=("dss",)) reports the test-set joint DSS (KF:556-563) of its final fit."""
    import gpscore
    from gpscore import experiment as E
    sheets = E.synthetic_sheets(4, n_pool=400, n_test=60, d=8)
    data = E.replicate(sheets, j=1, n_train=120, num_va=30, n_test=60, n_pool=400)
    g = gpscore.GP(ctx=gpu_ctx)
    meth = E.KF_METHODS["nlml"]
    res = E.run_method(g, data, meth, np.random.default_rng(2), itr=2, joint=("dss",))
    base = E.run_method(g, data, meth, np.random.default_rng(2), itr=2)
    assert "dss" not in base and all(base[k] == res[k] for k in E.METRICS)
    assert res["dss"] == g.joint_score("dss")
    mu, cov = g.predict_cov()
    r = (data["test_y"] - mu).reshape(-1, 1)
    ref = 0.5 * 60 * O.LOG2PI + O.ref_half_logdet(cov) + 0.5 * (r.T @ O.ref_chol_solve(r, cov)).item()
    assert abs(res["dss"] - ref) <= 1e-9 * max(1.0, abs(ref))
