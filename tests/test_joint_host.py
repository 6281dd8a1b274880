"""The joint test predictive on the host (no GPU): its six C-ABI entry points are declared, bound
and reject a NULL context; the FITC covariance identity the device path uses holds against the
dense reference form; the Python facade rejects bad arguments before any device call."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.linalg as sla

import gp_oracle as O
from conftest import ROOT, nrel

JOINT = ("gps_full_predict_cov", "gps_fitc_predict_cov", "gps_full_predict_joint",
         "gps_fitc_predict_joint", "gps_full_predict_draws", "gps_fitc_predict_draws")


def test_joint_symbols_declared_and_bound():
    from gpscore import _lib
    txt = open(os.path.join(ROOT, "include", "gpscore.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(gps_\w+)\s*\(", txt))
    for s in JOINT:
        assert s in _lib.SIGNATURES, s
        assert s in declared, s
    assert "#define GPS_ABI_VERSION %d" % _lib.ABI_VERSION in txt


def test_joint_calls_reject_null_context():
    """Plain ctypes, NULL context: -1 and a message that names it (bind, before any argument)."""
    from gpscore import _lib
    lib = _lib.load()
    z = np.zeros(4)
    P = _lib.ptr
    args = {"cov": (0, 1, P(z), P(z), 1), "joint": (1, 0, 2, 1.0, P(z), P(z), P(z)),
            "draws": (0, 1, 1, P(z), P(z))}
    for name in JOINT:
        rc = getattr(lib, name)(None, *args[name.rsplit("_", 1)[1]])
        assert rc == -1, (name, rc)
        assert b"NULL" in lib.gps_last_error(None), name


def _case(n, m, nt, d, seed):
    rng = np.random.default_rng(seed)
    X, Xt = rng.standard_normal((n, d)), rng.standard_normal((nt, d))
    w = rng.standard_normal(d) / np.sqrt(d)
    y = np.sin(3 * X @ w) + 0.1 * rng.standard_normal(n)
    Z = X[rng.choice(n, m, replace=False)]
    return X, y, Xt, Z, (0.0, np.log(2.0) * np.ones(d), np.log(0.01))


def test_woodbury_covariance_identity():
    """Sigma = sigma²I + K** − V₁ᵀV₁ + V₂ᵀV₂ (V₁ = Lm⁻¹Km*, V₂ = Lb⁻¹Km*, B = K̃mm + KmnΛ⁻¹Knm)
    equals the dense spgp_cal_mean_and_cov form (K20:76-83), and sigma²I + K** − VᵀV the dense
    cal_mean_and_cov (KF:121-126).  Bound: cond(Sigma) ≈ 3e2 times a few hundred roundings of
    2.2e-16 in the n = 300 sums, 1e-12 normwise (the agreement is ~1e-15)."""
    X, y, Xt, Z, th = _case(300, 20, 137, 8, 5)
    n, nt = 300, 137
    sn2 = np.exp(th[2])
    k_ff = O.ref_ard(X, X, *th[:2])
    Q_ff = O.ref_Q(X, Z, X, *th[:2])
    big_Q = Q_ff + np.diag(np.diag(k_ff - Q_ff + sn2 * np.eye(n)))
    Q_sf = O.ref_Q(Xt, Z, X, *th[:2])
    dense = sn2 * np.eye(nt) + O.ref_ard(Xt, Xt, *th[:2]) - Q_sf @ O.ref_chol_solve(Q_sf.T, big_Q)
    Kmm = O.fast_gram(Z, Z, *th[:2], diag_add=1e-3)
    Knm, Kms = O.fast_gram(X, Z, *th[:2]), O.fast_gram(Z, Xt, *th[:2])
    Lm = np.linalg.cholesky(Kmm)
    lam = np.exp(th[0]) - np.sum(sla.solve_triangular(Lm, Knm.T, lower=True) ** 2, 0) + sn2
    Lb = np.linalg.cholesky(Kmm + (Knm.T / lam) @ Knm)
    V1 = sla.solve_triangular(Lm, Kms, lower=True)
    V2 = sla.solve_triangular(Lb, Kms, lower=True)
    wood = sn2 * np.eye(nt) + O.fast_gram(Xt, Xt, *th[:2]) - V1.T @ V1 + V2.T @ V2
    assert nrel(wood, dense) <= 1e-12, nrel(wood, dense)
    A = k_ff + sn2 * np.eye(n)
    k_sf = O.ref_ard(Xt, X, *th[:2])
    dense = sn2 * np.eye(nt) + O.ref_ard(Xt, Xt, *th[:2]) - k_sf @ O.ref_chol_solve(k_sf.T, A)
    V = sla.solve_triangular(np.linalg.cholesky(A), O.fast_gram(X, Xt, *th[:2]), lower=True)
    full = sn2 * np.eye(nt) + O.fast_gram(Xt, Xt, *th[:2]) - V.T @ V
    assert nrel(full, dense) <= 1e-12, nrel(full, dense)


class _RecordingCtx:
    """Stands in for a device context: records the C-ABI calls the facade would make."""

    def __init__(self):
        self.resident = {}
        self.calls = []

    def call(self, name, *args):
        self.calls.append(name)


@pytest.mark.parametrize("kind", ["full", "fitc"])
def test_python_argument_checks(kind):
    import gpscore
    X, y, Xt, Z, _ = _case(40, 5, 12, 3, 1)
    ctx = _RecordingCtx()
    gp = gpscore.GP(ctx=ctx)
    gp.set_data(X, y, kind=kind, Z=Z if kind == "fitc" else None)
    with pytest.raises(ValueError, match="test set"):
        gp.predict_cov()
    gp.set_test(Xt)  # no targets
    with pytest.raises(ValueError, match="targets"):
        gp.joint_score("dss")
    gp.set_test(Xt, np.zeros(12))
    for rows in ((-1, 3), (3, 3), (5, 2), (0, 13)):
        with pytest.raises(ValueError, match="rows"):
            gp.predict_cov(rows)
        with pytest.raises(ValueError, match="rows"):
            gp.sample(2, rows)
    with pytest.raises(ValueError, match="objective"):
        gp.joint_score("kc")
    with pytest.raises(ValueError, match="nblock"):
        gp.joint_score("dss", nblock=13)
    with pytest.raises(ValueError, match="draws"):  # an energy score with draws of the wrong size
        gp.joint_score("es", num_sim=10, draws=np.zeros(2 * 10 * 12 - 1))
    with pytest.raises(ValueError, match="xi"):
        gp.sample(3, xi=np.zeros((3, 11)))
    with pytest.raises(ValueError, match="nsamp"):
        gp.sample(0)
    assert not [c for c in ctx.calls if "predict" in c], ctx.calls
    # well-formed calls reach the model's own entry points
    gp.predict_cov((2, 9))
    gp.joint_score("es", nblock=3, num_sim=10, rng=0)
    gp.sample(2, xi=np.zeros((2, 12)))
    pre = "gps_full_predict_" if kind == "full" else "gps_fitc_predict_"
    assert ctx.calls[-3:] == [pre + "cov", pre + "joint", pre + "draws"]
