"""The validated tall FITC fits (gps_fitc_train_tall_va / gps_fitc_blockloo_train_tall_va, DESIGN
§37): every validation row against the oracle at the θ and Z it stands for, the scripts' row under
stale_noise, the fit bitwise that of the plain calls, a row bitwise the final pass of an itr = 0
call, the launch split, batch size and position change no bit, va_every, problems that fail
mid-fit, the C-ABI refusals, and run_fitc_validated_batch against its parts.  Runs on the GPU box.

Tolerances: the six scores of a row against oracle/gp_oracle.py's fast_fitc at max(1e-8, 30 × the
case's conditioning floor), the floor being the oracle on X and Z perturbed by 1e-15 relative, same
metrics, with the cap 30 × floor <= 5e-9 asserted on the oracle alone before the GPU figure is
looked at (tests/test_gpu_full_tall_va.py's row_tol).  Everything else is bitwise."""
import numpy as np
import pytest

import gp_oracle as O
from test_gpu_fitc_batch import (SCORES, close, edge_problem, result_fields, same_bits,
                                 small_problems, th_of)

pytestmark = pytest.mark.gpu

TOL8 = 1e-8
BLOCK = ("dss", "kc")
# the small steps of the tall SGD tests: no problem fails at any of the shapes below
LR = {"nlml": (1e-4, 1e-3), "loo_crps": (0.05, 0.02), "loo_logs": (0.05, 0.02),
      "dss": (1e-3, 1e-3), "kc": (0.05, 0.02)}


def call(gpu_ctx, obj, X, y, Z, th, *va, nfold=None, validated=True, **kw):
    import gpscore
    kw.setdefault("lr", LR[obj][0])
    kw.setdefault("lr_z", LR[obj][1])
    if obj in BLOCK:
        f = gpscore.fitc_blockloo_train_tall_validated if validated \
            else gpscore.fitc_blockloo_train_tall
        return f(X, y, Z, th, *va, objective=obj, nfold=nfold or 4, ctx=gpu_ctx, **kw)
    f = gpscore.fitc_train_tall_validated if validated else gpscore.fitc_train_tall
    return f(X, y, Z, th, *va, objective=obj, ctx=gpu_ctx, **kw)


def edge_va_batch(B, n, nv, m, d, per):
    """edge_problem's recipe for B problems, plus nv validation rows drawn the same way."""
    ps = [edge_problem(n, m, d, per, q) for q in range(B)]
    X, y, Z, th = (np.stack([p[k] for p in ps]) for k in range(4))
    rng = np.random.default_rng(77 + 1000 * n + nv)
    Xv = rng.standard_normal((B, nv, d))
    yv = np.sin(Xv.sum(2)) + 0.1 * rng.standard_normal((B, nv))
    return X, y, Z, th, Xv, yv


def va_small(B, n, nv=70, nt=9, seed=3):
    """small_problems with nv validation rows."""
    X, y, Z, th, Xt, yt = small_problems(B, n=n, nt=nt, seed=seed)
    rng = np.random.default_rng(seed + 50)
    Xv = rng.standard_normal((B, nv, X.shape[2]))
    yv = np.sin(Xv.sum(2)) + 0.1 * rng.standard_normal((B, nv))
    return X, y, Z, th, Xt, yt, Xv, yv


def theta_of_row(res, th0, q, r):
    step = int(res.va_steps[r])
    if r == len(res.va_steps) - 1:
        return res.theta[q]
    return th0[q] if step == 0 else res.series["theta"][q, step - 1]


def oracle_scores(X, y, Xv, yv, Z, th):
    out = O.fast_fitc(X, y, Xv, yv, Z, *th_of(th))
    return np.array([out[k] for k in SCORES])


def row_tol(X, y, Xv, yv, Z, th):
    """(the oracle's six scores, the tolerance from the case's conditioning floor)."""
    with np.errstate(all="ignore"):
        ref = oracle_scores(X, y, Xv, yv, Z, th)
        r = np.random.default_rng(1)
        Xp = X * (1 + 1e-15 * r.standard_normal(X.shape))
        Zp = Z * (1 + 1e-15 * r.standard_normal(Z.shape))
        per = oracle_scores(Xp, y, Xv, yv, Zp, th)
    ok = np.isfinite(ref)
    floor = float(np.max(np.abs(per[ok] - ref[ok]) / np.maximum(1.0, np.abs(ref[ok])), initial=0.0))
    assert 30 * floor <= 5e-9, floor  # the hard cap, on the reference alone
    return ref, max(TOL8, 30 * floor)


def check_row(got, ref, tol, what):
    worst = 0.0
    for k, g, r in zip(SCORES, got, ref):
        print(what, k, "got %.17g ref %.17g" % (g, r))
        if np.isnan(r):  # n = 1: the train targets have no variance, MSLL is NaN in both
            assert np.isnan(g), (what, k, g, r)
        else:
            worst = max(worst, abs(g - r) / max(1.0, abs(r)) / tol)
            assert close(g, r, tol), (what, k, g, r, tol)
    print(what, "worst error / tolerance %.3g" % worst)


def rows_of(res, q):
    return np.stack([res.va_scores[k][q] for k in SCORES], axis=1)  # (nva, 6)


# ------------------------------------------------------------------ 1. against the oracle
ORACLE_CASES = [(1, 5, 1, 1, False, "nlml", None),
                (127, 1, 1, 1, False, "loo_crps", None),
                (128, 3, 5, 8, True, "loo_logs", None),
                (129, 4, 20, 16, True, "loo_crps", None),
                (257, 5, 32, 8, False, "nlml", None),
                (129, 70, 32, 1, False, "loo_logs", None),
                (128, 4, 5, 8, True, "dss", 2),
                (129, 5, 20, 16, True, "kc", 4),
                (257, 70, 32, 8, False, "dss", 4),
                (130, 3, 1, 1, False, "kc", 2)]


@pytest.mark.parametrize("n,nv,m,d,per,obj,nfold", ORACLE_CASES)
def test_rows_vs_oracle(gpu_ctx, n, nv, m, d, per, obj, nfold):
    """itr = 4, va_every = 2: rows for steps 0 and 2 and the final pass, each against the oracle at
    the row's θ (θ0, the series, the returned θ) and the row's Z (va_Z)."""
    B = 2
    X, y, Z, th, Xv, yv = edge_va_batch(B, n, nv, m, d, per)
    res = call(gpu_ctx, obj, X, y, Z, th, Xv, yv, nfold=nfold, itr=4, va_every=2, keep_z=True)
    assert not res.info.any(), res.info
    assert list(res.va_steps) == [0, 2, 4] and res.va_Z.shape == (B, 3, m, d)
    assert same_bits(res.va_Z[:, 0], Z) and same_bits(res.va_Z[:, 2], res.Z)
    for q in range(B):
        got = rows_of(res, q)
        for r in range(3):
            t = theta_of_row(res, th, q, r)
            ref, tol = row_tol(X[q], y[q], Xv[q], yv[q], res.va_Z[q, r], t)
            check_row(got[r], ref, tol, (q, r))
        assert not same_bits(got[0], got[2])  # θ and Z moved


# ------------------------------------------------------------------ 2. the scripts' row
@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("stale", [True, False])
def test_final_row_is_the_scripts_row(gpu_ctx, k, stale):
    """With stale_noise and itr = k the final row is the oracle at (θ_k, Z_k) with the log σ² of
    θ_{k−1} (θ0's for k = 1): va_series[k − 1] of the scripts; without the flag, (θ_k, Z_k)."""
    X, y, Z, th, _, _, Xv, yv = va_small(2, 140, nv=33)
    res = call(gpu_ctx, "loo_crps", X, y, Z, th, Xv, yv, lr=0.3, lr_z=0.1, itr=k,
               stale_noise=stale)
    assert not res.info.any() and res.va_steps[-1] == k
    for q in range(2):
        t = res.theta[q].copy()
        prev = th[q] if k == 1 else res.series["theta"][q, k - 2]
        assert prev[-1] != t[-1]  # the two noises differ, so the flag matters
        if stale:
            t[-1] = prev[-1]
        ref, tol = row_tol(X[q], y[q], Xv[q], yv[q], res.Z[q], t)
        check_row(rows_of(res, q)[-1], ref, tol, (q, "final"))


# ------------------------------------------------------------------ 3. the fit is untouched
@pytest.mark.parametrize("obj", ["loo_crps", "nlml", "dss", "kc"])
def test_validation_does_not_touch_the_fit(gpu_ctx, obj):
    """n = 130 is two chunks: 32 steps a launch on the pointwise path, 16 on the block path, so
    itr = 40 spans more than one launch on both; every field of the plain call's result, Z and
    both series, bitwise."""
    X, y, Z, th, Xt, yt, Xv, yv = va_small(3, 130)
    kw = dict(itr=40, Xt=Xt, yt=yt, stale_noise=True)
    a = call(gpu_ctx, obj, X, y, Z, th, Xv, yv, va_every=3, **kw)
    b = call(gpu_ctx, obj, X, y, Z, th, validated=False, **kw)
    assert not b.info.any() and list(b.steps_done) == [40] * 3
    fa, fb = result_fields(a), result_fields(b)
    assert set(fa) == set(fb)
    for k in fb:
        assert same_bits(fa[k], fb[k]), k
    for k in ("objective", "theta"):
        assert same_bits(a.series[k], b.series[k]), k
    assert same_bits(a.info, b.info) and same_bits(a.steps_done, b.steps_done)
    assert np.isfinite(rows_of(a, 0)).all() and a.va_Z is None


# ------------------------------------------------------------------ 4. a row is an itr = 0 call
@pytest.mark.parametrize("obj", ["loo_logs", "dss"])
def test_a_row_is_an_itr0_call(gpu_ctx, obj):
    """Step 0, an interior checkpoint and the final row: bitwise the scores of the plain call's
    final pass at that θ and Z with the validation rows as its test rows (nv = 70: seventeen
    whole passes of four rows and a partial one)."""
    X, y, Z, th, _, _, Xv, yv = va_small(2, 130)
    res = call(gpu_ctx, obj, X, y, Z, th, Xv, yv, itr=7, va_every=2, keep_z=True)
    assert not res.info.any() and list(res.va_steps) == [0, 2, 4, 6, 7]
    for r in (0, 2, 4):
        t = np.stack([theta_of_row(res, th, q, r) for q in range(2)])
        one = call(gpu_ctx, obj, X, y, res.va_Z[:, r], t, validated=False, itr=0, Xt=Xv, yt=yv)
        assert not one.info.any()
        for k in SCORES:
            assert same_bits(res.va_scores[k][:, r], one.scores[k]), (r, k)


# ------------------------------------------------------------------ 5. launch split
@pytest.mark.parametrize("obj", ["loo_logs", "kc"])
def test_launch_split_changes_no_row(gpu_ctx, obj):
    """n = 150 is two chunks: 32 (block: 16) steps a launch, so itr = 40 takes two (three)
    launches.  Against 24 + 16 steps in two calls, the second from the first call's θ and Z (the
    split is a multiple of va_every so that the step indices coincide): steps 0..21 are the first
    call's rows, step 24 is the first call's final row (no stale noise: the final pass at θ_24, Z_24
    is step 24's forward) and the second call's row 0, and 27..39 and the final row are the second
    call's."""
    X, y, Z, th, Xt, yt, Xv, yv = va_small(3, 150)
    kw = dict(va_every=3, Xt=Xt, yt=yt, keep_z=True)
    whole = call(gpu_ctx, obj, X, y, Z, th, Xv, yv, itr=40, **kw)
    first = call(gpu_ctx, obj, X, y, Z, th, Xv, yv, itr=24, **kw)
    second = call(gpu_ctx, obj, X, y, first.Z, first.theta, Xv, yv, itr=16, **kw)
    assert not whole.info.any() and list(whole.steps_done) == [40] * 3
    assert list(whole.va_steps) == list(range(0, 40, 3)) + [40]
    assert list(first.va_steps) == list(range(0, 24, 3)) + [24]
    assert list(second.va_steps) == list(range(0, 16, 3)) + [16]
    assert same_bits(whole.theta, second.theta) and same_bits(whole.Z, second.Z)
    for k in SCORES:
        w = whole.va_scores[k]
        assert same_bits(w[:, :9], first.va_scores[k]), k        # steps 0..21 and 24
        assert same_bits(w[:, 8:], second.va_scores[k]), k       # steps 24..39 and the final row
    assert same_bits(whole.va_Z[:, :9], first.va_Z) and same_bits(whole.va_Z[:, 8:], second.va_Z)
    assert not same_bits(whole.va_scores["test_crps"][:, 0], whole.va_scores["test_crps"][:, -1])


def test_row_budget_splits_change_no_row(gpu_ctx):
    """nv = 1500 leaves floor(4096 / 1500) = 2 checkpoints a launch: with va_every = 1 a launch runs
    2 steps, with va_every = 2 four — the rows of the coarser run are the matching rows of the
    finer one, and the fit is the plain call's."""
    X, y, Z, th, _, _, Xv, yv = va_small(2, 130, nv=1500)
    a = call(gpu_ctx, "loo_crps", X, y, Z, th, Xv, yv, itr=6, va_every=1)
    b = call(gpu_ctx, "loo_crps", X, y, Z, th, Xv, yv, itr=6, va_every=2)
    p = call(gpu_ctx, "loo_crps", X, y, Z, th, validated=False, itr=6)
    assert not a.info.any()
    for k in SCORES:
        assert same_bits(b.va_scores[k], a.va_scores[k][:, [0, 2, 4, 6]]), k
    for r in (a, b):
        assert same_bits(r.theta, p.theta) and same_bits(r.Z, p.Z)
        assert same_bits(r.series["theta"], p.series["theta"])


# ------------------------------------------------------------------ 6. batch size and position
def test_batch_size_and_position_change_no_row(gpu_ctx):
    X, y, Z, th, Xt, yt, Xv, yv = va_small(5, 130)
    kw = dict(itr=5, va_every=2, keep_z=True)
    for obj in ("loo_crps", "kc"):
        full = call(gpu_ctx, obj, X, y, Z, th, Xv, yv, Xt=Xt, yt=yt, **kw)
        rev = call(gpu_ctx, obj, X[::-1], y[::-1], Z[::-1], th[::-1], Xv[::-1], yv[::-1],
                   Xt=Xt[::-1], yt=yt[::-1], **kw)
        one = slice(3, 4)
        alone = call(gpu_ctx, obj, X[one], y[one], Z[one], th[one], Xv[one], yv[one], Xt=Xt[one],
                     yt=yt[one], **kw)
        assert not full.info.any()
        for k in SCORES:
            assert same_bits(full.va_scores[k][3], alone.va_scores[k][0]), (obj, k)
            assert same_bits(full.va_scores[k], rev.va_scores[k][::-1]), (obj, k)
        assert same_bits(full.va_Z[3], alone.va_Z[0]) and same_bits(full.va_Z, rev.va_Z[::-1])
        assert not same_bits(full.va_scores["test_crps"][0], full.va_scores["test_crps"][1])


def test_problem_277_of_300(gpu_ctx):
    """Two rounds of workgroups on 256 CUs: problem 277's rows are those of the problem alone."""
    X, y, Z, th, _, _, Xv, yv = va_small(300, 130, nv=9, nt=1)
    kw = dict(itr=2, keep_z=True)
    full = call(gpu_ctx, "loo_crps", X, y, Z, th, Xv, yv, **kw)
    one = slice(277, 278)
    alone = call(gpu_ctx, "loo_crps", X[one], y[one], Z[one], th[one], Xv[one], yv[one], **kw)
    assert not full.info.any()
    for k in SCORES:
        assert same_bits(full.va_scores[k][277], alone.va_scores[k][0]), k
    assert same_bits(full.va_Z[277], alone.va_Z[0])
    assert not same_bits(full.va_scores["test_crps"][277], full.va_scores["test_crps"][276])


# ------------------------------------------------------------------ 7. va_every
def test_va_every(gpu_ctx):
    X, y, Z, th, _, _, Xv, yv = va_small(2, 130, nv=64)
    kw = dict(itr=7, keep_z=True)
    r1 = call(gpu_ctx, "loo_crps", X, y, Z, th, Xv, yv, va_every=1, **kw)
    r3 = call(gpu_ctx, "loo_crps", X, y, Z, th, Xv, yv, va_every=3, **kw)
    r9 = call(gpu_ctx, "loo_crps", X, y, Z, th, Xv, yv, va_every=9, **kw)
    r0 = call(gpu_ctx, "loo_crps", X, y, r1.Z, r1.theta, Xv, yv, va_every=4, itr=0, keep_z=True)
    assert list(r1.va_steps) == list(range(8)) and list(r3.va_steps) == [0, 3, 6, 7]
    assert list(r9.va_steps) == [0, 7] and list(r0.va_steps) == [0]
    for k in SCORES:
        a = r1.va_scores[k]
        assert a.shape == (2, 8) and np.isfinite(a).all(), k
        assert same_bits(r3.va_scores[k], a[:, [0, 3, 6, 7]]), k
        assert same_bits(r9.va_scores[k], a[:, [0, 7]]), k
        assert r0.va_scores[k].shape == (2, 1)
        assert same_bits(r0.va_scores[k][:, 0], a[:, 7]), k  # the final pass alone, at the final θ, Z
    assert same_bits(r3.va_Z, r1.va_Z[:, [0, 3, 6, 7]]) and same_bits(r9.va_Z, r1.va_Z[:, [0, 7]])
    assert same_bits(r0.va_Z[:, 0], r1.Z)
    for r in (r1, r3, r9):
        assert same_bits(r.theta, r1.theta) and same_bits(r.series["theta"], r1.series["theta"])
        assert same_bits(r.Z, r1.Z) and same_bits(r.series["objective"], r1.series["objective"])


# ------------------------------------------------------------------ 8. failure
@pytest.mark.parametrize("block", [False, True])
def test_problems_that_fail_mid_fit(gpu_ctx, block):
    """test_failed_problems_leave_the_others_alone's construction at n = 140 (two chunks): problem 1
    has a NaN inducing coordinate and problem 3 a NaN training row in the second chunk (both fail
    at step 0: no finite row); problem 4's targets are scaled by 1e150 under NLML (pointwise path),
    so its first step is of the order of 1e297 and a later forward fails: the rows it reached are
    finite and right, later rows of va_sc and va_Z and the final row NaN.  These are return codes
    in info.  The neighbours keep every bit; select picks among the finite rows or gives −1."""
    X, y, Z, th, Xt, yt, Xv, yv = va_small(6, 140, nv=33)
    m, itr = Z.shape[1], 6
    Z[1, 2, 1] = np.nan
    X[3, 133, :] = np.nan
    obj = "dss" if block else "nlml"
    if not block:
        y[4] *= 1e150
        yv[4] *= 1e150
    good = [0, 2, 5] + ([4] if block else [])
    kw = dict(lr=1e-3, lr_z=1e-3, itr=itr, Xt=Xt, yt=yt, select="crps")
    res = call(gpu_ctx, obj, X, y, Z, th, Xv, yv, **kw)
    ref = call(gpu_ctx, obj, X[good], y[good], Z[good], th[good], Xv[good], yv[good],
               **{**kw, "Xt": Xt[good], "yt": yt[good]})
    print("info", res.info, "steps_done", res.steps_done)
    assert 1 <= res.info[1] <= m and res.steps_done[1] == 0
    assert m + 1 <= res.info[3] <= 2 * m and res.steps_done[3] == 0
    for q in (1, 3):
        assert np.isnan(rows_of(res, q)).all() and np.isnan(res.va_Z[q]).all()
        assert res.best_step[q] == -1 and np.isnan(res.theta_best[q]).all()
        assert np.isnan(res.Z_best[q]).all()
    if not block:
        done = int(res.steps_done[4])
        assert res.info[4] > 0 and 0 < done < itr
        rows = rows_of(res, 4)
        # the forward of step `done` failed: rows 0..done−1 were reached (row 0 at θ0, Z0 is finite;
        # a later reached row stands for a θ of the order of 1e297 and need not be)
        assert np.isfinite(rows[0]).all(), rows
        assert np.isnan(rows[done:]).all() and np.isnan(res.va_Z[4, done:]).all()
        assert not np.isnan(res.va_Z[4, :done]).any() and same_bits(res.va_Z[4, 0], Z[4])
        o, tol = row_tol(X[4], y[4], Xv[4], yv[4], Z[4], th[4])
        check_row(rows[0], o, tol, "failing, row 0")
        one = slice(4, 5)
        alone = call(gpu_ctx, obj, X[one], y[one], Z[one], th[one], Xv[one], yv[one], lr=1e-3,
                     lr_z=1e-3, itr=done, keep_z=True)
        assert same_bits(rows_of(alone, 0)[:done], rows[:done])
        c = res.va_scores["test_crps"][4]
        assert 0 <= res.best_step[4] < done and res.best_step[4] == int(np.nanargmin(c))
        assert same_bits(res.Z_best[4], res.va_Z[4, res.best_step[4]])
    # the neighbours
    assert not res.info[good].any()
    fr, fref = result_fields(res), result_fields(ref)
    for k, v in fr.items():
        assert same_bits(v[good], fref[k]), k
    for k in SCORES:
        assert same_bits(res.va_scores[k][good], ref.va_scores[k]), k
    assert same_bits(res.va_Z[good], ref.va_Z)
    assert same_bits(res.best_step[good], ref.best_step)
    assert same_bits(res.theta_best[good], ref.theta_best)
    assert same_bits(res.Z_best[good], ref.Z_best)


# ------------------------------------------------------------------ 9. the C-ABI's refusals
B9, N9, D9, M9, NV9, ITR9 = 2, 6, 2, 3, 3, 2
ENTRIES = {"gps_fitc_train_tall_va": False, "gps_fitc_blockloo_train_tall_va": True}
REFUSALS = [("nv", 0, "batch: nv must be in 1..2^24"),
            ("nv", (1 << 24) + 1, "batch: nv must be in 1..2^24"),
            ("va_every", 0, "batch: va_every must be in 1..2^20"),
            ("va_every", (1 << 20) + 1, "batch: va_every must be in 1..2^20"),
            ("Xv", None, "batch: Xv is NULL, a validated fit needs its validation rows"),
            ("yv", None, "batch: yv is NULL, a validated fit needs its validation targets"),
            ("va_sc", None, "batch: va_sc is NULL, a validated fit needs room for its score rows"),
            # the existing refusals keep their texts and come first
            ("nt", -1, "batch: nt must be in 0..2^24"),
            ("itr", -1, "batch: itr must be in 0..2^20"),
            ("z_out", None, "NULL argument")]


def arguments(block, nprob=B9, itr=ITR9, series=True, keep_z=True):
    rng = np.random.default_rng(7)
    X = rng.normal(size=(B9, N9, D9))
    Xv = rng.normal(size=(B9, NV9, D9))
    a = dict(objective=0 if block else 1)
    if block:
        a["nfold"] = 2
    a.update(nprob=nprob, X=X, y=np.sin(X.sum(axis=2)), n=N9, d=D9,
             Z=rng.uniform(-1, 1, (B9, M9, D9)), m=M9,
             theta=np.tile([0.0, 0.1, -0.1, -2.0], (B9, 1)), n_ell=D9, itr=itr, lr=0.01, lr_z=0.01,
             Xv=Xv, yv=np.sin(Xv.sum(axis=2)), nv=NV9, va_every=1, Xt=None, yt=None, nt=0, flags=0,
             theta_out=np.zeros((B9, 2 + D9)), z_out=np.zeros((B9, M9, D9)),
             values=np.zeros((B9, ITR9)) if series else None,
             thetas=np.zeros((B9, ITR9, 2 + D9)) if series else None, obj=np.zeros((B9, 5)),
             mu=None, var=None, sc=None, va_sc=np.full((B9, ITR9 + 1, 6), -7.0),
             va_z=np.full((B9, ITR9 + 1, M9, D9), -7.0) if keep_z else None,
             info=np.full(B9, -1, np.int32), steps_done=np.full(B9, -1, np.int32))
    return a


def run_valid(gpu_ctx, entry):
    from test_gpu_batch_refusals import positional
    for keep_z in (True, False):
        ok = arguments(ENTRIES[entry], keep_z=keep_z)
        gpu_ctx.call(entry, *positional(ok))
        assert (ok["info"] == 0).all() and (ok["steps_done"] == ITR9).all()
        assert np.isfinite(ok["va_sc"]).all() and (ok["va_sc"] != -7.0).all()
        if keep_z:
            assert same_bits(ok["va_z"][:, 0], ok["Z"]) and same_bits(ok["va_z"][:, -1], ok["z_out"])


@pytest.mark.parametrize("entry", sorted(ENTRIES))
@pytest.mark.parametrize("arg,bad,msg", REFUSALS)
def test_refusal_and_recovery(gpu_ctx, entry, arg, bad, msg):
    from gpscore import GpsError
    from test_gpu_batch_refusals import positional
    a = arguments(ENTRIES[entry])
    assert arg in a
    a[arg] = bad
    with pytest.raises(GpsError) as e:
        gpu_ctx.call(entry, *positional(a))
    assert str(e.value) == f"{entry} failed (-1): {msg}"
    assert (a["va_sc"] == -7.0).all() if a["va_sc"] is not None else True
    assert (a["va_z"] == -7.0).all()
    run_valid(gpu_ctx, entry)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_va_sc_and_va_z_count_towards_the_8gib_guard(gpu_ctx, entry):
    """nprob = 2^15, n = 6, d = 2, m = 3, itr = 4000, no test rows: the plain outputs are
    2^15·(4000·5 + 11) = 0.61·2^30 doubles and pass the guard (the inputs and the workspace do
    too).  va_sc's 2^15·4001·6 = 0.73·2^30 more tip it over; with two rows (va_every = 4000) va_sc
    passes, and va_z's 2^15·2·6 passes too, but at va_every = 2 (2001 rows) va_sc's 0.37·2^30 passes
    alone and va_z's equal share tips it over.  The passing calls are not made, since nothing stands
    behind the small arrays they would read: the arithmetic is asserted instead.  A refused call
    reads none."""
    from gpscore import GpsError
    from test_gpu_batch_refusals import positional
    nprob, itr, nth, mz = 1 << 15, 4000, 2 + D9, M9 * D9
    plain = nprob * itr * (1 + nth) + nprob * (5 + 6)
    assert plain <= 1 << 30 < plain + nprob * (itr + 1) * 6
    assert plain + nprob * 2 * (6 + mz) <= 1 << 30
    assert plain + nprob * 2001 * 6 <= 1 << 30 < plain + nprob * 2001 * (6 + mz)
    block = ENTRIES[entry]
    stride = (4 * N9 * (M9 | 1) + 3 * M9 * (M9 | 1) + 11 * N9) if block \
        else (2 * N9 * (M9 | 1) + 9 * N9)
    assert nprob * stride <= 1 << 30 and nprob * (N9 + NV9) * (D9 + 1) + nprob * mz <= 1 << 30
    for va_every, keep_z in ((1, False), (2, True)):
        a = arguments(block, nprob=nprob, itr=itr, series=False, keep_z=keep_z)
        a["va_every"] = va_every
        with pytest.raises(GpsError) as e:
            gpu_ctx.call(entry, *positional(a))
        assert str(e.value) == (f"{entry} failed (-1): batch: more than 8 GiB of inputs or outputs, "
                                "split the batch")
    run_valid(gpu_ctx, entry)


def test_va_launches_have_their_own_profiling_tags(gpu_ctx):
    X, y, Z, th, _, _, Xv, yv = va_small(2, 150, nv=9)
    gpu_ctx.prof(True)
    call(gpu_ctx, "nlml", X, y, Z, th, Xv, yv, itr=40)  # two launches
    call(gpu_ctx, "dss", X, y, Z, th, Xv, yv, itr=3)
    rep = gpu_ctx.prof_collect()
    gpu_ctx.prof(False)
    assert rep["batch_fitc_tall_va_train"]["count"] == 1, rep
    assert rep["batch_fitc_tall_block_va_train"]["count"] == 1, rep
    assert rep["batch_fitc_tall_va_train"]["ms"] > 0
    assert "batch_fitc_tall_train" not in rep and "batch_fitc_tall_block_train" not in rep


# ------------------------------------------------------------------ 10. the harness
HARNESS_SEED = 3  # test_gpu_fitc_tall.py's and test_gpu_fitc_tall_block.py's: chosen on the CPU


def test_run_fitc_validated_batch_against_its_parts(gpu_ctx):
    """TT = 3 replicates of synthetic sheets, six steps a method, select = "crps": the standard
    entries are run_fitc_batch's and run_fitc_blockloo_batch's for the same seed and method set,
    bitwise; "selected" is a hand-made fitc_train_tall(itr=0) call at (theta_best, Z_best) on the
    problems the runner drew, and the first call's metrics where the best row is the final one."""
    import gpscore
    from gpscore import experiment as E
    sheets = E.synthetic_sheets(0)
    TT, itr, seed = 3, 6, HARNESS_SEED
    for names, plain in ((("crps", "logs"), E.run_fitc_batch), (("dss", "kc"),
                                                                 E.run_fitc_blockloo_batch)):
        methods = {k: E.K20_METHODS[k] for k in names}
        out = E.run_fitc_validated_batch(sheets, TT=TT, methods=methods, itr=itr, seed=seed,
                                         va_every=2, select="crps", ctx=gpu_ctx)
        ref = plain(sheets, TT=TT, methods=methods, itr=itr, seed=seed, ctx=gpu_ctx)
        rng = np.random.default_rng(seed)
        data = [E.replicate(sheets, j, n_pool=sheets["trainx"].shape[0]) for j in range(TT)]
        th0, Z0 = {k: [] for k in methods}, {k: [] for k in methods}
        for j in range(TT):
            for name, meth in methods.items():
                k, ell, noise = E.initial_theta(meth, 8, rng)
                th0[name].append(np.concatenate([[k], np.ravel(ell), [noise]]))
                Z0[name].append(rng.random((20, 8)) if meth.z_init == "rand"
                                else rng.standard_normal((20, 8)))
        st = lambda key: np.stack([dd[key] for dd in data])  # noqa: E731
        for name, meth in methods.items():
            o = out[name]
            assert set(o) == set(ref[name]) | {"va_scores", "va_steps", "best_step", "selected"}
            for k in ref[name]:
                assert same_bits(np.asarray(o[k], np.float64),
                                 np.asarray(ref[name][k], np.float64)), (name, k)
            assert list(o["va_steps"]) == [0, 2, 4, 6]
            assert o["va_scores"]["test_crps"].shape == (TT, 4)
            assert not np.asarray(o.get("failed", False)).any()
            kw = dict(lr=meth.lr, lr_z=meth.lr_z, itr=itr, va_every=2, select="crps",
                      Xt=st("test_x"), yt=st("test_y"), stale_noise=True)
            res = call(gpu_ctx, meth.objective, st("train_x"), st("train_y"), np.stack(Z0[name]),
                       np.stack(th0[name]), st("va_x"), st("va_y"), **kw)
            for k in SCORES:
                assert same_bits(o["va_scores"][k], res.va_scores[k]), (name, k)
            assert same_bits(o["best_step"], res.best_step)
            hand = gpscore.fitc_train_tall(st("train_x"), st("train_y"), res.Z_best, res.theta_best,
                                           itr=0, Xt=st("test_x"), yt=st("test_y"), ctx=gpu_ctx)
            final = res.best_step == itr
            for k in E.METRICS:
                want = np.where(final, o[k], hand.scores["test_" + k])
                assert same_bits(o["selected"][k], want), (name, k)
