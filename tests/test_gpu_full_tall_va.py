"""The validated tall full-GP fits (gps_full_train_tall_va / gps_full_blockloo_train_tall_va,
DESIGN §34): every validation row against the oracle at the θ it stands for, the scripts' row
under stale_noise, the fit bitwise that of the plain calls, a row bitwise the final pass of an
itr = 0 call, the launch split, batch size and position change no bit, va_every, a problem that
fails mid-fit, the C-ABI refusals, and run_full_validated_batch against its parts.  Runs on the
GPU box.

Tolerances: the six scores of a row against oracle/gp_oracle.py's fast_full at 1e-8 (TOL8 of
tests/test_gpu_full_tall.py, `close`: relative beyond 1), at the tile-edge shapes max(1e-8, 30 × the
case's conditioning floor), the floor being the oracle on X perturbed by 1e-15 relative, same
metrics, with the cap 30 × floor <= 5e-9 asserted on the oracle alone, as that file computes it.
Everything else is bitwise."""
import functools

import numpy as np
import pytest

import gp_oracle as O
from test_gpu_batch import SCORES, close, result_fields, same_bits, tup_of
from test_gpu_full_tall import TOL8

pytestmark = pytest.mark.gpu


def va_problems(B, n, nv, d, vec=True, nt=0, seed=5):
    """B problems with a validation set (and nt test rows) each, their own θ; one ℓ per dimension
    with vec."""
    rng = np.random.default_rng(seed + 7 * n + nv)
    X, Xv = rng.standard_normal((B, n, d)), rng.standard_normal((B, nv, d))
    Xt = rng.standard_normal((B, max(nt, 1), d))
    w = rng.standard_normal(d) / np.sqrt(d)
    y = np.sin(X @ w) + 0.1 * rng.standard_normal((B, n))
    yv = np.sin(Xv @ w) + 0.1 * rng.standard_normal((B, nv))
    yt = np.sin(Xt @ w) + 0.1 * rng.standard_normal((B, max(nt, 1)))
    ell = np.log(np.linspace(1.2, 2.4, d)) if vec else np.array([np.log(1.5)])
    th = np.stack([np.concatenate([[0.1 + 0.02 * q], ell + 0.03 * q, [np.log(0.05) + 0.05 * q]])
                   for q in range(B)])
    return X, y, Xv, yv, Xt, yt, th


def theta_of_row(res, th0, q, r):
    """The θ validation row r of problem q stands for."""
    step = int(res.va_steps[r])
    if r == len(res.va_steps) - 1:
        return res.theta[q]
    return th0[q] if step == 0 else res.series["theta"][q, step - 1]


def oracle_scores(X, y, Xv, yv, th, kind):
    out = O.fast_full(X, y, Xv, yv, *tup_of(th), kind=kind)
    return np.array([out[k] for k in SCORES])


def row_tol(X, y, Xv, yv, th, kind):
    """(the oracle's six scores, the tolerance from the case's conditioning floor)."""
    ref = oracle_scores(X, y, Xv, yv, th, kind)
    r = np.random.default_rng(1)
    Xp = X * (1 + 1e-15 * r.standard_normal(X.shape))
    per = oracle_scores(Xp, y, Xv, yv, th, kind)
    ok = np.isfinite(ref)
    floor = float(np.max(np.abs(per[ok] - ref[ok]) / np.maximum(1.0, np.abs(ref[ok])), initial=0.0))
    assert 30 * floor <= 5e-9, floor  # the hard cap, on the reference alone
    return ref, max(TOL8, 30 * floor)


def check_row(got, ref, tol, what):
    for k, g, r in zip(SCORES, got, ref):
        print(what, k, "got %.17g ref %.17g" % (g, r))
        if np.isnan(r):  # n = 1: the train targets have no variance, MSLL is NaN in both
            assert np.isnan(g), (what, k, g, r)
        else:
            assert close(g, r, tol), (what, k, g, r, tol)


def rows_of(res, q):
    return np.stack([res.va_scores[k][q] for k in SCORES], axis=1)  # (nva, 6)


def call(gpu_ctx, obj, *a, nfold=None, validated=True, **kw):
    import gpscore
    if obj in ("dss", "kc"):
        f = gpscore.blockloo_train_tall_validated if validated else gpscore.blockloo_train_tall
        return f(*a, objective=obj, nfold=nfold or 4, ctx=gpu_ctx, **kw)
    f = gpscore.train_tall_validated if validated else gpscore.train_tall
    return f(*a, objective=obj, ctx=gpu_ctx, **kw)


LR = {"nlml": 1e-3, "loo_crps": 0.5, "loo_logs": 0.05, "dss": 1e-3, "kc": 0.1}

# ------------------------------------------------------------------ 1. against the oracle
# (n, nv, d, one ℓ per dimension, rbf, objective, nfold): n and nv over {1, 63, 64, 65, 130} paired,
# d over {1, 8, 16}, n_ell 1 and d, both kernels, the five objectives, two fold counts
ORACLE_CASES = [(1, 130, 1, False, False, "nlml", None),
                (63, 1, 8, True, False, "loo_crps", None),
                (64, 65, 16, True, False, "loo_logs", None),
                (65, 64, 1, False, True, "loo_crps", None),
                (130, 63, 8, False, False, "nlml", None),
                (130, 130, 16, True, False, "loo_logs", None),
                (64, 63, 8, False, True, "loo_crps", None),
                (63, 65, 8, True, False, "dss", 2),
                (64, 1, 1, False, True, "kc", 4),
                (65, 130, 16, False, False, "dss", 4),
                (130, 64, 8, True, False, "kc", 2),
                (130, 130, 1, False, False, "dss", 4)]


@pytest.mark.parametrize("n,nv,d,vec,rbf,obj,nfold", ORACLE_CASES)
def test_rows_vs_oracle(gpu_ctx, n, nv, d, vec, rbf, obj, nfold):
    """itr = 4, va_every = 2: rows for steps 0 and 2 and the final pass, each against the oracle at
    θ0, θ after step 1 and the final θ."""
    B = 2
    X, y, Xv, yv, _, _, th = va_problems(B, n, nv, d, vec)
    res = call(gpu_ctx, obj, X, y, th, Xv, yv, nfold=nfold, lr=LR[obj], itr=4, va_every=2, rbf=rbf)
    assert not res.info.any(), res.info
    assert list(res.va_steps) == [0, 2, 4]
    kind = "rbf" if rbf else "ARD"
    for q in range(B):
        got = rows_of(res, q)
        for r in range(3):
            t = theta_of_row(res, th, q, r)
            ref, tol = row_tol(X[q], y[q], Xv[q], yv[q], t, kind)
            check_row(got[r], ref, tol, (q, r))
        assert not same_bits(got[0], got[2])  # θ moved


# ------------------------------------------------------------------ 2. the scripts' row
@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("stale", [True, False])
def test_final_row_is_the_scripts_row(gpu_ctx, k, stale):
    """With stale_noise and itr = k the final row is the oracle at the kernel parameters θ_k with
    the log σ² of θ_{k−1} (θ0's for k = 1): va_series[k − 1] of the scripts; without the flag, θ_k."""
    X, y, Xv, yv, _, _, th = va_problems(2, 70, 33, 3)
    res = call(gpu_ctx, "loo_crps", X, y, th, Xv, yv, lr=0.5, itr=k, stale_noise=stale)
    assert not res.info.any() and res.va_steps[-1] == k
    for q in range(2):
        t = res.theta[q].copy()
        prev = th[q] if k == 1 else res.series["theta"][q, k - 2]
        assert prev[-1] != t[-1]  # the two noises differ, so the flag matters
        if stale:
            t[-1] = prev[-1]
        ref, tol = row_tol(X[q], y[q], Xv[q], yv[q], t, "ARD")
        check_row(rows_of(res, q)[-1], ref, tol, (q, "final"))


# ------------------------------------------------------------------ 3. the fit is untouched
@pytest.mark.parametrize("obj", ["loo_crps", "nlml", "dss", "kc"])
def test_validation_does_not_touch_the_fit(gpu_ctx, obj):
    """n = 130: 37 steps a launch, so itr = 40 spans two launches; every field of the plain call's
    result, bitwise."""
    X, y, Xv, yv, Xt, yt, th = va_problems(3, 130, 70, 3, nt=9)
    kw = dict(lr=LR[obj], itr=40, Xt=Xt, yt=yt, stale_noise=True)
    a = call(gpu_ctx, obj, X, y, th, Xv, yv, va_every=3, **kw)
    b = call(gpu_ctx, obj, X, y, th, validated=False, **kw)
    assert not b.info.any() and list(b.steps_done) == [40] * 3
    fa, fb = result_fields(a), result_fields(b)
    assert set(fa) == set(fb)
    for k in fb:
        assert same_bits(fa[k], fb[k]), k
    assert np.isfinite(rows_of(a, 0)).all()


# ------------------------------------------------------------------ 4. a row is an itr = 0 call
@pytest.mark.parametrize("obj", ["loo_logs", "dss"])
def test_a_row_is_an_itr0_call(gpu_ctx, obj):
    """Step 0, an interior checkpoint and the final row: bitwise the scores of the plain call's
    final pass at that θ with the validation rows as its test rows (nv = 70: one whole block of
    rows and a partial one)."""
    X, y, Xv, yv, _, _, th = va_problems(2, 130, 70, 3)
    res = call(gpu_ctx, obj, X, y, th, Xv, yv, lr=LR[obj], itr=7, va_every=2)
    assert not res.info.any() and list(res.va_steps) == [0, 2, 4, 6, 7]
    for r in (0, 2, 4):
        t = np.stack([theta_of_row(res, th, q, r) for q in range(2)])
        one = call(gpu_ctx, obj, X, y, t, validated=False, lr=LR[obj], itr=0, Xt=Xv, yt=yv)
        assert not one.info.any()
        for k in SCORES:
            assert same_bits(res.va_scores[k][:, r], one.scores[k]), (r, k)


# ------------------------------------------------------------------ 5. split, size, position
def test_launch_split_changes_no_row(gpu_ctx):
    """n = 130 gives three tiles and 37 steps a launch: with itr = 40 and va_every = 3 the
    checkpoints 0..36 fall in the first launch and 39 in the second.  Against 24 + 16 steps in two
    calls, the second from the first call's θ (the split is a multiple of va_every so that the step
    indices coincide): steps 0..21 are the first call's rows, step 24 is the first call's final row
    (no stale noise: the final pass at θ_24 is step 24's forward) and the second call's row 0, and
    27..39 and the final row are the second call's."""
    X, y, Xv, yv, Xt, yt, th = va_problems(3, 130, 70, 3, nt=9)
    kw = dict(lr=0.05, va_every=3, Xt=Xt, yt=yt)
    whole = call(gpu_ctx, "loo_logs", X, y, th, Xv, yv, itr=40, **kw)
    first = call(gpu_ctx, "loo_logs", X, y, th, Xv, yv, itr=24, **kw)
    second = call(gpu_ctx, "loo_logs", X, y, first.theta, Xv, yv, itr=16, **kw)
    assert not whole.info.any() and list(whole.steps_done) == [40] * 3
    assert list(whole.va_steps) == list(range(0, 40, 3)) + [40]
    assert list(first.va_steps) == list(range(0, 24, 3)) + [24]
    assert list(second.va_steps) == list(range(0, 16, 3)) + [16]
    assert same_bits(whole.theta, second.theta)
    for k in SCORES:
        w = whole.va_scores[k]
        assert same_bits(w[:, :9], first.va_scores[k]), k        # steps 0..21 and 24
        assert same_bits(w[:, 8:], second.va_scores[k]), k       # steps 24..39 and the final row
    assert not same_bits(whole.va_scores["test_crps"][:, 0], whole.va_scores["test_crps"][:, -1])


def test_batch_size_and_position_change_no_row(gpu_ctx):
    X, y, Xv, yv, Xt, yt, th = va_problems(5, 130, 70, 3, nt=9)
    kw = dict(lr=0.5, itr=5, va_every=2)
    for obj in ("loo_crps", "kc"):
        full = call(gpu_ctx, obj, X, y, th, Xv, yv, Xt=Xt, yt=yt, **kw)
        rev = call(gpu_ctx, obj, X[::-1], y[::-1], th[::-1], Xv[::-1], yv[::-1], Xt=Xt[::-1],
                   yt=yt[::-1], **kw)
        one = slice(3, 4)
        alone = call(gpu_ctx, obj, X[one], y[one], th[one], Xv[one], yv[one], Xt=Xt[one],
                     yt=yt[one], **kw)
        assert not full.info.any()
        for k in SCORES:
            assert same_bits(full.va_scores[k][3], alone.va_scores[k][0]), (obj, k)
            assert same_bits(full.va_scores[k], rev.va_scores[k][::-1]), (obj, k)
        assert not same_bits(full.va_scores["test_crps"][0], full.va_scores["test_crps"][1])


# ------------------------------------------------------------------ 6. va_every
def test_va_every(gpu_ctx):
    X, y, Xv, yv, _, _, th = va_problems(2, 65, 64, 3)
    kw = dict(lr=0.5, itr=7)
    r1 = call(gpu_ctx, "loo_crps", X, y, th, Xv, yv, va_every=1, **kw)
    r3 = call(gpu_ctx, "loo_crps", X, y, th, Xv, yv, va_every=3, **kw)
    r9 = call(gpu_ctx, "loo_crps", X, y, th, Xv, yv, va_every=9, **kw)
    r0 = call(gpu_ctx, "loo_crps", X, y, r1.theta, Xv, yv, va_every=4, lr=0.5, itr=0)
    assert list(r1.va_steps) == list(range(8)) and list(r3.va_steps) == [0, 3, 6, 7]
    assert list(r9.va_steps) == [0, 7] and list(r0.va_steps) == [0]
    for k in SCORES:
        a = r1.va_scores[k]
        assert a.shape == (2, 8) and np.isfinite(a).all(), k
        assert same_bits(r3.va_scores[k], a[:, [0, 3, 6, 7]]), k
        assert same_bits(r9.va_scores[k], a[:, [0, 7]]), k
        assert r0.va_scores[k].shape == (2, 1)
        assert same_bits(r0.va_scores[k][:, 0], a[:, 7]), k  # the final pass alone, at the final θ
    for r in (r1, r3, r9):
        assert same_bits(r.theta, r1.theta) and same_bits(r.series["theta"], r1.series["theta"])


# ------------------------------------------------------------------ 7. failure
def test_a_problem_that_fails_mid_fit(gpu_ctx):
    """Problem 1's targets are scaled by 1e6: its NLML gradient is ~1e12 times its neighbours', so
    the first update at the shared step size throws its θ outside the representable kernels and a
    forward of one of the next steps meets a pivot that is not > 0 (a return code, as
    test_failure_in_a_later_step's lr = 1e6 for a whole batch).  Problem 3 has a NaN in θ and fails
    at step 0.  Rows before the failure are finite and right, later rows and the final row NaN,
    the neighbours keep every bit, and select picks among the finite rows."""
    X, y, Xv, yv, Xt, yt, th = va_problems(5, 70, 33, 3, nt=9)
    y[1] *= 1e6
    yv[1] *= 1e6
    th[3, 1] = np.nan
    good = [0, 2, 4]
    kw = dict(lr=1e-3, itr=6, Xt=Xt, yt=yt)
    res = call(gpu_ctx, "nlml", X, y, th, Xv, yv, select="crps", **kw)
    ref = call(gpu_ctx, "nlml", X[good], y[good], th[good], Xv[good], yv[good], select="crps",
               **{**kw, "Xt": Xt[good], "yt": yt[good]})
    assert not res.info[good].any() and res.info[1] > 0 and res.info[3] > 0, res.info
    done = int(res.steps_done[1])
    assert 1 <= done <= 3 and res.steps_done[3] == 0, res.steps_done
    rows = rows_of(res, 1)
    assert np.isfinite(rows[:done]).all() and np.isnan(rows[done:]).all(), rows
    assert np.isnan(rows_of(res, 3)).all()
    assert np.isnan(res.scores["test_crps"][[1, 3]]).all()
    # right: row 0 against the oracle, and all of them bitwise the same problem alone, stopped
    # before the failing forward
    o, tol = row_tol(X[1], y[1], Xv[1], yv[1], th[1], "ARD")
    check_row(rows[0], o, tol, "failing, row 0")
    one = slice(1, 2)
    alone = call(gpu_ctx, "nlml", X[one], y[one], th[one], Xv[one], yv[one], lr=1e-3, itr=done)
    assert same_bits(rows_of(alone, 0)[:done], rows[:done])
    # the neighbours
    fr, fref = result_fields(res), result_fields(ref)
    for k, v in fr.items():
        assert same_bits(v[good], fref[k]), k
    for k in SCORES:
        assert same_bits(res.va_scores[k][good], ref.va_scores[k]), k
    assert same_bits(res.best_step[good], ref.best_step)
    assert same_bits(res.theta_best[good], ref.theta_best)
    # select: among the finite rows, −1 and NaN when there is none
    c = res.va_scores["test_crps"][1]
    assert 0 <= res.best_step[1] < done and res.best_step[1] == int(np.nanargmin(c))
    assert res.best_step[3] == -1 and np.isnan(res.theta_best[3]).all()
    assert np.isfinite(res.theta_best[1]).all()


# ------------------------------------------------------------------ 8. the C-ABI's refusals
B8, N8, D8, NV8, ITR8 = 2, 4, 2, 3, 2
ENTRIES = {"gps_full_train_tall_va": False, "gps_full_blockloo_train_tall_va": True}
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
            ("theta_out", None, "NULL argument")]


def arguments(block, nprob=B8, itr=ITR8, series=True):
    rng = np.random.default_rng(7)
    X = rng.normal(size=(B8, N8, D8))
    Xv = rng.normal(size=(B8, NV8, D8))
    a = dict(kind=0, objective=0 if block else 1)
    if block:
        a["nfold"] = 2
    a.update(nprob=nprob, X=X, y=np.sin(X.sum(axis=2)), n=N8, d=D8,
             theta=np.tile([0.0, 0.1, -0.1, -2.0], (B8, 1)), n_ell=D8, itr=itr, lr=0.01, Xv=Xv,
             yv=np.sin(Xv.sum(axis=2)), nv=NV8, va_every=1, Xt=None, yt=None, nt=0, flags=0,
             theta_out=np.zeros((B8, 2 + D8)),
             values=np.zeros((B8, ITR8)) if series else None,
             thetas=np.zeros((B8, ITR8, 2 + D8)) if series else None, obj=np.zeros((B8, 5)),
             mu=None, var=None, sc=None, va_sc=np.full((B8, ITR8 + 1, 6), -7.0),
             info=np.full(B8, -1, np.int32), steps_done=np.full(B8, -1, np.int32))
    return a


def run_valid(gpu_ctx, entry):
    from test_gpu_batch_refusals import positional
    ok = arguments(ENTRIES[entry])
    gpu_ctx.call(entry, *positional(ok))
    assert (ok["info"] == 0).all() and (ok["steps_done"] == ITR8).all()
    assert np.isfinite(ok["va_sc"]).all() and (ok["va_sc"] != -7.0).all()


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
    run_valid(gpu_ctx, entry)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_va_sc_counts_towards_the_8gib_guard(gpu_ctx, entry):
    """nprob = 2^15, n = 4, d = 2, itr = 4000, no test rows: the plain outputs are 2^15·(4000·5 +
    11) = 0.61·2^30 doubles and pass the guard (the inputs and the workspace, 2^15·8192 or
    2^15·16384 doubles, do too), va_sc's 2^15·4001·6 = 0.73·2^30 more tip it over.  With two rows
    (va_every = 4000) the sum would pass; that call is not made, since nothing stands behind the
    small arrays it would read: the arithmetic is asserted instead.  A refused call reads none."""
    from gpscore import GpsError
    from test_gpu_batch_refusals import positional
    nprob, itr, nth = 1 << 15, 4000, 2 + D8
    plain = nprob * itr * (1 + nth) + nprob * (5 + 6)
    assert plain <= 1 << 30 < plain + nprob * (itr + 1) * 6
    assert plain + nprob * 2 * 6 <= 1 << 30
    a = arguments(ENTRIES[entry], nprob=nprob, itr=itr, series=False)
    with pytest.raises(GpsError) as e:
        gpu_ctx.call(entry, *positional(a))
    assert str(e.value) == (f"{entry} failed (-1): batch: more than 8 GiB of inputs or outputs, "
                            "split the batch")
    run_valid(gpu_ctx, entry)


# ------------------------------------------------------------------ 9. the harness
def test_run_full_validated_batch_against_its_parts(gpu_ctx):
    """TT = 3 replicates of synthetic sheets, six steps a method, select = "crps": the standard
    metrics are run_full_batch's for the same seed, bitwise; "selected" is a hand-made
    train_tall(itr=0, theta0=theta_best) call on the problems the runner drew, and the first call's
    metrics where the best row is the final one."""
    import gpscore
    from gpscore import experiment as E
    sheets = E.synthetic_sheets(5, n_pool=2000, n_test=100)
    methods = {k: E.KF_METHODS[k] for k in ("crps", "logs")}
    TT, itr, seed = 3, 6, 7
    out = E.run_full_validated_batch(sheets, TT=TT, methods=methods, itr=itr, seed=seed,
                                     va_every=2, select="crps", ctx=gpu_ctx)
    ref = E.run_full_batch(sheets, TT=TT, methods=methods, itr=itr, seed=seed, ctx=gpu_ctx)
    rng = np.random.default_rng(seed)
    data = [E.replicate(sheets, j, n_pool=2000) for j in range(TT)]
    th0 = {k: [] for k in methods}
    for j in range(TT):
        for name, meth in methods.items():
            k, ell, noise = E.initial_theta(meth, 8, rng)
            th0[name].append(np.concatenate([[k], np.ravel(ell), [noise]]))
    st = lambda key: np.stack([dd[key] for dd in data])  # noqa: E731
    for name, meth in methods.items():
        o = out[name]
        assert set(o) == set(E.METRICS) | {"theta", "va_scores", "va_steps", "best_step", "selected"}
        for k in E.METRICS + ("theta",):
            assert same_bits(o[k], ref[name][k]), (name, k)
        assert list(o["va_steps"]) == [0, 2, 4, 6]
        assert o["va_scores"]["test_crps"].shape == (TT, 4)
        res = gpscore.train_tall_validated(st("train_x"), st("train_y"), np.stack(th0[name]),
                                           st("va_x"), st("va_y"), meth.objective, lr=meth.lr,
                                           itr=itr, va_every=2, select="crps", Xt=st("test_x"),
                                           yt=st("test_y"), stale_noise=True, ctx=gpu_ctx)
        for k in SCORES:
            assert same_bits(o["va_scores"][k], res.va_scores[k]), (name, k)
        assert same_bits(o["best_step"], res.best_step)
        hand = gpscore.train_tall(st("train_x"), st("train_y"), res.theta_best, itr=0,
                                  Xt=st("test_x"), yt=st("test_y"), ctx=gpu_ctx)
        final = res.best_step == itr
        for k in E.METRICS:
            want = np.where(final, o[k], hand.scores["test_" + k])
            assert same_bits(o["selected"][k], want), (name, k)
