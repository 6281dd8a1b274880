"""CPU side of the element-wise accuracy tests (test_gpu_elementwise.py): the fixture is what
its generator produces, the argument set of the exp_neg test covers the function's whole domain,
and every bound the GPU tests assert is met by plain float64 arithmetic — the libm exp and erf,
numpy's IEEE operations — on exactly the inputs the GPU tests use.  A bound that the reference
arithmetic itself could not meet would be a wish, not a derivation."""
import importlib.util
import os
from fractions import Fraction

import numpy as np
import pytest

import elementwise_cases as E

U, LD = E.U, E.LD


def _generator():
    path = os.path.join(E.GOLDEN, "make_score_terms.py")
    spec = importlib.util.spec_from_file_location("make_score_terms", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------ the fixture
def test_score_fixture_grid():
    """The committed inputs are the generator's grid (numpy's Generator stream is stable), the
    fixed z values all arrive in y, and the file stays small."""
    gen = _generator()
    g = E.load_score_fixture()
    m, c, y = gen.grid()
    nfix = len(gen.Z_FIXED) * len(gen.VARIANCES)
    assert len(m) == nfix + gen.N_RANDOM == len(g["m"])
    for k, v in (("m", m), ("c", c), ("y", y)):
        assert np.array_equal(g[k], v), k
    assert os.path.getsize(E.SCORE_FIXTURE) < 64 * 1024
    assert np.all(g["crps"] > 0) and np.all(np.isfinite(g["logs"].astype(np.float64)))
    # hi/lo is a non-overlapping pair: lo is below half a spacing of hi
    for k in ("crps", "logs"):
        assert np.all(np.abs(g[k + "_lo"]) <= 0.5 * np.spacing(np.abs(g[k + "_hi"])))


def test_score_fixture_regenerates_bitwise():
    """mpmath at 60 digits reproduces a sample of the committed references bit for bit."""
    pytest.importorskip("mpmath")
    gen = _generator()
    g = E.load_score_fixture()
    idx = np.arange(0, len(g["m"]), 5)
    r = gen.reference(g["m"][idx], g["c"][idx], g["y"][idx])
    for k, v in r.items():
        assert np.array_equal(g[k][idx], v), k


def test_score_term_bounds_hold_in_float64():
    """The float64 formulas with math.erf meet the per-term bounds on every fixture point."""
    g = E.load_score_fixture()
    t = E.score_terms_f64(g["m"], g["c"], g["y"])
    mse, sq0 = t[3], t[4]
    got = {E.SC_CRPS: t[0], E.SC_LOGS: t[1], E.SC_MSLL: t[2], E.SC_MSE: mse, E.SC_SMSE: mse / sq0}
    worst = {}
    for k, (ref, tol) in E.term_references(g).items():
        err = np.abs(got[k].astype(LD) - ref)
        assert np.all(err <= tol), (k, int(np.argmax(err - tol)))
        worst[k] = float(np.max(np.where(tol > 0, err / np.where(tol > 0, tol, 1), 0)))
    print("float64 error / bound:", worst)
    # the CRPS never cancels: CRPS/s >= 0.2337 (its value at z = 0)
    assert np.all(g["crps"] / np.sqrt(g["c"].astype(LD)) >= 0.2336)


# ------------------------------------------------------------------ exp_neg's argument set
def test_exp_argument_set_covers_the_domain():
    x, xp = E.exp_inputs()
    arg = E.exp_args(x, xp)
    assert arg.shape == (E.EXP_N, E.EXP_N) and np.all(arg <= 0)
    # reproduced exactly: each of the three operations is one correctly rounded IEEE operation
    # (checked against exact rational arithmetic on a sample that includes the row of x = 0,
    # where the squares go subnormal and −0.5·a rounds again)
    rows = np.r_[0, np.arange(1, E.EXP_N, 97)]
    for i in rows:
        for j in np.r_[np.arange(0, E.EXP_FINE, 53), np.arange(E.EXP_FINE, E.EXP_N)]:
            e = float(Fraction(float(x[i, 0])) - Fraction(float(xp[j, 0])))
            assert arg[i, j] == float(Fraction(float(Fraction(e) ** 2)) * Fraction(-1, 2))
    idx = E.exp_table_index(arg)
    a = arg.ravel()
    bands = {
        "zero": a == 0.0,
        "tiny": (a < 0) & (a >= -1e-290),
        "unit": (a < -1e-290) & (a >= -1.0),
        "normal": (a < -1.0) & (a >= -708.0),
        "subnormal": (a <= -708.4) & (a >= -745.2),
        "clamped": a < -746.0,
    }
    count = {k: int(v.sum()) for k, v in bands.items()}
    assert count["zero"] >= 1 and count["tiny"] >= 10 and count["unit"] >= 30000
    assert count["normal"] >= 800000 and count["subnormal"] >= 20000 and count["clamped"] >= 10000
    assert a[bands["tiny"]].max() >= -1e-300 and a.min() < -800.0
    # every table entry is read in the dense band, the wide band and the subnormal band
    for k in ("unit", "normal", "subnormal"):
        assert len(np.unique(idx.ravel()[bands[k]])) == 64, k
    # [−1, 0]: no gap above 1e-3 between neighbouring arguments; [−708, −1]: every one of 2048
    # uniform cells and of 512 logarithmic cells is hit
    unit = np.sort(a[(a >= -1.0)])
    assert np.max(np.diff(unit)) < 1e-3
    nrm = a[bands["normal"]]
    assert np.all(np.histogram(nrm, bins=2048, range=(-708.0, -1.0))[0] > 0)
    assert np.all(np.histogram(np.log(-nrm), bins=512, range=(0.0, np.log(708.0)))[0] > 0)
    assert np.all(np.histogram(a[bands["subnormal"]], bins=256, range=(-745.2, -708.4))[0] > 0)
    # decades of |arg| from 1e-300 to 1
    dec = np.floor(np.log10(-a[(a < 0) & (a > -1.0)])).astype(int)
    assert set(range(-301, 0, 2)) <= set(dec.tolist())


def test_exp_check_accepts_libm_and_rejects_a_coarse_exp():
    """The checker itself: the libm exp passes it; an exp that is 3e-14 off (a polynomial one
    degree short) or that flushes the subnormal results does not."""
    x, xp = E.exp_inputs()
    arg = E.exp_args(x, xp)[::4]
    ref = E.exp_reference(arg)
    good = np.exp(arg)
    assert E.exp_check(good, arg, ref) <= 1.0
    with pytest.raises(AssertionError):
        E.exp_check(good * (1.0 + 3e-14), arg, ref)
    with pytest.raises(AssertionError):
        E.exp_check(np.where(good < 2.0 ** -1022, 0.0, good), arg, ref)
    with pytest.raises(AssertionError):
        E.exp_check(np.where(arg < -700.0, np.exp(-700.0), good), arg, ref)


def test_exp_table_bias_sees_half_an_ulp_on_one_entry():
    """An exp whose results for one table entry are short by 0.4965 ulp of the entry's head (the
    tail of g_exp_tab[39], lost) moves that entry's mean error by that much and no other."""
    x, xp = E.exp_inputs()
    arg = E.exp_args(x, xp)
    ref = E.exp_reference(arg)
    good = ref.astype(np.float64)
    lost = float.fromhex("-0x1.fc6f89bd4f6bap-54") / float.fromhex("0x1.868d99b4492edp+0")
    # (exp rounded to float64 from the longdouble reference with the relative defect applied)
    bad = np.where(E.exp_table_index(arg) == 39, (ref * (1 - LD(lost))).astype(np.float64), good)
    shift = E.exp_table_bias(bad, arg, ref) - E.exp_table_bias(good, arg, ref)
    assert abs(shift[39] - 0.4965) < 0.05 and np.all(np.delete(shift, 39) == 0.0)
    assert abs(shift[39]) > 3 * E.EXP_BIAS_BOUND


# ------------------------------------------------------------------ Gram bounds
@pytest.mark.parametrize("n,m,uplo", E.GRAM_SHAPES)
@pytest.mark.parametrize("d", E.GRAM_DIMS)
def test_gram_bound_holds_for_direct_difference(d, n, m, uplo):
    case = E.GramCase(d, n, m, uplo)
    worst, where = case.worst(E.emulate_direct(case), case.tol_direct())
    assert worst <= 1.0, (worst, where)
    _inputs_cover(case)


def _inputs_cover(case):
    """One matrix holds arguments from 0 to below −800, exact and near duplicates included."""
    a = case.arg[case.mask].astype(np.float64)
    assert a.max() == 0.0 and a.min() < -800.0
    for lo, hi in ((-1e-27, -1e-33), (-0.5, -1e-3), (-10.0, -1.0), (-100.0, -10.0),
                   (-700.0, -100.0), (-745.0, -708.4), (-2000.0, -746.0)):
        assert np.any((a >= lo) & (a <= hi)), (lo, hi)
    i, j = E.gram_duplicates(case.uplo, case.n)
    assert np.all(case.arg[i, j] == 0)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("n,m,uplo", E.GRAM_SHAPES)
@pytest.mark.parametrize("d", [8, 16])
def test_gram_bound_holds_for_centred_expansion(d, n, m, uplo, fused):
    case = E.GramCase(d, n, m, uplo)
    worst, where = case.worst(E.emulate_centred(case, fused=fused), case.tol_centred())
    assert worst <= 1.0, (worst, where)


@pytest.mark.parametrize("d", [8, 16])
def test_gram_bound_tells_the_uncentred_expansion(d):
    """Without the shift the expansion loses u·(‖x‖² + ‖x'‖²): the centred bound must see it."""
    case = E.GramCase(d, 333, 201, 0)
    worst, _ = case.worst(E.emulate_centred(case, centred=False), case.tol_centred())
    assert worst > 4.0, worst


def test_gram_bound_holds_rbf():
    case = E.GramCase(8, 333, 201, 0, rbf=True)
    assert case.worst(E.emulate_direct(case), case.tol_direct())[0] <= 1.0
    assert case.worst(E.emulate_centred(case), case.tol_centred())[0] <= 1.0


# ------------------------------------------------------------------ score sums
@pytest.mark.parametrize("nt", [n for n in E.SEAM_NT if n <= 1000])
def test_sum_bound_holds_for_pairwise_float64(nt):
    """A float64 sum of the terms in a tree like the device's (np.sum is pairwise) is inside the
    bound of the reduction test, whose reference is math.fsum."""
    m, c, y = E.seam_inputs(nt)
    t = E.score_terms_f64(m, c, y)
    ref, tol = E.sum_references(m, c, y)
    s = t.sum(1)
    got = {E.SC_CRPS: s[0] / nt, E.SC_LOGS: s[1] / nt, E.SC_MSLL: s[2] / nt, E.SC_SMSE: s[3] / s[4],
           E.SC_MSE: s[3] / nt, E.SC_COVER: s[5] / nt}
    for k in ref:
        assert abs(got[k] - ref[k]) <= tol[k], (k, got[k], ref[k], tol[k])
    assert np.log10(c.max() / c.min()) > (8 if nt > 1 else -1)
