"""The gradient layer's term-by-term checks on the CPU (the device side is
test_gpu_grad_terms.py).  A numpy float64 restatement of each kernel — its operations and its
summation order, tests/grad_cases.py — runs on the very cases the GPU test uses:

  * every bound holds on it with room: the worst ratio error / bound must stay <= 0.5 (a
    restatement over half a bound would mean the bound's derivation is wrong);
  * each defect of the table below, built into a CPU copy only, fails the named check;
  * what the older normwise 1e-9 comparison computes for each defect is worked out here too.

Worst ratios of the restatement (x86-64 glibc; `pytest -s` prints them):
  loo_grad_terms     CRPS gm 0.10  gc 0.13  u 0.12  ct 0.10 | LogS gm 0.46  gc 0.33  u 0.40  ct 0.14
  fitc_grad_terms    CRPS ulam 0.10  h 0.10  hl2 0.11 | LogS ulam 0.26  h 0.07  hl2 0.09
                     alpha 0.57  dinv 0.22 (sharp three- and four-rounding bounds, held to 1)
  fold_terms         gm 0.09  gc 0.10  value 0.01 of 128u·Σ|t|
  fitc_grad_mdiag    mdiag 0.19  s1 0.30  s2 0.43 (sharp: one rounding against 1u)
  grad_contract      0.05 (nlml)  0.05 (loo)  0.05 (all four); n = 1473: 0.01
  fitc_grad_contract out 0.04  zout 0.21; fused row difference (one case) out 0.13  zout 0.30;
                     nr = 70 000: 0.00, nr = 4097: zout 0.31

Also, with no device: the three entry points are declared and bound at ABI 900, refuse a NULL
context and every bad argument before anything else.
"""
import math
import os

import numpy as np
import pytest

import grad_cases as C
from elementwise_cases import LD
from gpscore import _lib

HALF = 0.5
# alpha, dinv, v and s2 are one to four roundings each, bounded by exactly that count: a sharp
# bound, which plain rounding may approach, so for these four the restatement is held to 1
SHARP = ("alpha", "dinv", "v", "s2")
SEEN = {}


def record(name, ratio):
    SEEN[name] = max(SEEN.get(name, 0.0), ratio)
    print("ratio %-38s %.3f" % (name, ratio))
    return ratio


@pytest.fixture(scope="module")
def fx():
    return C.load_fixture()


ALL = slice(None)


# ====================================================================== the fixture
def _generator():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_grad_terms",
                                                  os.path.join(C.GOLDEN, "make_grad_terms.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_grid(fx):
    """The committed inputs are the generator's grid bit for bit, every listed z, d and y is
    there, the hi/lo pairs do not overlap, and the file stays small."""
    gen = _generator()
    grid = gen.grid()
    assert len(grid["y"]) == len(gen.Z_FIXED) * len(gen.D_LIST) * len(gen.Y_LIST) + gen.N_RANDOM
    for k, v in grid.items():
        assert np.array_equal(fx[k], v), k
    assert 0.8325546 in fx["z_target"] and -0.8325546 in fx["z_target"]
    assert set(gen.D_LIST) == set(fx["full_dinv"]) and set(gen.Y_LIST) == set(fx["y"])
    assert os.path.getsize(C.FIXTURE) < 256 * 1024
    for fam in ("full", "fitc", "fold"):
        for key in ("erf", "exp"):
            hi, lo = fx["%s_%s_hi" % (fam, key)], fx["%s_%s_lo" % (fam, key)]
            assert np.all(np.abs(lo) <= 0.5 * np.spacing(np.abs(hi))), (fam, key)
            assert np.all(np.abs(hi) <= 1.0)


def test_fixture_regenerates_bitwise(fx):
    """mpmath at 60 digits reproduces the committed references bit for bit."""
    pytest.importorskip("mpmath")
    gen = _generator()
    ref = gen.reference({k: fx[k] for k in gen.grid()})
    for k, v in ref.items():
        assert np.array_equal(fx[k], v), k


# ====================================================================== per-point terms
@pytest.mark.parametrize("obj", [C.OBJ_CRPS, C.OBJ_LOGS], ids=["crps", "logs"])
def test_loo_terms_restatement(fx, obj):
    n = len(fx["y"])
    ref, tol, _ = C.full_point_reference(fx, obj, ALL, n)
    u, ct = C.loo_terms_f64(fx["y"], fx["full_alpha"], fx["full_dinv"], n, obj)
    gm, gc = C.score_derivs_f64(obj, fx["full_alpha"] / fx["full_dinv"], 1.0 / fx["full_dinv"], n)
    for name, got in (("gm", gm / n), ("gc", gc / n), ("u", u), ("h", ct)):
        assert record("loo %d %s" % (obj, name), C.worst_ratio(got, ref[name], tol[name])) <= HALF


@pytest.mark.parametrize("obj", [C.OBJ_NLML, C.OBJ_CRPS, C.OBJ_LOGS], ids=["nlml", "crps", "logs"])
def test_fitc_terms_restatement(fx, obj):
    n = len(fx["y"])
    ref, tol = C.fitc_point_reference(fx, obj, ALL, n)
    got = C.fitc_terms_f64(fx["y"], fx["fitc_lam"], fx["fitc_r"], fx["fitc_g"], obj, float(n))
    for name in ("alpha", "dinv", "v", "ulam", "h", "hl2"):
        assert record("fitc %d %s" % (obj, name),
                      C.worst_ratio(got[name], ref[name], tol[name])) <= (1.0 if name in SHARP else HALF)
    if obj == C.OBJ_NLML:
        assert np.array_equal(got["v"], 0.5 * got["alpha"])
        assert not got["ulam"].any() and not got["h"].any() and not got["hl2"].any()


@pytest.mark.parametrize("b", C.FOLD_B)
def test_fold_terms_restatement(fx, b):
    idx = slice(100, 100 + b)
    r, c = fx["fold_r"][idx], fx["fold_c"][idx]
    ref, tol = C.fold_point_reference(fx, idx, b)
    gm, gc, val = C.fold_terms_f64(r, c, b)
    assert record("fold gm", C.worst_ratio(gm, ref["gm"], tol["gm"])) <= HALF
    assert record("fold gc", C.worst_ratio(gc, ref["gc"], tol["gc"])) <= HALF
    want, vt = C.fold_sum_reference(r, c, b)
    assert record("fold value", abs(val - want) / vt) <= HALF


@pytest.mark.parametrize("m_pad", C.MDIAG_MPAD)
@pytest.mark.parametrize("kn,h", [(True, True), (False, False), (True, False)])
def test_mdiag_restatement(m_pad, kn, h):
    p = C.mdiag_inputs(m_pad)
    ref, tol = C.mdiag_reference(p, m_pad, kn, h)
    got = C.mdiag_f64(p, m_pad, kn, h)
    for name in ("mdiag", "s1", "s2"):
        assert record("mdiag " + name,
                      C.worst_ratio(got[name], ref[name], tol[name])) <= (1.0 if name in SHARP else HALF)
    assert np.array_equal(got["s3"], -2.0 * got["mdiag"])


# ====================================================================== contractions
def check_full(case, coef, out, name):
    ref, tol = case.reference(coef)
    assert np.isfinite(out).all(), (name, out)
    r = C.worst_ratio(out, ref, tol)
    dead = np.ones((case.passes, 16), bool)
    dead.reshape(-1)[:case.d] = False
    assert not out[:, 2:][dead].any(), "slots of dimensions >= d must be exactly 0"
    return r


@pytest.mark.parametrize("n,d", C.FULL_CASES + [C.FULL_LARGE],
                         ids=["n%d_d%d" % c for c in C.FULL_CASES + [C.FULL_LARGE]])
def test_full_contraction_restatement(n, d):
    case = C.FullCase(n, d)
    for cname, coef in C.COEF_SETS.items():
        out = C.emulate_full(case, coef, case.operands(coef))
        assert record("full %s%s" % (cname, " large" if n > 1000 else ""),
                      check_full(case, coef, out, cname)) <= HALF


def test_full_contraction_permuted_dimensions():
    case = C.FullCase(65, 17)
    coef = C.COEF_SETS["all"]
    base = C.emulate_full(case, coef)
    perm = np.random.default_rng(3).permutation(case.d)
    other = C.FullCase(65, 17)
    other.x, other.inv = np.ascontiguousarray(case.x[:, perm]), case.inv[perm]
    out = C.emulate_full(other, coef)
    flat = lambda o: o[:, 2:].reshape(-1)[:case.d]
    ref, tol = case.reference(coef)
    assert C.worst_ratio(flat(out), flat(ref)[perm], flat(tol)[perm]) <= HALF
    assert C.worst_ratio(out[:, :2], ref[:, :2], tol[:, :2]) <= HALF
    assert C.worst_ratio(flat(base), flat(ref), flat(tol)) <= HALF


FITC_ALL = C.fitc_cases()


def fitc_id(c):
    return "nr%d_nc%d_pad%d_d%d_nt%d" % (c[0], c[1], c[2], c[3], c[4][0])


def check_fitc(case, out, zout):
    ref, zref, tol, ztol = case.reference()
    assert np.isfinite(out).all() and np.isfinite(zout).all()
    dead = np.ones((case.passes, 16), bool)
    dead.reshape(-1)[:case.d] = False
    assert not out[:, 1:][dead].any()
    assert not zout[case.zero_col].any(), "an all-zero G column must give exactly 0"
    return C.worst_ratio(out, ref, tol), C.worst_ratio(zout, zref, ztol)


@pytest.mark.parametrize("c", FITC_ALL + list(C.FITC_LARGE), ids=fitc_id)
def test_fitc_contraction_restatement(c):
    case = C.FitcCase(*c)
    out, zout = C.emulate_fitc(case)
    ro, rz = check_fitc(case, out, zout)
    tag = " large%d" % c[0] if c[0] > 1000 else ""
    assert record("fitc out" + tag, ro) <= HALF and record("fitc zout" + tag, rz) <= HALF


def test_fitc_contraction_fused_row_difference():
    """The row-side difference in one rounding (what a contracting compiler makes of
    xri[k]*inv_ell[k] − xj[k]) is inside the same bound, thanks to its R_ij term."""
    case = C.FitcCase(63, 20, 128, 8, C.FITC_CONFIGS[0])
    out, zout = C.emulate_fitc(case, fused=True)
    ro, rz = check_fitc(case, out, zout)
    assert record("fitc out fused", ro) <= HALF and record("fitc zout fused", rz) <= HALF


# ====================================================================== the defect table
def test_defect_residual_detour(fx):
    """r = y − (y − α/d): fails the per-point bounds on the large-|y| points, and gives a LogS
    gm of exactly 0 at α = 1e-300 where the value is not."""
    n = len(fx["y"])
    worst = {}
    for obj in (C.OBJ_CRPS, C.OBJ_LOGS):
        ref, tol, _ = C.full_point_reference(fx, obj, ALL, n)
        u, ct = C.loo_terms_f64(fx["y"], fx["full_alpha"], fx["full_dinv"], n, obj, detour=True)
        worst[obj] = (C.worst_ratio(u, ref["u"], tol["u"]), C.worst_ratio(ct, ref["h"], tol["h"]))
        print("detour obj %d: u %.3g, ct %.3g x bound" % ((obj,) + worst[obj]))
        assert min(worst[obj]) > 1.0
        big = np.abs(fx["y"]) >= 0.3
        err = np.abs(C.ld(u) - ref["u"])
        q = np.where(err == 0, LD(0), err / np.where(tol["u"] > 0, tol["u"], LD(1)))
        assert float(np.max(q[big])) > 1.0 and float(np.max(q[~big], initial=0)) <= HALF
    k = np.flatnonzero((np.abs(fx["full_alpha"]) < 1e-200) & (fx["full_alpha"] != 0) & (fx["y"] == 0.3))
    u, _ = C.loo_terms_f64(fx["y"][k], fx["full_alpha"][k], fx["full_dinv"][k], n, C.OBJ_LOGS, detour=True)
    assert len(k) and not u.any()
    u, _ = C.loo_terms_f64(fx["y"][k], fx["full_alpha"][k], fx["full_dinv"][k], n, C.OBJ_LOGS)
    assert u.all()


def test_defect_truncated_constant(fx):
    n = len(fx["y"])
    ref, tol, _ = C.full_point_reference(fx, C.OBJ_CRPS, ALL, n)
    _, ct = C.loo_terms_f64(fx["y"], fx["full_alpha"], fx["full_dinv"], n, C.OBJ_CRPS, isp=C.K_ISP_SHORT)
    r = C.worst_ratio(ct, ref["h"], tol["h"])
    print("truncated constant: ct %.3g x bound" % r)
    assert r > 1.0


def test_defect_hl2_scaling(fx):
    n = len(fx["y"])
    ref, tol = C.fitc_point_reference(fx, C.OBJ_LOGS, ALL, n)
    got = C.fitc_terms_f64(fx["y"], fx["fitc_lam"], fx["fitc_r"], fx["fitc_g"], C.OBJ_LOGS, float(n),
                           hl2_once=True)
    assert C.worst_ratio(got["hl2"], ref["hl2"], tol["hl2"]) > 1.0
    assert C.worst_ratio(got["h"], ref["h"], tol["h"]) <= HALF


@pytest.mark.parametrize("defect,slots", [("diag_weight", "value"), ("row_guard", "trace"),
                                           ("pass_offset", "second pass")])
def test_defect_full_contraction(defect, slots):
    case = C.FullCase(65, 17)
    coef = C.COEF_SETS["all"]
    ref, tol = case.reference(coef)
    out = C.emulate_full(case, coef, defect=defect)
    q = np.abs(C.ld(out) - ref) / np.where(tol > 0, tol, 1)
    print("%s: worst %.3g x bound" % (defect, float(q.max())))
    if defect == "diag_weight":
        assert q[0, 0] > 1.0 and q[0, 1] <= HALF
    elif defect == "row_guard":
        assert out[0, 1] == 0.0 and q[0, 1] > 1.0
    else:
        assert q[0].max() <= HALF and q[1, 2] > 1.0


@pytest.mark.parametrize("defect", ["ungated_a0", "ungated_a2", "ungated_a3"])
def test_defect_ungated_operand(defect):
    """An absent operand is NaN on the device; a term that is not gated by its coefficient
    carries it to the output (0·NaN), and the finiteness check sees it."""
    case = C.FullCase(65, 8)
    coef = {"ungated_a0": C.COEF_SETS["loo"], "ungated_a2": C.COEF_SETS["nlml"],
            "ungated_a3": C.COEF_SETS["nlml"]}[defect]
    assert np.isfinite(C.emulate_full(case, coef, case.operands(coef))).all()
    assert not np.isfinite(C.emulate_full(case, coef, case.operands(coef), defect=defect)).all()


@pytest.mark.parametrize("defect", ["row_group", "missing_rs", "pass_offset", "ungated_pc"])
def test_defect_fitc_contraction(defect):
    case = C.FitcCase(257, 65, 128, 17, C.FITC_CONFIGS[0] if defect != "ungated_pc"
                      else C.FITC_CONFIGS[3])
    ref, zref, tol, ztol = case.reference()
    if defect == "ungated_pc":
        out, zout = C.emulate_fitc(case, poison_off=True)
        assert not np.isfinite(out[0]).any()
        return
    out, zout = C.emulate_fitc(case, defect=defect)
    ro, rz = C.worst_ratio(out, ref, tol), C.worst_ratio(zout, zref, ztol)
    print("%s: out %.3g, zout %.3g x bound" % (defect, ro, rz))
    if defect == "row_group":
        assert rz > 1.0 and ro <= HALF
    elif defect == "missing_rs":
        assert ro > 1.0 and rz > 1.0
    else:
        assert ro > 1.0 and C.worst_ratio(out[0], ref[0], tol[0]) <= HALF


def test_older_normwise_check_on_the_defects(fx):
    """What the older style of check (max|a − b| / max|b| <= 1e-9 on benign inputs: N(0, I)
    features, length-scales and variances near 1, |y| ~ 1, finite zeros where a kernel must not
    read, d <= 20) computes for each defect.  The kernels' outputs enter the gradient linearly,
    so the normwise error of the output vector is the figure.  Blind (the figure passes 1e-9):
    the detour, the truncated constant, the dropped pass offset at d <= 16, every ungated
    operand (0·0 adds 0).  Seen: the rest, at any shape that runs the code."""
    rng = np.random.default_rng(11)
    n = 500
    y, d = rng.standard_normal(n), rng.uniform(0.5, 20.0, n)
    a = rng.standard_normal(n) * np.sqrt(d)
    nrel = lambda got, ref: float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
    fig = {}
    for obj in (C.OBJ_CRPS, C.OBJ_LOGS):
        good = C.loo_terms_f64(y, a, d, n, obj)
        fig["detour %d" % obj] = max(nrel(g, w) for g, w in
                                     zip(C.loo_terms_f64(y, a, d, n, obj, detour=True), good))
    good = C.loo_terms_f64(y, a, d, n, C.OBJ_CRPS)
    fig["constant"] = nrel(C.loo_terms_f64(y, a, d, n, C.OBJ_CRPS, isp=C.K_ISP_SHORT)[1], good[1])
    lam, r, g = rng.uniform(0.5, 2.0, n), rng.uniform(0.0, 0.2, n), rng.standard_normal(n)
    good = C.fitc_terms_f64(y, lam, r, g, C.OBJ_CRPS, float(n))
    fig["hl2"] = nrel(C.fitc_terms_f64(y, lam, r, g, C.OBJ_CRPS, float(n), hl2_once=True)["hl2"], good["hl2"])
    coef = C.COEF_SETS["all"]
    for dd in (8, 20):
        case = C.benign_full(200, dd)
        good = C.emulate_full(case, coef)
        for defect in ("diag_weight", "row_guard", "pass_offset"):
            fig["%s d%d" % (defect, dd)] = nrel(C.emulate_full(case, coef, defect=defect), good)
    case = C.benign_full(200, 8)
    for defect, cs in (("ungated_a0", "loo"), ("ungated_a2", "nlml"), ("ungated_a3", "nlml")):
        zero = tuple(np.zeros_like(z) if o is None else o for o, z in
                     zip(case.operands(C.COEF_SETS[cs]), (case.Ainv, case.Mx, case.v)))
        good = C.emulate_full(case, C.COEF_SETS[cs], zero)
        fig[defect] = nrel(C.emulate_full(case, C.COEF_SETS[cs], zero, defect=defect), good)
    fc = C.benign_fitc(300, 40, 8, C.FITC_CONFIGS[0])
    go, gz = C.emulate_fitc(fc)
    for defect in ("row_group", "missing_rs"):
        o, z = C.emulate_fitc(fc, defect=defect)
        fig[defect] = max(nrel(o, go), nrel(z, gz))
    for k, v in fig.items():
        print("older normwise check, %-16s %.3g" % (k, v))
    blind = ("detour 1", "detour 2", "constant", "pass_offset d8", "ungated_a0", "ungated_a2", "ungated_a3")
    for k, v in fig.items():
        assert (v < 1e-9) == (k in blind), (k, v)


# ====================================================================== the entry points
NEW = ("gps_grad_terms_diag", "gps_grad_contract_diag", "gps_fitc_contract_diag")


def test_entry_points_declared_and_bound_at_abi_900():
    from test_abi import header_symbols
    syms = header_symbols()
    lib = _lib.load()
    assert _lib.ABI_VERSION == 900 and lib.gps_version() == 900
    for s in NEW:
        assert s in syms and s in _lib.SIGNATURES and hasattr(lib, s)


def last():
    return _lib.load().gps_last_error(None).decode()


def terms_args(which):
    v = np.ones(8)
    m = np.ones((8, 4))
    ins = {0: [v, v, v], 1: [v, v, v, v], 2: [v, v, v], 3: [m, m, v, v, v, v, v, v]}[which]
    outs = [np.zeros(8) for _ in range({0: 2, 1: 6, 2: 3, 3: 4}[which])]
    return dict(which=which, obj=1, n=8, n_pad=8, ins=ins, outs=outs, scal=1.0, m_pad=4)


def contract_args():
    n, d = 5, 3
    return dict(n=n, d=d, X=np.ones((n, d)), inv_ell=np.ones(d), sf2=1.0, Ainv=np.ones((n, n)),
                Mx=np.ones((n, n)), ld=n, alpha=np.ones(n), v=np.ones(n), a=np.ones(4),
                out=np.zeros(18))


def fitc_args():
    nr, nc, d = 6, 4, 3
    return dict(nr=nr, nc=nc, nc_pad=128, d=d, xr=np.ones((nr, d)), xc=np.ones((nc, d)),
                inv_ell=np.ones(d), sf2=1.0, R=[np.ones((nr, nc))], coef=[1.0], rs=[np.ones(nr)],
                pc=[1.0, 0.0], pv=[np.ones(nr), None], qv=[np.ones(nc), None], out=np.zeros(17),
                zout=np.zeros((nc, d)))


def test_null_context_is_refused():
    """Well-formed arguments and no context: each call gets as far as bind() and stops there."""
    for w in range(4):
        assert _lib.grad_terms_diag_raw(None, **terms_args(w)) == -1 and last() == "NULL context", w
    assert _lib.grad_contract_diag_raw(None, **contract_args()) == -1 and last() == "NULL context"
    assert _lib.fitc_contract_diag_raw(None, **fitc_args()) == -1 and last() == "NULL context"


def T(w=0, **kw):
    a = terms_args(w)
    a.update(kw)
    return a


def drop(seq, k):
    s = list(seq)
    s[k] = None
    return s


TERMS_REFUSED = [
    ("NULL in", T(ins=None), "NULL argument"),
    ("NULL out", T(outs=None), "NULL argument"),
    ("which 4", T(which=4), "which"),
    ("which -1", T(which=-1), "which"),
    ("n 0", T(n=0), "n must"),
    ("n too large", T(n=(1 << 20) + 1, n_pad=(1 << 20) + 1), "n must"),
    ("n_pad below n", T(n_pad=7), "n_pad"),
    ("n_pad too large", T(n_pad=(1 << 20) + 1), "n_pad"),
    ("non-finite scalar", T(1, scal=math.nan), "finite"),
    ("loo terms under NLML", T(obj=0), "objective"),
    ("loo terms objective 3", T(obj=3), "objective"),
    ("loo terms without alpha", T(ins=drop(terms_args(0)["ins"], 1)), "NULL input"),
    ("loo terms without ct", T(outs=drop(terms_args(0)["outs"], 1)), "NULL output"),
    ("fitc terms objective 3", T(1, obj=3), "objective"),
    ("fitc terms n_total 0", T(1, scal=0.0), "n_total"),
    ("fitc terms without g", T(1, ins=drop(terms_args(1)["ins"], 3)), "NULL input"),
    ("fitc terms without hl2", T(1, outs=drop(terms_args(1)["outs"], 5)), "NULL output"),
    ("fold terms padded", T(2, n_pad=32), "no padding"),
    ("fold terms gm without gc", T(2, outs=drop(terms_args(2)["outs"], 1)), "gm without gc"),
    ("fold terms without the value", T(2, outs=drop(terms_args(2)["outs"], 2)), "NULL output"),
    ("fold terms without c", T(2, ins=drop(terms_args(2)["ins"], 2)), "NULL input"),
    ("mdiag odd m_pad", T(3, m_pad=3), "m_pad"),
    ("mdiag m_pad 0", T(3, m_pad=0), "m_pad"),
    ("mdiag m_pad too large", T(3, m_pad=4098), "m_pad"),
    ("mdiag too many entries", T(3, n=1 << 20, n_pad=1 << 20, m_pad=64), "2^24"),
    ("mdiag KN without K", T(3, ins=drop(terms_args(3)["ins"], 1)), "KN without K"),
    ("mdiag without lam", T(3, ins=drop(terms_args(3)["ins"], 2)), "NULL input"),
    ("mdiag without s3", T(3, outs=drop(terms_args(3)["outs"], 3)), "NULL output"),
]


@pytest.mark.parametrize("why,kw,frag", TERMS_REFUSED, ids=[r[0] for r in TERMS_REFUSED])
def test_terms_diag_refusals(why, kw, frag):
    assert _lib.grad_terms_diag_raw(None, **kw) == -1
    assert last().startswith("gps_grad_terms_diag: ") and frag in last(), (why, last())


def test_terms_diag_accepts_the_optional_arrays():
    """NULL where the header allows it is not an argument error (the call reaches bind())."""
    ok = [T(2, outs=[None, None, np.zeros(1)]), T(3, ins=drop(drop(terms_args(3)["ins"], 0), 1)),
          T(3, ins=drop(terms_args(3)["ins"], 7)), T(2, outs=[None, np.zeros(8), np.zeros(1)])]
    for kw in ok:
        assert _lib.grad_terms_diag_raw(None, **kw) == -1 and last() == "NULL context", last()


def G(**kw):
    a = contract_args()
    a.update(kw)
    return a


CONTRACT_REFUSED = [
    ("no X", G(X=None), "NULL"), ("no inv_ell", G(inv_ell=None), "NULL"),
    ("no alpha", G(alpha=None), "NULL"), ("no coefficients", G(a=None), "NULL"),
    ("no out", G(out=None), "NULL"), ("d 0", G(d=0), "d must"), ("d 65", G(d=65), "d must"),
    ("n 0", G(n=0), "n must"), ("n too large", G(n=8193, ld=8193), "n must"),
    ("ld below n", G(ld=4), "ld must"), ("ld too large", G(ld=16385), "ld must"),
    ("sf2 not finite", G(sf2=math.inf), "finite"),
    ("a coefficient not finite", G(a=np.array([1.0, math.nan, 0.0, 0.0])), "finite"),
    ("a0 without Ainv", G(Ainv=None), "needs Ainv"),
    ("a2 without v", G(v=None), "needs v"),
    ("a3 without Mx", G(Mx=None), "needs Mx"),
]


@pytest.mark.parametrize("why,kw,frag", CONTRACT_REFUSED, ids=[r[0] for r in CONTRACT_REFUSED])
def test_contract_diag_refusals(why, kw, frag):
    assert _lib.grad_contract_diag_raw(None, **kw) == -1
    assert last().startswith("gps_grad_contract_diag: ") and frag in last(), (why, last())


def test_contract_diag_accepts_absent_operands_with_zero_coefficients():
    kw = G(Ainv=None, Mx=None, v=None, a=np.array([0.0, 1.0, 0.0, 0.0]))
    assert _lib.grad_contract_diag_raw(None, **kw) == -1 and last() == "NULL context", last()


def F(**kw):
    a = fitc_args()
    a.update(kw)
    return a


FITC_REFUSED = [
    ("no xr", F(xr=None), "NULL"), ("no xc", F(xc=None), "NULL"), ("no inv_ell", F(inv_ell=None), "NULL"),
    ("no pc", F(pc=None), "NULL"), ("no out", F(out=None), "NULL"), ("no zout", F(zout=None), "NULL"),
    ("d 0", F(d=0), "d must"), ("d 65", F(d=65), "d must"),
    ("nr 0", F(nr=0), "nr must"), ("nr too large", F(nr=(1 << 20) + 1), "nr must"),
    ("nc 0", F(nc=0), "nc must"), ("nc too large", F(nc=16385, nc_pad=16385), "nc must"),
    ("nc_pad below nc", F(nc_pad=3), "nc_pad"), ("nc_pad far above nc", F(nc_pad=256), "nc_pad"),
    ("nt 5", F(nt=5), "nt must"), ("nt -1", F(nt=-1), "nt must"),
    ("terms without R", F(R=[], nt=1, ldr=[4]), "need R"),
    ("a NULL matrix", F(R=[None], ldr=[4]), "NULL matrix"),
    ("ldr below nc", F(ldr=[3]), "ldr must"), ("ldr too large", F(ldr=[32769]), "ldr must"),
    ("coef not finite", F(coef=[math.nan]), "finite"),
    ("sf2 not finite", F(sf2=math.nan), "finite"),
    ("pc not finite", F(pc=[math.inf, 0.0]), "finite"),
    ("terms too large", F(nr=1 << 20, ldr=[16384]), "2^26"),
    ("rank-one term without pv", F(pv=[None, None]), "rank-one"),
    ("rank-one term without qv", F(qv=None), "rank-one"),
]


@pytest.mark.parametrize("why,kw,frag", FITC_REFUSED, ids=[r[0] for r in FITC_REFUSED])
def test_fitc_diag_refusals(why, kw, frag):
    assert _lib.fitc_contract_diag_raw(None, **kw) == -1
    assert last().startswith("gps_fitc_contract_diag: ") and frag in last(), (why, last())


def test_fitc_diag_accepts_no_terms_and_no_row_scales():
    for kw in (F(R=[], coef=[], rs=None, pc=[0.0, 0.0], pv=None, qv=None), F(rs=None), F(rs=[None])):
        assert _lib.fitc_contract_diag_raw(None, **kw) == -1 and last() == "NULL context", last()
