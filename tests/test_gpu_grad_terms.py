"""The gradient layer's kernels on the device, term by term: loo_grad_terms,
fitc_grad_terms, fold_terms, fitc_grad_mdiag, grad_contract (<1>, <8>, <16> and the generic
instance) and fitc_grad_contract with their reductions, each launched alone through the
gps_*_diag entry points on the cases of tests/grad_cases.py and held, output by output, to the
extended-precision references and the derived bounds there.  Everything the kernels must not
read is NaN on the device, so every check starts with "all finite".  tests/test_grad_terms_host.py
shows on the CPU that a float64 restatement of each kernel meets the same bounds at half or less,
and that each built-in defect misses them.

Worst measured error / bound on an MI355X (`pytest -s` prints this run's; DESIGN §23 has the
table beside the CPU restatement's figures):
  loo terms           CRPS u 0.12  ct 0.10 | LogS u 0.40  ct 0.16
  fitc terms          CRPS ulam 0.10  h 0.08  hl2 0.10 | LogS ulam 0.26  h 0.09  hl2 0.09
                      alpha 0.57  dinv 0.22 (sharp three- and four-rounding bounds)
  fold terms          gm 0.11  gc 0.11  value 0.04
  mdiag               mdiag 0.19  s1 0.30  s2 0.43
  grad_contract       <0> 0.05  <1> 0.03  <8> 0.05  <16> 0.03; n = 1473: 0.01
  fitc_grad_contract  out 0.28  zout 0.70 (the row difference is one fma: the bound's R term);
                      nr = 70 000: 0.00, nr = 4097: zout 0.31
With the parent commit's loo_grad_terms_kernel (r = y − (y − α/d)) the same run gives CRPS u
68 / 825 / 1.3e8 × bound at y = 0.3 / −7 / 1e6 and LogS u 1.5e15.
"""
import numpy as np
import pytest

import grad_cases as C
from elementwise_cases import LD

pytestmark = pytest.mark.gpu

RATIOS = {}


def record(name, ratio):
    RATIOS[name] = max(RATIOS.get(name, 0.0), float(ratio))
    print("grad terms gpu %-34s %.3f" % (name, ratio))
    return ratio


@pytest.fixture(scope="module")
def fx():
    return C.load_fixture()


def nan(*shape):
    return np.full(shape, np.nan)


def held(name, got, ref, tol):
    assert np.isfinite(got).all(), name
    r = record(name, C.worst_ratio(got, ref, tol))
    assert r <= 1.0, (name, r)


# ====================================================================== per-point terms
def term_slices(total):
    """The whole fixture once, then the seam sizes as windows into it."""
    yield 0, total
    for k, n in enumerate(C.TERM_N):
        yield 37 * k, n


def run_loo(ctx, fx, obj, lo, n, n_pad):
    idx = slice(lo, lo + n)
    y, a, d = (np.ascontiguousarray(fx[k][idx]) for k in ("y", "full_alpha", "full_dinv"))
    u, ct = nan(n_pad), nan(n_pad)
    ctx.grad_terms_diag(0, obj, n, n_pad, [y, a, d], [u, ct])
    return idx, u, ct


@pytest.mark.parametrize("obj", [C.OBJ_CRPS, C.OBJ_LOGS], ids=["crps", "logs"])
def test_loo_grad_terms(gpu_ctx, fx, obj):
    """u and ct of every fixture point, large |y| against small s included (the residual is
    α/d, not y − (y − α/d)); the pad entries are exactly 0."""
    for lo, n in term_slices(len(fx["y"])):
        for n_pad in C.pads_of(n):
            idx, u, ct = run_loo(gpu_ctx, fx, obj, lo, n, n_pad)
            ref, tol, _ = C.full_point_reference(fx, obj, idx, n)
            assert not u[n:].any() and not ct[n:].any(), (n, n_pad)
            held("loo %s u" % obj, u[:n], ref["u"], tol["u"])
            held("loo %s ct" % obj, ct[:n], ref["h"], tol["h"])


def test_loo_grad_terms_tiny_alpha(gpu_ctx, fx):
    """α = ±1e-300-sized with y = 0.3: the LogS u is not 0 (the detour through the LOO mean
    returned exactly 0 here)."""
    k = np.flatnonzero((np.abs(fx["full_alpha"]) < 1e-200) & (fx["full_alpha"] != 0) & (fx["y"] == 0.3))
    assert len(k) >= 14
    y, a, d = (np.ascontiguousarray(fx[q][k]) for q in ("y", "full_alpha", "full_dinv"))
    u, ct = nan(len(k)), nan(len(k))
    gpu_ctx.grad_terms_diag(0, C.OBJ_LOGS, len(k), len(k), [y, a, d], [u, ct])
    assert u.all() and np.isfinite(u).all()


@pytest.mark.parametrize("obj", [C.OBJ_NLML, C.OBJ_CRPS, C.OBJ_LOGS], ids=["nlml", "crps", "logs"])
def test_fitc_grad_terms(gpu_ctx, fx, obj):
    names = ("alpha", "dinv", "v", "ulam", "h", "hl2")
    for lo, n in term_slices(len(fx["y"])):
        idx = slice(lo, lo + n)
        ins = [np.ascontiguousarray(fx[k][idx]) for k in ("y", "fitc_lam", "fitc_r", "fitc_g")]
        ref, tol = C.fitc_point_reference(fx, obj, idx, n)
        for n_pad in C.pads_of(n):
            outs = [nan(n_pad) for _ in names]
            gpu_ctx.grad_terms_diag(1, obj, n, n_pad, ins, outs, scal=float(n))
            for name, o in zip(names, outs):
                assert not o[n:].any(), (name, n, n_pad)
                held("fitc %s %s" % (obj, name), o[:n], ref[name], tol[name])
            if obj == C.OBJ_NLML:
                assert np.array_equal(outs[2][:n], 0.5 * outs[0][:n])
                assert not outs[3].any() and not outs[4].any() and not outs[5].any()
            else:
                assert not outs[2].any()


@pytest.mark.parametrize("b", C.FOLD_B)
def test_fold_terms(gpu_ctx, fx, b):
    idx = slice(100, 100 + b)
    y, r, c = (np.ascontiguousarray(fx[k][idx]) for k in ("y", "fold_r", "fold_c"))
    gm, gc, val = nan(b), nan(b), nan(1)
    gpu_ctx.grad_terms_diag(2, C.OBJ_CRPS, b, b, [y, r, c], [gm, gc, val])
    ref, tol = C.fold_point_reference(fx, idx, b)
    held("fold gm", gm, ref["gm"], tol["gm"])
    held("fold gc", gc, ref["gc"], tol["gc"])
    want, vt = C.fold_sum_reference(r, c, b)
    assert np.isfinite(val[0]) and record("fold value", abs(val[0] - want) / vt) <= 1.0
    val2 = nan(1)
    gpu_ctx.grad_terms_diag(2, C.OBJ_CRPS, b, b, [y, r, c], [None, None, val2])   # gm = NULL
    assert val2[0] == val[0]


@pytest.mark.parametrize("m_pad", C.MDIAG_MPAD)
@pytest.mark.parametrize("kn,h", [(True, True), (False, False), (True, False)],
                         ids=["kn_h", "no_kn_no_h", "kn_no_h"])
def test_fitc_grad_mdiag(gpu_ctx, m_pad, kn, h):
    p = C.mdiag_inputs(m_pad)
    n, n_pad = C.MDIAG_N, C.MDIAG_NPAD
    ins = [p["KN"] if kn else None, p["K"] if kn else None, p["lam"], p["r"], p["dinv"], p["alpha"],
           p["v"], p["h"] if h else None]
    outs = [nan(n_pad) for _ in range(4)]
    gpu_ctx.grad_terms_diag(3, 0, n, n_pad, ins, outs, scal=p["a"], m_pad=m_pad)
    ref, tol = C.mdiag_reference(p, m_pad, kn, h)
    for name, o in zip(("mdiag", "s1", "s2"), outs):
        assert not o[n:].any(), name
        held("mdiag " + name, o[:n], ref[name], tol[name])
    assert np.array_equal(outs[3][:n], -2.0 * outs[0][:n]) and not outs[3][n:].any()


# ====================================================================== the full contraction
def run_full(ctx, case, coef):
    A, X, v = case.operands(coef)
    return ctx.grad_contract_diag(case.x, case.inv, case.sf2, A, X, case.ld, case.alpha, v,
                                  np.array(coef))


def check_full(case, coef, out, name):
    ref, tol = case.reference(coef)
    assert np.isfinite(out).all(), (name, out)
    dead = np.ones((case.passes, 16), bool)
    dead.reshape(-1)[:case.d] = False
    assert not out[:, 2:][dead].any(), "slots of dimensions >= d must be exactly 0"
    r = record(name, C.worst_ratio(out, ref, tol))
    assert r <= 1.0, (name, case.n, case.d, r)


FULL_ALL = C.FULL_CASES + [C.FULL_LARGE]


@pytest.mark.parametrize("n,d", FULL_ALL, ids=["n%d_d%d" % c for c in FULL_ALL])
def test_grad_contract(gpu_ctx, n, d):
    """Every coefficient set; absent operands and everything outside the real lower triangle
    are NaN, so a wrong guard shows as a non-finite output.  Two calls agree bitwise."""
    case = C.FullCase(n, d)
    inst = {1: "<1>", 8: "<8>", 16: "<16>"}.get(d, "<0>")
    for cname, coef in C.COEF_SETS.items():
        out = run_full(gpu_ctx, case, coef)
        check_full(case, coef, out, "contract %s %s%s" % (inst, cname, " n1473" if n > 1000 else ""))
        assert np.array_equal(out, run_full(gpu_ctx, case, coef))


def test_grad_contract_template_against_generic(gpu_ctx):
    """<8> and the generic instance on the same d = 8 input (the generic one reached with a
    ninth feature that is identically zero: Δ_9 = 0 adds nothing to any sum) agree within the
    bound; they need not be bitwise equal."""
    case = C.FullCase(129, 8)
    wide = C.FullCase(129, 8)
    wide.d, wide.x = 9, np.ascontiguousarray(np.hstack([case.x, np.zeros((case.n, 1))]))
    wide.inv = np.append(case.inv, 1.0)
    coef = C.COEF_SETS["all"]
    ref, tol = case.reference(coef)
    o8, o9 = run_full(gpu_ctx, case, coef), run_full(gpu_ctx, wide, coef)
    assert np.isfinite(o9).all() and not o9[0, 10:].any()
    assert record("contract <0> on d = 8", C.worst_ratio(o9[:, :10], ref[:, :10], tol[:, :10])) <= 1.0
    assert record("contract <8> on d = 8", C.worst_ratio(o8, ref, tol)) <= 1.0
    assert np.all(np.abs(LD(1) * o8[:, :10] - o9[:, :10]) <= 2 * tol[:, :10])


def test_grad_contract_permuted_dimensions(gpu_ctx):
    case = C.FullCase(65, 17)
    coef = C.COEF_SETS["all"]
    perm = np.random.default_rng(3).permutation(case.d)
    other = C.FullCase(65, 17)
    other.x, other.inv = np.ascontiguousarray(case.x[:, perm]), case.inv[perm]
    out = run_full(gpu_ctx, other, coef)
    assert np.isfinite(out).all()
    flat = lambda o: o[:, 2:].reshape(-1)[:case.d]
    ref, tol = case.reference(coef)
    assert C.worst_ratio(flat(out), flat(ref)[perm], flat(tol)[perm]) <= 1.0
    assert C.worst_ratio(out[:, :2], ref[:, :2], tol[:, :2]) <= 1.0


# ====================================================================== the FITC contraction
def fitc_id(c):
    return "nr%d_nc%d_pad%d_d%d_nt%d" % (c[0], c[1], c[2], c[3], c[4][0])


def run_fitc(ctx, case):
    return ctx.fitc_contract_diag(case.xr, case.xc, case.nc_pad, case.inv, case.sf2, **case.call_args())


FITC_ALL = C.fitc_cases() + list(C.FITC_LARGE)


@pytest.mark.parametrize("c", FITC_ALL, ids=fitc_id)
def test_fitc_grad_contract(gpu_ctx, c):
    """Rows >= nr and columns >= nc of every operand are NaN on the device, as are the vectors of
    a rank-one term that is off."""
    case = C.FitcCase(*c)
    out, zout = run_fitc(gpu_ctx, case)
    ref, zref, tol, ztol = case.reference()
    assert np.isfinite(out).all() and np.isfinite(zout).all()
    dead = np.ones((case.passes, 16), bool)
    dead.reshape(-1)[:case.d] = False
    assert not out[:, 1:][dead].any()
    assert not zout[case.zero_col].any(), "an all-zero G column must give exactly 0"
    inst = {1: "<1>", 8: "<8>", 16: "<16>"}.get(case.d, "<0>")
    tag = " nr%d" % case.nr if case.nr > 1000 else ""
    assert record("fitc contract %s out%s" % (inst, tag), C.worst_ratio(out, ref, tol)) <= 1.0
    assert record("fitc contract %s zout%s" % (inst, tag), C.worst_ratio(zout, zref, ztol)) <= 1.0
    if case.nr == 257 and case.nc == 65:
        o2, z2 = run_fitc(gpu_ctx, case)
        assert np.array_equal(out, o2) and np.array_equal(zout, z2)


def test_zz_report():
    """The worst error / bound per check over this run (DESIGN §23 quotes them; needs -s)."""
    for k in sorted(RATIOS):
        print("grad terms gpu worst %-34s %.3f" % (k, RATIOS[k]))
