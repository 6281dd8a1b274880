"""The vector layer's kernels on the device, one launch at a time: every kernel of
csrc/kernels_vec.hip — gemv_rows, colred, slab_sum, sym_slab_sum, sym_pack, sym_unpack,
partials_sum<2/4>, dot, full_loo_rows with full_loo_obj, fitc_lambda_rows, fitc_loo_rows,
pred_finalize, fitc_pred_finalize, surface_point_rows, pad_copy, local_sum — through its
production launcher and gps_vec_diag, on the cases of tests/vec_cases.py, held output by output to
the extended-precision references and the derived bounds there.  Everything a kernel must not
read is NaN on the device, so every check starts with "all finite"; then the bitwise parts, then
error / bound <= 1.  Each launch runs twice and must give the same bits (the file's header claims
fixed-order reductions).  tests/test_vec_host.py shows on the CPU that a float64 restatement of
each kernel meets the same bounds at half or less (at 1 for the few-rounding ones), and that
each built-in defect misses them.

Worst measured error / bound on an MI355X (`pytest -s` prints this run's; DESIGN §30 has the
table beside the CPU restatement's figures):
  gemv y 0.02 (at most four terms: 0.19) | colred s1 0.06 s2 0.05 (few terms 0.33, 0.51),
  chunk partials 0.20 | slab_sum 0.32 | sym_slab_sum 0.47 (few 0.53) | sym_pack packed 0.48
  dot 0.00 (few 0.09) | local_sum 0.09 (few 0.41) | pad_copy and every other exact check: bitwise
  full_loo    mu 0.82  var 1.00 (two roundings and one against exactly that count)
              sum crps 0.03  logs 0.02  logdiag 0.01  beta2 0.02 | nlml 0.03  loo_crps 0.02
              loo_logs 0.02; n_pad = 262 272: every sum <= 0.01
  fitc_lambda lam 0.51  inv_lam 0.62  ys 0.56 | sum loglam 0.02  y2/lam 0.03
  fitc_loo    mu 0.56  var 0.29 | sum crps 0.04  logs 0.03
  pred var 0.98 (one and two roundings) | surface sum crps 0.04  logs 0.02
  fitc chain  lam 0.13  var 0.20  logdet 0.01, mu and the other objectives 0.00
No kernel missed a bound.
"""
import numpy as np
import pytest

import vec_cases as C

pytestmark = pytest.mark.gpu

RATIOS = {}


def record(name, ratio):
    RATIOS[name] = max(RATIOS.get(name, 0.0), float(ratio))
    return ratio


def same_bits(a, b):
    return all((x is None and y is None) or C.exact(x, y) == 0.0 for x, y in zip(a, b))


def held(ctx, case, twice=True):
    """One case: all finite, the bitwise parts, every ratio <= 1; a second launch on the same
    input gives the same bits."""
    outs = C.run(ctx, case)
    res = C.check(case, outs)
    order = sorted(res, key=lambda k: (not k.startswith("finite"), not k.startswith("exact"), k))
    for name in order:
        tag = "%s %s%s" % (C.NAMES[case.which], name, " (few terms)" if C.few_terms(case) else "")
        r = record(tag, res[name])
        assert r <= (0.0 if name.startswith(("finite", "exact")) else 1.0), (case, name, r)
    if twice:
        assert same_bits(outs, C.run(ctx, case)), (case, "two launches differ")
    return outs


@pytest.mark.parametrize("which", range(14), ids=C.NAMES)
def test_vec_kernel(gpu_ctx, which):
    """Every case of one launcher (vec_cases.CASES[which]; the bounds are in the docstrings of
    the cases_* functions there)."""
    for case in C.CASES[which]():
        held(gpu_ctx, case)
    for k in sorted(RATIOS):
        if k.startswith(C.NAMES[which] + " "):
            print("vec gpu %-44s %.3f" % (k, RATIOS[k]))


def test_second_trip_of_the_partial_sums(gpu_ctx):
    """n_pad = 262 272 rows, 1025 workgroups: partials_sum_kernel<4> (full_loo) and <2>
    (fitc_lambda) walk their strided loop twice."""
    for case in C.large_cases():
        res = C.check(case, C.run(gpu_ctx, case))
        for name, r in res.items():
            record("%s %s (n_pad 262272)" % (C.NAMES[case.which], name), r)
            assert r <= (0.0 if name.startswith(("finite", "exact")) else 1.0), (case, name, r)
        print("vec gpu second trip", case, {k: round(v, 3) for k, v in res.items() if v})


def test_pack_at_large_e(gpu_ctx):
    """M = 2048, m = 2047, one slab: the packed triangle is the slab's, bit for bit, up to
    e = 2 096 127."""
    case = C.case_sym_pack_large()
    outs = held(gpu_ctx, case, twice=False)
    il = np.tril_indices(C.PACK_LARGE[0])
    assert np.array_equal(outs[0], case.ins[0][0].reshape(C.PACK_LARGE[1], -1)[il])


def test_pack_unpack_reproduces_sym_slab_sum(gpu_ctx):
    """The sharded path (pack, all-reduce, unpack + base) and the single-device path
    (sym_slab_sum + base) leave the same bits in the lower tiles."""
    for c4, c5 in C.roundtrip_cases():
        d4 = held(gpu_ctx, c4)[0]
        d5 = held(gpu_ctx, c5)[1]
        assert C.exact(d5, d4) == 0.0, c5


@pytest.mark.parametrize("n,m,d", C.CHAIN_SHAPES, ids=["n%d_m%d_d%d" % s for s in C.CHAIN_SHAPES])
def test_fitc_forward_chain(gpu_ctx, n, m, d):
    """gps_fitc_fit through the resident path at shapes ragged in both dimensions: λ, b, c, g, r
    recomputed in longdouble from the device's own Knm, λ, Lm⁻¹ and Lb⁻¹, and the library's
    λ, μ, σ², Σ log λ and five objectives held to the bounds of the same chain
    (vec_cases.fitc_chain) — the slab counts, offsets and operands between the kernels."""
    import math
    import gpscore
    from gpscore import _lib
    X, y, Z, th = C.chain_data(n, m, d)
    gp = gpscore.GP(ctx=gpu_ctx)
    res = gp.fit(X, y, th, kind="fitc", Z=Z)
    Knm, lam, Lm, Lb = np.full((n, m), np.nan), np.full(n, np.nan), np.full((m, m), np.nan), np.full((m, m), np.nan)
    gpu_ctx.call("gps_fitc_intermediates", *(_lib.ptr(a) for a in (Knm, lam, Lm, Lb)), None)
    assert all(np.isfinite(a).all() for a in (Knm, lam, np.tril(Lm), np.tril(Lb), res.mu_loo, res.var_loo))
    ref, tol = C.fitc_chain(y, math.exp(th[0]), math.exp(th[2]), Knm, lam, Lm, Lb)
    got = dict(res.objectives, lam=lam, mu=res.mu_loo, var=res.var_loo)
    for k, r in C.chain_ratios(got, ref, tol).items():
        print("vec gpu fitc chain n%d m%d %-9s %.3f" % (n, m, k, record("fitc chain %s" % k, r)))
        assert r <= 1.0, (k, r)


def test_zz_report():
    """The worst error / bound per check over this run (DESIGN §30 quotes them; needs -s)."""
    for k in sorted(RATIOS):
        if not k.split(" ", 1)[1].startswith(("finite", "exact")):
            print("vec gpu worst %-44s %.3f" % (k, RATIOS[k]))
