"""The block-LOO, energy-score and joint kernels on the device, one launch at a time:
every kernel of csrc/kernels_block.hip but fold_terms (which gps_grad_terms_diag launches) —
fold_grad, row_dots, lr_fold_vec, lr_combine, fold_sum, fold_logdet, row_scale, vec_mul, blk_mdiag,
ns_init, diag_add_const, sym_avg, scaled_row, row_axpy, ns_resid, es_dist, es_reduce — every kernel
of csrc/kernels_joint.hip — joint_cov, joint_resid, joint_dss, sign_fill, row_add — and fitc_grad_v
and fitc_grad_y of csrc/kernels_fitc_grad.hip, through its production launcher and gps_block_diag,
on the cases of tests/block_cases.py, held output by output to the extended-precision references
and the derived bounds there.  Everything a kernel must not read is NaN on the device, so every
check starts with "all finite" where finite is owed; then the bitwise parts (what the kernel
must leave alone still NaN among them), then error / bound <= 1.  Each launch runs twice and must
give the same bits (both files claim fixed-order sums).  tests/test_block_host.py shows on the CPU
that a float64 restatement of each kernel meets the same bounds at half or less (at 1 for the
few-rounding ones), and that each built-in defect misses them.

es_reduce's β != 1 path calls the device pow: its worst error over the fixture's D values, measured
on an MI355X against mpmath with tools/pow_probe.hip, is 1.056 ulp at β = 0.5 and 1.118 ulp at
β = 1.5 (block_cases.POW_MEASURED_ULP["device"] = 1.12), and the allowance c in es_reduce's bounds
is twice that, rounded up to a whole ulp: 3 ulp, c = 6u (POW_ALLOW_ULP["device"]).

Worst measured error / bound on an MI355X (`pytest -s` prints this run's; DESIGN §39 has the
table beside the CPU restatement's figures):
  row_dots at 0.14  ab 0.23 | fold_grad G 0.32  g 0.00 | lr_fold_vec o1 kc 0.36  dss 0.32
  lr_combine 0.44 | fold_logdet 0.05 | blk_mdiag md 0.27  Y 0.94 (two roundings)
  fitc_grad_y Y 0.94 (two roundings) | ns_resid 0.06 | es_dist D 0.12
  es_reduce out 0.06  W 0.59  rs 0.17  cs 0.14; pow recovered from W: 3.2 ulp (1.12 + at most 5)
  joint_cov 0.32 | joint_dss 0.03 | every exact check: bitwise
No kernel missed a bound.
"""
import pytest

import block_cases as C

pytestmark = pytest.mark.gpu

RATIOS = {}
N = len(C.NAMES)


@pytest.fixture(autouse=True)
def device_pow():
    C.POW_WHERE = "device"
    yield
    C.POW_WHERE = "host"


def record(name, ratio):
    RATIOS[name] = max(RATIOS.get(name, 0.0), float(ratio))
    return ratio


def same_bits(a, b):
    return all((x is None and y is None) or C.exact(x, y) == 0.0 for x, y in zip(a, b))


def held(ctx, case):
    """One case: all finite, the bitwise parts, every ratio <= 1; a second launch on the same
    input gives the same bits."""
    outs = C.run(ctx, case)
    res = C.check(case, outs)
    order = sorted(res, key=lambda k: (not k.startswith("finite"), not k.startswith("exact"), k))
    for name in order:
        r = record("%s %s" % (C.NAMES[case.which], name), res[name])
        assert r <= (0.0 if name.startswith(("finite", "exact")) else 1.0), (case, name, r)
    assert same_bits(outs, C.run(ctx, case)), (case, "two launches differ")
    return outs


@pytest.mark.parametrize("which", range(N), ids=C.NAMES)
def test_block_kernel(gpu_ctx, which):
    """Every case of one launcher (block_cases.CASES[which]; the bounds are in the docstrings of
    the cases_* functions there)."""
    for case in C.CASES[which]():
        held(gpu_ctx, case)
    for k in sorted(RATIOS):
        if k.startswith(C.NAMES[which] + " "):
            print("block gpu %-36s %.3f" % (k, RATIOS[k]))


def test_pow_through_w(gpu_ctx):
    """The power behind every W entry of the β != 1 gradient cases, recovered from W: within the
    measured figure plus the 5 ulp the five other roundings of W can add (u each, an ulp being
    between u and 2u)."""
    worst = 0.0
    for case in C.CASES[16]():
        if case.dims[3] and case.scal[0] != 1.0:
            worst = max(worst, C.pow_error_ulps(C.view(C.run(gpu_ctx, case)[0], case.dims[1], case.dims[2]), case))
    print("block gpu pow through W: %.3f ulp (pow alone measured %.2f)" % (worst, C.POW_MEASURED_ULP["device"]))
    assert worst <= C.POW_MEASURED_ULP["device"] + 5.0


def test_zz_report():
    """The worst error / bound per check over this run (DESIGN §39 quotes them; needs -s)."""
    for k in sorted(RATIOS):
        if not k.split(" ", 1)[1].startswith(("finite", "exact")):
            print("block gpu worst %-36s %.3f" % (k, RATIOS[k]))
