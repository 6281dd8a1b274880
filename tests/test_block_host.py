"""The block-LOO, energy-score and joint kernels' launch-by-launch checks on the CPU (DESIGN §39;
the device side is test_gpu_block.py).  A numpy float64 restatement of each kernel of
csrc/kernels_block.hip and csrc/kernels_joint.hip, and of fitc_grad_v / fitc_grad_y — its
operations and, where the bound is sharp, its order (tests/block_cases.py) — runs on the very
cases the GPU test uses:

  * every bound holds on it with room: the worst ratio error / bound stays <= 0.5, and <= 1 for
    the bounds that count one to three roundings (block_cases.SHARP), which plain rounding may
    approach; the bitwise checks hold;
  * each defect of DEFECTS below, built into a CPU copy only, fails the named check;
  * numpy's pow stays within the figure block_cases.POW_MEASURED_ULP["host"] records, and the
    longdouble exp agrees with mpmath's on joint_cov's sample.

Also, with no device: gps_block_diag is declared and bound at ABI 900, and refuses every bad
argument — the launchers' own refusals among them — before it looks at the context.
`pytest -s` prints the restatement's worst ratios (DESIGN §39 has them beside the device's).
"""
import os

import numpy as np
import pytest

import block_cases as C
from gpscore import _lib

HALF = 0.5
SEEN = {}
N = len(C.NAMES)


def record(name, ratio):
    SEEN[name] = max(SEEN.get(name, 0.0), ratio)
    return ratio


def held(case, res):
    for name, r in res.items():
        record("%s %s" % (C.NAMES[case.which], name), r)
        limit = 0.0 if name.startswith(("exact", "finite")) else 1.0 if name in C.SHARP else HALF
        assert r <= limit, (case, name, r)


# ====================================================================== the fixture
def test_fixture_is_small_and_well_formed():
    g = C.fixture()
    assert os.path.getsize(C.FIXTURE) < 200 * 1024
    for k in g:
        if k.endswith("_hi"):
            hi, lo = g[k], g[k[:-3] + "_lo"]
            assert np.all(np.abs(lo) <= 0.5 * np.spacing(np.abs(hi))), k


def test_fixture_regenerates_bitwise():
    """mpmath at 60 digits reproduces the committed references bit for bit."""
    pytest.importorskip("mpmath")
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_block_terms", os.path.join(C.GOLDEN, "make_block_terms.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    g = C.fixture()
    ref = gen.reference(C.term_inputs())
    assert set(ref) == set(g)
    for k, v in ref.items():
        assert np.array_equal(g[k], v), k


def test_longdouble_exp_agrees_with_mpmath_on_the_sample():
    """joint_cov's reference takes exp from mpmath on the sampled entries and from numpy
    longdouble elsewhere: on the sample the two agree to 2^-62 relative."""
    for b in C.JC_B:
        for d in C.JC_D:
            i, j = C.jc_sample(b, d)
            mp_, np_ = C.hilo(C.fixture(), "exp_b%d_d%d" % (b, d)), np.exp(C.jc_args(b, d))[i, j]
            assert np.all(np.abs(mp_ - np_) <= np.ldexp(C.LD(1), -62) * mp_), (b, d)


def test_host_pow_is_within_its_recorded_figure():
    """numpy's pow over es_reduce's pool against mpmath's: the worst error in ulps is the figure
    block_cases records for the host, and the allowance is twice it, rounded up."""
    D = C.es_pool()
    worst = 0.0
    for beta in (0.5, 1.5):
        ref = C.hilo(C.fixture(), "pow%g" % beta)
        err = np.abs(C.ld(np.power(D, beta)) - ref) / np.spacing(ref.astype(np.float64)).astype(C.LD)
        worst = max(worst, float(err.max()))
    print("host pow worst %.3f ulp" % worst)
    assert worst <= C.POW_MEASURED_ULP["host"]
    assert C.POW_ALLOW_ULP["host"] == int(np.ceil(2 * C.POW_MEASURED_ULP["host"]))


# ====================================================================== the restatements
@pytest.mark.parametrize("which", range(N), ids=C.NAMES)
def test_restatement_meets_every_bound(which):
    n = 0
    for case in C.CASES[which]():
        held(case, C.check(case, C.restate(case)))
        n += 1
    assert n >= 4


def test_shapes_cover_the_seams():
    """Ragged sizes, padded strides and NULL optional operands are in every launcher's list."""
    names = {w: [c.name for c in C.CASES[w]()] for w in range(N)}
    assert len(names[1]) == 25 and {n.rsplit("_", 1)[-1] for n in names[1]} >= {"t", "B", "apart"}
    assert len(names[2]) == 20 and len(names[3]) == 12 and len(names[0]) == 15
    assert len(names[4]) == (2 + 4 + 4) * 4 and any("inplace" in n for n in names[4])
    assert len(names[8]) == 20 and any("alias" in n for n in names[8]) and any("apart" in n for n in names[8])
    assert len(names[15]) == 15 and len(names[16]) == 72 and len(names[17]) == 48
    assert {"n%d_ld%d_below" % (n, n + (2 if k % 2 else 0)) for k, n in enumerate(C.NSR_N)} <= set(names[14])
    for w in range(N):      # a NULL optional operand wherever the launcher has one
        if w in (0, 1, 2, 3, 4, 9, 16, 22, 23):
            assert any(any(a is None for a in c.ins) or any(o is None for o in c.outs0) for c in C.CASES[w]()), w


# ====================================================================== the defects
def pick(which, frag):
    for c in C.CASES[which]():
        if frag in c.name:
            return c
    raise KeyError(frag)


# (defect, which, case name, the check it must fail)
DEFECTS = [
    ("half_missing", 0, "b17_kc", "G"),
    ("g_every_column", 0, "b37_dss", "g"),
    ("stride_short", 1, "1x258_", "at"),
    ("stride_short", 1, "4x130_", "ab"),
    ("pads_unwritten", 2, "mode0_b257_bp384", "exact pads"),
    ("no_two", 2, "mode2_b255_bp256", "o1 kc"),
    ("pads_unwritten", 3, "37_128x20_x2", "exact pads"),
    ("rs_skipped", 3, "37_128x20_x2", "out"),
    ("skip_off_by_one", 4, "ns9_skip4_len257", "finite"),
    ("skip_off_by_one", 4, "ns4_skip3_len256", "finite"),
    ("skip_off_by_one", 4, "ns4_skip-1_len255", "exact dst"),
    ("lam_to_m", 5, "m257_b125", "finite"),
    ("lam_to_m", 5, "m20_b125", "out"),
    ("no_half", 5, "m20_b300", "out"),
    ("scale_by_pair", 6, "17x18", "exact out"),
    ("last_missing", 7, "n257", "finite"),
    ("pads_kept", 8, "n5_pad8_m130", "exact pads"),
    ("p_once", 8, "n130_pad256_m128", "md"),
    ("pad_from_b_plus_1", 9, "b63_bp64_C_pad1", "exact out"),
    ("ld_is_n", 10, "n17", "exact out"),
    ("lower_only", 11, "n130", "exact out"),
    ("pads_unwritten", 12, "b257_bp384", "finite"),
    ("two_roundings", 13, "17x66", "exact out"),
    ("no_delta", 14, "n32_ld32_below", "out"),
    ("no_delta", 14, "n32_ld32_below", "exact verdict"),
    ("ld_is_n", 14, "n31_ld33_small", "finite"),
    ("j_lt_S", 15, "S16_bp64", "finite"),
    ("one_chunk", 15, "S17_bp192", "D"),
    ("last_col_coef", 16, "S15_Sp64_ld64_beta1_grad1", "W"),
    ("last_col_coef", 16, "S33_Sp34_ld34_beta0.5_grad1", "rs"),
    ("pads_kept", 16, "S17_Sp128_ld128_beta1.5_grad1", "exact zeros"),
    ("no_mirror", 17, "b33_d2_ks3", "exact symmetric"),
    ("pad_nan", 17, "b100_d8_ks1", "finite"),
    ("sn2_even_only", 17, "b31_d1_ks1", "out"),
    ("pads_unwritten", 18, "b1_bp128", "finite"),
    ("first_trip_only", 19, "b1025", "out"),
    ("no_half", 19, "b1023", "out"),
    ("le", 20, "npos128_n257", "exact out"),
    ("mu_by_row", 21, "18x17", "exact out"),
    ("reciprocal", 22, "n257_lam", "exact out"),
    ("s1_for_both", 23, "17x66_alias", "Y"),
]


@pytest.mark.parametrize("defect,which,frag,fails", DEFECTS, ids=["%s_%s_%s" % (C.NAMES[d[1]], d[0], d[3].replace(" ", "_")) for d in DEFECTS])
def test_defect_fails_its_check(defect, which, frag, fails):
    case = pick(which, frag)
    clean = C.check(case, C.restate(case))
    assert clean[fails] <= 1.0
    bad = C.check(case, C.restate(case, defect))
    print("defect %-18s %-16s %s: %.3g" % (defect, C.NAMES[which], fails, bad[fails]))
    assert bad[fails] > 1.0, (defect, bad)


def test_every_launcher_has_a_defect():
    assert {d[1] for d in DEFECTS} == set(range(N))


# ====================================================================== the entry point
def last():
    return _lib.load().gps_last_error(None).decode()


def valid(which):
    c = next(iter(C.CASES[which]()))
    return dict(which=which, dims=list(c.dims) + [0] * (8 - len(c.dims)), scal=c.scal, ins=c.ins + [None] * (12 - len(c.ins)),
                outs=c.fresh_outs())


def V(w, dims=None, **kw):
    a = valid(w)
    for k, v in (dims or {}).items():
        a["dims"][k] = v
    a.update(kw)
    return a


def drop(lst, k):
    return [None if i == k else v for i, v in enumerate(lst)]


def test_block_diag_is_bound_at_abi_900():
    assert "gps_block_diag" in _lib.SIGNATURES and _lib.load().gps_version() == 900
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "gpscore.h")).read()
    assert "#define GPS_ABI_VERSION 900" in text and "int gps_block_diag(" in text


@pytest.mark.parametrize("which", range(N), ids=C.NAMES)
def test_null_context_is_refused(which):
    """Well-formed arguments and no context: the call gets as far as bind() and stops there."""
    assert _lib.block_diag_raw(None, **valid(which)) == -1 and last() == "NULL context", last()


REFUSALS = [
    ("which", V(0, which=24), "which must be 0..23"),
    ("which negative", V(0, which=-1), "which must be 0..23"),
    ("no inputs", V(0, ins=None), "NULL argument"),
    ("no outputs", V(0, outs=None), "NULL argument"),
    ("scalar", V(0, scal=(np.nan,)), "the scalars must be finite"),
    ("fold_grad PI", V(0, ins=drop(valid(0)["ins"], 0)), "NULL input array"),
    ("fold_grad G", V(0, outs=drop(valid(0)["outs"], 0)), "NULL output array"),
    ("fold_grad ldg", V(0, {3: 0}), "fold_grad: ldg must be in b"),
    ("fold_grad H", V(0, ins=drop(valid(0)["ins"], 1)), "fold_grad: c3 needs H"),
    ("fold_grad w", V(0, ins=drop(valid(0)["ins"], 3)), "fold_grad: c2 and gw need w"),
    ("row_dots odd cols", V(1, {1: 3, 2: 4}), "row_dots: cols must be even"),
    ("row_dots odd lda", V(1, {2: 3}), "row_dots: lda must be even"),
    ("row_dots short lda", V(1, {1: 4, 2: 2}), "row_dots: lda must be in cols"),
    ("row_dots odd ldb", V(1, {3: 5}, ins=[np.zeros((1, 2)), np.zeros((1, 2)), None], outs=[None, np.zeros(17)]), "row_dots: ldb must be even"),
    ("row_dots nothing", V(1, ins=[np.zeros((1, 2)), None, None], outs=[None, None]), "row_dots: neither t nor B"),
    ("row_dots at", V(1, outs=[None, None]), "row_dots: at goes with t"),
    ("lr_fold_vec mode", V(2, {0: 4}), "lr_fold_vec: mode must be 0..3"),
    ("lr_fold_vec bp", V(2, {1: 2, 2: 1}), "lr_fold_vec: 1 <= b <= bp"),
    ("lr_fold_vec o2", V(2, outs=drop(valid(2)["outs"], 1)), "NULL output array"),
    ("lr_fold_vec at", V(2, ins=drop(valid(2)["ins"], 2)), "NULL input array"),
    ("lr_combine pad", V(3, {0: 2, 1: 1}), "lr_combine: 1 <= rows <= rows_pad"),
    ("lr_combine ldo", V(3, {5: 1}), "lr_combine: ldo must be in cols"),
    ("lr_combine v1", V(3, ins=drop(valid(3)["ins"], 5)), "lr_combine: u1 goes with v1"),
    ("fold_sum nslab", V(4, {0: 0}), "fold_sum: nslab must be in"),
    ("fold_sum skip", V(4, {1: 1}), "fold_sum: skip must be in -1..nslab-1"),
    ("fold_sum stride", V(4, {3: 0}), "fold_sum: stride must be in len"),
    ("fold_sum inplace", V(4, {4: 1}, ins=[np.zeros((1, 1)), np.zeros(1), None]), "fold_sum: in place the base comes through out[0]"),
    ("fold_logdet m", V(5, {0: 0}), "fold_logdet: m must be in"),
    ("row_scale odd cols", V(6, {1: 1}), "row_scale: cols must be even"),
    ("row_scale odd ld", V(6, {2: 5}), "row_scale: ld must be even"),
    ("row_scale short ld", V(6, {2: 0}), "row_scale: ld must be in cols"),
    ("vec_mul n", V(7, {0: 0}), "vec_mul: n must be in"),
    ("blk_mdiag odd m_pad", V(8, {2: 3}), "blk_mdiag: m_pad must be even"),
    ("blk_mdiag odd ldf", V(8, {3: 5}), "blk_mdiag: ldf must be even"),
    ("blk_mdiag odd ldus", V(8, {4: 7}), "blk_mdiag: ldus must be even"),
    ("blk_mdiag odd ldu", V(8, {5: 9}), "blk_mdiag: ldu must be even"),
    ("blk_mdiag odd ldy", V(8, {6: 7}), "blk_mdiag: ldy must be even"),
    ("blk_mdiag alias ld", V(8, {6: 10, 7: 1}), "blk_mdiag: Y over US needs ldy == ldus"),
    ("ns_init bp", V(9, {0: 2, 1: 1}), "ns_init: 1 <= b <= bp"),
    ("diag_add_const ld", V(10, {1: 0}), "diag_add_const: ld must be in n"),
    ("sym_avg n", V(11, {0: 0}), "sym_avg: n must be in"),
    ("scaled_row bp", V(12, {0: 2, 1: 1}), "scaled_row: 1 <= b <= bp"),
    ("row_axpy ldz", V(13, {3: 1}), "row_axpy: ldz must be in cols"),
    ("ns_resid ld", V(14, {1: 0}), "ns_resid: ld must be in n"),
    ("es_dist bp", V(15, {1: 96}), "es_dist: bp must be a multiple of 64"),
    ("es_dist ldd", V(15, {2: 2}), "es_dist: ldd must be in S + 1"),
    ("es_reduce S", V(16, {0: 1}), "es_reduce: S must be at least 2"),
    ("es_reduce Sp", V(16, {1: 2}), "es_reduce: Sp must be at least S + 1"),
    ("es_reduce beta", V(16, scal=(0.0,)), "es_reduce: beta must be positive"),
    ("es_reduce rs", V(16, {3: 1}), "NULL output array"),
    ("joint_cov bp", V(17, {1: 192}), "joint_cov: bp must be a multiple of 128"),
    ("joint_cov b", V(17, {0: 129}), "joint_cov: b must be in 1..bp"),
    ("joint_cov d zero", V(17, {2: 0}), "joint_cov: d must be in 1..GPS_MAX_D"),
    ("joint_cov d large", V(17, {2: 4096}), "joint_cov: d must be in 1..GPS_MAX_D"),
    ("joint_cov ks", V(17, {3: 0}), "joint_cov: ks must be at least 1"),
    ("joint_cov stride", V(17, {4: 100}), "joint_cov: stride must be in bp*bp"),
    ("joint_resid bp", V(18, {0: 2, 1: 1}), "joint_resid: 1 <= b <= bp"),
    ("joint_dss b", V(19, {0: 0}), "joint_dss: b must be in"),
    ("sign_fill npos", V(20, {0: 2, 1: 1}), "sign_fill: npos must be in 0..n"),
    ("row_add ld", V(21, {2: 0}), "row_add: ld must be in cols"),
    ("fitc_grad_v n", V(22, {0: 0}), "fitc_grad_v: n must be in"),
    ("fitc_grad_y odd cols", V(23, {1: 1}), "fitc_grad_y: cols must be even"),
    ("fitc_grad_y odd ld", V(23, {2: 5}), "fitc_grad_y: ld must be even"),
    ("fitc_grad_y s2", V(23, ins=[np.zeros((1, 2)), None, np.zeros(1), np.zeros(1)]), "fitc_grad_y: s2 goes with UP"),
]


@pytest.mark.parametrize("why,kw,frag", REFUSALS, ids=[r[0].replace(" ", "_") for r in REFUSALS])
def test_block_diag_refusals(why, kw, frag):
    """Each refusal by its message, before the context is looked at; the same call made valid
    again then gets as far as bind()."""
    assert _lib.block_diag_raw(None, **kw) == -1
    assert last().startswith("gps_block_diag: ") and frag in last(), (why, last())
    assert _lib.block_diag_raw(None, **valid(kw["which"] if 0 <= kw["which"] < N else 0)) == -1
    assert last() == "NULL context", last()


def test_zz_report():
    """The worst error / bound per check over this run (DESIGN §39 quotes them; needs -s)."""
    for k in sorted(SEEN):
        if not k.split(" ", 1)[1].startswith(("finite", "exact")):
            print("block host worst %-34s %.3f" % (k, SEEN[k]))
