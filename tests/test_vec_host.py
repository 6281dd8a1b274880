"""The vector layer's launch-by-launch checks on the CPU (the device side is
test_gpu_vec.py).  A numpy float64 restatement of each kernel of csrc/kernels_vec.hip — its
operations and, where the bound is sharp, its order (tests/vec_cases.py) — runs on the very cases
the GPU test uses:

  * every bound holds on it with room: the worst ratio error / bound stays <= 0.5, and <= 1 for
    the sharp bounds of one to three roundings (vec_cases.SHARP) and the sums of at most four
    terms (vec_cases.few_terms), which plain rounding may approach; the bitwise checks hold;
  * each defect of DEFECTS below, built into a CPU copy only, fails the named check;
  * what the older normwise 1e-9 comparison (conftest.nrel) gives for two of them is worked out;
  * the FITC forward chain's bounds hold within half on the oracle's own float64 values.

Worst ratios of the restatement (x86-64 glibc; `pytest -s` prints them; "few": <= 4 terms):
  gemv y 0.02 (few 0.19) | colred s1 0.06 s2 0.05 (few 0.33, 0.51), partials 0.20
  slab_sum 0.32 | sym_slab_sum 0.47 (few 0.53) | sym_pack packed 0.48 | dot 0.00 (few 0.09)
  local_sum 0.09 (few 0.41)
  full_loo mu 0.82 var 1.00 (sharp: two roundings, one), sum crps 0.03 logs 0.02 logdiag 0.01
           beta2 0.02, obj nlml 0.03 loo_crps 0.02 loo_logs 0.02; n_pad = 262 272: sums <= 0.02
  fitc_lambda lam 0.51 inv_lam 0.62 ys 0.56 (sharp), sum loglam 0.02 y2/lam 0.03
  fitc_loo mu 0.56 var 0.31 (sharp), sum crps 0.10 logs 0.05
  pred var 0.98 (sharp: one and two roundings) | surface sum crps 0.04 logs 0.02
  fitc chain on the oracle: lam 0.10 var 0.23, the rest <= 0.02

Also, with no device: gps_vec_diag is declared and bound at ABI 900, and refuses every bad
argument — the launchers' own refusals among them — before it looks at the context.
"""
import os

import numpy as np
import pytest

import vec_cases as C
from conftest import nrel
from gpscore import _lib

HALF = 0.5
SEEN = {}


def record(name, ratio):
    SEEN[name] = max(SEEN.get(name, 0.0), ratio)
    return ratio


def held(case, res):
    """Every check of one restated case: exact and finite checks 0, sharp bounds (SHARP, and the
    sums of at most three terms) <= 1, the rest <= 1/2."""
    sharp = C.few_terms(case)
    for name, r in res.items():
        record("%s %s%s" % (C.NAMES[case.which], name, " (few terms)" if sharp else ""), r)
        limit = 0.0 if name.startswith(("exact", "finite")) else 1.0 if (sharp or name in C.SHARP) else HALF
        assert r <= limit, (case, name, r)


# ====================================================================== the fixture
def test_fixture_inputs_and_size():
    """The committed inputs are build_pool()'s bit for bit, the hi/lo pairs do not overlap, the
    corners are there, and the file stays small."""
    g = C.load_pool()
    for k, v in C.build_pool().items():
        assert np.array_equal(g[k], v), k
    assert os.path.getsize(C.FIXTURE) < 512 * 1024
    for fam in ("full", "fitc", "surf0", "surf1"):
        for key in ("erf", "exp"):
            hi, lo = g["%s_%s_hi" % (fam, key)], g["%s_%s_lo" % (fam, key)]
            assert np.all(np.abs(lo) <= 0.5 * np.spacing(np.abs(hi))) and np.all(np.abs(hi) <= 1.0)
    q = C.inorder(g["lam_qs"])
    assert np.all(np.abs(q[:16] - C.LAM_SF2) <= 16 * np.spacing(C.LAM_SF2))      # q within ulps of sf2
    rl = g["r"] / g["fitc_lam"]
    assert (np.abs(rl - 1.0) < 2e-6).sum() >= 100 and (rl == 0).sum() >= 100   # r/λ close to 1, and 0
    big = np.abs(g["y"]) == 1e6
    assert (np.abs(g["alpha"] / g["dinv"])[big] < 1e-3).any()                    # |y| large against α/d
    assert np.all(np.array(C.SURF_S2)[:, None] * g["dinv"][None, :] < 2.0)


def test_fixture_regenerates_bitwise():
    """mpmath at 60 digits reproduces the committed references bit for bit."""
    pytest.importorskip("mpmath")
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_vec_terms", os.path.join(C.GOLDEN, "make_vec_terms.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    g = C.load_pool()
    for k, v in gen.reference({k: g[k] for k in C.POOL_INPUTS}).items():
        assert np.array_equal(g[k], v), k


# ====================================================================== the restatements
@pytest.mark.parametrize("which", range(14), ids=C.NAMES)
def test_restatement_meets_every_bound(which):
    n = 0
    for case in C.CASES[which]():
        held(case, C.check(case, C.restate(case)))
        n += 1
    assert n >= 4


def test_restatement_second_trip():
    for case in C.large_cases():
        held(case, C.check(case, C.restate(case)))


def test_restatement_pack_large():
    case = C.case_sym_pack_large()
    out = C.restate(case)
    held(case, C.check(case, out))
    il = np.tril_indices(C.PACK_LARGE[0])
    assert np.array_equal(out[0], case.ins[0][0].reshape(C.PACK_LARGE[1], -1)[il])


def test_pack_unpack_reproduces_sym_slab_sum():
    for c4, c5 in C.roundtrip_cases():
        d4, d5 = C.restate(c4)[0], C.restate(c5)[1]
        held(c4, C.check(c4, [d4]))
        assert C.exact(d5, d4) == 0.0, c5


def test_shapes_cover_the_seams():
    """The case lists hold the sizes at which each kernel changes path."""
    names = {w: [c.name for c in C.CASES[w]()] for w in range(14)}
    assert {"lower128_mode1", "lower256_mode1", "lower256_mode2", "lower384_mode1"} <= set(names[0])
    assert sum(n.startswith("full") for n in names[0]) == 25
    assert sum(n.startswith("full") for n in names[1]) >= 25
    for frag in ("lower640x640_ld640_cr256_s2", "lower256x256_ld256_cr32_w_s1_s2", "lower128x128", "lower384x384"):
        assert any(frag in n for n in names[1]), frag
    assert len(names[3]) == 20 and len(names[4]) == 12
    for m, M in C.PACK_MM:
        assert any(n.startswith("m%d_M%d_r0_%d_" % (m, M, m)) for n in names[5])
    for w in (6, 7, 8):
        for n in C.FIN_N:
            assert any(s.startswith("n%d_" % n) and "ns1" in s for s in names[w])
            assert any(s.startswith("n%d_" % n) and "ns9" in s for s in names[w])
    assert C.pad_to(C.FIN_LARGE_N) > 1024 * 256


# ====================================================================== the defects
def pick(which, frag):
    for c in C.CASES[which]():
        if frag in c.name:
            return c
    raise KeyError(frag)


# (defect, which, case, the check it must fail)
DEFECTS = [
    ("kend_short", 0, lambda: pick(0, "lower256_mode1"), "y"),
    ("kend_long", 0, lambda: pick(0, "lower256_mode1"), "finite"),
    ("no_clip", 1, lambda: pick(1, "lower640x640_ld640_cr256_w_s1_s2"), "finite"),
    ("drop_last_chunk", 1, lambda: pick(1, "full257x514_ld514_cr256_w_s1_s2"), "s1"),
    ("skip_last", 3, lambda: pick(3, "ns9_len257"), "out"),
    ("no_init", 3, lambda: pick(3, "ns8_len255_init"), "out"),
    ("pack_row_off", 5, lambda: pick(5, "m37_M128_r0_37"), "finite"),
    ("unpack_swap", 5, lambda: pick(5, "m37_M128_r0_37"), "exact dst"),
    ("pad_inv_lam", 7, lambda: pick(7, "n300_pad384_ns9"), "exact pads"),
    ("first_trip_only", 6, lambda: C.large_cases()[0], "sum crps"),
    ("first_trip_only", 7, lambda: C.large_cases()[1], "sum loglam"),
    ("nlml_const", 6, lambda: pick(6, "n300_ns9"), "obj nlml"),
    ("nlml_half", 6, lambda: pick(6, "n300_ns9"), "obj nlml"),
    ("qb_sign", 9, lambda: pick(9, "fitc_nt257"), "var"),
    ("identity_inside", 12, lambda: pick(12, "37x37_lds300_to_128x128_ldd128_id1"), "exact dst"),
]


@pytest.mark.parametrize("defect,which,get,fails", DEFECTS, ids=["%s_%d" % d[:2] for d in DEFECTS])
def test_defect_fails_its_check(defect, which, get, fails):
    case = get()
    clean = C.check(case, C.restate(case))
    assert clean[fails] <= 1.0
    bad = C.check(case, C.restate(case, defect))
    print("defect %-18s %-16s %s: %.3g" % (defect, C.NAMES[which], fails, bad[fails]))
    assert bad[fails] > 1.0, (defect, bad)


def test_normwise_comparison_passes_two_of_them():
    """What conftest.nrel at 1e-9 makes of two defects: log 2π to ten digits moves nlml by
    2e-11 of its size, and a pad row of 1/λ that carries weight changes no real row at all."""
    case = pick(6, "n300_ns9")
    good, bad = C.restate(case), C.restate(case, "nlml_const")
    assert nrel(bad[4][:1], good[4][:1]) < 1e-9 and C.check(case, bad)["obj nlml"] > 1.0
    case = pick(7, "n300_pad384_ns9")
    good, bad = C.restate(case), C.restate(case, "pad_inv_lam")
    n = case.dims[0]
    assert nrel(bad[2][:n], good[2][:n]) == 0.0 and C.check(case, bad)["exact pads"] > 1.0


# ====================================================================== the FITC forward chain
def oracle_chain(n, m, d):
    """The oracle's float64 FITC forward (numpy / LAPACK) with its stage arrays."""
    import math
    import gp_oracle as O
    X, y, Z, th = C.chain_data(n, m, d)
    Kmm, Lm_inv, logdet_m = O.fitc_shared(Z, th[0], th[1])
    part = O.fitc_partials(X, y, Z, Lm_inv, *th)
    Lb_inv, logdet_b, c = O.fitc_finish_shared(Kmm, part["B"], part["b"])
    mu, var = O.fitc_loo_terms(part, y, Lb_inv, c)
    logdet = part["s"][0] + logdet_b - logdet_m
    quad = part["s"][1] - float(part["b"] @ c)
    got = dict(lam=part["_lam"], mu=mu, var=var, nlml=0.5 * n * O.LOG2PI + 0.5 * logdet + 0.5 * quad,
               loo_crps=O.crps(mu, var, y), loo_logs=O.logs(mu, var, y), logdet=logdet, quad=quad)
    stages = (y, math.exp(th[0]), math.exp(th[2]), part["_Knm"], part["_lam"], Lm_inv, Lb_inv)
    return got, stages, c


@pytest.mark.parametrize("n,m,d", C.CHAIN_SHAPES, ids=["n%d_m%d_d%d" % s for s in C.CHAIN_SHAPES])
def test_fitc_chain_bounds_hold_for_the_oracle(n, m, d):
    """The chain's bounds (vec_cases.fitc_chain) on the oracle's own float64 values: within half."""
    got, stages, _ = oracle_chain(n, m, d)
    ref, tol = C.fitc_chain(*stages)
    for k, r in C.chain_ratios(got, ref, tol).items():
        record("fitc chain %s" % k, r)
        assert r <= HALF, (k, r)


def test_fitc_chain_sees_a_wrong_slab_count():
    """One of the r pass's column tiles left out of the sum (m = 129: two tiles) — a defect of
    the wiring between the kernels — misses the bounds on μ and σ²."""
    got, stages, c = oracle_chain(*C.CHAIN_SHAPES[1])
    y, sf2, sn2, Knm, lam, Lm_inv, Lb_inv = stages
    U = Knm @ np.tril(Lb_inv).T
    r = np.sum(U[:, :128] ** 2, axis=1)                # the second tile's partial dropped
    dinv = 1.0 / lam - r / lam ** 2
    alpha = (y - Knm @ c) / lam
    bad = dict(got, mu=y - alpha / dinv, var=1.0 / dinv)
    ref, tol = C.fitc_chain(*stages)
    ratios = C.chain_ratios(bad, ref, tol)
    assert ratios["var"] > 1.0 and ratios["mu"] > 1.0, ratios


# ====================================================================== the entry point
def last():
    return _lib.load().gps_last_error(None).decode()


def valid(which):
    c = next(iter(C.CASES[which]()))
    return dict(which=which, dims=list(c.dims) + [0] * (8 - len(c.dims)), scal=c.scal, ins=c.ins,
                outs=c.fresh_outs())


def V(w, dims=None, **kw):
    a = valid(w)
    for k, v in (dims or {}).items():
        a["dims"][k] = v
    a.update(kw)
    return a


def test_vec_diag_is_bound_at_abi_900():
    assert "gps_vec_diag" in _lib.SIGNATURES and _lib.load().gps_version() == 900


@pytest.mark.parametrize("which", range(14), ids=C.NAMES)
def test_null_context_is_refused(which):
    """Well-formed arguments and no context: the call gets as far as bind() and stops there."""
    assert _lib.vec_diag_raw(None, **valid(which)) == -1 and last() == "NULL context", last()


def drop(lst, k):
    return [None if i == k else v for i, v in enumerate(lst)]


REFUSALS = [
    ("which", V(0, which=14), "which must be 0..13"),
    ("which negative", V(0, which=-1), "which must be 0..13"),
    ("no inputs", V(0, ins=None), "NULL argument"),
    ("no outputs", V(0, outs=None), "NULL argument"),
    ("gemv M", V(0, ins=drop(valid(0)["ins"], 0)), "NULL input array"),
    ("gemv y", V(0, outs=[None]), "NULL output array"),
    ("gemv mode", V(0, {0: 3}), "gemv: mode must be"),
    ("gemv odd cols", V(0, {0: 0, 1: 4, 2: 127, 3: 128}), "gemv: cols must be even"),
    ("gemv odd ldm", V(0, {0: 0, 1: 4, 2: 126, 3: 127}), "gemv: ldm must be even"),
    ("gemv short ldm", V(0, {0: 0, 1: 4, 2: 126, 3: 124}), "gemv: ldm must be even, in cols"),
    ("gemv lower ragged", V(0, {0: 1, 1: 130, 2: 130, 3: 130}), "gemv: the lower form is square"),
    ("trmv trans", V(0, {0: 2, 4: 1}), "launch_trmv_lower has no transposed form"),
    ("colred odd cols", V(1, {1: 3, 2: 4}), "colred: cols must be even"),
    ("colred odd ldm", V(1, {2: 3}), "colred: ldm must be even"),
    ("colred short ldm", V(1, {1: 4, 2: 2}), "colred: ldm must be in cols"),
    ("colred crows", V(1, {4: 0}), "colred: crows must be at least 1"),
    ("colred lower ragged", V(1, {3: 1}), "colred: the lower form is square"),
    ("colred nothing", V(1, outs=[None, None]), "colred: neither s1 nor s2"),
    ("colred s1 without w", V(1, ins=drop(valid(1)["ins"], 1), outs=[np.zeros(2), None]), "colred: s1 needs w"),
    ("partials odd cols", V(2, {1: 639, 2: 640}), "colred_partials: cols must be even"),
    ("partials odd ldm", V(2, {2: 641}), "colred_partials: ldm must be even"),
    ("partials w", V(2, ins=drop(valid(2)["ins"], 1)), "NULL input array"),
    ("slab nslab", V(3, {0: 0}), "slab_sum: nslab must be in"),
    ("slab ld", V(3, {1: 5, 2: 4}), "slab_sum: ld must be in len"),
    ("sym M", V(4, {1: 130}), "sym_slab_sum: M must be a multiple of 128"),
    ("sym stride", V(4, {2: 100}), "sym_slab_sum: stride must be at least M*M"),
    ("pack m", V(5, {3: 129}), "sym_pack: m must be in 1..M"),
    ("pack rows", V(5, {4: 1, 5: 0}), "sym_pack: the rows must satisfy"),
    ("pack r1", V(5, {5: 2}), "sym_pack: the rows must satisfy"),
    ("pack flags", V(5, {7: 2}), "sym_pack: unpack and full are flags"),
    ("pack dst", V(5, {6: 1}, outs=[np.zeros(1), None]), "NULL output array"),
    ("full_loo n", V(6, {0: 0}), "full_loo: n must be in"),
    ("full_loo ld", V(6, {2: 127}), "full_loo: ld must be in n_pad"),
    ("lambda n_pad", V(7, {0: 2, 1: 1}), "fitc_lambda: n_pad must be in n"),
    ("lambda sf2", V(7, scal=(np.inf, 1.0)), "fitc_lambda: sf2 and sn2 must be finite"),
    ("loo nslab", V(8, {2: 0}), "fitc_loo: nslab must be in"),
    ("loo ld", V(8, {3: 1}), "fitc_loo: ld must be in n_pad"),
    ("pred nt", V(9, {0: 0}), "pred_finalize: nt must be in"),
    ("pred mu", V(9, outs=[None, np.zeros(1)]), "NULL output array"),
    ("surface flag", V(10, {1: 2}), "surface_point: add_noise is a flag"),
    ("dot n", V(11, {0: 0}), "dot: n must be in"),
    ("pad rows", V(12, {0: 129}), "pad_copy: 1 <= rows <= rows_pad"),
    ("pad lds", V(12, {2: 2}), "pad_copy: lds must be in cols"),
    ("pad ldd", V(12, {5: 127}), "pad_copy: ldd must be in cols_pad"),
    ("local_sum none", V(13, {0: 0}), "local_sum: n must be in 1..64"),
    ("local_sum 65", V(13, {0: 65}), "local_sum: n must be in 1..64"),
    ("local_sum count", V(13, {1: 0}), "local_sum: count must be in"),
]


@pytest.mark.parametrize("why,kw,frag", REFUSALS, ids=[r[0].replace(" ", "_") for r in REFUSALS])
def test_vec_diag_refusals(why, kw, frag):
    """Each refusal by its message, before the context is looked at; the same call made valid
    again then gets as far as bind()."""
    assert _lib.vec_diag_raw(None, **kw) == -1
    assert last().startswith("gps_vec_diag: ") and frag in last(), (why, last())
    assert _lib.vec_diag_raw(None, **valid(kw["which"] if 0 <= kw["which"] <= 13 else 0)) == -1
    assert last() == "NULL context", last()


def test_zz_report():
    """The worst error / bound per check over this run (DESIGN §30 quotes them; needs -s)."""
    for k in sorted(SEEN):
        print("vec host worst %-34s %.3f" % (k, SEEN[k]))
