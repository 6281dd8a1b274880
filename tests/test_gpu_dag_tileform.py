"""The persistent factorisation's tile-form tasks on the device (GPS_OPT_DAG_TILE_FORM, DESIGN
§29), through gps_potrf_diag as tests/test_gpu_dag_kbatch.py drives it: a K batch of an
off-diagonal tile as ONE task on one workgroup, each wave a 64×64 block, instead of four strips.

* T = 5, B = 2, d = 0, minlen = 2 — the smallest block with a tile-form UPD and a tile-form UPDX
  batch that does not hold the clipped first term (asserted from the task list; the clipped
  batches are in tile form there too) — and T = 11, B = 8, d = 1, a full run of eight in tile form
  next to a single-term remainder in strips: the componentwise bounds and the structure checks of
  tests/factor_cases.py hold; the factors are bitwise those of the form off, of queue orders
  0 / 1 / 2 and of 4 / 64 / 256 workgroups; a graph replay gives the bits of the first run;
* a non-positive-definite block at T = 5 reports its minor, and the next clean run is bitwise the
  one before;
* a full fit at n = 5000 (one 40-tile block) under the library's defaults, with the form on
  (d = 1, minlen = 2) and with it off: objectives and LOO vectors bitwise equal.
tests/test_dag_tileform_logic.py checks the task lists themselves on the CPU."""
import numpy as np
import pytest

import factor_cases as FC
from dag_model import decode, task_list, tf_of

pytestmark = pytest.mark.gpu


@pytest.fixture
def opt(gpu_ctx):
    """Sets factorisation options for one test and puts the library's defaults back."""
    from gpscore import _lib as G
    keys = {"tiles": (G.GPS_OPT_DAG_TILES, 20), "graph": (G.GPS_OPT_GRAPH, 1),
            "wgs": (G.GPS_OPT_DAG_WGS, 0), "order": (G.GPS_OPT_DAG_ORDER, 1),
            "kbatch": (G.GPS_OPT_DAG_KBATCH, G.DAG_KBATCH_DEFAULT),
            "form": (G.GPS_OPT_DAG_TILE_FORM, G.DAG_TILE_FORM_DEFAULT),
            "tiles_full": (G.GPS_OPT_DAG_TILES_FULL, G.DAG_TILES_FULL_DEFAULT)}

    def set_(**kw):
        for k, (key, default) in keys.items():
            gpu_ctx.call("gps_ctx_set_option", key, int(kw.get(k, default)))

    set_()
    yield set_
    set_()


def same(a, b):
    return all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(a[:3], b[:3]))


def tile_words(T, kb, tf):
    return [t for t in decode(task_list(T, kb=kb, tf=tf)) if t[7]]


CASES = [(5, 2, tf_of(0, 2), "a"), (5, 2, tf_of(0, 2), "b6"), (11, 8, tf_of(1, 2), "a"),
         (11, 8, tf_of(1, 2), "b6")]


def test_case_lists():
    tw = tile_words(5, 2, tf_of(0, 2))
    assert any(t[0] == 2 for t in tw) and any(t[0] == 3 and t[3] > t[4] for t in tw)
    assert any(t[0] == 3 and t[3] == t[4] for t in tw)   # a batch holding the clipped first term
    tl = decode(task_list(11, kb=8, tf=tf_of(1, 2)))
    assert (2, 0, 10, 9, 0, 0, 8, 1) in tl and (2, 0, 10, 9, 8, 0, 1, 0) in tl


@pytest.mark.parametrize("nt,kb,tf,fam", CASES)
def test_tile_form_block(gpu_ctx, opt, nt, kb, tf, fam):
    n = FC.TILE * nt - 37
    A = FC.family(fam, n)
    opt(tiles=nt, kbatch=kb, form=tf)
    base = gpu_ctx.potrf_diag(A)
    plan = base[4]
    assert (plan["leaves"], plan["dags"], plan["dag_tmax"], plan["gemms"]) == (0, 1, nt, 0), plan
    assert base[3] == 0
    bad, r = FC.check_factor(FC.pad_identity(A), base[0], base[1], FC.rows_for(n, True, nt), True, nt)
    print(f"tile form gpu T={nt} B={kb} form={tf} {fam}: " + " ".join(f"{k}={v:.3g}" for k, v in r.items()))
    assert bad == [], r
    assert FC.check_structure(base[0], base[1], base[2], n) == []
    replay = gpu_ctx.potrf_diag(A)
    assert replay[4]["replayed"] == 1 and replay[3] == 0 and same(base, replay)
    opt(tiles=nt, kbatch=kb, form=0)
    strips = gpu_ctx.potrf_diag(A)
    assert strips[3] == 0 and same(base, strips)
    for kw in ({"order": 0}, {"order": 2}, {"wgs": 4}, {"wgs": 64}, {"wgs": 256}):
        opt(tiles=nt, kbatch=kb, form=tf, **kw)
        v = gpu_ctx.potrf_diag(A)
        assert v[3] == 0 and same(base, v), kw


@pytest.mark.parametrize("k", [140, 600])
def test_not_positive_definite_ends(gpu_ctx, opt, k):
    n = 640
    A, info_want = FC.bad_pivot_matrix(n, (k,))
    Ag = FC.fam_a(n, seed=1)
    opt(tiles=5, kbatch=2, form=tf_of(0, 2))
    before = gpu_ctx.potrf_diag(Ag)
    assert before[3] == 0
    L, X, ld, info, plan = gpu_ctx.potrf_diag(A)
    assert plan["dags"] == 1 and plan["dag_tmax"] == 5
    assert info == info_want
    after = gpu_ctx.potrf_diag(Ag)
    assert after[3] == 0 and same(before, after)


def test_full_fit_40_tile_block_same_bits(gpu_ctx, opt):
    import gpscore
    rng = np.random.default_rng(41)
    n, d = 5000, 8
    X = rng.standard_normal((n, d))
    w = rng.standard_normal(d) / np.sqrt(d)
    y = np.sin(3 * X @ w) + 0.1 * rng.standard_normal(n)
    th = (0.0, np.log(2.0) * np.ones(d), np.log(0.01))
    gp = gpscore.GP(ctx=gpu_ctx)
    assert tile_words(40, 8, tf_of(1, 2))
    outs = []
    for form in (None, tf_of(1, 2), 0):   # the defaults; the form on; strips only
        opt(**({} if form is None else {"form": form}))
        r = gp.fit(X, y, th)
        outs.append((dict(r.objectives), np.array(r.mu_loo), np.array(r.var_loo)))
    for o in outs[:2]:
        assert o[0] == outs[2][0]
        assert np.array_equal(o[1].view(np.uint64), outs[2][1].view(np.uint64))
        assert np.array_equal(o[2].view(np.uint64), outs[2][2].view(np.uint64))
