"""The persistent factorisation with K-batched UPD / UPDX tasks on the device
(GPS_OPT_DAG_KBATCH), through gps_potrf_diag as tests/test_gpu_factor.py drives it: at
the block sizes where the batching first acts, first leaves a shortened run, splits oddly (21) and
at the 40-tile block the full GP's fit takes under GPS_OPT_DAG_TILES_FULL = 40 —

* the componentwise bounds and the structure checks of tests/factor_cases.py hold;
* queue orders 0, 1, 2 and 4, 64, 256 workgroups give the same bits, and a graph replay the bits
  of the first run;
* a non-positive-definite block reports its minor and the launch ends;
* a full fit whose factorisation is one 40-tile block agrees with the oracle.
tests/test_dag_kbatch_logic.py checks the task lists themselves on the CPU."""
import numpy as np
import pytest

import factor_cases as FC
import gp_oracle as O
from conftest import nrel
from dag_model import decode, task_list

pytestmark = pytest.mark.gpu


@pytest.fixture
def opt(gpu_ctx):
    """Sets factorisation options for one test and puts the library's defaults back."""
    from gpscore import _lib as G
    keys = {"tiles": (G.GPS_OPT_DAG_TILES, 20), "graph": (G.GPS_OPT_GRAPH, 1),
            "wgs": (G.GPS_OPT_DAG_WGS, 0), "order": (G.GPS_OPT_DAG_ORDER, 1),
            "kbatch": (G.GPS_OPT_DAG_KBATCH, G.DAG_KBATCH_DEFAULT),
            "tiles_full": (G.GPS_OPT_DAG_TILES_FULL, G.DAG_TILES_FULL_DEFAULT)}

    def set_(**kw):
        for k, (key, default) in keys.items():
            gpu_ctx.call("gps_ctx_set_option", key, int(kw.get(k, default)))

    set_()
    yield set_
    set_()


def tiles(T, kb, kg):
    """Per (type, tile row, tile column): the sorted (first term within the tile, length) of its
    UPD / UPDX tasks in the queue."""
    out = {}
    for typ, part, i, j, k, fine, ln, _ in decode(task_list(T, kb=kb, kg=kg)):
        if typ in (2, 3) and part == 0:
            key, first = ((typ, i, j), k) if typ == 2 else ((typ, i, k), j - k)
            out.setdefault(key, []).append((first, ln))
    return {k: sorted(v) for k, v in out.items()}


def lens(T, kb, kg):
    return {fl for v in tiles(T, kb, kg).values() for fl in v}


def smallest_T(pred):
    return next(T for T in range(2, 65) if pred(T))


def same(a, b):
    return all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(a[:3], b[:3]))


KB, KG = 4, 1
# the smallest block with a batch of two terms, and the smallest with a full batch of KB terms
# followed by a shortened one (found from the task lists: no device needed)
T_FIRST = smallest_T(lambda T: any(ln == 2 for _, ln in lens(T, KB, KG)))
# (a tile with KB + 1 batched terms: one full run, a run of one, then the KG single terms — the
#  first block in which some tile's first KB + 1 terms are not one run of KB and a kept term)
T_REMAINDER = smallest_T(lambda T: any(len(v) > 1 + KG and v[0] == (0, KB)
                                       for v in tiles(T, KB, KG).values()))
CASES = [(T_FIRST, KB, KG, "a"), (T_FIRST, 2, 0, "b6"), (T_REMAINDER, KB, KG, "a"),
         (T_REMAINDER, KB, KG, "b6"), (21, 8, 2, "a"), (21, 8, 0, "b6"), (40, 8, 0, "b2")]


def test_case_sizes():
    assert (T_FIRST, T_REMAINDER) == (KG + 3, KB + KG + 2)
    assert tiles(T_REMAINDER, KB, KG)[(3, T_REMAINDER - 1, 0)] == [(0, KB), (KB, 1), (KB + 1, 1)]
    assert max(ln for _, ln in lens(40, 8, 0)) == 8


@pytest.mark.parametrize("nt,kb,kg,fam", CASES)
def test_batched_block(gpu_ctx, opt, nt, kb, kg, fam):
    n = FC.TILE * nt - 37
    A = FC.family(fam, n)
    kbatch = kb | kg << 4
    opt(tiles=nt, kbatch=kbatch)
    base = gpu_ctx.potrf_diag(A)
    plan = base[4]
    assert (plan["leaves"], plan["dags"], plan["dag_tmax"], plan["gemms"]) == (0, 1, nt, 0), plan
    assert base[3] == 0
    rows = FC.rows_for(n, True, nt)
    if nt == 40:
        # the longdouble references cost ~0.25 s per row at this size: every fourth sampled row
        # (tile boundaries across the block) and the last real and padded rows; the same bounds
        rows = np.unique(np.concatenate([rows[::4], [n - 1, FC.n_pad_of(n) - 1]]))
    bad, r = FC.check_factor(FC.pad_identity(A), base[0], base[1], rows, True, nt)
    print(f"kbatch gpu T={nt} B={kb} g={kg} {fam}: " + " ".join(f"{k}={v:.3g}" for k, v in r.items()))
    assert bad == [], r
    assert FC.check_structure(base[0], base[1], base[2], n) == []
    replay = gpu_ctx.potrf_diag(A)
    assert replay[4]["replayed"] == 1 and replay[3] == 0 and same(base, replay)
    for kw in ({"order": 0}, {"order": 2}, {"wgs": 4}, {"wgs": 64}, {"wgs": 256}):
        opt(tiles=nt, kbatch=kbatch, **kw)
        v = gpu_ctx.potrf_diag(A)
        assert v[3] == 0 and same(base, v), kw
    if nt <= 21:  # the batched queue did run: another summation order than every term a task
        opt(tiles=nt, kbatch=0)
        single = gpu_ctx.potrf_diag(A)
        assert single[3] == 0 and not same(base, single)


@pytest.mark.parametrize("k", [128, 300])
def test_not_positive_definite_ends(gpu_ctx, opt, k):
    """T = 3 with batches (B = 2, g = 0): the minor is reported, the launch ends, and the next
    clean factorisation is bitwise the one before."""
    n = 384
    A, info_want = FC.bad_pivot_matrix(n, (k,))
    Ag = FC.fam_a(n, seed=1)
    opt(tiles=3, kbatch=2)
    assert any(ln == 2 for _, ln in lens(3, 2, 0))
    before = gpu_ctx.potrf_diag(Ag)
    assert before[3] == 0
    L, X, ld, info, plan = gpu_ctx.potrf_diag(A)
    assert plan["dags"] == 1 and plan["dag_tmax"] == 3
    assert info == info_want
    after = gpu_ctx.potrf_diag(Ag)
    assert after[3] == 0 and same(before, after)


def test_full_fit_one_40_tile_block_vs_oracle(gpu_ctx, opt):
    """n = 5000 pads to 40 tiles: with GPS_OPT_DAG_TILES_FULL = 40 the fit's factorisation is one
    persistent launch (GPS_OPT_DAG_TILES stays 20: two blocks and four products otherwise); every
    objective, LOO and predictive output against the oracle at the parity tolerance."""
    import gpscore
    rng = np.random.default_rng(41)
    n, nt, d = 5000, 300, 8
    X, Xt = rng.standard_normal((n, d)), rng.standard_normal((nt, d))
    w = rng.standard_normal(d) / np.sqrt(d)
    y, yt = np.sin(3 * X @ w) + 0.1 * rng.standard_normal(n), np.sin(3 * Xt @ w)
    th = (0.0, np.log(2.0) * np.ones(d), np.log(0.01))
    ref = O.fast_full(X, y, Xt, yt, *th)
    gp = gpscore.GP(ctx=gpu_ctx)
    outs = []
    for tiles_full, kbatch in ((40, 8 | 256), (0, 0)):   # the defaults; the schedule of before
        opt(tiles_full=tiles_full, kbatch=kbatch)
        r = gp.fit(X, y, th)
        mu, var, sc = gp.predict(Xt, yt, with_scores=True)
        for k, v in (("loo_mu", r.mu_loo), ("loo_var", r.var_loo), ("pred_mu", mu), ("pred_var", var)):
            assert nrel(v, ref[k]) <= 1e-9, (tiles_full, k, nrel(v, ref[k]))
        for k in ("nlml", "loo_crps", "loo_logs", "logdet", "quad"):
            assert abs(r.objectives[k] - ref[k]) <= 1e-9 * max(1.0, abs(ref[k])), (tiles_full, k)
        for k in ("test_crps", "test_logs"):
            assert abs(sc[k] - ref[k]) <= 1e-9 * max(1.0, abs(ref[k])), (tiles_full, k)
        outs.append(r.objectives["logdet"])
    assert outs[0] != outs[1]   # another schedule ran (the cap and the batches took effect)
