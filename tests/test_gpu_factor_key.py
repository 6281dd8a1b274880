"""What a factorisation's captured sequence depends on, and what a caller can ask of it (DESIGN
§36): a characterisation of potrf_inv's graph-cache key (api.hip factor_key) and of the requests
(FactorReq) the FITC forward makes.  The first test walks the options one by one on
gps_potrf_diag: each one the sequence reads gets a graph of its own and comes back to the first
graph — and the first bits — when it is put back; each one it does not read leaves the cache
alone.  The second runs every request the FITC forward can make (the pre-pass with and without
signals, top-level signals, none) with a full-GP fit between any two: nothing one factorisation
was asked for reaches the next.  Reference: the GD loops' repeated fits under fixed settings
(KF:237-260, K20:222-234)."""
import numpy as np
import pytest

import factor_cases as FC

pytestmark = pytest.mark.gpu


def _opts():
    """name -> (key, default); TINY_GEMM, STREAM_K, SLAB_XCD and GRAM_REG are process-wide."""
    from gpscore import _lib as G
    return {"OVERLAP": (G.GPS_OPT_OVERLAP, 1), "GEMM_MAP": (G.GPS_OPT_GEMM_MAP, 0),
            "GEMM_LIVE": (G.GPS_OPT_GEMM_LIVE, 1), "TINY_GEMM": (G.GPS_OPT_TINY_GEMM, 1),
            "STREAM_K": (G.GPS_OPT_STREAM_K, 2), "SLAB_XCD": (G.GPS_OPT_SLAB_XCD, 1),
            "DAG": (G.GPS_OPT_DAG, 1), "DAG_TILES": (G.GPS_OPT_DAG_TILES, 20),
            "DAG_KBATCH": (G.GPS_OPT_DAG_KBATCH, G.DAG_KBATCH_DEFAULT),
            "DAG_TILE_FORM": (G.GPS_OPT_DAG_TILE_FORM, G.DAG_TILE_FORM_DEFAULT),
            "DAG_GROUP": (G.GPS_OPT_DAG_GROUP, 3), "DAG_WGS": (G.GPS_OPT_DAG_WGS, 0),
            "DAG_ORDER": (G.GPS_OPT_DAG_ORDER, 1),
            "DAG_TILES_FULL": (G.GPS_OPT_DAG_TILES_FULL, G.DAG_TILES_FULL_DEFAULT),
            "FITC_DEP": (G.GPS_OPT_FITC_DEP, 1), "PRED_PRE": (G.GPS_OPT_PRED_PRE, 1),
            "AR_CHUNKS": (G.GPS_OPT_AR_CHUNKS, 4), "GRAM_REG": (G.GPS_OPT_GRAM_REG, 2),
            "GRAPH": (G.GPS_OPT_GRAPH, 1)}


def _set(ctx, name, value=None):
    key, default = _opts()[name]
    ctx.call("gps_ctx_set_option", key, default if value is None else value)


def _defaults(ctx):
    for name in _opts():
        _set(ctx, name)


def _bits(a, b):
    return all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(a[:3], b[:3]))


# the options the captured sequence reads, each with a value other than its default
IN_KEY = [("OVERLAP", 0), ("GEMM_MAP", 1), ("GEMM_LIVE", 0), ("TINY_GEMM", 0), ("STREAM_K", 0),
          ("SLAB_XCD", 0), ("DAG", 0), ("DAG_TILES", 3), ("DAG_KBATCH", 4), ("DAG_TILE_FORM", 0),
          ("DAG_GROUP", 2), ("DAG_WGS", 64), ("DAG_ORDER", 2)]
# ... and those it does not: the full GP's cap without the full GP's request, the options that act
# through the FITC request, the all-reduce's chunks and the Gram kernels' choice
OUT_OF_KEY = [("DAG_TILES_FULL", 10), ("FITC_DEP", 0), ("PRED_PRE", 0), ("AR_CHUNKS", 1),
              ("GRAM_REG", 1)]


def test_key_rows_on_the_mixed_plan():
    import gpscore
    n, tiles = FC.MIXED
    A = FC.fam_b(n, 1e-2)
    ctx = gpscore.Context(0)
    try:
        _defaults(ctx)
        _set(ctx, "DAG_TILES", tiles)
        first = ctx.potrf_diag(A)
        assert first[3] == 0 and first[4]["replayed"] == 0, first[4]
        assert (first[4]["leaves"], first[4]["dags"], first[4]["gemms"]) == (1, 2, 8), first[4]
        again = ctx.potrf_diag(A)
        assert again[4]["replayed"] == 1 and _bits(again, first)
        assert ctx.stats()["graphs"] == 1
        for i, (name, value) in enumerate(IN_KEY):
            _set(ctx, name, value)
            new = ctx.potrf_diag(A)
            assert new[3] == 0 and new[4]["replayed"] == 0, (name, new[4])
            rep = ctx.potrf_diag(A)
            assert rep[4]["replayed"] == 1 and _bits(rep, new), (name, rep[4])
            assert ctx.stats()["graphs"] == 2 + i, (name, ctx.stats())
            _set(ctx, name, tiles if name == "DAG_TILES" else None)
            back = ctx.potrf_diag(A)
            assert back[4]["replayed"] == 1 and _bits(back, first), (name, back[4])
        graphs = ctx.stats()["graphs"]
        for name, value in OUT_OF_KEY:
            _set(ctx, name, value)
            got = ctx.potrf_diag(A)
            assert got[4]["replayed"] == 1 and _bits(got, first), (name, got[4])
            assert ctx.stats()["graphs"] == graphs, (name, ctx.stats())
            _set(ctx, name)
        s = ctx.stats()
        assert s["graphs"] == 1 + len(IN_KEY) == 14 and s["graph_evicted"] == 0, s
    finally:
        _defaults(ctx)
        ctx.close()


FITC_VEC = ("loo_mu", "loo_var", "pred_mu", "pred_var")


def _fitc_unit(gp, th):
    """fit + predict as test_gpu_fitc_dep._unit; a queue that did not run to completion or a
    dependency wait that timed out raises GpsError in either call."""
    r = gp.fit(theta=th)
    mu, var, sc = gp.predict(with_scores=True)
    out = dict(r.objectives)
    out.update(loo_mu=r.mu_loo, loo_var=r.var_loo, pred_mu=mu, pred_var=var, **sc)
    return out


def _same_fitc(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        if k in FITC_VEC:
            assert np.array_equal(a[k], b[k]), (what, k)
        else:
            assert float(a[k]) == float(b[k]), (what, k, a[k], b[k])


# m_pad of 4 tiles.  GPS_OPT_DAG_TILES 2: both m×m factorisations recurse 2 + 2 and carry the q / r
# pre-pass, with its signals under FITC_DEP (pre-pass on aux[1] behind L11's launch), without them
# under FITC_DEP 0 (aux[0]) and OVERLAP 0 (main stream), and no pre-pass under PRED_PRE 0.
# GPS_OPT_DAG_TILES 20: one launch each, Lm's with the top-level signals under FITC_DEP.
FITC_GROUPS = [(2, [{}, {}, {"FITC_DEP": 0}, {"PRED_PRE": 0}, {"OVERLAP": 0}, {"GRAPH": 0}, {}]),
               (20, [{}, {}, {"FITC_DEP": 0}, {"GRAPH": 0}, {}])]


def test_fitc_requests_leave_nothing_behind():
    import gpscore
    rng = np.random.default_rng(36)
    n, nt, m, d = 700, 100, 500, 4
    X, Xt = rng.standard_normal((n, d)), rng.standard_normal((nt, d))
    Z = X[rng.choice(n, m, replace=False)]
    y, yt = np.sin(X.sum(1)), np.sin(Xt.sum(1))
    th = (0.0, np.log(1.5) * np.ones(d), np.log(0.05))
    Xf = rng.standard_normal((300, d))
    yf = np.sin(Xf.sum(1))
    ctx = gpscore.Context(0)
    try:
        _defaults(ctx)
        fitc, full = gpscore.GP(ctx=ctx), gpscore.GP(ctx=ctx)
        fitc.set_data(X, y, kind="fitc", Z=Z)
        fitc.set_test(Xt, yt)
        full.set_data(Xf, yf)
        full_first = None
        for tiles, variants in FITC_GROUPS:
            _set(ctx, "DAG_TILES", tiles)
            base = None
            for i, variant in enumerate(variants):
                for name, value in variant.items():
                    _set(ctx, name, value)
                got = _fitc_unit(fitc, th)
                for name in variant:
                    _set(ctx, name)
                if base is None:
                    base = got
                _same_fitc(got, base, (tiles, i, variant))
                # (the full fit at the defaults: GPS_OPT_DAG_KBATCH's bit 8 ties the K batches of its
                #  3-tile block to GPS_OPT_DAG_TILES, and batches change the summation order)
                _set(ctx, "DAG_TILES")
                r = full.fit(theta=th)
                _set(ctx, "DAG_TILES", tiles)
                f = (r.objectives, r.mu_loo, r.var_loo)
                if full_first is None:
                    full_first = f
                assert f[0] == full_first[0], (tiles, i, variant)
                assert np.array_equal(f[1], full_first[1]), (tiles, i, variant)
                assert np.array_equal(f[2], full_first[2]), (tiles, i, variant)
    finally:
        _defaults(ctx)
        ctx.close()
