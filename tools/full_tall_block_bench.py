#!/usr/bin/env python3
"""Times a batch of KF-shaped full-GP fits on the 4-fold block-LOO DSS objective (n = 500, d = 8,
500 test points from experiment.synthetic_sheets, the dss method's 150 steps with lr = 1e-3 from
KF's start, KF:487-601) two ways on one context; the work timed is fit + predictive + scores:

  (a) loop    one GP.train(objective="dss") (+ fit + predict) per problem, one after another:
              every step is one gps_full_blockloo call (experiment.run(kind="full")'s route,
              which blockloo_train_tall does not change)
  (b) tall    one blockloo_train_tall call for all B problems (one workgroup each)

for B in --batches.  Each side is warmed up at every B, then timed --repeats times, the two
sides alternating; the table reports the median and the spread (min..max).  A host clock around
calls that end in a device synchronise.  (a) is a sequential loop and therefore linear in B:
only min(B, --loop-cap) problems are looped and the time is SCALED by B / that, and the row says
so.  Also recorded:

  * the per-step time of the block kernel at n in --ns (d = 8, nfold = 4; B = 1 and B = 256; DSS
    and KC), from calls of a few launches each, timed by the profiling events around the launches
    alone, next to the arithmetic floor of the step's tile products on one CU;
  * the longest single launch (the steps-per-launch rule's worth of DSS steps plus the final
    forward, B = 256: every CU busy) at the corner n = 512, d = 16 and at KF's shape, against the
    project's "a launch is at most ~20 ms".

    python tools/full_tall_block_bench.py --out profiles/full_tall_block_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scoring-rules-for-gaussian-process-regression-a-new-approach-to-inference_amd"))

T = 64
CU_GFLOPS = 78.6e3 / 256  # one CU's share of the FP64 matrix rate


def steps_per_launch(n):
    nb = (n + T - 1) // T
    return min(64, max(1, 1024 // nb ** 3))


def factor_products(nb):
    """T³ tile products of a factorisation, its inverse and XᵀX on nb×nb tiles."""
    fac = sum((nb - k) * k + (nb - 1 - k) for k in range(nb))
    inv = sum((i - j) + 1 for i in range(nb) for j in range(i))
    xtx = sum(nb - i for i in range(nb) for j in range(i + 1))
    return fac + inv + xtx


def tile_products(n, nfold, kc):
    """T³ tile products of one block step: A's factorisation, inverse and XᵀX; the same per fold
    (KC: and Π diag(gc) Π); Y = Gblk·P over the clipped k ranges; the lower tiles of P·Y."""
    nb = (n + T - 1) // T
    edges = [f * n // nfold for f in range(nfold + 1)]
    folds = 0
    for a, b in zip(edges[:-1], edges[1:]):
        nbf = (b - a + T - 1) // T
        folds += factor_products(nbf) + (nbf ** 3 if kc else 0)
    yprod = 0
    for bi in range(nb):
        r0, r1 = bi * T, min(n, bi * T + T) - 1
        lo = max(a for a in edges[:-1] if a <= r0)
        hi = min(b for b in edges[1:] if b > r1)
        yprod += nb * ((hi + T - 1) // T - lo // T)
    return factor_products(nb) + folds + yprod + nb * (nb * (nb + 1) // 2)


def floor_us(n, nfold, kc):
    return 1e6 * tile_products(n, nfold, kc) * 2 * T ** 3 / (CU_GFLOPS * 1e9)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--batches", default="1,30,256")
    ap.add_argument("--ns", default="128,256,500,512")
    ap.add_argument("--itr", type=int, default=None, help="override the method's step count")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--loop-cap", type=int, default=2, help="loop at most this many problems")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import gpscore
    from gpscore import experiment as E

    meth = E.KF_METHODS["dss"]
    nfold = 4
    itr = meth.itr if args.itr is None else args.itr
    ctx = gpscore.Context(0)
    gp = gpscore.GP(ctx=ctx)
    batches = [int(b) for b in args.batches.split(",")]
    Bmax = max(batches + [256])
    d = 8
    sheets = E.synthetic_sheets(0)
    rng = np.random.default_rng(0)
    data = [E.replicate(sheets, j, n_pool=sheets["trainx"].shape[0]) for j in range(Bmax)]
    X = np.stack([dd["train_x"] for dd in data])
    y = np.stack([dd["train_y"] for dd in data])
    Xt = np.stack([dd["test_x"] for dd in data])
    yt = np.stack([dd["test_y"] for dd in data])
    th0 = []
    for _ in range(Bmax):  # run_method's draw
        k, ell, noise = E.initial_theta(meth, d, rng)
        th0.append(np.concatenate([[k], ell, [noise]]))
    th0 = np.stack(th0)

    def loop(B):
        out = None
        for q in range(B):
            try:
                theta, series = gp.train((th0[q, 0], th0[q, 1:-1], th0[q, -1]), meth.objective,
                                         lr=meth.lr, itr=itr, X=X[q], y=y[q])
                gp.fit(theta=theta, return_loo=False)
                gp.predict(Xt[q], yt[q], with_scores=True)
                r = np.concatenate([[theta[0]], theta[1], [theta[2]]])
            except gpscore.NotPositiveDefinite:  # the fit left the positive-definite region
                r = np.full(th0.shape[1], np.nan)
            out = r if q == 0 else out
        return out

    def tall(B):
        return gpscore.blockloo_train_tall(X[:B], y[:B], th0[:B], meth.objective, nfold=nfold,
                                           lr=meth.lr, itr=itr, Xt=Xt[:B], yt=yt[:B], ctx=ctx)

    def timed(f, B):
        t0 = time.perf_counter()
        r = f(B)
        return time.perf_counter() - t0, r

    rows = []
    for B in batches:
        Bl = min(B, max(1, args.loop_cap))
        _, ra = timed(loop, 1)   # warm-up of both sides at this shape
        _, rb = timed(tall, B)
        ta, tb = [], []
        for _ in range(args.repeats):
            t, ra = timed(loop, Bl)
            ta.append(t * B / Bl)
            t, rb = timed(tall, B)
            tb.append(t)
        err = float(np.max(np.abs(ra - rb.theta[0])) / np.max(np.abs(ra)))
        rows.append({"B": B, "looped": Bl, "loop_s": statistics.median(ta), "loop_min": min(ta),
                     "loop_max": max(ta), "tall_s": statistics.median(tb), "tall_min": min(tb),
                     "tall_max": max(tb), "theta0_nrel": err,
                     "failed": int(np.count_nonzero(rb.info)),
                     "loop_failed": bool(np.isnan(ra).any())})
        print(json.dumps(rows[-1]), flush=True)

    def launches_ms(tag, f):
        """Device time of the launches of one call (the profiling events around them)."""
        ctx.prof(True)
        f()
        rep = ctx.prof_collect()
        ctx.prof(False)
        return rep[tag]["ms"]

    def shaped(B, n, dd, seed):
        """B problems of n rows from a synthetic pool of dd inputs, a tame start."""
        sh = sheets if dd == d else E.synthetic_sheets(1, d=dd)
        r = np.random.default_rng(seed)
        idx = np.stack([r.choice(sh["trainx"].shape[0], n, replace=False) for _ in range(B)])
        return (sh["trainx"][idx], sh["trainy"][idx, 0],
                np.column_stack([np.zeros(B), 0.5 + 0.5 * r.random((B, dd)), np.full(B, -3.0)]))

    # per-step time at n (d = 8): about four launches' worth of steps, no final predictive; the
    # step size is tiny so every problem stays where it started
    steps = []
    for n in [int(v) for v in args.ns.split(",")]:
        k = max(8, min(32, 4 * steps_per_launch(n)))
        row = {"n": n, "steps_per_launch": steps_per_launch(n), "steps": k}
        for obj, kc in (("dss", False), ("kc", True)):
            row["floor_us_" + obj] = floor_us(n, nfold, kc)
            row["tile_products_" + obj] = tile_products(n, nfold, kc)
            for B in (1, 256):
                Xn, yn, tn = shaped(B, n, d, n)
                f = lambda: gpscore.blockloo_train_tall(Xn, yn, tn, obj, nfold=nfold, lr=1e-9,  # noqa: E731
                                                        itr=k, ctx=ctx)
                row["failed_%s_B%d" % (obj, B)] = int(np.count_nonzero(f().info))
                ms = [launches_ms("batch_full_tall_block_train", f) for _ in range(args.repeats)]
                # k steps and the final forward (about a quarter of a block step)
                row["step_us_%s_B%d" % (obj, B)] = 1e3 * statistics.median(ms) / k
                row["step_us_%s_B%d_min" % (obj, B)] = 1e3 * min(ms) / k
                row["step_us_%s_B%d_max" % (obj, B)] = 1e3 * max(ms) / k
        steps.append(row)
        print(json.dumps(row), flush=True)

    # the longest single launch: one launch's worth of DSS steps + the final forward, every CU busy
    longest = []
    for name, n, dd in (("kf", 500, 8), ("corner", 512, 16)):
        k = steps_per_launch(n)
        Xn, yn, tn = shaped(256, n, dd, 7)
        f = lambda: gpscore.blockloo_train_tall(Xn, yn, tn, "dss", nfold=nfold, lr=1e-9, itr=k,  # noqa: E731
                                                ctx=ctx)
        r = f()
        ms = [launches_ms("batch_full_tall_block_train", f) for _ in range(args.repeats)]
        longest.append({"shape": name, "n": n, "d": dd, "B": 256, "steps": k,
                        "launch_ms": statistics.median(ms), "launch_ms_min": min(ms),
                        "launch_ms_max": max(ms), "failed": int(np.count_nonzero(r.info))})
        print(json.dumps(longest[-1]), flush=True)

    by = {r["B"]: r for r in rows}
    one = by.get(1, rows[0])
    res = {"shape": {"n": 500, "d": d, "nt": 500, "itr": itr, "objective": meth.objective,
                     "lr": meth.lr, "nfold": nfold}, "repeats": args.repeats,
           "loop_is_scaled_beyond": args.loop_cap, "rows": rows,
           "tall_step_us_B%d" % one["B"]: 1e6 * one["tall_s"] / max(itr, 1),
           "loop_step_us_per_problem": 1e6 * one["loop_s"] / one["B"] / max(itr, 1),
           "per_step": steps, "longest_launch": longest}
    if 1 in by and 256 in by:
        res["B256_over_B1"] = by[256]["tall_s"] / by[1]["tall_s"]
    if 30 in by:
        res["bar_B30_tall_max_below_loop_min"] = by[30]["tall_max"] < by[30]["loop_min"]
    print("| B | (a) loop s (min..max) | (b) tall s (min..max) | a / b |")
    print("|---|---|---|---|")
    for r in rows:
        note = "" if r["looped"] == r["B"] else " (from %d problems, scaled)" % r["looped"]
        print("| %d | %.3f (%.3f..%.3f)%s | %.4f (%.4f..%.4f) | %.1f |"
              % (r["B"], r["loop_s"], r["loop_min"], r["loop_max"], note, r["tall_s"],
                 r["tall_min"], r["tall_max"], r["loop_s"] / r["tall_s"]))
    if "B256_over_B1" in res:
        print("B256_over_B1 = %.3f" % res["B256_over_B1"])
    if 30 in by:
        print("bar (B = 30: (b) max < (a) min):", res["bar_B30_tall_max_below_loop_min"])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
