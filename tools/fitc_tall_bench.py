#!/usr/bin/env python3
"""Times a batch of K20-shaped FITC fits (n = 500, d = 8, m = 20 inducing inputs, 500 test points
from experiment.synthetic_sheets, the LOO-CRPS method's 2000 steps with lr = lr_z = 1 from K20's
random start, K20:207-247) two ways on one context:

  (a) loop    one GP.train (+ fit + predict) per problem, one after another: every step is one
              gps_fitc_grad call with a set_inducing upload (experiment.run(kind="fitc")'s route,
              unchanged by fitc_train_tall)
  (b) tall    one fitc_train_tall call for all B problems (one workgroup each)

for B in --batches.  Each side is warmed up at every B, then timed --repeats times, the two
sides alternating; the table reports the median and the spread (min..max).  A host clock around
calls that end in a device synchronise.  (a) is a sequential loop and therefore linear in B:
only min(B, --loop-cap) problems are looped and the time is SCALED by B / that, and the row says
so.  Also recorded:

  * the per-step time of the tall kernel at n in --ns (m = 20, d = 8; B = 1 and B = 256), from
    calls of a few launches each, timed by the profiling events around the launches alone;
  * the longest single launch (the steps-per-launch rule's worth of steps plus the final forward,
    B = 256: every CU busy) at K20's shape and at the corner n = 2048, m = 32, d = 16, against the
    project's "a launch is at most ~20 ms";
  * the small batch kernel against the tall one at SF's shape n = 120, d = 1, m = 5 (1000 LOO-CRPS
    steps, B = 256), where the small kernel stays the route.

    python tools/fitc_tall_bench.py --out profiles/fitc_tall_bench.json
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


def steps_per_launch(n):
    return max(1, 64 // ((n + 127) // 128))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--batches", default="1,10,30,256,300")
    ap.add_argument("--ns", default="128,500,1024,2048")
    ap.add_argument("--itr", type=int, default=None, help="override the method's step count")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--loop-cap", type=int, default=2, help="loop at most this many problems")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import gpscore
    from gpscore import experiment as E

    meth = E.K20_METHODS["crps"]
    itr = meth.itr if args.itr is None else args.itr
    ctx = gpscore.Context(0)
    gp = gpscore.GP(ctx=ctx)
    batches = [int(b) for b in args.batches.split(",")]
    Bmax = max(batches + [256])
    m, d = 20, 8
    sheets = E.synthetic_sheets(0)
    rng = np.random.default_rng(0)
    data = [E.replicate(sheets, j, n_pool=sheets["trainx"].shape[0]) for j in range(Bmax)]
    X = np.stack([dd["train_x"] for dd in data])
    y = np.stack([dd["train_y"] for dd in data])
    Xt = np.stack([dd["test_x"] for dd in data])
    yt = np.stack([dd["test_y"] for dd in data])
    th0, Z0 = [], []
    for _ in range(Bmax):  # run_method's draws: initial_theta, then Z0
        k, ell, noise = E.initial_theta(meth, d, rng)
        th0.append(np.concatenate([[k], ell, [noise]]))
        Z0.append(rng.random((m, d)))
    th0, Z0 = np.stack(th0), np.stack(Z0)

    def loop(B):
        out = None
        for q in range(B):
            try:
                theta, series = gp.train((th0[q, 0], th0[q, 1:-1], th0[q, -1]), meth.objective,
                                         lr=meth.lr, itr=itr, X=X[q], y=y[q], Z0=Z0[q],
                                         lr_z=meth.lr_z)
                gp.fit(theta=theta, return_loo=False)
                gp.predict(Xt[q], yt[q], with_scores=True)
                r = np.concatenate([[theta[0]], theta[1], [theta[2]], series["Z"].ravel()])
            except gpscore.NotPositiveDefinite:  # the fit left the positive-definite region
                r = np.full(th0.shape[1] + Z0[q].size, np.nan)
            out = r if q == 0 else out
        return out

    def tall(B):
        return gpscore.fitc_train_tall(X[:B], y[:B], Z0[:B], th0[:B], meth.objective, lr=meth.lr,
                                       lr_z=meth.lr_z, itr=itr, Xt=Xt[:B], yt=yt[:B], ctx=ctx)

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
        b0 = np.concatenate([rb.theta[0], rb.Z[0].ravel()])
        err = float(np.max(np.abs(ra - b0)) / np.max(np.abs(ra)))
        rows.append({"B": B, "looped": Bl, "loop_s": statistics.median(ta), "loop_min": min(ta),
                     "loop_max": max(ta), "tall_s": statistics.median(tb), "tall_min": min(tb),
                     "tall_max": max(tb), "theta_z0_nrel": err,
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

    def shaped(B, n, mm, dd, seed):
        """B problems of n rows from a synthetic pool of dd inputs, K20's start."""
        sh = sheets if dd == d else E.synthetic_sheets(1, d=dd)
        r = np.random.default_rng(seed)
        idx = np.stack([r.choice(sh["trainx"].shape[0], n, replace=False) for _ in range(B)])
        return (sh["trainx"][idx], sh["trainy"][idx, 0], r.random((B, mm, dd)),
                np.column_stack([np.ones(B), r.random((B, dd)), np.ones(B)]))

    # per-step time at n (m = 20, d = 8): four launches' worth of steps, no final predictive
    steps = []
    for n in [int(v) for v in args.ns.split(",")]:
        k = 4 * steps_per_launch(n)
        row = {"n": n, "steps_per_launch": steps_per_launch(n), "steps": k}
        for B in (1, 256):
            Xn, yn, Zn, tn = shaped(B, n, m, d, n)
            f = lambda: gpscore.fitc_train_tall(Xn, yn, Zn, tn, meth.objective, lr=meth.lr,
                                                lr_z=meth.lr_z, itr=k, ctx=ctx)
            row["failed_B%d" % B] = int(np.count_nonzero(f().info))
            ms = statistics.median(launches_ms("batch_fitc_tall_train", f)
                                   for _ in range(args.repeats))
            row["step_us_B%d" % B] = 1e3 * ms / (k + 1)  # k steps and the final forward
        steps.append(row)
        print(json.dumps(row), flush=True)

    # the longest single launch: one launch's worth of steps + the final forward, every CU busy
    longest = []
    for name, n, mm, dd in (("k20", 500, 20, 8), ("corner", 2048, 32, 16)):
        k = steps_per_launch(n)
        Xn, yn, Zn, tn = shaped(256, n, mm, dd, 7)
        f = lambda: gpscore.fitc_train_tall(Xn, yn, Zn, tn, "loo_crps", lr=0.01, lr_z=0.01, itr=k,
                                            ctx=ctx)
        r = f()
        ms = [launches_ms("batch_fitc_tall_train", f) for _ in range(args.repeats)]
        longest.append({"shape": name, "n": n, "m": mm, "d": dd, "B": 256, "steps": k,
                        "launch_ms": statistics.median(ms), "launch_ms_max": max(ms),
                        "failed": int(np.count_nonzero(r.info))})
        print(json.dumps(longest[-1]), flush=True)

    # SF's shape: the small kernel against the tall one (the small kernel stays the route there)
    sf = E.SF_METHODS["crps"]
    sd = [E.simple_data(j) for j in range(256)]
    Xs = np.stack([q["train_x"] for q in sd])
    ys = np.stack([q["train_y"] for q in sd])
    Zs = np.stack([E.simple_inducing(j) for j in range(256)])
    small_vs_tall = {}
    for B in (1, 256):
        kw = dict(lr=sf.lr, lr_z=sf.lr_z, itr=sf.itr, ctx=ctx)
        fs = lambda B_: gpscore.fitc_train_batch(Xs[:B_], ys[:B_], Zs[:B_], (1.0, 1.0, 1.0),
                                                 sf.objective, **kw)
        ft = lambda B_: gpscore.fitc_train_tall(Xs[:B_], ys[:B_], Zs[:B_], (1.0, 1.0, 1.0),
                                                sf.objective, **kw)
        fs(B), ft(B)
        ts, tt = [], []
        for _ in range(args.repeats):
            ts.append(timed(fs, B)[0])
            t, rt = timed(ft, B)
            tt.append(t)
        rs = fs(B)
        small_vs_tall["B%d" % B] = {
            "small_s": statistics.median(ts), "tall_s": statistics.median(tt),
            "tall_over_small": statistics.median(tt) / statistics.median(ts),
            "theta_nrel": float(np.max(np.abs(rs.theta - rt.theta)) / np.max(np.abs(rs.theta)))}
        print(json.dumps(small_vs_tall["B%d" % B]), flush=True)

    by = {r["B"]: r for r in rows}
    one = by.get(1, rows[0])
    res = {"shape": {"n": 500, "d": d, "m": m, "nt": 500, "itr": itr, "objective": meth.objective,
                     "lr": meth.lr, "lr_z": meth.lr_z}, "repeats": args.repeats,
           "loop_is_scaled_beyond": args.loop_cap, "rows": rows,
           "tall_step_us_B%d" % one["B"]: 1e6 * one["tall_s"] / max(itr, 1),
           "loop_step_us_per_problem": 1e6 * one["loop_s"] / one["B"] / max(itr, 1),
           "per_step": steps, "longest_launch": longest, "sf_shape_n120_m5": small_vs_tall}
    if 1 in by and 256 in by:
        res["B256_over_B1"] = by[256]["tall_s"] / by[1]["tall_s"]
    if 256 in by and 300 in by:
        res["B300_over_B256"] = by[300]["tall_s"] / by[256]["tall_s"]
    print("| B | (a) loop s (min..max) | (b) tall s (min..max) | a / b |")
    print("|---|---|---|---|")
    for r in rows:
        note = "" if r["looped"] == r["B"] else " (from %d problems, scaled)" % r["looped"]
        print("| %d | %.3f (%.3f..%.3f)%s | %.4f (%.4f..%.4f) | %.1f |"
              % (r["B"], r["loop_s"], r["loop_min"], r["loop_max"], note, r["tall_s"],
                 r["tall_min"], r["tall_max"], r["loop_s"] / r["tall_s"]))
    for k in ("B256_over_B1", "B300_over_B256"):
        if k in res:
            print("%s = %.3f" % (k, res[k]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
