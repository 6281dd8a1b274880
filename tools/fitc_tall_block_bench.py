#!/usr/bin/env python3
"""Times a batch of K20-shaped FITC block-LOO fits (n = 500, d = 8, m = 20 inducing inputs, four
folds, 500 test points from experiment.synthetic_sheets; K20's dss method, 3000 steps at lr = lr_z
= 1e-3 from N(0,1) inducing inputs, K20:523-593, and its kc method, 3000 steps at 0.1, K20:655-726)
two ways on one context, fit + predictive + scores:

  (a) loop    one GP.train(objective) (+ fit + predict) per problem, one after another: every step
              is one gps_fitc_blockloo call with a set_inducing upload (experiment.run(kind="fitc")'s
              route, unchanged by fitc_blockloo_train_tall)
  (b) tall    one fitc_blockloo_train_tall call for all B problems (one workgroup each)

for B in --batches and both methods.  Each side is warmed up at every B, then timed --repeats
times, the two sides alternating; the table reports the median and the spread (min..max).  A host
clock around calls that end in a device synchronise.  (a) is a sequential loop and therefore
linear in B: only min(B, --loop-cap) problems are looped and the time is SCALED by B / that, and
the row says so.  --itr overrides the step count on BOTH sides (the JSON records it).  Also
recorded:

  * the per-step time of the kernel at n in --ns (m = 20, d = 8, four folds; B = 1 and B = 256; both
    objectives), from calls of a few launches each, timed by the profiling events around the
    launches alone;
  * the longest single launch (the steps-per-launch rule's worth of steps plus the final forward,
    B = 256, KC: every CU busy) at K20's shape and at the corner n = 2048, m = 32, d = 16, nfold =
    4, against the project's "a launch is at most ~20 ms".

    python tools/fitc_tall_block_bench.py --out profiles/fitc_tall_block_bench.json
"""
import argparse
import json
import os
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "scoring-rules-for-gaussian-process-regression-a-new-approach-to-inference_amd")
sys.path.insert(0, PKG)
TAG = "batch_fitc_tall_block_train"


def steps_per_launch(n):
    """batch_fitc_tall_block_steps, the divisor read from the header the library was built from."""
    src = open(os.path.join(PKG, "csrc", "gps_internal.h"), encoding="utf-8").read()
    div = int(re.search(r"kBatchFitcTallBlockDiv = (\d+);", src)[1])
    return max(1, 64 // div // ((n + 127) // 128))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--batches", default="1,10,30,256")
    ap.add_argument("--ns", default="128,500,1024,2048")
    ap.add_argument("--itr", type=int, default=None, help="override the methods' step count")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--loop-cap", type=int, default=2, help="loop at most this many problems")
    ap.add_argument("--skip", default="", help="comma list of sections to skip: rows,steps,longest")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    skip = set(filter(None, args.skip.split(",")))

    import gpscore
    from gpscore import experiment as E

    methods = {k: E.K20_METHODS[k] for k in ("dss", "kc")}
    ctx = gpscore.Context(0)
    gp = gpscore.GP(ctx=ctx)
    batches = [int(b) for b in args.batches.split(",")]
    Bmax = max(batches + [256])
    m, d, nfold = 20, 8, 4
    sheets = E.synthetic_sheets(0)
    rng = np.random.default_rng(0)
    data = [E.replicate(sheets, j, n_pool=sheets["trainx"].shape[0]) for j in range(Bmax)]
    X = np.stack([dd["train_x"] for dd in data])
    y = np.stack([dd["train_y"] for dd in data])
    Xt = np.stack([dd["test_x"] for dd in data])
    yt = np.stack([dd["test_y"] for dd in data])
    th0, Z0 = {k: [] for k in methods}, {k: [] for k in methods}
    for _ in range(Bmax):  # run_method's draws: initial_theta, then Z0, U(0,1) or N(0,1)
        for name, meth in methods.items():
            k, ell, noise = E.initial_theta(meth, d, rng)
            th0[name].append(np.concatenate([[k], ell, [noise]]))
            Z0[name].append(rng.random((m, d)) if meth.z_init == "rand"
                            else rng.standard_normal((m, d)))
    th0 = {k: np.stack(v) for k, v in th0.items()}
    Z0 = {k: np.stack(v) for k, v in Z0.items()}

    def timed(f, B):
        t0 = time.perf_counter()
        r = f(B)
        return time.perf_counter() - t0, r

    rows = {}
    for name, meth in ([] if "rows" in skip else methods.items()):
        itr = meth.itr if args.itr is None else args.itr
        t0_, z0_ = th0[name], Z0[name]

        def loop(B):
            out = None
            for q in range(B):
                try:
                    theta, series = gp.train((t0_[q, 0], t0_[q, 1:-1], t0_[q, -1]), meth.objective,
                                             lr=meth.lr, itr=itr, X=X[q], y=y[q], Z0=z0_[q],
                                             lr_z=meth.lr_z)
                    gp.fit(theta=theta, return_loo=False)
                    gp.predict(Xt[q], yt[q], with_scores=True)
                    r = np.concatenate([[theta[0]], theta[1], [theta[2]], series["Z"].ravel()])
                except gpscore.NotPositiveDefinite:  # the fit left the positive-definite region
                    r = np.full(t0_.shape[1] + z0_[q].size, np.nan)
                out = r if q == 0 else out
            return out

        def tall(B):
            return gpscore.fitc_blockloo_train_tall(X[:B], y[:B], z0_[:B], t0_[:B], meth.objective,
                                                    nfold=nfold, lr=meth.lr, lr_z=meth.lr_z,
                                                    itr=itr, Xt=Xt[:B], yt=yt[:B], ctx=ctx)

        rows[name] = []
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
            rows[name].append({"method": name, "B": B, "itr": itr, "looped": Bl,
                               "loop_s": statistics.median(ta), "loop_min": min(ta),
                               "loop_max": max(ta), "tall_s": statistics.median(tb),
                               "tall_min": min(tb), "tall_max": max(tb), "theta_z0_nrel": err,
                               "failed": int(np.count_nonzero(rb.info)),
                               "loop_failed": bool(np.isnan(ra).any()),
                               "bar_met": max(tb) < min(ta)})
            print(json.dumps(rows[name][-1]), flush=True)

    def launches_ms(f):
        """Device time of the launches of one call (the profiling events around them)."""
        ctx.prof(True)
        f()
        rep = ctx.prof_collect()
        ctx.prof(False)
        return rep[TAG]["ms"]

    def shaped(B, n, mm, dd, seed):
        """B problems of n rows from a synthetic pool of dd inputs, K20's KC start."""
        sh = sheets if dd == d else E.synthetic_sheets(1, d=dd)
        r = np.random.default_rng(seed)
        idx = np.stack([r.choice(sh["trainx"].shape[0], n, replace=False) for _ in range(B)])
        return (sh["trainx"][idx], sh["trainy"][idx, 0], r.random((B, mm, dd)),
                np.column_stack([np.ones(B), r.random((B, dd)), np.ones(B)]))

    # per-step time at n (m = 20, d = 8, four folds): four launches' worth of steps
    steps = []
    for n in ([] if "steps" in skip else [int(v) for v in args.ns.split(",")]):
        k = 4 * steps_per_launch(n)
        row = {"n": n, "steps_per_launch": steps_per_launch(n), "steps": k}
        for name, meth in methods.items():
            for B in (1, 256):
                Xn, yn, Zn, tn = shaped(B, n, m, d, n)
                f = lambda: gpscore.fitc_blockloo_train_tall(  # noqa: E731
                    Xn, yn, Zn, tn, meth.objective, nfold=nfold, lr=1e-3, lr_z=1e-3, itr=k, ctx=ctx)
                row["failed_%s_B%d" % (name, B)] = int(np.count_nonzero(f().info))
                ms = statistics.median(launches_ms(f) for _ in range(args.repeats))
                row["step_us_%s_B%d" % (name, B)] = 1e3 * ms / (k + 1)  # k steps + the final forward
        steps.append(row)
        print(json.dumps(row), flush=True)

    # the longest single launch: one launch's worth of steps + the final forward, every CU busy
    longest = []
    for name, n, mm, dd in ([] if "longest" in skip else
                            (("k20", 500, 20, 8), ("corner", 2048, 32, 16))):
        k = steps_per_launch(n)
        Xn, yn, Zn, tn = shaped(256, n, mm, dd, 7)
        f = lambda: gpscore.fitc_blockloo_train_tall(  # noqa: E731
            Xn, yn, Zn, tn, "kc", nfold=nfold, lr=1e-3, lr_z=1e-3, itr=k, ctx=ctx)
        r = f()
        ms = [launches_ms(f) for _ in range(args.repeats)]
        longest.append({"shape": name, "n": n, "m": mm, "d": dd, "nfold": nfold, "B": 256,
                        "objective": "kc", "steps": k, "launch_ms": statistics.median(ms),
                        "launch_ms_max": max(ms), "failed": int(np.count_nonzero(r.info))})
        print(json.dumps(longest[-1]), flush=True)

    res = {"shape": {"n": 500, "d": d, "m": m, "nfold": nfold, "nt": 500,
                     "methods": {k: {"objective": v.objective,
                                     "itr": v.itr if args.itr is None else args.itr,
                                     "lr": v.lr, "lr_z": v.lr_z, "z_init": v.z_init}
                                 for k, v in methods.items()}},
           "itr_overridden": args.itr is not None, "repeats": args.repeats,
           "loop_is_scaled_beyond": args.loop_cap, "rows": rows, "per_step": steps,
           "longest_launch": longest}
    for name, rr in rows.items():
        print("%s" % name)
        print("| B | (a) loop s (min..max) | (b) tall s (min..max) | a / b | (b) max < (a) min |")
        print("|---|---|---|---|---|")
        for r in rr:
            note = "" if r["looped"] == r["B"] else " (from %d problems, scaled)" % r["looped"]
            print("| %d | %.3f (%.3f..%.3f)%s | %.4f (%.4f..%.4f) | %.1f | %s |"
                  % (r["B"], r["loop_s"], r["loop_min"], r["loop_max"], note, r["tall_s"],
                     r["tall_min"], r["tall_max"], r["loop_s"] / r["tall_s"],
                     "yes" if r["bar_met"] else "no"))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
