#!/usr/bin/env python3
"""Times a batch of SD-shaped fits (n = 120, d = 1, 300 test points, 250 LOO-CRPS steps from
(1, 1, 1), SD:192-231) two ways on one context:

  (a) loop    one GP.train per problem, one after another (the only route before train_batch)
  (b) batch   one train_batch call for all B problems (one workgroup each)

for B in --batches.  Each side is warmed up at every B, then timed --repeats times, the two
sides alternating; the table reports the median and the spread (min..max).  A host clock around
calls that end in a device synchronise.  (a) is a sequential loop and therefore linear in B:
with --loop-cap C only min(B, C) problems are looped and the time is scaled by B / C, and the
row says so.  Also reports how far the two sides' final θ of problem 0 are apart (normwise).

    python tools/batch_train_bench.py --out profiles/batch_train_bench.json
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--batches", default="1,8,64,256,300")
    ap.add_argument("--itr", type=int, default=250)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--loop-cap", type=int, default=0, help="loop at most this many problems (0: all B)")
    ap.add_argument("--objective", default="loo_crps")
    ap.add_argument("--lr", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import gpscore
    from gpscore import experiment as E

    ctx = gpscore.Context(0)
    gp = gpscore.GP(ctx=ctx)
    batches = [int(b) for b in args.batches.split(",")]
    data = [E.simple_data(j) for j in range(max(batches))]
    X = np.stack([d["train_x"] for d in data])
    y = np.stack([d["train_y"] for d in data])
    Xt = np.stack([d["test_x"] for d in data])
    yt = np.stack([d["test_y"] for d in data])
    th0 = (1.0, 1.0, 1.0)

    def loop(B):
        out = None
        for q in range(B):
            try:
                theta, _ = gp.train(th0, args.objective, lr=args.lr, itr=args.itr, X=X[q], y=y[q])
                gp.fit(theta=theta, return_loo=False)
                gp.predict(Xt[q], yt[q], with_scores=True)
            except gpscore.NotPositiveDefinite:  # the fit left the positive-definite region
                theta = (np.nan, np.array([np.nan]), np.nan)
            out = theta if q == 0 else out
        return out

    def batch(B):
        return gpscore.train_batch(X[:B], y[:B], th0, args.objective, lr=args.lr, itr=args.itr,
                                   Xt=Xt[:B], yt=yt[:B], ctx=ctx)

    def timed(f, B):
        t0 = time.perf_counter()
        r = f(B)
        return time.perf_counter() - t0, r

    rows = []
    for B in batches:
        Bl = B if args.loop_cap <= 0 else min(B, args.loop_cap)
        _, ra = timed(loop, 1)   # warm-up of both sides at this shape
        _, rb = timed(batch, B)
        ta, tb = [], []
        for _ in range(args.repeats):
            t, ra = timed(loop, Bl)
            ta.append(t * B / Bl)
            t, rb = timed(batch, B)
            tb.append(t)
        a0 = np.concatenate([[ra[0]], ra[1], [ra[2]]])
        err = float(np.max(np.abs(a0 - rb.theta[0])) / np.max(np.abs(a0)))
        rows.append({"B": B, "looped": Bl, "loop_s": statistics.median(ta), "loop_min": min(ta),
                     "loop_max": max(ta), "batch_s": statistics.median(tb), "batch_min": min(tb),
                     "batch_max": max(tb), "theta0_nrel": err, "failed": int(np.count_nonzero(rb.info))})
        print(json.dumps(rows[-1]), flush=True)
    one = next((r for r in rows if r["B"] == 1), rows[0])
    res = {"shape": {"n": 120, "d": 1, "nt": 300, "itr": args.itr, "objective": args.objective,
                     "lr": args.lr}, "repeats": args.repeats, "rows": rows,
           "batch_step_us_B%d" % one["B"]: 1e6 * one["batch_s"] / max(args.itr, 1),
           "loop_step_us_per_problem": 1e6 * one["loop_s"] / one["B"] / max(args.itr, 1)}
    print("| B | (a) loop s (min..max) | (b) batch s (min..max) | a / b |")
    print("|---|---|---|---|")
    for r in rows:
        note = "" if r["looped"] == r["B"] else " (from %d problems, scaled)" % r["looped"]
        print("| %d | %.3f (%.3f..%.3f)%s | %.4f (%.4f..%.4f) | %.1f |"
              % (r["B"], r["loop_s"], r["loop_min"], r["loop_max"], note, r["batch_s"],
                 r["batch_min"], r["batch_max"], r["loop_s"] / r["batch_s"]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
