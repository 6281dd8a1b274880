#!/usr/bin/env python3
"""Times a batch of SF-shaped FITC fits (n = 120, d = 1, m = 5 inducing inputs, 300 test points,
the LOO-CRPS method's 1000 steps from (1, 1, 1) with lr = lr_z = 1, SF:189-237) two ways on one
context:

  (a) loop    one GP.train (+ fit + predict) per problem, one after another: every step is one
              gps_fitc_grad call with a set_inducing upload (the only route before
              fitc_train_batch, and unchanged by it)
  (b) batch   one fitc_train_batch call for all B problems (one workgroup each)

for B in --batches.  Each side is warmed up at every B, then timed --repeats times, the two
sides alternating; the table reports the median and the spread (min..max).  A host clock around
calls that end in a device synchronise.  (a) is a sequential loop and therefore linear in B:
only min(B, --loop-cap) problems are looped and the time is scaled by B / that, and the row says
so.  Also reports how far the two sides' final θ and Z of problem 0 are apart (normwise), and
whether B = 256 costs what B = 1 costs (one round of workgroups on 256 CUs) and B = 300 about
twice that.

    python tools/fitc_batch_bench.py --out profiles/fitc_batch_bench.json
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
    ap.add_argument("--batches", default="1,8,100,256,300")
    ap.add_argument("--method", default="crps", help="a key of experiment.SF_METHODS")
    ap.add_argument("--itr", type=int, default=None, help="override the method's step count")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--loop-cap", type=int, default=8, help="loop at most this many problems")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import gpscore
    from gpscore import experiment as E

    meth = E.SF_METHODS[args.method]
    itr = meth.itr if args.itr is None else args.itr
    ctx = gpscore.Context(0)
    gp = gpscore.GP(ctx=ctx)
    batches = [int(b) for b in args.batches.split(",")]
    data = [E.simple_data(j) for j in range(max(batches))]
    X = np.stack([d["train_x"] for d in data])
    y = np.stack([d["train_y"] for d in data])
    Xt = np.stack([d["test_x"] for d in data])
    yt = np.stack([d["test_y"] for d in data])
    Z0 = np.stack([E.simple_inducing(j) for j in range(max(batches))])
    th0 = (1.0, np.array([1.0]), 1.0)

    def loop(B):
        out = None
        for q in range(B):
            try:
                theta, series = gp.train(th0, meth.objective, lr=meth.lr, itr=itr, X=X[q], y=y[q],
                                         Z0=Z0[q], lr_z=meth.lr_z)
                gp.fit(theta=theta, return_loo=False)
                gp.predict(Xt[q], yt[q], with_scores=True)
                r = np.concatenate([[theta[0]], theta[1], [theta[2]], series["Z"].ravel()])
            except gpscore.NotPositiveDefinite:  # the fit left the positive-definite region
                r = np.full(3 + Z0[q].size, np.nan)
            out = r if q == 0 else out
        return out

    def batch(B):
        return gpscore.fitc_train_batch(X[:B], y[:B], Z0[:B], (1.0, 1.0, 1.0), meth.objective,
                                        lr=meth.lr, lr_z=meth.lr_z, itr=itr, Xt=Xt[:B], yt=yt[:B],
                                        ctx=ctx)

    def timed(f, B):
        t0 = time.perf_counter()
        r = f(B)
        return time.perf_counter() - t0, r

    rows = []
    for B in batches:
        Bl = min(B, max(1, args.loop_cap))
        _, ra = timed(loop, 1)   # warm-up of both sides at this shape
        _, rb = timed(batch, B)
        ta, tb = [], []
        for _ in range(args.repeats):
            t, ra = timed(loop, Bl)
            ta.append(t * B / Bl)
            t, rb = timed(batch, B)
            tb.append(t)
        b0 = np.concatenate([rb.theta[0], rb.Z[0].ravel()])
        err = float(np.max(np.abs(ra - b0)) / np.max(np.abs(ra)))
        rows.append({"B": B, "looped": Bl, "loop_s": statistics.median(ta), "loop_min": min(ta),
                     "loop_max": max(ta), "batch_s": statistics.median(tb), "batch_min": min(tb),
                     "batch_max": max(tb), "theta_z0_nrel": err,
                     "failed": int(np.count_nonzero(rb.info))})
        print(json.dumps(rows[-1]), flush=True)
    by = {r["B"]: r for r in rows}
    one = by.get(1, rows[0])
    res = {"shape": {"n": 120, "d": 1, "m": 5, "nt": 300, "itr": itr, "objective": meth.objective,
                     "lr": meth.lr, "lr_z": meth.lr_z}, "repeats": args.repeats, "rows": rows,
           "batch_step_us_B%d" % one["B"]: 1e6 * one["batch_s"] / max(itr, 1),
           "loop_step_us_per_problem": 1e6 * one["loop_s"] / one["B"] / max(itr, 1)}
    if 1 in by and 256 in by:
        res["B256_over_B1"] = by[256]["batch_s"] / by[1]["batch_s"]
    if 256 in by and 300 in by:
        res["B300_over_B256"] = by[300]["batch_s"] / by[256]["batch_s"]
    print("| B | (a) loop s (min..max) | (b) batch s (min..max) | a / b |")
    print("|---|---|---|---|")
    for r in rows:
        note = "" if r["looped"] == r["B"] else " (from %d problems, scaled)" % r["looped"]
        print("| %d | %.3f (%.3f..%.3f)%s | %.4f (%.4f..%.4f) | %.1f |"
              % (r["B"], r["loop_s"], r["loop_min"], r["loop_max"], note, r["batch_s"],
                 r["batch_min"], r["batch_max"], r["loop_s"] / r["batch_s"]))
    for k in ("B256_over_B1", "B300_over_B256"):
        if k in res:
            print("%s = %.3f" % (k, res[k]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
