#!/usr/bin/env python3
"""Times a batch of KF-shaped full-GP fits on the 4-fold block-LOO energy score (n = 500, d = 8,
500 test points from experiment.synthetic_sheets, the es method's 25 steps with lr = 0.1 from KF's
start and 300 draws a fold redrawn every step, KF:607-732) two ways on one context; the work timed
is fit + predictive + scores:

  (a) loop    per problem 25 × (GP.block_loo(θ, "es", grad=True, draws=set_i) + the update), then
              GP.fit + GP.predict, one problem after another (experiment.run(kind="full")'s route,
              which es_train_tall does not change)
  (b) tall    one es_train_tall call for all B problems

for B in --batches.  The draws of both sides are made before the clock starts (the host generator
is common to both) and their time is reported on its own.  Each side is warmed up at every B, then
timed --repeats times, the two sides alternating; the table reports the median and the spread
(min..max).  A host clock around calls that end in a device synchronise.  (a) is a sequential loop
and therefore linear in B: only min(B, --loop-cap) problems are looped and the time is SCALED by B /
that, and the row says so.  A batch's draws are kept under --max-draw-gb (2 GB: 25 sets at B = 30),
well inside the 8 GiB a call may take, by using fewer draw sets (B = 256: 3 sets, cycled; stated in
the row); (a) cycles through the same sets.  Also recorded, from the profiling events around the
launches of a one-step fit: the launch times at KF's shape and at the corner n = 512, d = 16,
num_sim = 512, against the project's "a launch is at most ~20 ms" — at B = 64, where the fold work
is ONE launch of 256 workgroups (the most a fold launch holds: one round of the chip), and at the
largest B <= 256 whose workspace passes the 8 GiB rule, where the per-problem launches have every
CU busy and the "folds" figure is the sum of ceil(B / 64) launches.

    python tools/full_tall_es_bench.py --out profiles/full_tall_es_bench.json
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
MAX_DOUBLES = 1 << 30  # api_batch.hip's kMaxDoubles
PHASES = ("forward", "folds", "tail", "final")


def pad(n):
    return T * ((n + T - 1) // T)


def ws_doubles(n, nfold, S):
    """batch_full_tall_es_ws_doubles."""
    np_, bp, Sp = pad(n), pad(-(-n // nfold)), pad(S + 1)
    return 3 * np_ * np_ + 2 * np_ + 72 + nfold * (11 * bp * bp + 6 * Sp * bp + Sp * Sp)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--batches", default="1,30,256")
    ap.add_argument("--itr", type=int, default=None, help="override the method's step count")
    ap.add_argument("--num-sim", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--loop-cap", type=int, default=2, help="loop at most this many problems")
    ap.add_argument("--max-draw-gb", type=float, default=2.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import gpscore
    from gpscore import experiment as E
    from gpscore.gp import es_draws

    meth = E.KF_METHODS["es"]
    nfold, S = 4, args.num_sim
    itr = meth.itr if args.itr is None else args.itr
    ctx = gpscore.Context(0)
    gp = gpscore.GP(ctx=ctx)
    batches = [int(b) for b in args.batches.split(",")]
    Bmax = max(batches)
    d, n = 8, 500
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
    per = 2 * S * n

    def sets_for(B):
        """The most draw sets (<= itr) that keep the draws under --max-draw-gb."""
        return int(max(1, min(max(itr, 1), args.max_draw_gb * 1e9 // (8 * B * per))))

    def loop(B, draws):
        out = None
        for q in range(B):
            th = th0[q].copy()
            gp.set_data(X[q], y[q], kind="full")
            try:
                for i in range(itr):
                    _, g, _ = gp.block_loo((th[0], th[1:-1], th[-1]), "es", nfold, grad=True,
                                           num_sim=S, draws=draws[q, i % draws.shape[1]])
                    th -= meth.lr * g
                gp.fit(theta=(th[0], th[1:-1], th[-1]), return_loo=False)
                gp.predict(Xt[q], yt[q], with_scores=True)
                r = th
            except gpscore.NotPositiveDefinite:  # the fit left the positive-definite region
                r = np.full(th0.shape[1], np.nan)
            out = r if q == 0 else out
        return out

    def tall(B, draws):
        return gpscore.es_train_tall(X[:B], y[:B], th0[:B], nfold=nfold, num_sim=S, lr=meth.lr,
                                     itr=itr, draws=draws, draw_sets=draws.shape[1], Xt=Xt[:B],
                                     yt=yt[:B], ctx=ctx)

    def timed(f, *a):
        t0 = time.perf_counter()
        r = f(*a)
        return time.perf_counter() - t0, r

    rows = []
    for B in batches:
        Bl = min(B, max(1, args.loop_cap))
        sets = sets_for(B)
        gen = np.random.default_rng(B)
        t0 = time.perf_counter()
        draws = np.empty((B, sets, per))
        for q in range(B):
            for k in range(sets):
                draws[q, k] = es_draws(n, nfold, S, gen)
        t_draws = time.perf_counter() - t0
        _, ra = timed(loop, 1, draws)   # warm-up of both sides at this shape
        _, rb = timed(tall, B, draws)
        ta, tb = [], []
        for _ in range(args.repeats):
            t, ra = timed(loop, Bl, draws)
            ta.append(t * B / Bl)
            t, rb = timed(tall, B, draws)
            tb.append(t)
        err = float(np.max(np.abs(ra - rb.theta[0])) / np.max(np.abs(ra)))
        rows.append({"B": B, "looped": Bl, "draw_sets": sets, "draws_host_s": t_draws,
                     "draws_GB": draws.nbytes / 1e9,
                     "loop_s": statistics.median(ta), "loop_min": min(ta), "loop_max": max(ta),
                     "tall_s": statistics.median(tb), "tall_min": min(tb), "tall_max": max(tb),
                     "theta0_nrel": err, "failed": int(np.count_nonzero(rb.info)),
                     "loop_failed": bool(np.isnan(ra).any())})
        print(json.dumps(rows[-1]), flush=True)
        del draws

    def launches_ms(f):
        """Device time of every launch of one call (the profiling events around each)."""
        ctx.prof(True)
        f()
        rep = ctx.prof_collect()
        ctx.prof(False)
        return {ph: rep["batch_full_tall_es_" + ph]["ms"] for ph in PHASES
                if "batch_full_tall_es_" + ph in rep}

    longest = []
    shapes = (("kf", 500, 8, S), ("corner", 512, 16, 512))
    for name, nn, dd, SS, B in [sh + (b,) for sh in shapes
                                for b in (256 // nfold,
                                          int(min(256, MAX_DOUBLES // ws_doubles(sh[1], nfold, sh[3]))))]:
        sh = sheets if dd == d else E.synthetic_sheets(1, d=dd)
        r = np.random.default_rng(7)
        idx = np.stack([r.choice(sh["trainx"].shape[0], nn, replace=False) for _ in range(B)])
        Xn, yn = sh["trainx"][idx], sh["trainy"][idx, 0]
        tn = np.column_stack([np.zeros(B), 0.5 + 0.5 * r.random((B, dd)), np.full(B, -3.0)])
        dr = np.stack([es_draws(nn, nfold, SS, r) for _ in range(B)])[:, None]
        f = lambda: gpscore.es_train_tall(Xn, yn, tn, nfold=nfold, num_sim=SS, lr=1e-9, itr=1,  # noqa: E731
                                          draws=dr, Xt=Xn[:, :64], yt=yn[:, :64], ctx=ctx)
        res = f()
        ms = [launches_ms(f) for _ in range(args.repeats)]
        row = {"shape": name, "n": nn, "d": dd, "num_sim": SS, "B": B,
               "fold_launches": -(-B * nfold // 256), "failed": int(np.count_nonzero(res.info))}
        for ph in PHASES:
            v = [m[ph] for m in ms]
            row[ph + "_ms"] = statistics.median(v)
            row[ph + "_ms_min"], row[ph + "_ms_max"] = min(v), max(v)
        row["longest_ms"] = max(row[ph + "_ms"] / (row["fold_launches"] if ph == "folds" else 1)
                                for ph in PHASES)
        longest.append(row)
        print(json.dumps(row), flush=True)

    by = {r["B"]: r for r in rows}
    res = {"shape": {"n": n, "d": d, "nt": 500, "itr": itr, "objective": "es", "lr": meth.lr,
                     "nfold": nfold, "num_sim": S}, "repeats": args.repeats,
           "loop_is_scaled_beyond": args.loop_cap, "rows": rows, "longest_launch": longest}
    if 1 in by and 256 in by:
        res["B256_over_B1"] = by[256]["tall_s"] / by[1]["tall_s"]
    if 30 in by:
        res["bar_B30_tall_max_below_loop_min"] = by[30]["tall_max"] < by[30]["loop_min"]
    print("| B | draw sets | host draws s | (a) loop s (min..max) | (b) tall s (min..max) | a / b |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        note = "" if r["looped"] == r["B"] else " (from %d problems, scaled)" % r["looped"]
        print("| %d | %d | %.2f | %.3f (%.3f..%.3f)%s | %.4f (%.4f..%.4f) | %.1f |"
              % (r["B"], r["draw_sets"], r["draws_host_s"], r["loop_s"], r["loop_min"],
                 r["loop_max"], note, r["tall_s"], r["tall_min"], r["tall_max"],
                 r["loop_s"] / r["tall_s"]))
    if 30 in by:
        print("bar (B = 30: (b) max < (a) min):", res["bar_B30_tall_max_below_loop_min"])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
