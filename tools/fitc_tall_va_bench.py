#!/usr/bin/env python3
"""Times the validated tall FITC fit (fitc_train_tall_validated) at K20's shape — n =
500, d = 8, m = 20, nv = 300 validation and nt = 500 test rows from experiment.synthetic_sheets, B =
10 replicates, K20's LOO-CRPS method (2000 steps, its lr, lr_z and start) — three ways in ONE
process, tools/full_tall_va_bench.py's protocol: the work timed is a whole call (upload, fit,
predictive, scores, download) on a host clock around calls that end in a device synchronise,
median (min..max) of --calls calls after a warm-up, the routes interleaved:

  (a) fitc_train_tall;
  (b) fitc_train_tall_validated with va_every in --every (1, 10, 50), as a ratio to (a);
  (c) the only route to the same curve without it: the fit plus one fitc_train_tall(itr=0, Z0=…,
      theta0=…, Xt=Xv, yt=yv) call per step.  --route-steps of those calls are timed and their median
      is SCALED to the method's step count (the figure is an extrapolation, not a run of 2000
      calls; the plain fit does not even return the Z of each step, the timed calls use the
      validated fit's va_Z), reported as a ratio to (b) at va_every = 1.

One more row: the block-LOO DSS method (3000 steps) plain and validated at va_every = 1.
--probe adds the steps-per-launch measurement: one checkpoint's time at nv = 4096, m = 32, d = 16
from the profiling events around one-step launches (a validated call of one step scores 2·nv rows,
its checkpoint and the final row; the same call at nv = 4 is subtracted), and the longest validated
launch at K20's shape with nv = 300, va_every = 1 and at the corner n = 2048, m = 32, d = 16.

    python tools/fitc_tall_va_bench.py --probe --out profiles/fitc_tall_va_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "scoring-rules-for-gaussian-process-regression-a-new-approach-to-inference_amd")
sys.path.insert(0, PKG)

B, D, M = 10, 8, 20


def problems(name):
    """K20's replicates and the method's starting points, run_method's draws."""
    from gpscore import experiment as E
    meth = E.K20_METHODS[name]
    sheets = E.synthetic_sheets(0)
    rng = np.random.default_rng(0)
    data = [E.replicate(sheets, j, n_pool=sheets["trainx"].shape[0]) for j in range(B)]
    st = lambda k: np.stack([dd[k] for dd in data])  # noqa: E731
    th0, Z0 = [], []
    for _ in range(B):
        k, ell, noise = E.initial_theta(meth, D, rng)
        th0.append(np.concatenate([[k], np.ravel(ell), [noise]]))
        Z0.append(rng.random((M, D)) if meth.z_init == "rand" else rng.standard_normal((M, D)))
    return meth, st("train_x"), st("train_y"), st("va_x"), st("va_y"), st("test_x"), st("test_y"), \
        np.stack(th0), np.stack(Z0)


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return time.perf_counter() - t0, r


def stats(ts):
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "calls": len(ts)}


def interleaved(fs, calls):
    """{key: [seconds]} of `calls` rounds over the routes after one warm-up each, and the failures."""
    for f in fs.values():
        f()
    ts, failed = {k: [] for k in fs}, 0
    for _ in range(calls):
        for k, f in fs.items():
            t, r = timed(f)
            ts[k].append(t)
            failed = max(failed, int(np.count_nonzero(r.info)))
    return ts, failed


def tag_ms(ctx, tag, f, reps=5):
    """median device milliseconds under a profiling tag over reps calls, after a warm-up."""
    f()
    ms = []
    for _ in range(reps):
        ctx.prof(True)
        f()
        rep = ctx.prof_collect()
        ctx.prof(False)
        ms.append(rep[tag]["ms"])
    return statistics.median(ms)


def probe(ctx):
    import gpscore

    def data(nb, n, m, d, nv, seed=1):
        rng = np.random.default_rng(seed)
        X, Xv = rng.standard_normal((nb, n, d)), rng.standard_normal((nb, nv, d))
        y = np.sin(X.sum(2) / np.sqrt(d)) + 0.1 * rng.standard_normal((nb, n))
        yv = np.sin(Xv.sum(2) / np.sqrt(d)) + 0.1 * rng.standard_normal((nb, nv))
        Z = rng.uniform(-2, 2, (nb, m, d))
        th = np.tile(np.concatenate([[0.0], np.full(d, np.log(0.5 * np.sqrt(d))), [np.log(0.05)]]),
                     (nb, 1))
        return X, y, Z, th, Xv, yv

    out = {}
    # one checkpoint: a one-step launch scores its checkpoint and the final row
    for nb in (1, 256):
        ms = {}
        for nv in (4, 4096):
            X, y, Z, th, Xv, yv = data(nb, 500, 32, 16, nv)
            ms[nv] = tag_ms(ctx, "batch_fitc_tall_va_train", lambda: gpscore.fitc_train_tall_validated(
                X, y, Z, th, Xv, yv, "loo_crps", lr=1e-3, itr=1, ctx=ctx))
        out["row_B%d" % nb] = {"ms_nv4": ms[4], "ms_nv4096": ms[4096],
                               "ns_per_row": (ms[4096] - ms[4]) * 1e6 / (2 * (4096 - 4))}
    # the longest launches: the rule's steps in one launch, plus the final pass, every CU busy
    for key, n, m, d, steps, bsteps in (("k20", 500, 20, 8, 13, 8), ("corner", 2048, 32, 16, 4, 2)):
        X, y, Z, th, Xv, yv = data(256, n, m, d, 300)
        out["longest_" + key] = {
            "steps": steps, "block_steps": bsteps,
            "va_ms": tag_ms(ctx, "batch_fitc_tall_va_train", lambda: gpscore.fitc_train_tall_validated(
                X, y, Z, th, Xv, yv, "loo_crps", lr=1e-3, itr=steps, ctx=ctx), 3),
            "plain_ms": tag_ms(ctx, "batch_fitc_tall_train", lambda: gpscore.fitc_train_tall(
                X, y, Z, th, "loo_crps", lr=1e-3, itr=steps, ctx=ctx), 3),
            "block_va_ms": tag_ms(
                ctx, "batch_fitc_tall_block_va_train",
                lambda: gpscore.fitc_blockloo_train_tall_validated(
                    X, y, Z, th, Xv, yv, "dss", lr=1e-4, itr=bsteps, ctx=ctx), 3),
            "block_plain_ms": tag_ms(
                ctx, "batch_fitc_tall_block_train", lambda: gpscore.fitc_blockloo_train_tall(
                    X, y, Z, th, "dss", lr=1e-4, itr=bsteps, ctx=ctx), 3)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--calls", type=int, default=5, help="timed calls of each route")
    ap.add_argument("--every", default="1,10,50")
    ap.add_argument("--route-steps", type=int, default=10)
    ap.add_argument("--itr", type=int, default=None, help="override the methods' step counts")
    ap.add_argument("--probe", action="store_true", help="add the steps-per-launch measurement")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import gpscore
    ctx = gpscore.Context(0)
    res = {"shape": {"n": 500, "d": D, "m": M, "nv": 300, "nt": 500, "B": B}, "calls": args.calls}

    meth, X, y, Xv, yv, Xt, yt, th0, Z0 = problems("crps")
    itr = meth.itr if args.itr is None else args.itr
    kw = dict(lr=meth.lr, lr_z=meth.lr_z, itr=itr, Xt=Xt, yt=yt, stale_noise=True, ctx=ctx)
    every = [int(v) for v in args.every.split(",")]
    fs = {0: lambda: gpscore.fitc_train_tall(X, y, Z0, th0, meth.objective, **kw)}
    for e in every:
        fs[e] = (lambda e: lambda: gpscore.fitc_train_tall_validated(
            X, y, Z0, th0, Xv, yv, meth.objective, va_every=e, **kw))(e)
    ts, failed = interleaved(fs, args.calls)
    base = statistics.median(ts[0])
    b = {"fitc_train_tall": stats(ts[0])}
    for e in every:
        b["va_every_%d" % e] = dict(stats(ts[e]), ratio_to_plain=statistics.median(ts[e]) / base)
    res["crps"] = {"objective": meth.objective, "itr": itr, "lr": meth.lr, "lr_z": meth.lr_z,
                   "failed": failed, "b": b}
    print(json.dumps({"crps": res["crps"]}), flush=True)

    # (c): the itr = 0 route, --route-steps calls timed and scaled
    k = max(1, min(args.route_steps, itr))
    fit = gpscore.fitc_train_tall_validated(X, y, Z0, th0, Xv, yv, meth.objective, keep_z=True,
                                            **{**kw, "itr": k})
    one = lambda i: gpscore.fitc_train_tall(  # noqa: E731
        X, y, fit.va_Z[:, i + 1], fit.series["theta"][:, i], meth.objective, itr=0, Xt=Xv, yt=yv,
        ctx=ctx)
    one(0)
    rts = [timed(lambda: one(i))[0] for i in range(k)]
    per, va1 = statistics.median(rts), b["va_every_%d" % every[0]]["median_s"]
    res["route"] = {"calls_timed": k, "per_call": stats(rts), "scaled_to_steps": itr,
                    "scaled": True, "extra_s": per * itr, "route_s": base + per * itr,
                    "route_over_validated": (base + per * itr) / va1,
                    "validated_is": "va_every_%d" % every[0]}
    print(json.dumps({"route": res["route"]}), flush=True)

    meth, X, y, Xv, yv, Xt, yt, th0, Z0 = problems("dss")
    itr = meth.itr if args.itr is None else args.itr
    kw = dict(nfold=4, lr=meth.lr, lr_z=meth.lr_z, itr=itr, Xt=Xt, yt=yt, stale_noise=True, ctx=ctx)
    ts, failed = interleaved(
        {0: lambda: gpscore.fitc_blockloo_train_tall(X, y, Z0, th0, "dss", **kw),
         1: lambda: gpscore.fitc_blockloo_train_tall_validated(X, y, Z0, th0, Xv, yv, "dss",
                                                               va_every=1, **kw)},
        max(2, args.calls // 2))
    res["dss"] = {"itr": itr, "lr": meth.lr, "failed": failed,
                  "fitc_blockloo_train_tall": stats(ts[0]),
                  "va_every_1": dict(stats(ts[1]), ratio_to_plain=statistics.median(ts[1])
                                     / statistics.median(ts[0]))}
    print(json.dumps({"dss": res["dss"]}), flush=True)

    if args.probe:
        res["probe"] = probe(ctx)
        print(json.dumps({"probe": res["probe"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
