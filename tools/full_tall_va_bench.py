#!/usr/bin/env python3
"""Times the validated tall full-GP fit (train_tall_validated) at the kin40k-FULL shape
— n = 500, d = 8, nv = 300 validation and nt = 500 test rows from experiment.synthetic_sheets, B =
30 replicates, KF's LOO-CRPS method (400 steps, lr = 1, KF's start) — three ways; the work timed is
a whole call (upload, fit, predictive, scores, download), a host clock around calls that end in a
device synchronise, medians with min..max of --calls calls after a warm-up:

  (a) train_tall with this commit's library and with the parent commit's (--parent-lib), each in
      child processes of its own that alternate (this, parent, parent, this, ...): the VA = false
      kernel is to be the text it was, so this commit's median is required to lie within the
      parent's own min..max spread ("a_within_parent_spread").  Without --parent-lib only this
      commit is timed and the requirement is recorded as null.
  (b) train_tall_validated with va_every in --every (1, 10, 50), interleaved with train_tall in one
      process, as a ratio to that process's train_tall median.  No threshold.
  (c) the only route to the same curve without it: after the fit, one train_tall(itr=0,
      theta0=thetas[:, i - 1], Xt=Xv, yt=yv) call per step.  --route-steps of those calls are timed
      and their median is scaled to the method's 400; route = fit + 400 such calls, reported as a
      ratio to (b) at va_every = 1, and the extra cost alone (the 400 calls against (b) − fit).

    python tools/full_tall_va_bench.py --parent-lib /path/to/parent/libgpscore.so \\
        --out profiles/full_tall_va_bench.json
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "scoring-rules-for-gaussian-process-regression-a-new-approach-to-inference_amd")
sys.path.insert(0, PKG)

B, D = 30, 8


def problems():
    """KF's replicates and crps starting points, run_method's draws."""
    from gpscore import experiment as E
    meth = E.KF_METHODS["crps"]
    sheets = E.synthetic_sheets(0)
    rng = np.random.default_rng(0)
    data = [E.replicate(sheets, j, n_pool=sheets["trainx"].shape[0]) for j in range(B)]
    st = lambda k: np.stack([dd[k] for dd in data])  # noqa: E731
    th0 = []
    for _ in range(B):
        k, ell, noise = E.initial_theta(meth, D, rng)
        th0.append(np.concatenate([[k], ell, [noise]]))
    return meth, st("train_x"), st("train_y"), st("va_x"), st("va_y"), st("test_x"), st("test_y"), \
        np.stack(th0)


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return time.perf_counter() - t0, r


def worker(args):
    """One process: --worker plain | va | route; prints one JSON line."""
    from gpscore import _lib
    if os.environ.get("GPSCORE_LIB"):  # a parent library lacks the new entries: leave them unbound
        probe = ctypes.CDLL(os.environ["GPSCORE_LIB"])
        for name in list(_lib.SIGNATURES):
            if not hasattr(probe, name):
                del _lib.SIGNATURES[name]
    import gpscore
    meth, X, y, Xv, yv, Xt, yt, th0 = problems()
    itr = meth.itr if args.itr is None else args.itr
    ctx = gpscore.Context(0)
    kw = dict(lr=meth.lr, itr=itr, Xt=Xt, yt=yt, stale_noise=True, ctx=ctx)
    plain = lambda: gpscore.train_tall(X, y, th0, meth.objective, **kw)  # noqa: E731
    out = {"mode": args.worker, "itr": itr}
    if args.worker == "plain":
        plain()
        ts = []
        for _ in range(args.calls):
            t, r = timed(plain)
            ts.append(t)
        out.update(times=ts, failed=int(np.count_nonzero(r.info)))
    elif args.worker == "va":
        every = [int(v) for v in args.every.split(",")]
        fs = {0: plain}
        for e in every:
            fs[e] = (lambda e: lambda: gpscore.train_tall_validated(
                X, y, th0, Xv, yv, meth.objective, va_every=e, **kw))(e)
        for f in fs.values():
            f()
        ts = {e: [] for e in fs}
        for _ in range(args.calls):
            for e, f in fs.items():
                t, r = timed(f)
                ts[e].append(t)
        out.update(times={str(e): v for e, v in ts.items()}, failed=int(np.count_nonzero(r.info)))
    else:  # route
        k = min(args.route_steps, itr)
        t_fit, fit = timed(lambda: gpscore.train_tall(X, y, th0, meth.objective,
                                                      **{**kw, "itr": k}))
        one = lambda i: gpscore.train_tall(X, y, fit.series["theta"][:, i], meth.objective, lr=meth.lr,  # noqa: E731
                                           itr=0, Xt=Xv, yt=yv, ctx=ctx)
        one(0)
        ts = []
        for i in range(k):
            t, r = timed(lambda: one(i))
            ts.append(t)
        out.update(times=ts, steps_timed=k, failed=int(np.count_nonzero(r.info)))
    print("RESULT " + json.dumps(out), flush=True)


def spawn(mode, args, lib=None):
    env = dict(os.environ)
    env.pop("GPSCORE_LIB", None)
    if lib:
        env["GPSCORE_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--calls", str(args.calls),
           "--every", args.every, "--route-steps", str(args.route_steps)]
    if args.itr is not None:
        cmd += ["--itr", str(args.itr)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.worker_timeout)
    if p.returncode != 0:  # nothing more is started on the device after a failed worker
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit("worker %s failed (%d)" % (mode, p.returncode))
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def stats(ts):
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "calls": len(ts)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--parent-lib", default=None, help="libgpscore.so built from the parent commit")
    ap.add_argument("--calls", type=int, default=5, help="timed calls a worker makes of each kind")
    ap.add_argument("--rounds", type=int, default=4,
                    help="(a): this / parent alternations, a fresh process a side each (a process's\n"
                         "calls agree to 0.1 %%, two processes of one library differ by up to 0.5 %%:\n"
                         "the spread has to see several)")
    ap.add_argument("--every", default="1,10,50")
    ap.add_argument("--route-steps", type=int, default=10)
    ap.add_argument("--itr", type=int, default=None, help="override the method's step count")
    ap.add_argument("--worker-timeout", type=int, default=400)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)

    this, parent, failed = [], [], 0
    for rnd in range(args.rounds):  # this, parent | parent, this | ...: neither always goes first
        for side in (("this", "parent") if rnd % 2 == 0 else ("parent", "this")):
            if side == "this":
                r = spawn("plain", args)
                this += r["times"]
                failed += r["failed"]
            elif args.parent_lib:
                parent += spawn("plain", args, os.path.abspath(args.parent_lib))["times"]
    itr = r["itr"]
    a = {"this": stats(this), "parent": stats(parent) if parent else None,
         "a_within_parent_spread": (min(parent) <= statistics.median(this) <= max(parent))
         if parent else None}
    print(json.dumps({"a": a}), flush=True)

    v = spawn("va", args)
    failed += v["failed"]
    base = statistics.median(v["times"]["0"])
    b = {"train_tall": stats(v["times"]["0"])}
    for e in args.every.split(","):
        b["va_every_%s" % e] = dict(stats(v["times"][e]),
                                    ratio_to_train_tall=statistics.median(v["times"][e]) / base)
    print(json.dumps({"b": b}), flush=True)

    rt = spawn("route", args)
    failed += rt["failed"]
    per = statistics.median(rt["times"])
    first = args.every.split(",")[0]
    va1 = b["va_every_%s" % first]["median_s"]
    c = {"calls_timed": rt["steps_timed"], "per_call": stats(rt["times"]), "scaled_to_steps": itr,
         "extra_s": per * itr, "route_s": base + per * itr,
         "route_over_validated": (base + per * itr) / va1,
         "extra_over_validated_extra": per * itr / (va1 - base) if va1 > base else None,
         "validated_is": "va_every_%s" % first}
    print(json.dumps({"c": c}), flush=True)

    res = {"shape": {"n": 500, "d": D, "nv": 300, "nt": 500, "B": B, "objective": "loo_crps",
                     "itr": itr, "lr": 1.0}, "calls": args.calls, "rounds": args.rounds,
           "failed": failed, "a": a, "b": b, "c": c}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
