"""Time of the joint test predictive (GP.predict_cov / joint_score / sample) on one GPU against
(a) the only route to the covariance before it, gpscore.compat.cal_mean_and_cov on host arrays,
and (b) the diagonal-only GP.predict at the same shape.

    python tools/joint_predict_bench.py [--out profiles/joint_predict.json] [--reps 9]

Shapes: "scripts" n = 500, n* = 500 (the scripts' size, one block), "c2" n = 5000, n* = 1250,
"c3" n = 20 000, n* = 5000 (covariance only; the compat route is not run there).  Each shape runs
in a child process of its own under a time limit, and the first failure ends the run.  A number
is the median over --reps calls after two warm-up calls of (dev) the time between two hipEvents
on the context's stream around the call — everything the call enqueues, its device-to-host copy
of the result included — and (wall) the host clock around the same call, which ends in a stream
synchronise.  The compat route is timed by the host clock only (it synchronises per helper)."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scoring-rules-for-gaussian-process-regression-a-new-approach-to-inference_amd"))

SHAPES = {"scripts": (500, 500, 8, True, 120), "c2": (5000, 1250, 8, True, 240),
          "c3": (20000, 5000, 8, False, 420)}  # n, n*, d, compat too, time limit (s)


class Events:
    """Two hipEvents on the context's stream (libamdhip64 through ctypes)."""

    def __init__(self, stream):
        try:
            self.hip = ctypes.CDLL("libamdhip64.so")
        except OSError:  # not on the loader's path: where csrc/Makefile links it from
            self.hip = ctypes.CDLL("/opt/rocm/lib/libamdhip64.so")
        self.stream = ctypes.c_void_p(stream)
        self.e = [ctypes.c_void_p(), ctypes.c_void_p()]
        for e in self.e:
            self._ok(self.hip.hipEventCreate(ctypes.byref(e)))

    @staticmethod
    def _ok(rc):
        if rc != 0:
            raise RuntimeError(f"HIP call failed ({rc})")

    def time(self, fn):
        self._ok(self.hip.hipEventRecord(self.e[0], self.stream))
        t0 = time.perf_counter()
        fn()
        wall = time.perf_counter() - t0
        self._ok(self.hip.hipEventRecord(self.e[1], self.stream))
        self._ok(self.hip.hipEventSynchronize(self.e[1]))
        ms = ctypes.c_float()
        self._ok(self.hip.hipEventElapsedTime(ctypes.byref(ms), self.e[0], self.e[1]))
        return float(ms.value), 1e3 * wall


def run_shape(name, reps):
    import numpy as np

    import gpscore
    from gpscore import compat
    n, nt, d, with_compat, _ = SHAPES[name]
    rng = np.random.default_rng(n)
    X, Xt = rng.standard_normal((n, d)), rng.standard_normal((nt, d))
    w = rng.standard_normal(d) / np.sqrt(d)
    y = np.sin(3 * X @ w) + 0.1 * rng.standard_normal(n)
    yt = np.sin(3 * Xt @ w) + 0.1 * rng.standard_normal(nt)
    th = (0.0, np.log(2.0) * np.ones(d), np.log(0.01))
    gp = gpscore.GP(device=0)
    gp.fit(X, y, th, return_loo=False)
    gp.set_test(Xt, yt)
    ev = Events(gp.ctx.lib.gps_ctx_stream(gp.ctx.h))

    def med(fn):
        fn()
        fn()
        ts = np.array([ev.time(fn) for _ in range(reps)])
        return {"dev_ms": float(np.median(ts[:, 0])), "wall_ms": float(np.median(ts[:, 1])),
                "dev_min_ms": float(ts[:, 0].min()), "dev_max_ms": float(ts[:, 0].max())}

    out = {"shape": name, "n": n, "nt": nt, "d": d, "reps": reps,
           "predict_diag": med(lambda: gp.predict()),
           "predict_cov": med(lambda: gp.predict_cov()),
           "joint_dss": med(lambda: gp.joint_score("dss"))}
    if name != "c3":
        xi = rng.standard_normal((16, nt))
        draws = gpscore.gp.es_draws(nt, 1, 300, 1)
        out["sample_16"] = med(lambda: gp.sample(16, xi=xi))
        out["joint_es_300"] = med(lambda: gp.joint_score("es", num_sim=300, draws=draws))
    out["cov_over_diag_dev"] = out["predict_cov"]["dev_ms"] / out["predict_diag"]["dev_ms"]
    if with_compat:
        compat.state.para_k, compat.state.para_l = th[0], th[1]
        compat.state.sigma_noise_sq = np.exp(th[2])
        K, Ksf = compat.ARD(X, X, th[0], th[1]), compat.ARD(Xt, X, th[0], th[1])
        Kss = compat.ARD(Xt, Xt, th[0], th[1])
        ycol = y.reshape(-1, 1)

        def route():
            return compat.cal_mean_and_cov(Ksf, K, Kss, nt, n, ycol)

        route()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            _, cc = route()
            ts.append(1e3 * (time.perf_counter() - t0))
        out["compat_cal_mean_and_cov"] = {"wall_ms": float(np.median(ts)),
                                          "note": "the three Gram matrices are built outside "
                                                  "the timed call"}
        _, cov = gp.predict_cov()
        out["cov_vs_compat_nrel"] = float(np.max(np.abs(cov - cc)) / np.max(np.abs(cc)))
        out["compat_over_cov_wall"] = (out["compat_cal_mean_and_cov"]["wall_ms"]
                                       / out["predict_cov"]["wall_ms"])
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "joint_predict.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--shape", choices=sorted(SHAPES))
    ap.add_argument("--shapes", default="scripts,c2,c3")
    a = ap.parse_args()
    if a.shape:
        run_shape(a.shape, a.reps)
        return 0
    res = []
    for name in a.shapes.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", name, "--reps",
                                str(a.reps)], capture_output=True, text=True,
                               timeout=SHAPES[name][4])
        except subprocess.TimeoutExpired:
            print(f"{name}: time limit of {SHAPES[name][4]} s reached; stopping", file=sys.stderr)
            return 1
        if r.returncode != 0:
            print(f"{name}: exit {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
            return 1
        res.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(res[-1]), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/joint_predict_bench.py", "shapes": res}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
