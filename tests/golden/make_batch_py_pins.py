"""Generate tests/golden/batch_py_pins.json: what gpscore.batch's fourteen wrappers and
gpscore.experiment's five run_*_batch runners do on the host, recorded so that a fold of that
Python layer cannot move it unseen.  No device and no library call is made: the
wrappers run against a recording context, the runners against a stub training call.

  refusals   bad calls → the exception class, its FULL message (the other host tests only match
             fragments) and the number of library calls made (0).  Every check of a wrapper is
             broken alone and together with the next one in the documented order (problems, Z, θ,
             objective or the ES triple, nfold, itr / lr, lr_z, draw_sets, test rows, draws), which
             pins the order: the earlier check's message must win.
  calls      well-formed calls at B = 3, n = 10, d = 2, m = 3, nfold = 3, num_sim = 4, itr = 2 →
             the entry name and every slot: scalars as they are, an input pointer as the name of
             the array it points to, an output pointer as "out"; and for every array of the return
             value the slot it came from (the context writes each slot's number through its
             pointer), its shape and dtype.
  runners    the five runners' refusals; then per runner the training calls it makes (arguments by
             parameter name; arrays — the stacked data, θ0, Z0, the draws, hence the order in which
             the generator is consumed — as SHA-256) and what it returns or raises when the call
             reports failed replicates.

Usage:  python tests/golden/make_batch_py_pins.py   (rewrites the file)
The file must come out byte for byte the same before and after any change to that layer;
tests/test_batch_py_pins_host.py replays collect() against it.
"""
import ctypes
import hashlib
import inspect
import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from test_full_tall_host import _RecordingCtx, _ok, _sheets  # noqa: E402

OUT = os.path.join(HERE, "batch_py_pins.json")

# wrapper: (fitc, objective rule, trains, limit on n)
WRAPPERS = {
    "value_and_grad_batch": (False, "point", False, 128),
    "train_batch": (False, "point", True, 128),
    "value_and_grad_tall": (False, "point", False, 512),
    "train_tall": (False, "point", True, 512),
    "blockloo_value_and_grad_tall": (False, "block", False, 512),
    "blockloo_train_tall": (False, "block", True, 512),
    "es_value_and_grad_tall": (False, "es", False, 512),
    "es_train_tall": (False, "es", True, 512),
    "fitc_value_and_grad_batch": (True, "point", False, 128),
    "fitc_train_batch": (True, "point", True, 128),
    "fitc_value_and_grad_tall": (True, "point", False, 2048),
    "fitc_train_tall": (True, "point", True, 2048),
    "fitc_blockloo_value_and_grad_tall": (True, "block", False, 2048),
    "fitc_blockloo_train_tall": (True, "block", True, 2048),
}


def _good(name):
    """Keyword arguments of a well-formed call of wrapper `name`."""
    fitc, rule, train, _ = WRAPPERS[name]
    X, y = _ok()  # B = 3, n = 10, d = 2
    kw = {"X": X, "y": y, "theta0" if train else "theta": (0.0, 0.0, -1.0)}
    if fitc:
        kw["Z0" if train else "Z"] = np.random.default_rng(1).standard_normal((3, 3, 2))
    if rule != "es":
        kw["objective"] = "kc" if rule == "block" else "loo_crps"
    if rule != "point":
        kw["nfold"] = 3
    if rule == "es":
        kw.update(num_sim=4, beta=1.5, rng=0)
    if train:
        kw.update(lr=0.5, itr=2)
        if fitc:
            kw["lr_z"] = 0.25
    return kw


def _set(**over):
    return lambda name, kw: {**kw, **over}


def _bad_n(name, kw):
    N = WRAPPERS[name][3] + 1
    return {**kw, "X": np.zeros((2, N, 1)), "y": np.zeros((2, N))}


def _bad_z(m=None, B=None, d=None):
    def f(name, kw):
        b, _, dd = kw["X"].shape
        key = "Z0" if WRAPPERS[name][2] else "Z"
        return {**kw, key: np.zeros((b if B is None else B, 3 if m is None else m,
                                     dd if d is None else d))}
    return f


def _bad_theta(value):
    return lambda name, kw: {**kw, ("theta0" if WRAPPERS[name][2] else "theta"): value}


# The checks in their documented order: (stage, applies(fitc, rule, train), [(label, mutation)]);
# the first mutation of a stage is the one paired with the next stage's first.
STAGES = [
    ("problems", lambda f, r, t: True, [
        ("n over the limit", _bad_n),
        ("n = 0", _set(X=np.zeros((2, 0, 1)), y=np.zeros((2, 0)))),
        ("d = 17", _set(X=np.zeros((3, 5, 17)), y=np.zeros((3, 5)))),
        ("empty batch", _set(X=np.zeros((0, 5, 2)), y=np.zeros((0, 5)))),
        ("y disagrees", _set(y=np.zeros((3, 9)))),
        ("X of four axes", _set(X=np.zeros((3, 10, 2, 1)))),
    ]),
    ("Z", lambda f, r, t: f, [
        ("m = 33", _bad_z(m=33)), ("m = 0", _bad_z(m=0)), ("Z of another batch", _bad_z(B=2)),
        ("Z of another d", _bad_z(d=3)),
    ]),
    ("theta", lambda f, r, t: True, [
        ("log_ell of 3", _bad_theta((0.0, np.zeros(3), -1.0))),
        ("theta a row short", _bad_theta(np.zeros((2, 4)))),
        ("theta of width 6", _bad_theta(np.zeros((3, 6)))),
    ]),
    ("objective", lambda f, r, t: r != "es", [
        ("objective logdet", _set(objective="logdet")), ("objective es", _set(objective="es")),
        ("objective dss", _set(objective="dss")), ("objective nlml", _set(objective="nlml")),
        ("objective 0", _set(objective=0)),
    ]),
    ("es nfold", lambda f, r, t: r == "es", [
        ("nfold = 1", _set(nfold=1)), ("nfold = 11", _set(nfold=11)),
        ("folds of 129 rows", _set(X=np.zeros((1, 258, 1)), y=np.zeros((1, 258)), nfold=2)),
    ]),
    ("es num_sim", lambda f, r, t: r == "es", [
        ("num_sim = 1", _set(num_sim=1)), ("num_sim = 513", _set(num_sim=513)),
        ("num_sim = 7.5", _set(num_sim=7.5)), ("num_sim = True", _set(num_sim=True)),
    ]),
    ("es beta", lambda f, r, t: r == "es", [
        ("beta = 2.5", _set(beta=2.5)), ("beta = 0", _set(beta=0.0)),
        ("beta = nan", _set(beta=float("nan"))),
    ]),
    ("nfold", lambda f, r, t: r == "block", [
        ("nfold = 1", _set(nfold=1)), ("nfold = 11", _set(nfold=11)),
        ("nfold = 2.5", _set(nfold=2.5)), ("nfold = True", _set(nfold=True)),
        ("nfold = 33 of n = 40", _set(X=np.zeros((3, 40, 2)), y=np.zeros((3, 40)), nfold=33)),
    ]),
    ("itr", lambda f, r, t: t, [("itr = -1", _set(itr=-1)), ("itr = 2.5", _set(itr=2.5))]),
    ("lr", lambda f, r, t: t, [("lr = nan", _set(lr=float("nan"))),
                               ("lr = inf", _set(lr=float("inf")))]),
    ("lr_z", lambda f, r, t: t and f, [("lr_z = inf", _set(lr_z=float("inf"))),
                                       ("lr_z = nan", _set(lr_z=float("nan")))]),
    ("draw_sets", lambda f, r, t: t and r == "es", [
        ("draw_sets = 3", _set(draw_sets=3)), ("draw_sets = 0", _set(draw_sets=0)),
        ("draw_sets = 1.5", _set(draw_sets=1.5)), ("draw_sets = True", _set(draw_sets=True)),
    ]),
    ("tests", lambda f, r, t: t, [
        ("Xt of another d", _set(Xt=np.zeros((3, 4, 5)))),
        ("Xt without rows", _set(Xt=np.zeros((3, 0, 2)))),
        ("yt of another nt", _set(Xt=np.zeros((3, 4, 2)), yt=np.zeros((3, 5)))),
        ("yt without Xt", _set(yt=np.zeros((3, 5)))),
    ]),
    ("draws", lambda f, r, t: r == "es", [
        ("draws of 21 values", _set(draws=np.zeros((3, 7)))),
    ]),
]


def _refused(f, ctx):
    """The exception a call raises: class, full message, library calls made."""
    try:
        f()
    except Exception as e:  # noqa: BLE001: whatever it is, it is the record
        return {"type": type(e).__name__, "message": str(e), "calls": len(ctx.calls)}
    return {"type": None, "message": None, "calls": len(ctx.calls)}


def wrapper_refusals():
    import gpscore
    out = []
    for name, (fitc, rule, train, _) in WRAPPERS.items():
        fn = getattr(gpscore, name)
        stages = [(s, muts) for s, on, muts in STAGES if on(fitc, rule, train)]
        for q, (stage, muts) in enumerate(stages):
            for label, mut in muts:
                ctx = _RecordingCtx()
                kw = mut(name, _good(name))
                out.append({"call": name, "case": label,
                            **_refused(lambda: fn(ctx=ctx, **kw), ctx)})
            if q + 1 < len(stages):  # this check and the next one both broken: this one reports
                (la, ma), (lb, mb) = muts[0], stages[q + 1][1][0]
                ctx = _RecordingCtx()
                kw = mb(name, ma(name, _good(name)))
                out.append({"call": name, "case": la + " and " + lb,
                            **_refused(lambda: fn(ctx=ctx, **kw), ctx)})
    return out


class _SlotCtx(_RecordingCtx):
    """Records every slot of a call and fills the array behind every output pointer with slot +
    offset / 1024, so that the arrays of the wrapper's return value name the slot they were handed
    to and the place they were cut from.  np.empty is replaced for the length of the call, so that
    the output arrays are known by address and nothing in the record is left uninitialised."""

    def __init__(self, inputs):
        super().__init__()
        self.inputs = inputs  # name → the first value of that input array
        self.slots = []
        self.made = []

    def __enter__(self):
        self._empty = np.empty

        def empty(shape, dtype=np.float64):
            self.made.append(np.zeros(shape, dtype))
            return self.made[-1]

        np.empty = empty
        return self

    def __exit__(self, *exc):
        np.empty = self._empty

    def call(self, name, *args):
        from gpscore._lib import _P, _PI
        super().call(name, *args)
        rec = []
        for q, a in enumerate(args):
            if a is None:
                rec.append("NULL")
            elif isinstance(a, _P):
                who = [k for k, v in self.inputs.items() if a[0] == v]
                rec.append(who[0] if who else "out")
                for arr in self.made:
                    if arr.ctypes.data == ctypes.addressof(a.contents):
                        arr.ravel()[:] = q + np.arange(arr.size) / 1024.0
            elif isinstance(a, _PI):
                rec.append("out int32")
                a[0] = q
            else:
                rec.append(a if isinstance(a, (int, float)) and not isinstance(a, bool)
                           else repr(a))
        self.slots.append(rec)


def _describe(v):
    """A returned value: arrays as (slot written into their first entry, shape, dtype)."""
    if v is None:
        return None
    if isinstance(v, dict):
        return {k: _describe(x) for k, x in v.items()}
    if isinstance(v, (tuple, list)):
        return [_describe(x) for x in v]
    if isinstance(v, np.ndarray):
        return {"slot": float(v.ravel()[0]) if v.size else None, "shape": list(v.shape),
                "dtype": str(v.dtype)}
    if hasattr(v, "__dataclass_fields__"):
        return {"class": type(v).__name__,
                "fields": {k: _describe(getattr(v, k)) for k in v.__dataclass_fields__}}
    return repr(v)


def wrapper_calls():
    import gpscore
    out = []
    rng = np.random.default_rng(2)
    Xt, yt = rng.standard_normal((3, 4, 2)), rng.standard_normal((3, 4))
    for name, (fitc, rule, train, _) in WRAPPERS.items():
        fn = getattr(gpscore, name)
        plain = _good(name)
        rich = dict(plain)
        rich["theta0" if train else "theta"] = rng.standard_normal((3, 4))
        if not fitc:
            rich["rbf"] = True
        if rule == "es":
            sets = 1
            rich.pop("rng")
            rich["draws"] = rng.standard_normal((3, sets, 2 * 4 * 10))
        if train:
            rich.update(Xt=Xt, yt=yt, stale_noise=True, itr=3)
            if rule == "es":
                rich["draw_sets"] = sets
            if fitc:
                rich["lr_z"] = None
        for label, kw in (("plain", plain), ("every option", rich)):
            first = {k: float(np.ravel(v)[0]) for k, v in kw.items()
                     if isinstance(v, np.ndarray)}
            with _SlotCtx(first) as ctx:
                res = fn(ctx=ctx, **kw)
            out.append({"call": name, "case": label, "entries": ctx.calls, "slots": ctx.slots,
                        "returns": _describe(res)})
    # the defaults of every wrapper: only X, y, (Z,) θ given
    for name, (fitc, rule, train, _) in WRAPPERS.items():
        kw = {k: v for k, v in _good(name).items() if k in ("X", "y", "Z", "Z0", "theta", "theta0")}
        if rule == "es":
            kw.update(num_sim=2, rng=0)  # (300 draws a fold by default: kept small here)
        with _SlotCtx({}) as ctx:
            getattr(gpscore, name)(ctx=ctx, **kw)
        out.append({"call": name, "case": "defaults", "entries": ctx.calls,
                    "scalars": [a for a in ctx.slots[0] if not isinstance(a, str)]})
    return out


def es_default_draws():
    """draws=None: es_draws from rng once per (problem, set), problems outermost — the SHA-256 of
    what reaches the call."""
    import gpscore
    out = []
    for name, kw, slot, count in (("es_value_and_grad_tall", {}, 11, 3 * 1),
                                  ("es_train_tall", {"itr": 2}, 17, 3 * 2)):
        got = {}

        class Ctx(_RecordingCtx):
            def call(self, entry, *args):
                super().call(entry, *args)
                got["draws"] = np.ctypeslib.as_array(args[slot], (count * 2 * 4 * 10,)).copy()

        X, y = _ok()
        getattr(gpscore, name)(X, y, (0.0, 0.0, -1.0), nfold=3, num_sim=4,
                               rng=np.random.default_rng(5), ctx=Ctx(), **kw)
        out.append({"call": name, "sha256": _sha(got["draws"])})
    return out


def _sha(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


# runner: (the training call it makes, FITC, its methods table, the names it takes by default are
# recorded from the call itself)
RUNNERS = {
    "run_fitc_batch": ("fitc_train_tall", True, "K20_METHODS"),
    "run_full_batch": ("train_tall", False, "KF_METHODS"),
    "run_full_blockloo_batch": ("blockloo_train_tall", False, "KF_METHODS"),
    "run_full_es_batch": ("es_train_tall", False, "KF_METHODS"),
    "run_fitc_blockloo_batch": ("fitc_blockloo_train_tall", True, "K20_METHODS"),
}


def runner_refusals():
    from gpscore import experiment as E
    sheets = _sheets()
    out = []
    for name, (_, fitc, table) in RUNNERS.items():
        fn = getattr(E, name)
        methods = dict(getattr(E, table))
        methods.setdefault("es", E.KF_METHODS["es"])
        methods.setdefault("kc", E.K20_METHODS["kc"])
        cases = [("method " + k, {"methods": {k: m}}) for k, m in methods.items()]
        cases += [("method " + k + " after crps", {"methods": {"crps": methods["crps"], k: m}})
                  for k, m in methods.items() if k in ("dss", "es")]
        cases += [("TT = %r" % (bad,), {"TT": bad}) for bad in (0, -1, 2.5)]
        cases += [("method es and TT = 0", {"methods": {"es": methods["es"], "nlml": methods["nlml"]},
                                            "TT": 0})]
        if fitc:
            cases += [("m = %r" % (bad,), {"m": bad}) for bad in (0, 2.5)]
            cases += [("TT = 0 and m = 0", {"TT": 0, "m": 0}), ("m = 33", {"m": 33})]
        cases += [("itr = -1", {"itr": -1})]
        if "nfold" in inspect.signature(fn).parameters:
            cases += [("nfold = 1", {"nfold": 1}), ("itr = -1 and nfold = 1", {"itr": -1, "nfold": 1})]
        if "num_sim" in inspect.signature(fn).parameters:
            cases += [("num_sim = 1", {"num_sim": 1})]
        for label, kw in cases:
            ctx = _RecordingCtx()
            kw = {"TT": 2, **kw}
            if "num_sim" in inspect.signature(fn).parameters:
                kw.setdefault("num_sim", 4)
            rec = _refused(lambda: fn(sheets, ctx=ctx, seed=3, **kw), ctx)
            if rec["type"] is not None:  # (an accepted method is no refusal)
                out.append({"call": name, "case": label, **rec})
    return out


def _stub(real, log, info):
    """Stands in for a gpscore.batch training call: records its arguments by parameter name and
    returns a result whose scores count up from 1 and whose info is `info`."""
    from gpscore import batch as Bt
    sig = inspect.signature(real)

    def call(*a, **kw):
        b = sig.bind(*a, **kw)
        b.apply_defaults()
        rec = {}
        for k, v in b.arguments.items():
            if k == "ctx":
                continue
            rec[k] = {"sha256": _sha(v), "shape": list(v.shape)} if isinstance(v, np.ndarray) else v
        log.append(rec)
        B, nth = b.arguments["X"].shape[0], b.arguments["theta0"].shape[1]
        itr = b.arguments["itr"]
        sc = {k: (1.0 + q) + 0.125 * np.arange(B) for q, k in enumerate(Bt.SCORE_NAMES)}
        common = dict(theta=np.full((B, nth), 2.0), series={"objective": np.zeros((B, itr)),
                                                            "theta": np.zeros((B, itr, nth))},
                      objectives={}, mu=None, var=None, scores=sc,
                      info=np.asarray(info[:B], np.int32), steps_done=np.full(B, 7, np.int32))
        if "Z0" in b.arguments:
            return Bt.FitcBatchTrainResult(Z=np.full(b.arguments["Z0"].shape, 3.0), **common)
        return Bt.BatchTrainResult(**common)

    return call


def _returned(out):
    return {name: {k: {"dtype": str(np.asarray(v).dtype), "shape": list(np.shape(v)),
                       "values": np.asarray(v, np.float64).ravel().tolist()}
                   for k, v in o.items()} for name, o in out.items()}


def runner_calls():
    from gpscore import experiment as E
    sheets = _sheets()
    out = []
    for name, (target, fitc, table) in RUNNERS.items():
        fn = getattr(E, name)
        real = getattr(E, target)
        every = getattr(E, table)
        accepted = [k for k, m in every.items()
                    if _refused(lambda: fn(sheets, TT=0, methods={k: m}), _RecordingCtx())
                    ["message"].startswith("TT must")]
        cases = [("defaults, itr of the methods", {}, [0, 0]),
                 ("itr = 2", {"itr": 2}, [0, 0]),
                 ("one unseeded stream", {"itr": 2, "reseed": False, "stale_noise": False}, [0, 0])]
        cases += [("replicate 1 fails, method " + k, {"itr": 2, "methods": {k: every[k]}}, [0, 5])
                  for k in accepted]
        for label, kw, info in cases:
            kw = dict(kw)
            if fitc:
                kw["m"] = 3
            if "num_sim" in inspect.signature(fn).parameters:
                kw["num_sim"] = 4
            if "nfold" in inspect.signature(fn).parameters and "itr" in kw:
                kw["nfold"] = 3
            log = []
            setattr(E, target, _stub(real, log, info))
            plain_random = random.Random
            if kw.get("reseed") is False:  # the runner's own unseeded random.Random(), made repeatable
                random.Random = lambda *a: plain_random(17)
            try:
                try:
                    rec = {"returns": _returned(fn(sheets, TT=2, seed=11, **kw))}
                except E.NotPositiveDefinite as e:
                    rec = {"raises": {"type": type(e).__name__, "info": e.info, "message": str(e)}}
            finally:
                setattr(E, target, real)
                random.Random = plain_random
            out.append({"call": name, "case": label, "training_calls": log, **rec})
    return out


def collect():
    import gpscore
    from gpscore import batch as Bt, experiment as E
    return {
        "exports": {k: getattr(Bt, k) for k in ("BATCH_BLOCK_MAX_FOLDS", "BATCH_ES_MAX_FOLD",
                                                "BATCH_ES_MAX_SIM")},
        "batch_objectives": [list(E.BATCH_OBJECTIVES), list(Bt.BATCH_OBJS)],
        "signatures": {k: str(inspect.signature(getattr(gpscore, k))) for k in WRAPPERS}
        | {k: str(inspect.signature(getattr(E, k))) for k in RUNNERS},
        "wrapper_refusals": wrapper_refusals(),
        "wrapper_calls": wrapper_calls(),
        "es_default_draws": es_default_draws(),
        "runner_refusals": runner_refusals(),
        "runner_calls": runner_calls(),
    }


def dumps(pins):
    return json.dumps(pins, indent=1, sort_keys=True) + "\n"


if __name__ == "__main__":
    with open(OUT, "w") as f:
        f.write(dumps(collect()))
    print("wrote", OUT)
