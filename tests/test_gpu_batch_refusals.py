"""The C-ABI refusals of the eight batch entry points (gps_{full,fitc}_{grad,train}_{batch,tall}).

gpscore/batch.py refuses a bad argument before it calls the library, so no other test reaches the
entries' own argument checks.  Here each entry is called through Context.call with tiny valid
arrays (B = 2, n = 4, d = 2, m = 2) and ONE bad argument: the call must return -1 with exactly the
message below (Context.check turns that into GpsError("<entry> failed (-1): <message>")), and a
valid call on the same context must succeed right after, so a refusal leaves nothing half done.
No kernel runs in a refused call.

The messages are the library's as they stood before the four api_batch*.hip files became one.
The batch objectives share the GPS_OBJ_* numbering, and the block-LOO objectives number 0..2 in
an enum of their own (GPS_BLOCK_*), so no integer says "block-LOO" to these entries: the refused
objective codes are the first two beyond the trainable ones (3 = GPS_OBJ_LOGDET, 4 =
GPS_OBJ_QUAD)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, N, D, M, NT, ITR = 2, 4, 2, 2, 3, 2

#         entry                   FITC   train  limit on n
ENTRIES = {"gps_full_grad_batch": (False, False, 128),
           "gps_full_train_batch": (False, True, 128),
           "gps_fitc_grad_batch": (True, False, 128),
           "gps_fitc_train_batch": (True, True, 128),
           "gps_fitc_grad_tall": (True, False, 2048),
           "gps_fitc_train_tall": (True, True, 2048),
           "gps_full_grad_tall": (False, False, 512),
           "gps_full_train_tall": (False, True, 512)}

NULL_ARG = "NULL argument"
OBJECTIVE = "objective must be GPS_OBJ_NLML, GPS_OBJ_LOO_CRPS or GPS_OBJ_LOO_LOGS"
LIMIT = "LIMIT"  # stands for the entry's own limit on n, plus one

# (argument, bad value, message, which entries have the argument: "all", "full", "fitc", "grad",
#  "train" or "fitc_train")
CASES = [("X", None, NULL_ARG, "all"),
         ("theta", None, NULL_ARG, "all"),
         ("Z", None, NULL_ARG, "fitc"),
         ("grad", None, NULL_ARG, "grad"),
         ("theta_out", None, NULL_ARG, "train"),
         ("kind", 7, "kind must be GPS_ARD or GPS_RBF", "full"),
         ("objective", 3, OBJECTIVE, "all"),
         ("objective", 4, OBJECTIVE, "all"),
         ("nprob", 0, "batch: nprob must be in 1..2^20", "all"),
         ("n", LIMIT, "batch: n must be in 1..{limit}", "all"),
         ("m", 33, "batch: m must be in 1..32", "fitc"),
         ("d", 17, "batch: d must be in 1..16", "all"),
         ("n_ell", 3, "n_ell must be 1 or d", "all"),
         ("itr", -1, "batch: itr must be in 0..2^20", "train"),
         ("lr", float("inf"), "batch: lr must be finite", "train"),
         ("lr_z", float("nan"), "batch: lr_z must be finite", "fitc_train"),
         ("nt", -1, "batch: nt must be in 0..2^24", "train"),
         ("flags", 2, "unknown batch flag", "train")]


def applies(where, fitc, train):
    return {"all": True, "full": not fitc, "fitc": fitc, "grad": not train, "train": train,
            "fitc_train": fitc and train}[where]


PARAMS = [pytest.param(entry, arg, bad, msg, id=f"{entry}-{arg}={bad}")
          for entry, (fitc, train, _) in ENTRIES.items()
          for arg, bad, msg, where in CASES if applies(where, fitc, train)]


def arguments(fitc, train):
    """The entry's arguments by name, in the order of include/gpscore.h, all valid; the arrays are
    numpy arrays (turned into pointers by positional())."""
    rng = np.random.default_rng(7)
    X = rng.normal(size=(B, N, D))
    a = {}
    if not fitc:
        a["kind"] = 0
    a.update(objective=1, nprob=B, X=X, y=np.sin(X.sum(axis=2)), n=N, d=D)
    if fitc:
        a.update(Z=X[:, :M, :].copy(), m=M)
    a.update(theta=np.tile([0.0, 0.1, -0.1, -2.0], (B, 1)), n_ell=D)
    if train:
        a.update(itr=ITR, lr=0.01)
        if fitc:
            a["lr_z"] = 0.01
        Xt = rng.normal(size=(B, NT, D))
        a.update(Xt=Xt, yt=np.sin(Xt.sum(axis=2)), nt=NT, flags=0, theta_out=np.zeros((B, 2 + D)))
        if fitc:
            a["z_out"] = np.zeros((B, M, D))
        a.update(values=np.zeros((B, ITR)), thetas=np.zeros((B, ITR, 2 + D)), obj=np.zeros((B, 5)),
                 mu=np.zeros((B, NT)), var=np.zeros((B, NT)), sc=np.zeros((B, 6)),
                 info=np.full(B, -1, np.int32), steps_done=np.full(B, -1, np.int32))
    else:
        a.update(obj=np.zeros((B, 5)), grad=np.zeros((B, 2 + D)))
        if fitc:
            a["grad_z"] = np.zeros((B, M, D))
        a["info"] = np.full(B, -1, np.int32)
    return a


def positional(a):
    import ctypes
    from gpscore._lib import ptr
    out = []
    for v in a.values():
        if isinstance(v, np.ndarray):
            v = (v.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if v.dtype == np.int32
                 else ptr(np.ascontiguousarray(v)))
        out.append(v)
    return out


@pytest.mark.parametrize("entry,arg,bad,msg", PARAMS)
def test_refusal_and_recovery(gpu_ctx, entry, arg, bad, msg):
    from gpscore import GpsError
    fitc, train, limit = ENTRIES[entry]
    a = arguments(fitc, train)
    assert arg in a
    a[arg] = limit + 1 if bad is LIMIT else bad
    with pytest.raises(GpsError) as e:
        gpu_ctx.call(entry, *positional(a))
    assert str(e.value) == f"{entry} failed (-1): {msg.format(limit=limit)}"
    # the same context runs a valid call straight away
    ok = arguments(fitc, train)
    gpu_ctx.call(entry, *positional(ok))
    assert (ok["info"] == 0).all()
    assert np.isfinite(ok["obj"]).all() and (ok["obj"] != 0).any()
    if train:
        assert (ok["steps_done"] == ITR).all()
        assert np.isfinite(ok["theta_out"]).all() and np.isfinite(ok["sc"]).all()
    else:
        assert np.isfinite(ok["grad"]).all() and (ok["grad"] != 0).any()
