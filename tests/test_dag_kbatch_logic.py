"""The persistent factorisation's K-batched task lists on CPU (no GPU): gps_dag_task_list_ex
(GPS_OPT_DAG_KBATCH) against the single-term lists of test_dag_logic.py.

A batched UPD(i, j, k0..k1) / UPDX(i, k, j0..j1) strip is ONE product over the adjacent K tiles
of its terms; it polls the counts of its LAST term only.  Checked here:

* B = 1 is the legacy list word for word; every term is covered exactly once; the composition of
  the batches is the same for every queue order;
* the queue is topological, the final counter values are the legacy ones, and whenever the counts
  a task polls are met, the counts of EVERY term it reads are met (the implication the kernel
  relies on) — in queue order at every size, and under emulated workgroups that pick the latest
  ready task;
* a numpy replay with the device's 128-tiles meets factor_cases.check_factor, and every worker
  count and execution order gives the same bits.
"""
import ctypes

import numpy as np
import pytest

import dag_model as M
import factor_cases as fc
from dag_model import NP_, NPF, U, arrival, final_counts, inputs, polled, replay
from test_dag_logic import task_list

E = fc.TILE  # the emulated tile edge: the device's
TS = (2, 3, 4, 5, 8, 9, 20, 21, 40, 64)
BS = (1, 2, 4, 8)
GS = (0, 1, 2)


def raw_list(T, kb, kg, order=1, fine=1):
    """The words of gps_dag_task_list_ex itself."""
    from gpscore import _lib
    lib = _lib.load()
    n = lib.gps_dag_task_list_ex(T, M.flags(order, fine), kb, kg, None, 0)
    assert n > 0
    out = (ctypes.c_uint32 * n)()
    assert lib.gps_dag_task_list_ex(T, M.flags(order, fine), kb, kg, ctypes.cast(out, ctypes.c_void_p), n) == n
    return np.frombuffer(out, dtype=np.uint32).copy()


def decode(words):
    """(type, part, i, j, k, fine, len) per word; k (UPD) resp. j (UPDX) the batch's first term."""
    return [t[:7] for t in M.decode(words)]


@pytest.mark.parametrize("T", TS)
def test_lists(T):
    """Per size: B = 1 is the legacy list; and for every (B, g, order): exact cover, topological
    queue, polled counts imply final inputs, legacy final counters, one composition per (B, g)."""
    from gpscore import _lib
    lib = _lib.load()
    fa, fx = final_counts(T)
    for order in (0, 1, 2):
        legacy = task_list(T, 1, order)
        for fine in (0, 1):
            n = lib.gps_dag_task_list(T, M.flags(order, fine), None, 0)
            old = (ctypes.c_uint32 * n)()
            lib.gps_dag_task_list(T, M.flags(order, fine), ctypes.cast(old, ctypes.c_void_p), n)
            for g in GS:  # batching off: word for word, whatever g
                assert np.array_equal(raw_list(T, 1, g, order, fine), np.frombuffer(old, dtype=np.uint32))
        assert [t[:6] for t in decode(raw_list(T, 1, 0, order))] == legacy
    for kb in BS:
        for g in GS:
            if kb == 1 and g:
                continue   # (word for word the g = 0 list: asserted above)
            comp = None
            for order in (0, 1, 2):
                tl = decode(raw_list(T, kb, g, order))
                cnt = {"a": [[0] * T for _ in range(T)], "x": [[0] * T for _ in range(T)]}
                upd, updx = {}, {}
                at = 0
                while at < len(tl):
                    t = tl[at]
                    typ, part, i, j, k, fine, ln = t
                    # the strips of a task are adjacent in the queue and poll the same counts, and
                    # counts only grow: what holds for strip 0 holds for the others
                    parts = 1 if typ == 0 else NPF[typ] if fine else NP_
                    assert tl[at:at + parts] == [(typ, q, i, j, k, fine, ln) for q in range(parts)], t
                    at += parts
                    assert 1 <= ln <= kb and (ln == 1 or typ in (2, 3)) and not (fine and ln > 1), t
                    assert all(cnt[a][p][q] >= v for a, p, q, v in polled(t)), t   # topological
                    assert all(cnt[a][p][q] >= v for a, p, q, v in inputs(t)), t
                    for a, p, q, v in arrival(t):
                        cnt[a][p][q] += v * parts
                    if typ == 2:
                        for q in range(k, k + ln):
                            upd[(i, j, q)] = upd.get((i, j, q), 0) + U
                    elif typ == 3:
                        for q in range(j, j + ln):
                            updx[(i, k, q)] = updx.get((i, k, q), 0) + U
                assert np.array_equal(np.array(cnt["a"]), fa) and np.array_equal(np.array(cnt["x"]), fx)
                want_upd = {(i, j, k): U for j in range(T) for i in range(j, T) for k in range(j)}
                want_updx = {(i, k, j): U for i in range(T) for k in range(i) for j in range(k, i)}
                assert upd == want_upd and updx == want_updx    # every term once, all its strips
                # the chain's parts stay what they were
                chain = sorted(t for t in tl if t[5])
                assert chain == sorted(t + (1,) for t in task_list(T, 1, order) if t[5])
                if comp is None:
                    comp = sorted(tl)
                assert sorted(tl) == comp, (kb, g, order)          # composition: (T, B, g) only
            if kb > 1:
                # the batches are what the rule says: of a tile's nt terms the first nt − keep in
                # runs of kb from term 0, the rest single (keep = g, at least 1 on the fine chain tile)
                for t in comp:
                    typ, part, i, j, k, fine, ln = t
                    if typ not in (2, 3) or part or fine:
                        continue
                    nt, first, keep = (j, k, max(g, 1 if i == j else 0)) if typ == 2 else (i - k, j - k, g)
                    nbat = max(0, nt - keep)
                    want = min(kb, nbat - first) if first < nbat else 1
                    assert ln == want and (first >= nbat or first % kb == 0), t


def test_ex_rejections_and_sizes():
    from gpscore import _lib
    lib = _lib.load()
    for bad in ((1, 1, 1, 0), (65, 1, 1, 0), (8, 2, 1, 0), (8, 16, 1, 0), (8, 1, 0, 0), (8, 1, 9, 0),
                (8, 1, 2, -1), (8, 1, 2, 4)):
        assert lib.gps_dag_task_list_ex(*bad, None, 0) < 0, bad
    for T in (2, 20, 40):
        assert lib.gps_dag_task_list_ex(T, 1, 1, 0, None, 0) == lib.gps_dag_task_list(T, 1, None, 0)
    assert lib.gps_dag_task_list_ex(40, 1, 8, 1, None, 0) < lib.gps_dag_task_list(40, 1, None, 0) // 3


# ------------------------------------------------------------------ numpy replay, 128-tiles
@pytest.mark.parametrize("g", GS)
@pytest.mark.parametrize("kb", (2, 4, 8))
@pytest.mark.parametrize("T", (3, 5, 8))
def test_replay_meets_the_factor_bounds(T, kb, g):
    n = E * T - 37   # (a padded last tile, as the library pads it)
    A = fc.pad_identity(fc.fam_a(n))
    tl = decode(raw_list(T, kb, g))
    L, X = replay(tl, T, A, 1, False)
    failed, ratios = fc.check_factor(A, L, X, fc.rows_for(n, True, T), True, T)
    print(T, kb, g, ratios)
    assert not failed, ratios
    Lr = np.linalg.cholesky(A)
    assert np.allclose(L, Lr, rtol=1e-11, atol=1e-12)
    for workers, latest in ((3, False), (3, True), (64, False), (64, True)):
        L2, X2 = replay(tl, T, A, workers, latest)
        assert np.array_equal(L2, L) and np.array_equal(X2, X), (workers, latest)
    for order in (0, 2):   # another queue order: the same bits (the composition is the same)
        L2, X2 = replay(decode(raw_list(T, kb, g, order)), T, A, 64, True)
        assert np.array_equal(L2, L) and np.array_equal(X2, X), order
