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

import factor_cases as fc
from test_dag_logic import NP_, NPF, U, task_list

E = fc.TILE  # the emulated tile edge: the device's
TS = (2, 3, 4, 5, 8, 9, 20, 21, 40, 64)
BS = (1, 2, 4, 8)
GS = (0, 1, 2)
ORDER_FLAG = {0: 3, 1: 1, 2: 2}


def raw_list(T, kb, kg, order=1, fine=1):
    from gpscore import _lib
    lib = _lib.load()
    flags = fine | (ORDER_FLAG[order] << 2)
    n = lib.gps_dag_task_list_ex(T, flags, kb, kg, None, 0)
    assert n > 0
    out = (ctypes.c_uint32 * n)()
    assert lib.gps_dag_task_list_ex(T, flags, kb, kg, ctypes.cast(out, ctypes.c_void_p), n) == n
    return np.frombuffer(out, dtype=np.uint32).copy()


def decode(words):
    """(type, part, i, j, k, fine, len) per word; k (UPD) resp. j (UPDX) the batch's first term."""
    w = words.astype(np.int64)
    cols = (w & 7, (w >> 3) & 15, (w >> 8) & 63, (w >> 16) & 63, (w >> 24) & 63, (w >> 7) & 1,
            1 + ((w >> 14) & 3) + 4 * ((w >> 22) & 1))
    return list(zip(*(c.tolist() for c in cols)))


def polled(t):
    """(counter array, i, j, threshold) the kernel polls for a strip (its switch)."""
    typ, _, i, j, k, _, ln = t
    if typ == 0:
        return [("a", i, i, U * i)]
    if typ == 1:
        return [("a", i, k, U * k), ("x", k, k, 1)]
    if typ == 2:
        kl = k + ln - 1
        return [("a", i, kl, U * (kl + 1)), ("a", j, kl, U * (kl + 1)), ("a", i, j, U * k)]
    if typ == 3:
        jl = j + ln - 1
        return [("a", i, jl, U * (jl + 1)), ("x", jl, k, 1 if jl == k else U * (jl - k + 1)),
                ("x", i, k, U * (j - k))]
    return [("x", i, k, U * (i - k)), ("x", i, i, 1)]


def inputs(t):
    """The counts that say every tile the strip READS is final (and its own tile's earlier terms
    are in): the legacy thresholds of every term of the batch."""
    typ, _, i, j, k, _, ln = t
    if typ == 2:
        need = [("a", i, j, U * k)]
        for q in range(k, k + ln):
            need += [("a", i, q, U * (q + 1)), ("a", j, q, U * (q + 1))]
        return need
    if typ == 3:
        need = [("x", i, k, U * (j - k))]
        for q in range(j, j + ln):
            need += [("a", i, q, U * (q + 1)), ("x", q, k, 1 if q == k else U * (q - k + 1))]
        return need
    return polled(t)


def arrival(t):
    """(counter array, i, j, increment)s a finished strip adds."""
    typ, _, i, j, k, fine, ln = t
    if typ == 0:
        return [("a", i, i, 1), ("x", i, i, 1)]
    if fine:
        return [("a", i, k if typ == 1 else j, U // NPF[typ])]
    if typ == 1:
        return [("a", i, k, U // NP_)]
    if typ == 2:
        return [("a", i, j, ln * (U // NP_))]
    return [("x", i, k, (ln if typ == 3 else 1) * (U // NP_))]


def final_counts(T):
    a, x = np.zeros((T, T), int), np.zeros((T, T), int)
    for i in range(T):
        a[i, i], x[i, i] = U * i + 1, 1
        for j in range(i):
            a[i, j], x[i, j] = U * (j + 1), U * (i - j + 1)
    return a, x


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
            n = lib.gps_dag_task_list(T, fine | (ORDER_FLAG[order] << 2), None, 0)
            old = (ctypes.c_uint32 * n)()
            lib.gps_dag_task_list(T, fine | (ORDER_FLAG[order] << 2), ctypes.cast(old, ctypes.c_void_p), n)
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
class Emu:
    """A (lower tiles, in place), X = L⁻¹ (stale NaNs until written), the leaves' L_kk."""

    def __init__(self, A, T):
        self.T, self.A = T, A.copy()
        self.X = np.full_like(A, np.nan)
        self.Ld = {}
        self.cnt = {"a": np.zeros((T, T), int), "x": np.zeros((T, T), int)}

    def met(self, needs):
        return all(self.cnt[a][i, j] >= v for a, i, j, v in needs)

    @staticmethod
    def blk(M, i, j, ni=1, nj=1):
        return M[i * E:(i + ni) * E, j * E:(j + nj) * E]

    def run(self, t):
        typ, part, i, j, k, fine, ln = t
        A, X, blk = self.A, self.X, self.blk
        s = E // NP_
        rows = slice(part * s, (part + 1) * s)
        if typ == 0:
            D = blk(A, i, i)
            L = np.linalg.cholesky(np.tril(D) + np.tril(D, -1).T)
            self.Ld[i] = L
            blk(X, i, i)[:] = np.tril(np.linalg.inv(L))
        elif fine and typ == 1:
            e = E // 8
            C = blk(A, i, k)
            C[part * e:(part + 1) * e] = C[part * e:(part + 1) * e] @ blk(X, k, k).T
        elif fine:
            e = E // 8
            rb, h = part >> 1, part & 1
            rws, cols = slice(rb * e, (rb + 1) * e), slice(h * E // 2, (h + 1) * E // 2)
            upd = blk(A, i, k)[rws] @ blk(A, j, k)[cols].T
            upd[:, (np.arange(h * E // 2, (h + 1) * E // 2) // e) > rb] = 0.0
            blk(A, i, j)[rws, cols] -= upd
        elif typ == 1:
            C = blk(A, i, k)
            C[rows] = C[rows] @ blk(X, k, k).T
        elif typ == 2:  # one product over the batch's K tiles
            upd = blk(A, i, k, 1, ln)[rows] @ blk(A, j, k, 1, ln).T
            if i == j:
                upd[:, (part + 1) * s:] = 0.0
            blk(A, i, j)[rows] -= upd
        elif typ == 3:
            prod = blk(A, i, j, 1, ln)[rows] @ blk(X, j, k, ln, 1)
            C = blk(X, i, k)
            C[rows] = prod if j == k else C[rows] + prod
        else:
            C = blk(X, i, k)
            C[:, rows] = -blk(X, i, i) @ C[:, rows]
        for a, p, q, v in arrival(t):
            self.cnt[a][p, q] += v

    def factors(self):
        L = np.tril(self.A, -1)
        for i, Lkk in self.Ld.items():
            self.blk(L, i, i)[:] = Lkk
        return L, np.tril(self.X)


def replay(tl, T, A, workers, latest):
    """`workers` emulated workgroups fetch the queue in order, each holding one task until its
    polled counts are met; among the ready ones the earliest (or the latest) fetched runs next."""
    em = Emu(A, T)
    head, held = 0, []
    while head < len(tl) or held:
        while len(held) < workers and head < len(tl):
            held.append((head, tl[head]))
            head += 1
        ready = [x for x in held if em.met(polled(x[1]))]
        assert ready, "no held task can run: the queue order does not guarantee progress"
        pick = max(ready) if latest else min(ready)
        assert em.met(inputs(pick[1])), pick   # the polled counts imply every input final
        em.run(pick[1])
        held.remove(pick)
    return em.factors()


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
