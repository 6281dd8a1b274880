"""The persistent factorisation's task lists and counter protocol for the CPU tests (no GPU):
ONE Python model of dag::potrf_dag_kernel's queue.

What a task word means — its fields, the counts it polls, what it adds when done — is READ from
the library (gps_dag_task_protocol, i.e. csrc/dag_task.h, the text the generator and the kernel
use), never transcribed here.  What stays in Python is the independent statement of what must
hold: `inputs` (the legacy threshold of every term a task reads), `final_counts` (the closed-form
end state) and a numpy emulator of the products.

A task is the tuple (type, part, i, j, k, fine, len, tile); the helpers also take its first six or
seven fields (len 1, strip form).  Counts are (array "a" | "x", i, j, value).
"""
import numpy as np

import factor_cases as fc

NP_ = 4              # strips per tile task (dag::NP)
NPF = {1: 8, 2: 16}  # fine parts of the chain's TRSM / UPD (dag::NPF_TRSM, NPF_UPD)
U = 16               # arrivals per finished tile task (dag::U)
ORDER_FLAG = {0: 3, 1: 1, 2: 2}  # GPS_OPT_DAG_ORDER's value in bits 2-3 of the list calls' flags

_PROTO = {}  # task -> (polled, arrival), of every word decode() has seen
_SEEN = np.zeros(0, np.uint32)  # those words, sorted


def flags(order=1, fine=1):
    return fine | (ORDER_FLAG[order] << 2)


def tf_of(d, minlen):
    return minlen | d << 4


def task_list(T, order=1, fine=1, kb=1, kg=0, tf=0):
    """The queue's words (uint32) from gps_dag_task_list_tf."""
    from gpscore import _lib
    lib = _lib.load()
    n = lib.gps_dag_task_list_tf(T, flags(order, fine), kb, kg, tf, None, 0)
    assert n > 0
    out = np.zeros(n, np.uint32)
    assert lib.gps_dag_task_list_tf(T, flags(order, fine), kb, kg, tf, out.ctypes.data, n) == n
    return out


def decode(words):
    """The tasks of the words, in order."""
    global _SEEN
    from gpscore import _lib
    words = np.asarray(words, np.uint32)
    rows = _lib.dag_task_protocol(64, words)  # (fields and counts do not depend on T)
    tl = list(zip(*rows[:, (0, 1, 3, 4, 5, 2, 6, 7)].T.tolist()))
    new = np.flatnonzero(~np.isin(words, _SEEN))
    for at, r in zip(new.tolist(), rows[new].tolist()):
        _PROTO[tl[at]] = tuple([("ax"[r[q]], r[q + 1], r[q + 2], r[q + 3]) for q in qs if r[q] >= 0]
                               for qs in ((8, 12, 16), (20, 24)))
    _SEEN = np.union1d(_SEEN, words[new])
    return tl


def _task(t):
    return tuple(t) + (1, 0)[len(t) - 6:]


def polled(t):
    """The counts the kernel polls before it runs t (a word decode() returned)."""
    return _PROTO[_task(t)][0]


def arrival(t):
    """The counts t adds when it is done."""
    return _PROTO[_task(t)][1]


def inputs(t):
    """The counts that say every tile the task READS is final (and its own tile's earlier terms
    are in): the legacy thresholds of every term of the batch."""
    typ, _, i, j, k, _, ln, _ = _task(t)
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


def final_counts(T):
    a, x = np.zeros((T, T), int), np.zeros((T, T), int)
    for i in range(T):
        a[i, i], x[i, i] = U * i + 1, 1
        for j in range(i):
            a[i, j], x[i, j] = U * (j + 1), U * (i - j + 1)
    return a, x


class Emu:
    """A (lower tiles, in place: L_ik lands in A_ik), X = L⁻¹ (stale NaNs until written) and the
    leaves' L_kk, of T×T tiles of edge `edge` (the device's 128; the algebra is edge-independent),
    with the arrival counters."""

    def __init__(self, A, T, edge=fc.TILE):
        self.T, self.E, self.A = T, edge, A.copy()
        self.X = np.full_like(A, np.nan)
        self.Ld = {}
        self.cnt = {"a": np.zeros((T, T), int), "x": np.zeros((T, T), int)}

    def met(self, needs):
        return all(self.cnt[a][i, j] >= v for a, i, j, v in needs)

    def ready(self, t):
        return self.met(polled(t))

    def blk(self, M, i, j, ni=1, nj=1):
        E = self.E
        return M[i * E:(i + ni) * E, j * E:(j + nj) * E]

    def run(self, t):
        typ, part, i, j, k, fine, ln, tile = _task(t)
        for q in (range(NP_) if tile else (part,)):  # a tile-form task: its four strips' products
            self.product(typ, q, i, j, k, fine, ln)
        for a, p, q, v in arrival(t):
            self.cnt[a][p, q] += v

    def product(self, typ, part, i, j, k, fine, ln):
        A, X, blk, E = self.A, self.X, self.blk, self.E
        s = E // NP_  # strip width (32 of 128 on the device)
        rows = slice(part * s, (part + 1) * s)
        if typ == 0:  # LEAF(k = i): the leaf reads A_kk's lower triangle
            D = blk(A, i, i)
            L = np.linalg.cholesky(np.tril(D) + np.tril(D, -1).T)
            self.Ld[i] = L
            blk(X, i, i)[:] = np.tril(np.linalg.inv(L))
        elif fine and typ == 1:  # the chain's TRSM(k+1, k) by 16-row strips (E / 8 here)
            assert i == k + 1
            e = E // 8
            C = blk(A, i, k)
            C[part * e:(part + 1) * e] = C[part * e:(part + 1) * e] @ blk(X, k, k).T
        elif fine:  # UPD(k+1, k+1, k) by (row block, column half), blocks right of the diagonal idle
            assert typ == 2 and i == j == k + 1
            e = E // 8
            rb, h = part >> 1, part & 1
            rws, cols = slice(rb * e, (rb + 1) * e), slice(h * E // 2, (h + 1) * E // 2)
            upd = blk(A, i, k)[rws] @ blk(A, j, k)[cols].T
            upd[:, (np.arange(h * E // 2, (h + 1) * E // 2) // e) > rb] = 0.0
            blk(A, i, j)[rws, cols] -= upd
        elif typ == 1:  # TRSM(i, k): row strip of L_ik = A_ik X_kkᵀ (in place)
            C = blk(A, i, k)
            C[rows] = C[rows] @ blk(X, k, k).T
        elif typ == 2:  # UPD(i, j, k ..): row strip of A_ij −= L_ik L_jkᵀ, one product over the batch
            upd = blk(A, i, k, 1, ln)[rows] @ blk(A, j, k, 1, ln).T
            if i == j:  # waves right of the strip's diagonal block stay idle
                upd[:, (part + 1) * s:] = 0.0
            blk(A, i, j)[rows] -= upd
        elif typ == 3:  # UPDX(i, k, j ..): row strip of S_ik (+)= L_ij X_jk (first term overwrites)
            prod = blk(A, i, j, 1, ln)[rows] @ blk(X, j, k, ln, 1)
            C = blk(X, i, k)
            C[rows] = prod if j == k else C[rows] + prod
        else:  # FIN(i, k): column strip of X_ik = −X_ii S_ik (in place)
            C = blk(X, i, k)
            C[:, rows] = -blk(X, i, i) @ C[:, rows]

    def factors(self):
        L = np.tril(self.A, -1)
        for i, Lkk in self.Ld.items():
            self.blk(L, i, i)[:] = Lkk
        return L, np.tril(self.X)


def replay(tl, T, A, workers, latest, edge=fc.TILE):
    """`workers` emulated workgroups fetch the queue in order, each holding one task until its
    polled counts are met; among the ready ones the earliest (or the latest) fetched runs next."""
    em = Emu(A, T, edge)
    head, held = 0, []
    while head < len(tl) or held:
        while len(held) < workers and head < len(tl):
            held.append((head, tl[head]))
            head += 1
        ready = [x for x in held if em.ready(x[1])]
        assert ready, "no held task can run: the queue order does not guarantee progress"
        pick = max(ready) if latest else min(ready)
        assert em.met(inputs(pick[1])), pick   # the polled counts imply every input final
        em.run(pick[1])
        held.remove(pick)
    fa, fx = final_counts(T)
    assert np.array_equal(em.cnt["a"], fa) and np.array_equal(em.cnt["x"], fx)
    return em.factors()
