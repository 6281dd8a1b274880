"""The persistent factorisation's task lists with tile-form batches on CPU (no GPU):
gps_dag_task_list_tf (GPS_OPT_DAG_TILE_FORM) against the strip lists of
test_dag_kbatch_logic.py.

A tile-form word (bit 23, part 0) stands for the four strips of one K batch of an off-diagonal
tile: it polls the three counts a strip of that batch polls and arrives once with len · U.
Checked here:

* form 0 is gps_dag_task_list_ex's list word for word;
* with the form on, for every T in 2..64, B in {2, 4, 8} and a few (d, minlen): every term of
  every tile is applied exactly once; the tile-form words are exactly the batches the rule names
  (off-diagonal tile, at least minlen terms, the batch ending at least d tile columns short of the
  tile's consumer) and every other word is the strip list's; the final counters are the strip
  lists'; and in queue order, whenever the counts a task polls are met, the legacy thresholds of
  every term it reads are met;
* a numpy replay at T <= 8 on 1, 3 and 64 emulated workgroups, earliest and latest pick, meets
  factor_cases.check_factor and gives the bits of the strip list of the same (B, g).  (The
  emulated tile-form task runs its four strips' products: per output element the device's chain
  is the strip's, which is what the GPU tests assert bitwise.)
"""
import numpy as np
import pytest

import dag_model as M
import factor_cases as fc
from dag_model import NP_, NPF, arrival, final_counts, inputs, polled, replay, tf_of
from test_dag_kbatch_logic import E, decode, raw_list

BS = (2, 4, 8)
FORMS = ((0, 2), (1, 2), (3, 4), (1, 8))   # (d, minlen)


def raw_list_tf(T, kb, kg, tf, order=1, fine=1):
    return M.task_list(T, order, fine, kb, kg, tf)


decode_tf = M.decode   # decode()'s tuples with the tile-form bit appended


def rule(t, d, minlen):
    """Does the batch t = (type, part, i, j, k, fine, len) take the tile form?"""
    typ, _, i, j, k, fine, ln = t
    if fine or typ not in (2, 3) or ln < minlen:
        return False
    return (i > j and j - (k + ln) >= d) if typ == 2 else i - (j + ln) >= d


def test_form_off_is_the_strip_list():
    for T in (2, 3, 5, 8, 21, 40, 64):
        for kb, kg in ((1, 0), (2, 0), (4, 1), (8, 0), (8, 2)):
            for order in (0, 1, 2):
                for fine in (0, 1):
                    assert np.array_equal(raw_list_tf(T, kb, kg, 0, order, fine), raw_list(T, kb, kg, order, fine))


def test_rejections():
    from gpscore import _lib
    lib = _lib.load()
    for bad in ((8, 1, 2, 0, -1), (8, 1, 2, 0, 256), (8, 1, 2, 0, 9), (8, 1, 2, 0, 16), (1, 1, 2, 0, 2),
                (8, 1, 9, 0, 2), (8, 2, 2, 0, 2)):
        assert lib.gps_dag_task_list_tf(*bad, None, 0) < 0, bad
    # one word instead of four per tile-form batch
    n0 = lib.gps_dag_task_list_ex(40, 1, 8, 0, None, 0)
    n1 = lib.gps_dag_task_list_tf(40, 1, 8, 0, tf_of(1, 2), None, 0)
    tl = decode_tf(raw_list_tf(40, 8, 0, tf_of(1, 2)))
    assert n0 - n1 == 3 * sum(t[7] for t in tl) > 0


@pytest.mark.parametrize("T", range(2, 65))
def test_lists(T):
    fa, fx = final_counts(T)
    for kb in BS:
        kg = 1 if kb == 4 else 0
        strips = decode(raw_list(T, kb, kg))
        batches = [t for t in strips if t[1] == 0]
        for d, minlen in FORMS:
            if minlen > kb:
                continue
            want_tiles = sorted(t for t in batches if rule(t, d, minlen))
            want_rest = sorted(t for t in strips if not rule(t, d, minlen))
            for order in ((0, 1, 2) if T in (5, 11, 40) else (1,)):
                tl = decode_tf(raw_list_tf(T, kb, kg, tf_of(d, minlen), order))
                assert sorted(t[:7] for t in tl if t[7]) == want_tiles, (kb, d, minlen, order)
                assert sorted(t[:7] for t in tl if not t[7]) == want_rest, (kb, d, minlen, order)
                cnt = {"a": [[0] * T for _ in range(T)], "x": [[0] * T for _ in range(T)]}
                upd, updx = {}, {}
                at = 0
                while at < len(tl):
                    t, tile = tl[at][:7], tl[at][7]
                    typ, part, i, j, k, fine, ln = t
                    if tile:
                        assert part == 0 and not fine and typ in (2, 3) and i > (j if typ == 2 else k), t
                        parts, arr = 1, arrival(tl[at])
                    else:
                        parts = 1 if typ == 0 else NPF[typ] if fine else NP_
                        assert [x[:7] for x in tl[at:at + parts]] == [(typ, q, i, j, k, fine, ln) for q in range(parts)], t
                        assert not any(x[7] for x in tl[at:at + parts])
                        arr = [(a, p, q, v * parts) for a, p, q, v in arrival(t)]
                    at += parts
                    assert all(cnt[a][p][q] >= v for a, p, q, v in polled(t + (tile,))), t   # topological
                    assert all(cnt[a][p][q] >= v for a, p, q, v in inputs(t)), t   # polled => every input
                    for a, p, q, v in arr:
                        cnt[a][p][q] += v
                    if typ == 2:
                        for q in range(k, k + ln):
                            upd[(i, j, q)] = upd.get((i, j, q), 0) + 1
                    elif typ == 3:
                        for q in range(j, j + ln):
                            updx[(i, k, q)] = updx.get((i, k, q), 0) + 1
                assert np.array_equal(np.array(cnt["a"]), fa) and np.array_equal(np.array(cnt["x"]), fx)
                assert upd == {(i, j, k): 1 for j in range(T) for i in range(j, T) for k in range(j)}
                assert updx == {(i, k, j): 1 for i in range(T) for k in range(i) for j in range(k, i)}


def test_the_gpu_cases_have_what_they_say():
    """T = 5, B = 2, d = 0, minlen = 2: the smallest block with a tile-form UPD and a tile-form UPDX
    batch without the clipped first term; T = 11, B = 8, d = 1: a full run of eight in tile form
    next to a single-term remainder in strips."""
    def kinds(T, kb, tf):
        tl = [t for t in decode_tf(raw_list_tf(T, kb, 0, tf)) if t[7]]
        return (any(t[0] == 2 for t in tl), any(t[0] == 3 and t[3] > t[4] for t in tl))
    assert kinds(5, 2, tf_of(0, 2)) == (True, True)
    assert all(kinds(T, 2, tf_of(0, 2)) != (True, True) for T in range(2, 5))
    tl = decode_tf(raw_list_tf(11, 8, 0, tf_of(1, 2)))
    assert (2, 0, 10, 9, 0, 0, 8, 1) in tl and (2, 0, 10, 9, 8, 0, 1, 0) in tl


# ------------------------------------------------------------------ numpy replay, 128-tiles
@pytest.mark.parametrize("d,minlen", ((0, 2), (1, 2), (0, 1)))
@pytest.mark.parametrize("kb", BS)
@pytest.mark.parametrize("T", (5, 8))
def test_replay_meets_the_factor_bounds_and_the_strip_bits(T, kb, d, minlen):
    n = E * T - 37
    A = fc.pad_identity(fc.fam_a(n))
    strips = [t + (0,) for t in decode(raw_list(T, kb, 0))]
    L0, X0 = replay(strips, T, A, 1, False)
    tl = decode_tf(raw_list_tf(T, kb, 0, tf_of(d, minlen)))
    assert any(t[7] for t in tl) or d > 0   # (T = 5 has no batch a column short of its consumer at B = 4)
    L, X = replay(tl, T, A, 1, False)
    failed, ratios = fc.check_factor(A, L, X, fc.rows_for(n, True, T), True, T)
    print(T, kb, d, minlen, ratios)
    assert not failed, ratios
    assert np.array_equal(L, L0) and np.array_equal(X, X0)
    for workers, latest in ((1, True), (3, False), (3, True), (64, False), (64, True)):
        L2, X2 = replay(tl, T, A, workers, latest)
        assert np.array_equal(L2, L0) and np.array_equal(X2, X0), (workers, latest)
