"""The persistent factorisation's task graph on CPU (no GPU): the queue libgpscore builds
(gps_dag_task_list) replayed by a numpy emulator of the kernel's strip tasks and arrival
counters (kernels_potrf.hip, dag::potrf_dag_kernel).

* Every task's dependency counts are met when the queue is executed in order (the queue is a
  topological order: a worker never waits on a task behind it, so the launch always drains).
* Executing the strips in RANDOM orders allowed only by the counter thresholds (what the
  device's workgroups may do under any timing) still gives L and L⁻¹ of the block: the
  thresholds encode every true data dependency.
Reference: torch.potrf KF:26 / KF:332, chol_solve(I, A) KF:242 — numpy.linalg here.
"""
import functools

import numpy as np
import pytest

import dag_model as M
from dag_model import NP_, NPF

B = 8    # emulated tile edge (the device uses 128; the algebra is edge-independent)
Emu = functools.partial(M.Emu, edge=B)


def task_list(T, fine=1, order=1):
    """Queue words of the legacy call gps_dag_task_list itself, decoded as
    (type, part, i, j, k, fine); order as GPS_OPT_DAG_ORDER."""
    import ctypes
    from gpscore import _lib
    lib = _lib.load()
    n = lib.gps_dag_task_list(T, M.flags(order, fine), None, 0)
    assert n > 0
    out = (ctypes.c_uint32 * n)()
    assert lib.gps_dag_task_list(T, M.flags(order, fine), ctypes.cast(out, ctypes.c_void_p), n) == n
    return [t[:6] for t in M.decode(np.frombuffer(out, dtype=np.uint32))]


def spd(T, seed):
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((T * B, T * B))
    return M @ M.T / (T * B) + np.eye(T * B)


def check(em, A):
    n = A.shape[0]
    Lr = np.linalg.cholesky(A)
    L = np.tril(em.A, -1) + np.zeros_like(A)
    for t in range(em.T):  # diagonal tiles hold the updated A_kk; L_kk is the leaf's
        blk = slice(t * B, (t + 1) * B)
        L[blk, blk] = np.linalg.cholesky(np.tril(em.A[blk, blk]) + np.tril(em.A[blk, blk], -1).T)
    X = np.where(np.tril(np.ones((n, n), bool)), em.X, 0.0)
    assert np.allclose(L, Lr, rtol=1e-12, atol=1e-12)
    assert np.allclose(X, np.linalg.inv(Lr), rtol=1e-11, atol=1e-11)


@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("fine", [0, 1])
@pytest.mark.parametrize("T", [2, 3, 5, 8, 13])
def test_queue_order_is_topological(T, fine, order):
    tl = task_list(T, fine, order)
    A = spd(T, T)
    em = Emu(A, T)
    for t in tl:
        assert em.ready(t), t  # every input was produced by a task ahead in the queue
        em.run(t)
    check(em, A)
    kinds = [t[0] for t in tl]
    assert kinds.count(0) == T and not set(kinds) - {0, 1, 2, 3, 4}
    nf = sum(t[5] for t in tl if t[0] == 1)
    assert nf == (NPF[1] * (T - 1) if fine else 0)
    chain = (T - 1) * (NP_ - NPF[1] if fine else 0)
    assert kinds.count(1) == NP_ * T * (T - 1) // 2 - chain
    assert kinds.count(4) == NP_ * T * (T - 1) // 2
    assert all(t[1] < (NPF[t[0]] if t[5] else {0: 1}.get(t[0], NP_)) for t in tl)
    # the fine parts are exactly the chain's TRSM(k+1,k) and UPD(k+1,k+1,k)
    assert all(t[2] == t[4] + 1 and (t[0] == 1 or t[3] == t[2]) for t in tl if t[5])


@pytest.mark.parametrize("fine", [0, 1])
@pytest.mark.parametrize("T,seed", [(4, 0), (6, 1), (9, 2)])
def test_counters_cover_every_dependency(T, seed, fine):
    """Random execution orders permitted by the thresholds alone (any worker timing)."""
    tl = task_list(T, fine)
    A = spd(T, 10 + seed)
    em = Emu(A, T)
    rng = np.random.default_rng(seed)
    pending = list(tl)
    while pending:
        ready = [q for q, t in enumerate(pending) if em.ready(t)]
        assert ready, "deadlock"
        em.run(pending.pop(int(rng.choice(ready))))
    check(em, A)


@pytest.mark.parametrize("fine", [0, 1])
@pytest.mark.parametrize("T,seed", [(2, 3), (5, 4), (9, 5)])
def test_row_signals_flag_final_rows(T, seed, fine):
    """The row signals a dependent row-norm launch reads (DagParams::sig, GPS_OPT_FITC_DEP): the
    kernel flags row tile i of L⁻¹ final at LEAF(0) (i = 0) or when the NP·i-th FIN(i, ·) strip
    completes.  Under random threshold-permitted orders, every row is flagged exactly once, and
    at that moment its tiles X_i0..X_ii already hold their final values (nothing writes them
    later), so a consumer that waits for the flag reads the finished row."""
    tl = task_list(T, fine)
    A = spd(T, 40 + seed)
    Xr = np.linalg.inv(np.linalg.cholesky(A))
    em = Emu(A, T)
    rng = np.random.default_rng(seed)
    rowcnt, flagged = np.zeros(T, int), []
    pending = list(tl)
    while pending:
        ready = [q for q, t in enumerate(pending) if em.ready(t)]
        t = pending.pop(int(rng.choice(ready)))
        em.run(t)
        typ, i = t[0], t[2]
        row = None
        if typ == 0 and i == 0:
            row = 0
        elif typ == 4:
            rowcnt[i] += 1
            row = i if rowcnt[i] == NP_ * i else None
        if row is not None:
            flagged.append(row)
            got = em.X[row * B:(row + 1) * B, :(row + 1) * B]
            want = Xr[row * B:(row + 1) * B, :(row + 1) * B]
            assert np.allclose(np.tril(got, row * B), want, rtol=1e-11, atol=1e-11), row
    assert sorted(flagged) == list(range(T))
    check(em, A)


@pytest.mark.parametrize("T", [5, 20])
def test_orders_queue_the_same_tasks(T):
    """The orders differ only in sequence: same strip multiset, and they do differ."""
    lists = [task_list(T, 1, o) for o in (0, 1, 2)]
    assert sorted(lists[0]) == sorted(lists[1]) == sorted(lists[2])
    assert lists[1] != lists[2] and lists[1] != lists[0]
    assert task_list(T, 1) == lists[1]  # the default


def test_queue_sizes():
    """Strip counts per block size (the device's ntasks) and the 64-tile limit."""
    from gpscore import _lib
    lib = _lib.load()
    for T in (2, 20, 40):
        upd = T * (T - 1) * (T + 1) // 6          # Σ_k (T−1−k)(T−k)/2
        updx = (T - 1) * T * (T + 1) // 6         # Σ_j (T−1−j)(j+1)
        n0 = T + NP_ * (T * (T - 1) + upd + updx)
        assert lib.gps_dag_task_list(T, 0, None, 0) == n0
        assert lib.gps_dag_task_list(T, 1, None, 0) == n0 + (T - 1) * (NPF[1] + NPF[2] - 2 * NP_)
        # bit 1 (round 4's split chain, removed in round 5) and unknown bits are refused
        assert lib.gps_dag_task_list(T, 2, None, 0) < 0 and lib.gps_dag_task_list(T, 16, None, 0) < 0
    assert lib.gps_dag_task_list(65, 1, None, 0) < 0 and lib.gps_dag_task_list(1, 1, None, 0) < 0


def test_dag_kernel_loop_is_uniform():
    """Structural guard on the persistent kernel's code (no GPU): the task loop must be ONE loop
    whose first barrier follows its header directly.  Two `tid == 0` regions around the loop latch
    once got jump-threaded into a second back edge taken by lane 0 alone (a nested loop between
    the header and the barrier in the .s); the other lanes then re-ran a stale task forever."""
    import os
    import shutil
    import subprocess
    import tempfile
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "scoring-rules-for-gaussian-process-regression-a-new-approach-to-inference_amd", "csrc")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "potrf.s")
        subprocess.run([hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(root, "include"),
                        "-I" + csrc, "-munsafe-fp-atomics", "-mllvm", "-amdgpu-mfma-vgpr-form=1",
                        "--cuda-device-only", "-S", os.path.join(csrc, "kernels_potrf.hip"), "-o", out],
                       check=True, capture_output=True)
        text = open(out).read()
    import re
    variants = re.findall(r"^(_ZN3gps3dag16potrf_dag_kernelI\w*9DagParamsE):", text, re.M)
    assert len(variants) >= 2, variants  # the production and the trace instantiations
    for variant in variants:
        start = text.index(variant + ":")
        body = text[start:text.index("s_endpgm", start)]
        assert body.count("This Loop Header: Depth=1") == 1, variant
        head = body.index("This Loop Header: Depth=1")
        first_barrier = body.index("s_barrier", head)
        assert "Loop Header" not in body[head + 30:first_barrier], variant
