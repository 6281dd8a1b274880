"""The live-extent hints of the diagnostic GEMM launch, on the CPU.
gps_gemm_desc.reserved carries them as dead_m16 | dead_n16 << 8, the trailing dead 16-blocks of
M and N: gps_gemm_diag_check accepts 0 and in-range values and refuses the others with a message,
and gps_gemm_schedule returns the same work items with and without them — the hints change what a
tile's waves multiply, never which tiles and K ranges the workgroups run."""
import ctypes

import numpy as np
import pytest

from gpscore import _lib

STORE, COLRED = 0, 2


def desc(**kw):
    d = dict(lay_a=0, lay_b=1, epi=STORE, M=256, N=384, K=272, lda=272, ldb=272, ldc=384, alpha=1.0,
             beta=0.0, tri=0, tri_off=0, lower_out=0, mirror=0, kend=0, tile=0, ksplit=1,
             map_mode=0, use_ws=1, sk_alone=0, dep_mode=0, reserved=0, ld_out=0, c_kslice_stride=0)
    d.update(kw)
    return _lib.GemmDesc(**d)


def check(d, c=1, w=0, out0=0, out1=0):
    lib = _lib.load()
    rc = lib.gps_gemm_diag_check(ctypes.byref(d), c, 0, w, None, out0, out1)
    return rc, lib.gps_last_error(None).decode()


def hint(dm, dn):
    return dm | dn << 8


# M = 256 has 16 sixteen-blocks, N = 384 has 24
@pytest.mark.parametrize("reserved", [0, hint(1, 0), hint(0, 1), hint(7, 5), hint(16, 24),
                                      hint(15, 23), hint(4, 4)])
@pytest.mark.parametrize("tile", [0, 16, 64, 128])
def test_in_range_hints_accepted(reserved, tile):
    rc, why = check(desc(reserved=reserved, tile=tile))
    assert rc == 0, (reserved, tile, why)


def test_in_range_hints_accepted_colred():
    rc, why = check(desc(epi=COLRED, ld_out=384, reserved=hint(6, 7)), c=0, w=1, out0=1, out1=1)
    assert rc == 0, why


@pytest.mark.parametrize("what, reserved", [
    ("more dead row blocks than M/16", hint(17, 0)),
    ("more dead column blocks than N/16", hint(0, 25)),
    ("both beyond", hint(127, 127)),
    ("row field's eighth bit", 128),
    ("column field's eighth bit", 128 << 8),
    ("bits above the two fields", 1 << 16),
    ("high bits with valid fields", hint(1, 1) | 1 << 20),
    ("negative", -1),
    ("sign bit alone", -(1 << 31)),
])
def test_out_of_range_hints_refused(what, reserved):
    rc, why = check(desc(reserved=reserved))
    assert rc == -1, what
    assert "reserved" in why, (what, why)


_buf = np.zeros((1 << 14, 8), np.int32)
_plan = np.zeros(8, np.int32)


def schedule(d, slots=512):
    lib = _lib.load()
    n = lib.gps_gemm_schedule(ctypes.byref(d), None, 0, slots, _plan.ctypes.data_as(_lib._PI),
                              _buf.ctypes.data_as(_lib._PI), len(_buf))
    assert 0 < n <= len(_buf), (n, lib.gps_last_error(None))
    return _plan.copy(), _buf[:n].copy()


SCHEDULE_CASES = {
    "plain": dict(M=640, N=384, K=272, lda=272, ldb=272, ldc=384),
    "triangular": dict(M=640, N=384, K=1024, lda=1024, ldb=1024, ldc=384, tri=1, tri_off=256),
    "lower_out": dict(M=640, N=640, K=272, lda=272, ldb=272, ldc=640, lower_out=1),
}


@pytest.mark.parametrize("case", sorted(SCHEDULE_CASES))
@pytest.mark.parametrize("tile", [64, 128])
def test_schedule_identical_with_and_without_hints(case, tile):
    kw = dict(SCHEDULE_CASES[case], tile=tile)
    plan0, items0 = schedule(desc(**kw))
    for reserved in (hint(6, 0), hint(0, 7), hint(6, 7), hint(40, 24)):
        plan1, items1 = schedule(desc(reserved=reserved, **kw))
        assert np.array_equal(plan0, plan1), (case, tile, reserved)
        assert np.array_equal(items0, items1), (case, tile, reserved)
    assert plan0[0] == tile and len(items0) > 4


def test_schedule_refuses_out_of_range_hints():
    lib = _lib.load()
    d = desc(reserved=hint(17, 0))
    n = lib.gps_gemm_schedule(ctypes.byref(d), None, 0, 512, _plan.ctypes.data_as(_lib._PI),
                              _buf.ctypes.data_as(_lib._PI), len(_buf))
    assert n == -1 and "reserved" in lib.gps_last_error(None).decode()
