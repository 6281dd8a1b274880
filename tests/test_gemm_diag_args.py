"""gps_gemm_diag refuses, before anything touches a device, every launch description that
could make a GEMM kernel read or write outside the arrays it was given (include/gpscore.h).
The validator is device-less (gps_gemm_diag_check), and gps_gemm_diag itself judges the
description before it binds the context, so both are reachable here without a GPU."""
import ctypes

import numpy as np
import pytest

from gpscore import _lib

STORE, ROWSQ, COLRED, ROWSQ_DOT = 0, 1, 2, 3


def desc(**kw):
    d = dict(lay_a=0, lay_b=1, epi=STORE, M=128, N=256, K=48, lda=48, ldb=48, ldc=256, alpha=1.0,
             beta=0.0, tri=0, tri_off=0, lower_out=0, mirror=0, kend=0, tile=0, ksplit=1,
             map_mode=0, use_ws=1, sk_alone=0, dep_mode=0, ld_out=0, c_kslice_stride=0)
    d.update(kw)
    return _lib.GemmDesc(**d)


def check(d, c=1, kscale=0, w=0, kr=None, out0=0, out1=0):
    lib = _lib.load()
    krp = None if kr is None else np.ascontiguousarray(kr, np.int32)
    rc = lib.gps_gemm_diag_check(ctypes.byref(d), c, kscale, w,
                                 None if krp is None else krp.ctypes.data_as(_lib._PI), out0, out1)
    return rc, lib.gps_last_error(None).decode()


KR_OK = np.tile([0, 48], 256 // 16)

ACCEPTED = [
    (desc(), {}),
    (desc(lay_a=1, lay_b=0, lda=128, ldb=256), {}),
    (desc(lda=50, ldb=64, ldc=258), {}),
    (desc(tile=16, ksplit=2), {}),
    (desc(tile=32, ksplit=4), {}),
    (desc(tile=64, ksplit=3), {}),
    (desc(tile=128, ksplit=3), {}),
    (desc(tile=128, ksplit=2, use_ws=0, c_kslice_stride=128 * 256), {}),
    (desc(tri=1, tri_off=128, K=256, lda=256, ldb=256, map_mode=3), {}),
    (desc(tri=5), dict(kr=KR_OK)),
    (desc(N=128, ldc=128, lower_out=1, mirror=1), {}),
    (desc(kend=32), {}),
    (desc(epi=ROWSQ, ld_out=128), dict(c=0, out0=1)),
    (desc(epi=ROWSQ_DOT, tri=2, tri_off=128, K=384, lda=384, ldb=384, ld_out=128),
     dict(c=0, w=1, out0=1, out1=1)),
    (desc(epi=COLRED, ld_out=256), dict(c=0, w=1, out0=1, out1=1)),
    (desc(kend=16), dict(kscale=1)),
]

REFUSED = [
    ("M not a multiple of 128", desc(M=120), {}),
    ("N not a multiple of 128", desc(N=192), {}),
    ("M zero", desc(M=0), {}),
    ("K not a multiple of 16", desc(K=40, lda=40, ldb=40), {}),
    ("K zero", desc(K=0), {}),
    ("odd lda", desc(lda=49), {}),
    ("odd ldb", desc(ldb=49), {}),
    ("odd ldc", desc(ldc=257), {}),
    ("lda below K", desc(lda=46), {}),
    ("lda below M for the transposed layout", desc(lay_a=1, lda=126), {}),
    ("ldb below K", desc(ldb=32), {}),
    ("ldb below N for the k-major layout", desc(lay_b=0, ldb=128), {}),
    ("ldc below N", desc(ldc=128), {}),
    ("layout out of range", desc(lay_a=2), {}),
    ("epilogue out of range", desc(epi=4), {}),
    ("tri out of range", desc(tri=6), {}),
    ("negative tri_off", desc(tri=1, tri_off=-128), {}),
    ("tri_off not a multiple of 16", desc(tri=1, tri_off=8), {}),
    ("tri_off without a tri mode", desc(tri_off=128), {}),
    ("TRI_KR_J without kr", desc(tri=5), {}),
    ("kr entry above K", desc(tri=5), dict(kr=np.tile([0, 64], 16))),
    ("kr entry negative", desc(tri=5), dict(kr=np.tile([-16, 48], 16))),
    ("kr entry not a multiple of 16", desc(tri=5), dict(kr=np.tile([8, 48], 16))),
    ("kend not a multiple of 16", desc(kend=24), {}),
    ("kend negative", desc(kend=-16), {}),
    ("dep_mode 1", desc(dep_mode=1, epi=ROWSQ, tri=2, ld_out=128), dict(c=0, out0=1)),
    ("dep_mode 2", desc(dep_mode=2, epi=ROWSQ, tri=2, ld_out=128), dict(c=0, out0=1)),
    ("C missing", desc(), dict(c=0)),
    ("ROWSQ without out0", desc(epi=ROWSQ, ld_out=128), dict(c=0)),
    ("ROWSQ ld_out below M", desc(epi=ROWSQ, ld_out=64), dict(c=0, out0=1)),
    ("ROWSQ_DOT without w", desc(epi=ROWSQ_DOT, tri=2, tri_off=128, K=384, lda=384, ldb=384,
                                 ld_out=128), dict(c=0, out0=1, out1=1)),
    ("ROWSQ_DOT without out1", desc(epi=ROWSQ_DOT, tri=2, tri_off=128, K=384, lda=384, ldb=384,
                                    ld_out=128), dict(c=0, w=1, out0=1)),
    ("ROWSQ_DOT whose last tile does not span K (launch_gemm)",
     desc(epi=ROWSQ_DOT, tri=2, tri_off=0, K=384, lda=384, ldb=384, ld_out=128),
     dict(c=0, w=1, out0=1, out1=1)),
    ("ROWSQ_DOT without TRI_K_LE_J (launch_gemm)",
     desc(epi=ROWSQ_DOT, K=256, lda=256, ldb=256, ld_out=128), dict(c=0, w=1, out0=1, out1=1)),
    ("COLRED without w", desc(epi=COLRED, ld_out=256), dict(c=0, out0=1, out1=1)),
    ("COLRED without out1", desc(epi=COLRED, ld_out=256), dict(c=0, w=1, out0=1)),
    ("COLRED ld_out below N", desc(epi=COLRED, ld_out=128), dict(c=0, w=1, out0=1, out1=1)),
    ("epilogue in another layout", desc(epi=ROWSQ, lay_b=0, ldb=256, ld_out=128), dict(c=0, out0=1)),
    ("epilogue on 64-tiles (launch_gemm)", desc(epi=ROWSQ, tile=64, ld_out=128), dict(c=0, out0=1)),
    ("epilogue on the small kernel (launch_gemm)", desc(epi=COLRED, tile=16, ld_out=256),
     dict(c=0, w=1, out0=1, out1=1)),
    ("epilogue with a split (launch_gemm)", desc(epi=ROWSQ, ksplit=2, ld_out=128), dict(c=0, out0=1)),
    ("tile 48", desc(tile=48), {}),
    ("ksplit 0", desc(ksplit=0), {}),
    ("ksplit 9", desc(ksplit=9), {}),
    ("small kernel with 3 waves (launch_gemm)", desc(tile=16, ksplit=3), {}),
    ("small kernel with kscale (launch_gemm)", desc(tile=32), dict(kscale=1)),
    ("map_mode 7", desc(map_mode=7), {}),
    ("map 3 without a triangular operand (launch_gemm)", desc(map_mode=3), {}),
    ("map 3 with lower_out (launch_gemm)", desc(N=128, ldc=128, tri=4, lower_out=1, map_mode=3), {}),
    ("lower_out on a rectangle (launch_gemm)", desc(lower_out=1), {}),
    ("mirror without lower_out (launch_gemm)", desc(N=128, ldc=128, mirror=1), {}),
    ("unslabbed split with beta (launch_gemm)",
     desc(tile=128, ksplit=2, use_ws=0, beta=1.0, c_kslice_stride=128 * 256), {}),
    ("unslabbed split with mirror (launch_gemm)",
     desc(N=128, ldc=128, tile=128, ksplit=2, use_ws=0, lower_out=1, mirror=1,
          c_kslice_stride=128 * 128), {}),
    ("unslabbed split whose slices overlap", desc(tile=128, ksplit=2, use_ws=0,
                                                  c_kslice_stride=128 * 256 - 2), {}),
    ("unslabbed split with an odd stride", desc(tile=128, ksplit=2, use_ws=0,
                                                c_kslice_stride=128 * 256 + 1), {}),
    ("unslabbed split on 64-tiles", desc(tile=64, ksplit=2, use_ws=0,
                                         c_kslice_stride=128 * 256), {}),
    ("slabs beyond the workspace", desc(M=4096, N=4096, ldc=4096, tile=128, ksplit=3), {}),
]


@pytest.mark.parametrize("d,kw", ACCEPTED, ids=[str(i) for i in range(len(ACCEPTED))])
def test_runnable_descriptions_pass(d, kw):
    rc, msg = check(d, **kw)
    assert rc == 0, msg


@pytest.mark.parametrize("why,d,kw", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_before_any_launch(why, d, kw):
    rc, msg = check(d, **kw)
    assert rc == -1 and msg.startswith("gps_gemm_diag: "), (why, rc, msg)


def test_entry_point_judges_the_description_before_the_context():
    """gps_gemm_diag with no context: a refused description reports the validator's reason (it
    never reached bind()), a runnable one reports the missing context — and neither launches."""
    lib = _lib.load()
    a = np.zeros((256, 64))
    plan = np.zeros(8, np.int32)

    def call(d):
        rc = lib.gps_gemm_diag(None, ctypes.byref(d), _lib.ptr(a), _lib.ptr(a), _lib.ptr(a), None,
                               None, None, None, None, plan.ctypes.data_as(_lib._PI))
        return rc, lib.gps_last_error(None).decode()

    rc, msg = call(desc(K=40))
    assert rc == -1 and "multiples of 128" in msg, msg
    rc, msg = call(desc(dep_mode=1))
    assert rc == -1 and "dep_mode" in msg, msg
    rc, msg = call(desc())
    assert rc == -1 and msg == "NULL context", msg
    assert not plan.any()


def test_desc_layout_matches_the_header():
    """The ctypes structure has the C struct's size (api_diag.hip static_asserts the same 128)."""
    assert ctypes.sizeof(_lib.GemmDesc) == 128
