"""GPS_OPT_GEMM_PIPE on the host: the option's number agrees between the header and
the binding, it is a member of the struct the graph-cache key copies whole, and launch_gemm clears
the request wherever the pipelined loop is not compiled or not taken — asked through
gps_gemm_pipe_resolved, which resolves a launch as gps_gemm_schedule does and needs no device.
(That the option is accepted by a context, and that it gives a graph of its own, needs a device:
tests/test_gpu_gemm_pipe.py.)"""
import ctypes
import os
import re

import pytest

from gpscore import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STORE, ROWSQ, COLRED, ROWSQ_DOT = 0, 1, 2, 3


def desc(**kw):
    d = dict(lay_a=0, lay_b=1, epi=STORE, M=256, N=256, K=272, alpha=1.0, beta=0.0, tri=0, tri_off=0,
             lower_out=0, mirror=0, kend=0, tile=128, ksplit=1, map_mode=0, use_ws=1, sk_alone=0,
             dep_mode=0, reserved=0, c_kslice_stride=0)
    d.update(kw)
    d.setdefault("lda", d["K"] if d["lay_a"] == 0 else d["M"])
    d.setdefault("ldb", d["N"] if d["lay_b"] == 0 else d["K"])
    d.setdefault("ldc", d["N"] if d["epi"] == STORE else 0)
    d.setdefault("ld_out", {STORE: 0, COLRED: d["N"]}.get(d["epi"], d["M"]))
    return _lib.GemmDesc(**d)


def resolved(pipe, have_kscale=0, **kw):
    lib = _lib.load()
    r = lib.gps_gemm_pipe_resolved(ctypes.byref(desc(**kw)), None, have_kscale, pipe)
    assert r >= 0, (kw, lib.gps_last_error(None))
    return r


def test_option_number_in_header_and_binding():
    text = open(os.path.join(ROOT, "include", "gpscore.h")).read()
    m = re.search(r"GPS_OPT_GEMM_PIPE\s*=\s*(\d+)", text)
    assert m and int(m.group(1)) == 32 == _lib.GPS_OPT_GEMM_PIPE
    assert re.search(r"#define\s+GPS_ABI_VERSION\s+900\b", text)  # additive: the ABI number stays


def test_option_is_a_member_of_the_keyed_struct():
    """factor_key copies FactorOpts whole: a member of it is in the graph-cache key."""
    text = open(os.path.join(ROOT, "scoring-rules-for-gaussian-process-regression-a-new-approach-"
                             "to-inference_amd", "csrc", "api_internal.h")).read()
    body = text[text.index("struct FactorOpts {"):]
    body = body[:body.index("};")]
    assert re.search(r"\bint\s+gemm_pipe\s*=\s*1\s*;", body), body


KEPT = {
    "nt_store": dict(),
    "nn_store": dict(lay_b=0),
    "tn_store": dict(lay_a=1, lay_b=0),
    "tt_store": dict(lay_a=1, lay_b=1),
    "nt_lower_out": dict(lower_out=1, alpha=-1.0, beta=1.0),
    "nn_tri1": dict(lay_b=0, tri=1, tri_off=128),
    "nt_colred": dict(epi=COLRED, tri=1, tri_off=128),
    "nt_ksplit2": dict(ksplit=2),
    "nt_live_hints": dict(reserved=3 | 5 << 8),
    "auto_plan_128": dict(tile=0, M=4096, N=4096, K=4096),
}
CLEARED = {
    "tile_64": dict(tile=64),
    "small_16": dict(tile=16, ksplit=4),
    "small_32": dict(tile=32, ksplit=4),
    "auto_plan_small": dict(tile=0),
    "auto_plan_64": dict(tile=0, M=2048, N=2048, K=2048),
    "row_norms": dict(epi=ROWSQ, tri=2),
    "row_norms_dot": dict(epi=ROWSQ_DOT, tri=2, K=256),
}


@pytest.mark.parametrize("name", sorted(KEPT))
def test_request_kept_where_the_loop_is_compiled(name):
    assert resolved(1, **KEPT[name]) == 1
    assert resolved(0, **KEPT[name]) == 0


@pytest.mark.parametrize("name", sorted(CLEARED))
def test_request_cleared_where_it_is_not(name):
    assert resolved(1, **CLEARED[name]) == 0
    assert resolved(0, **CLEARED[name]) == 0


def test_request_cleared_for_a_k_scaled_launch():
    assert resolved(1, have_kscale=0) == 1
    assert resolved(1, have_kscale=1) == 0
