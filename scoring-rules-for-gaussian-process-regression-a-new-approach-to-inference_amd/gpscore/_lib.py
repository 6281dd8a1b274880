"""ctypes binding of libgpscore.so (C-ABI declared in include/gpscore.h).

This is the reference-side binding a maintainer adds under the reference
scripts: plain pointers and sizes, no torch types.  There is no
CPU fallback anywhere in this package: if the library is missing or no HIP
device is present, loading / context creation raises.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GPSCORE_LIB", os.path.join(_HERE, "libgpscore.so"))
ABI_VERSION = 900  # include/gpscore.h GPS_ABI_VERSION: the signatures below are this version's
GPS_N_STATS = 6
GPS_COMM_NONE, GPS_COMM_RCCL, GPS_COMM_LOCAL = 0, 1, 2
COMM_KINDS = {GPS_COMM_NONE: "none", GPS_COMM_RCCL: "rccl", GPS_COMM_LOCAL: "local"}

GPS_ARD, GPS_RBF = 0, 1
GPS_FULL, GPS_LOWER = 0, 1
GPS_OPT_OVERLAP, GPS_OPT_GEMM_MAP, GPS_OPT_TINY_GEMM, GPS_OPT_GRAM_REG = 0, 3, 7, 9
GPS_OPT_GRAPH = 10
GPS_OPT_PRED_PRE = 11
GPS_OPT_DAG = 12
GPS_OPT_DAG_TILES = 13
GPS_OPT_DAG_GROUP = 17
GPS_OPT_STREAM_K = 18
GPS_OPT_DAG_WGS = 19
GPS_OPT_DAG_ORDER = 25
GPS_OPT_SLAB_XCD = 26
GPS_OPT_FITC_DEP = 27
GPS_OPT_DAG_TILES_FULL = 28
GPS_OPT_DAG_KBATCH = 29
GPS_OPT_DAG_TILE_FORM = 30
GPS_OPT_GEMM_LIVE = 31  # 1 (default): edge tiles skip the MFMA blocks that lie in the padding
GPS_OPT_GEMM_PIPE = 32  # 1 (default): full 128-tiles run the pipelined GEMM loop
# the library's defaults of those two (api_internal.h): 40-tile blocks in the full GP's fit, and
# batches of 8 K tiles in the blocks above GPS_OPT_DAG_TILES (bit 8 of the batch option)
DAG_TILES_FULL_DEFAULT = 40
DAG_KBATCH_DEFAULT = 8 | 256
DAG_TILE_FORM_DEFAULT = 2 | 2 << 4  # minlen | d << 4; 0: strips only
GPS_OPT_AR_CHUNKS = 15
OBJ_NAMES = ("nlml", "loo_crps", "loo_logs", "logdet", "quad")
SURFACE_NAMES = ("loo_crps", "insample_crps", "nlml", "loo_logs")
GPS_SURF_LOGS_ADD_NOISE = 1
GPS_BATCH_STALE_NOISE = 1
BATCH_MAX_N, BATCH_MAX_D = 128, 16  # GPS_SURFACE_MAX_N, GPS_BATCH_MAX_D
BATCH_FITC_MAX_M = 32  # GPS_BATCH_FITC_MAX_M
BATCH_FITC_TALL_MAX_N = 2048  # GPS_BATCH_FITC_TALL_MAX_N
BATCH_FULL_TALL_MAX_N = 512  # GPS_BATCH_FULL_TALL_MAX_N
BATCH_BLOCK_MAX_FOLDS = 32  # GPS_BATCH_BLOCK_MAX_FOLDS
BATCH_ES_MAX_FOLD = 128  # GPS_BATCH_ES_MAX_FOLD: rows of the largest fold
BATCH_ES_MAX_SIM = 512  # GPS_BATCH_ES_MAX_SIM
SCORE_NAMES = ("test_crps", "test_logs", "test_msll", "test_smse", "test_mse", "test_cover")

_c_int, _c_i64, _c_dbl, _c_vp, _c_cp = (ctypes.c_int, ctypes.c_int64, ctypes.c_double,
                                        ctypes.c_void_p, ctypes.c_char_p)
_P = ctypes.POINTER(ctypes.c_double)

_PI = ctypes.POINTER(ctypes.c_int32)
_PI64 = ctypes.POINTER(ctypes.c_int64)
_PP = ctypes.POINTER(_P)  # an array of float64 pointers (the gradient diagnostics)


class GemmDesc(ctypes.Structure):
    """include/gpscore.h gps_gemm_desc: one internal GEMM launch (diagnostics, not API)."""
    _fields_ = [("lay_a", ctypes.c_int32), ("lay_b", ctypes.c_int32), ("epi", ctypes.c_int32),
                ("M", ctypes.c_int32), ("N", ctypes.c_int32), ("K", ctypes.c_int32),
                ("lda", _c_i64), ("ldb", _c_i64), ("ldc", _c_i64),
                ("alpha", _c_dbl), ("beta", _c_dbl),
                ("tri", ctypes.c_int32), ("tri_off", ctypes.c_int32),
                ("lower_out", ctypes.c_int32), ("mirror", ctypes.c_int32),
                ("kend", ctypes.c_int32),
                ("tile", ctypes.c_int32), ("ksplit", ctypes.c_int32), ("map_mode", ctypes.c_int32),
                ("use_ws", ctypes.c_int32), ("sk_alone", ctypes.c_int32),
                ("dep_mode", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("ld_out", _c_i64), ("c_kslice_stride", _c_i64)]


GEMM_PLAN_NAMES = ("tile", "ksplit", "map_mode", "sk_dp", "sk_wgs", "slab_xcd", "grid_x", "grid_y")
# gps_potrf_diag's plan (GPS_POTRF_PLAN_*; the last word is reserved)
POTRF_PLAN_NAMES = ("n_pad", "leaves", "dags", "dag_tmin", "dag_tmax", "gemms", "replayed",
                    "reserved")

# name -> (restype, argtypes); every symbol include/gpscore.h declares
SIGNATURES = {
    "gps_version": (_c_int, []),
    "gps_build_id": (_c_int, [_c_cp, _c_int]),
    "gps_ctx_create": (_c_int, [_c_int, ctypes.POINTER(_c_vp)]),
    "gps_ctx_destroy": (_c_int, [_c_vp]),
    "gps_last_error": (_c_cp, [_c_vp]),
    "gps_ctx_set_stream": (_c_int, [_c_vp, _c_vp]),
    "gps_ctx_stream": (_c_vp, [_c_vp]),
    "gps_ctx_synchronize": (_c_int, [_c_vp]),
    "gps_ctx_set_option": (_c_int, [_c_vp, _c_int, _c_int]),
    "gps_ctx_stats": (_c_int, [_c_vp, _c_vp, _c_int]),
    "gps_dag_task_list": (_c_int, [_c_int, _c_int, _c_vp, _c_int]),
    "gps_dag_task_list_ex": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_vp, _c_int]),
    "gps_dag_task_list_tf": (_c_int, [_c_int, _c_int, _c_int, _c_int, _c_int, _c_vp, _c_int]),
    "gps_dag_task_protocol": (_c_int, [_c_int, _c_vp, _c_int, _PI]),
    "gps_gemm_diag_check": (_c_int, [ctypes.POINTER(GemmDesc), _c_int, _c_int, _c_int, _PI, _c_int,
                                     _c_int]),
    "gps_gemm_schedule": (_c_i64, [ctypes.POINTER(GemmDesc), _PI, _c_int, _c_int, _PI, _PI, _c_i64]),
    "gps_gemm_pipe_resolved": (_c_int, [ctypes.POINTER(GemmDesc), _PI, _c_int, _c_int]),
    "gps_gemm_diag": (_c_int, [_c_vp, ctypes.POINTER(GemmDesc), _P, _P, _P, _P, _P, _PI, _P, _P,
                               _PI]),
    "gps_potrf_diag": (_c_int, [_c_vp, _c_i64, _P, _c_i64, _P, _P, _P, _PI, _PI]),
    "gps_grad_terms_diag": (_c_int, [_c_vp, _c_int, _c_int, _c_i64, _c_i64, _c_i64, _c_dbl, _PP,
                                     _PP]),
    "gps_grad_contract_diag": (_c_int, [_c_vp, _c_i64, _c_int, _P, _P, _c_dbl, _P, _P, _c_i64, _P,
                                        _P, _P, _P]),
    "gps_fitc_contract_diag": (_c_int, [_c_vp, _c_i64, _c_i64, _c_i64, _c_int, _P, _P, _P, _c_dbl,
                                        _c_int, _PP, _PI64, _P, _PP, _P, _PP, _PP, _P, _P]),
    "gps_vec_diag": (_c_int, [_c_vp, _c_int, _PI64, _P, _PP, _PP]),
    "gps_block_diag": (_c_int, [_c_vp, _c_int, _PI64, _P, _PP, _PP]),
    "gps_prof_enable": (_c_int, [_c_vp, _c_int]),
    "gps_prof_collect": (_c_int, [_c_vp, _c_cp, _c_i64]),
    "gps_phase_enable": (_c_int, [_c_vp, _c_int]),
    "gps_phase_collect": (_c_int, [_c_vp, _c_cp, _c_i64]),
    "gps_rccl_info": (_c_int, [ctypes.POINTER(_c_int), _c_cp, _c_int]),
    "gps_gram": (_c_int, [_c_vp, _c_int, _P, _c_i64, _P, _c_i64, _c_int, _c_dbl, _P, _c_int,
                          _c_dbl, _c_int, _P]),
    "gps_potrf": (_c_int, [_c_vp, _c_i64, _P, _c_i64, _P]),
    "gps_potrs": (_c_int, [_c_vp, _c_i64, _c_i64, _P, _c_i64, _P, _c_i64, _P, _c_i64]),
    "gps_diag_inv": (_c_int, [_c_vp, _c_i64, _P, _c_i64, _P]),
    "gps_gemm": (_c_int, [_c_vp, _c_int, _c_int, _c_i64, _c_i64, _c_i64, _c_dbl, _P, _c_i64, _P,
                          _c_i64, _c_dbl, _P, _c_i64]),
    "gps_scores": (_c_int, [_c_vp, _P, _P, _P, _c_i64, _c_dbl, _c_dbl, _P]),
    "gps_full_set_data": (_c_int, [_c_vp, _P, _P, _c_i64, _c_int]),
    "gps_full_set_test": (_c_int, [_c_vp, _P, _P, _c_i64]),
    "gps_full_fit": (_c_int, [_c_vp, _c_int, _P, _c_int, _P, _P, _P]),
    "gps_full_grad": (_c_int, [_c_vp, _c_int, _P, _c_int, _c_int, _P, _P]),
    "gps_full_predict": (_c_int, [_c_vp, _P, _P, _P]),
    "gps_fitc_set_data": (_c_int, [_c_vp, _P, _P, _c_i64, _c_int, _c_dbl, _c_dbl, _c_i64]),
    "gps_fitc_set_test": (_c_int, [_c_vp, _P, _P, _c_i64, _c_i64]),
    "gps_fitc_set_inducing": (_c_int, [_c_vp, _P, _c_i64]),
    "gps_fitc_fit": (_c_int, [_c_vp, _P, _c_int, _P, _P, _P]),
    "gps_fitc_grad": (_c_int, [_c_vp, _P, _c_int, _c_int, _P, _P, _P]),
    "gps_full_blockloo": (_c_int, [_c_vp, _c_int, _P, _c_int, _c_int, _c_int, _P, _P, _P]),
    "gps_full_blockloo_es": (_c_int, [_c_vp, _c_int, _P, _c_int, _c_int, _c_int, _c_dbl, _P, _P,
                                      _P, _P]),
    "gps_fitc_blockloo": (_c_int, [_c_vp, _P, _c_int, _c_int, _c_int, _P, _P, _P, _P]),
    "gps_energy_score": (_c_int, [_c_vp, _P, _P, _c_i64, _P, _c_int, _c_dbl, _P, _P]),
    "gps_fitc_predict": (_c_int, [_c_vp, _P, _P, _P]),
    "gps_fitc_intermediates": (_c_int, [_c_vp, _P, _P, _P, _P, _P]),
    "gps_full_predict_cov": (_c_int, [_c_vp, _c_i64, _c_i64, _P, _P, _c_i64]),
    "gps_fitc_predict_cov": (_c_int, [_c_vp, _c_i64, _c_i64, _P, _P, _c_i64]),
    "gps_full_predict_joint": (_c_int, [_c_vp, _c_int, _c_int, _c_int, _c_dbl, _P, _P, _P]),
    "gps_fitc_predict_joint": (_c_int, [_c_vp, _c_int, _c_int, _c_int, _c_dbl, _P, _P, _P]),
    "gps_full_predict_draws": (_c_int, [_c_vp, _c_i64, _c_i64, _c_int, _P, _P]),
    "gps_fitc_predict_draws": (_c_int, [_c_vp, _c_i64, _c_i64, _c_int, _P, _P]),
    "gps_full_surface": (_c_int, [_c_vp, _P, _P, _c_i64, _c_int, _c_dbl, _P, _c_i64, _P, _c_i64,
                                  _c_int, _P]),
    "gps_full_grad_batch": (_c_int, [_c_vp, _c_int, _c_int, _c_i64, _P, _P, _c_i64, _c_int, _P,
                                     _c_int, _P, _P, _PI]),
    "gps_full_train_batch": (_c_int, [_c_vp, _c_int, _c_int, _c_i64, _P, _P, _c_i64, _c_int, _P,
                                      _c_int, _c_i64, _c_dbl, _P, _P, _c_i64, _c_int, _P, _P, _P,
                                      _P, _P, _P, _P, _PI, _PI]),
    "gps_fitc_grad_batch": (_c_int, [_c_vp, _c_int, _c_i64, _P, _P, _c_i64, _c_int, _P, _c_int, _P,
                                     _c_int, _P, _P, _P, _PI]),
    "gps_fitc_train_batch": (_c_int, [_c_vp, _c_int, _c_i64, _P, _P, _c_i64, _c_int, _P, _c_int, _P,
                                      _c_int, _c_i64, _c_dbl, _c_dbl, _P, _P, _c_i64, _c_int, _P,
                                      _P, _P, _P, _P, _P, _P, _P, _PI, _PI]),
    "gps_fitc_grad_tall": (_c_int, [_c_vp, _c_int, _c_i64, _P, _P, _c_i64, _c_int, _P, _c_int, _P,
                                    _c_int, _P, _P, _P, _PI]),
    "gps_fitc_train_tall": (_c_int, [_c_vp, _c_int, _c_i64, _P, _P, _c_i64, _c_int, _P, _c_int, _P,
                                     _c_int, _c_i64, _c_dbl, _c_dbl, _P, _P, _c_i64, _c_int, _P,
                                     _P, _P, _P, _P, _P, _P, _P, _PI, _PI]),
    "gps_full_grad_tall": (_c_int, [_c_vp, _c_int, _c_int, _c_i64, _P, _P, _c_i64, _c_int, _P,
                                    _c_int, _P, _P, _PI]),
    "gps_full_train_tall": (_c_int, [_c_vp, _c_int, _c_int, _c_i64, _P, _P, _c_i64, _c_int, _P,
                                     _c_int, _c_i64, _c_dbl, _P, _P, _c_i64, _c_int, _P, _P, _P,
                                     _P, _P, _P, _P, _PI, _PI]),
    "gps_full_blockloo_grad_tall": (_c_int, [_c_vp, _c_int, _c_int, _c_int, _c_i64, _P, _P, _c_i64,
                                             _c_int, _P, _c_int, _P, _P, _P, _P, _PI]),
    "gps_full_blockloo_train_tall": (_c_int, [_c_vp, _c_int, _c_int, _c_int, _c_i64, _P, _P, _c_i64,
                                              _c_int, _P, _c_int, _c_i64, _c_dbl, _P, _P, _c_i64,
                                              _c_int, _P, _P, _P, _P, _P, _P, _P, _PI, _PI]),
    "gps_full_train_tall_va": (_c_int, [_c_vp, _c_int, _c_int, _c_i64, _P, _P, _c_i64, _c_int, _P,
                                        _c_int, _c_i64, _c_dbl, _P, _P, _c_i64, _c_i64, _P, _P,
                                        _c_i64, _c_int, _P, _P, _P, _P, _P, _P, _P, _P, _PI, _PI]),
    "gps_full_blockloo_train_tall_va": (_c_int, [_c_vp, _c_int, _c_int, _c_int, _c_i64, _P, _P,
                                                 _c_i64, _c_int, _P, _c_int, _c_i64, _c_dbl, _P, _P,
                                                 _c_i64, _c_i64, _P, _P, _c_i64, _c_int, _P, _P, _P,
                                                 _P, _P, _P, _P, _P, _PI, _PI]),
    "gps_full_es_grad_tall": (_c_int, [_c_vp, _c_int, _c_int, _c_int, _c_dbl, _c_i64, _P, _P, _c_i64,
                                       _c_int, _P, _c_int, _P, _P, _P, _P, _P, _PI]),
    "gps_full_es_train_tall": (_c_int, [_c_vp, _c_int, _c_int, _c_int, _c_dbl, _c_i64, _P, _P,
                                        _c_i64, _c_int, _P, _c_int, _c_i64, _c_dbl, _P, _P, _c_i64,
                                        _c_int, _P, _c_i64, _P, _P, _P, _P, _P, _P, _P, _PI, _PI]),
    "gps_fitc_blockloo_grad_tall": (_c_int, [_c_vp, _c_int, _c_int, _c_i64, _P, _P, _c_i64, _c_int,
                                             _P, _c_int, _P, _c_int, _P, _P, _P, _P, _P, _PI]),
    "gps_fitc_blockloo_train_tall": (_c_int, [_c_vp, _c_int, _c_int, _c_i64, _P, _P, _c_i64, _c_int,
                                              _P, _c_int, _P, _c_int, _c_i64, _c_dbl, _c_dbl, _P, _P,
                                              _c_i64, _c_int, _P, _P, _P, _P, _P, _P, _P, _P, _PI,
                                              _PI]),
    "gps_fitc_train_tall_va": (_c_int, [_c_vp, _c_int, _c_i64, _P, _P, _c_i64, _c_int, _P, _c_int, _P,
                                        _c_int, _c_i64, _c_dbl, _c_dbl, _P, _P, _c_i64, _c_i64, _P,
                                        _P, _c_i64, _c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                        _PI, _PI]),
    "gps_fitc_blockloo_train_tall_va": (_c_int, [_c_vp, _c_int, _c_int, _c_i64, _P, _P, _c_i64,
                                                 _c_int, _P, _c_int, _P, _c_int, _c_i64, _c_dbl,
                                                 _c_dbl, _P, _P, _c_i64, _c_i64, _P, _P, _c_i64,
                                                 _c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _PI,
                                                 _PI]),
    "gps_comm_unique_id": (_c_int, [_c_cp]),
    "gps_comm_init": (_c_int, [_c_vp, _c_int, _c_int, _c_cp]),
    "gps_comm_init_local": (_c_int, [_c_vp, _c_int, _c_int, ctypes.c_longlong]),
    "gps_comm_info": (_c_int, [_c_vp, ctypes.POINTER(_c_int), ctypes.POINTER(_c_int),
                               ctypes.POINTER(_c_int)]),
    "gps_comm_destroy": (_c_int, [_c_vp]),
}

_lib = None


def gemm_schedule(desc, kr=None, have_kscale=False, slots=512):
    """(plan dict, items [n][8]) of one internal GEMM launch (gps_gemm_schedule; no device):
    item columns wg, ti, tj, k begin, k end, slice, stream-K slot, tickets."""
    lib = load()
    plan = np.zeros(len(GEMM_PLAN_NAMES), np.int32)
    krp = None if kr is None else kr.ctypes.data_as(_PI)
    pp = plan.ctypes.data_as(_PI)
    n = lib.gps_gemm_schedule(ctypes.byref(desc), krp, int(have_kscale), slots, pp, None, 0)
    if n < 0:
        raise GpsError(lib.gps_last_error(None).decode())
    items = np.zeros((n, 8), np.int32)
    lib.gps_gemm_schedule(ctypes.byref(desc), krp, int(have_kscale), slots, pp,
                          items.ctypes.data_as(_PI), n)
    return dict(zip(GEMM_PLAN_NAMES, (int(v) for v in plan))), items


DAG_PROTO_ROW = 28  # GPS_DAG_PROTO_ROW


def dag_task_protocol(T, words):
    """[n][DAG_PROTO_ROW] int32 of the persistent factorisation's task words (gps_dag_task_protocol;
    no device): per word its fields type, part, fine, i, j, k, len, tile, three polled
    (array, i, j, threshold) and two arrival (array, i, j, increment) groups, array −1 = unused."""
    lib = load()
    words = np.ascontiguousarray(words, np.uint32)
    out = np.zeros((len(words), DAG_PROTO_ROW), np.int32)
    if len(words) and lib.gps_dag_task_protocol(T, words.ctypes.data, len(words),
                                                out.ctypes.data_as(_PI)) != len(words):
        raise GpsError(lib.gps_last_error(None).decode())
    return out


class GpsError(RuntimeError):
    """A HIP / RCCL / argument error reported by libgpscore (status < 0)."""


class NotPositiveDefinite(GpsError):
    """Cholesky hit a non-positive pivot (status > 0), as torch.potrf raises
    RuntimeError (the reference catches it at KF:726 / K20:784)."""

    def __init__(self, info, msg):
        super().__init__(msg)
        self.info = info


def load():
    """Load libgpscore.so once; raise if it is missing (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"libgpscore.so not found at {LIB_PATH}: build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (or make -C <pkg>/csrc)")
    lib = ctypes.CDLL(LIB_PATH)
    lib.gps_version.restype = _c_int
    lib.gps_version.argtypes = []
    if lib.gps_version() != ABI_VERSION:  # an old library under new signatures would misread
        raise ImportError(f"{LIB_PATH} has ABI version {lib.gps_version()}, this binding "
                          f"expects {ABI_VERSION}: rebuild the library")
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def rccl_info():
    """(ncclGetVersion, the file that holds ncclAllReduce as this process resolved it)."""
    lib = load()
    v = _c_int()
    buf = ctypes.create_string_buffer(4096)
    rc = lib.gps_rccl_info(ctypes.byref(v), buf, len(buf))
    if rc != 0:
        raise GpsError(f"gps_rccl_info failed ({rc})")
    return v.value, buf.value.decode()


def build_id():
    """The source hash the loaded library was built from (gps_build_id)."""
    lib = load()
    buf = ctypes.create_string_buffer(80)
    lib.gps_build_id(buf, len(buf))
    return buf.value.decode()


def check_build_id():
    """Refuse a library that was not built from the sources checked out beside it: the test
    suite and smoke() call this, so a passing GPU record names the HEAD sources' build.  Returns
    the id; when the sources are absent (a deployed library) nothing is compared."""
    from . import buildid
    want = buildid.source_hash()
    got = build_id()
    if want is not None and got != want:
        raise ImportError(f"{LIB_PATH} was built from other sources (build id {got[:16]}, the "
                          f"checked-out csrc/ hashes to {want[:16]}): rebuild it with "
                          "`make -C <pkg>/csrc`")
    return got


def ptr(a):
    """float64 pointer of a C-contiguous numpy array (None -> NULL)."""
    if a is None:
        return None
    return a.ctypes.data_as(_P)


def f64(a, ndim=None):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    if ndim == 2 and a.ndim == 1:
        a = a.reshape(-1, 1)
    return a


def _ptr_array(arrays, slots):
    """A C array of float64 pointers, NULL for None and for the unused slots."""
    a = (_P * slots)()
    for i, v in enumerate(arrays):
        if v is not None:
            a[i] = v.ctypes.data_as(_P)
    return a


# The gradient diagnostics' raw calls: the handle may be None (the argument checks come before the
# context is looked at, tests/test_grad_terms_host.py); they return the status.
def grad_terms_diag_raw(h, which, obj, n, n_pad, ins, outs, scal=1.0, m_pad=0):
    pi = None if ins is None else _ptr_array(ins, 8)
    po = None if outs is None else _ptr_array(outs, 6)
    return load().gps_grad_terms_diag(h, which, obj, n, n_pad, m_pad, scal, pi, po)


def vec_diag_raw(h, which, dims, scal, ins, outs):
    """gps_vec_diag: dims up to 8 integers, scal up to 2 doubles, ins / outs lists of float64 arrays
    or None (None for a list itself: a NULL argument)."""
    d = np.zeros(8, np.int64)
    d[:len(dims)] = dims
    sc = np.zeros(2)
    sc[:len(scal)] = scal
    pi = None if ins is None else _ptr_array(ins, 8)
    po = None if outs is None else _ptr_array(outs, 8)
    return load().gps_vec_diag(h, which, d.ctypes.data_as(_PI64), ptr(sc), pi, po)


def block_diag_raw(h, which, dims, scal, ins, outs):
    """gps_block_diag: dims up to 8 integers, scal up to 8 doubles, ins (up to 12) / outs (up to 4)
    lists of float64 arrays or None (None for a list itself: a NULL argument)."""
    d = np.zeros(8, np.int64)
    d[:len(dims)] = dims
    sc = np.zeros(8)
    sc[:len(scal)] = scal
    pi = None if ins is None else _ptr_array(ins, 12)
    po = None if outs is None else _ptr_array(outs, 4)
    return load().gps_block_diag(h, which, d.ctypes.data_as(_PI64), ptr(sc), pi, po)


def grad_contract_diag_raw(h, n, d, X, inv_ell, sf2, Ainv, Mx, ld, alpha, v, a, out):
    return load().gps_grad_contract_diag(h, n, d, ptr(X), ptr(inv_ell), sf2, ptr(Ainv), ptr(Mx), ld,
                                         ptr(alpha), ptr(v), ptr(a), ptr(out))


def fitc_contract_diag_raw(h, nr, nc, nc_pad, d, xr, xc, inv_ell, sf2, R, coef, rs, pc, pv, qv,
                           out, zout, nt=None, ldr=None):
    nt = len(R) if nt is None else nt
    ldr = np.array([m.shape[1] for m in R] if ldr is None else ldr, np.int64)
    coef = np.ascontiguousarray(coef, np.float64)
    pc = None if pc is None else np.ascontiguousarray(pc, np.float64)
    return load().gps_fitc_contract_diag(
        h, nr, nc, nc_pad, d, ptr(xr), ptr(xc), ptr(inv_ell), sf2, nt,
        _ptr_array(R, 4) if len(R) else None, ldr.ctypes.data_as(_PI64) if len(ldr) else None,
        ptr(coef) if len(coef) else None, None if rs is None else _ptr_array(rs, 4), ptr(pc),
        None if pv is None else _ptr_array(pv, 2), None if qv is None else _ptr_array(qv, 2),
        ptr(out), ptr(zout))


class Context:
    """One device + one HIP stream + the device-resident buffers of the hot path."""

    def __init__(self, device=0):
        self.lib = load()
        h = _c_vp()
        rc = self.lib.gps_ctx_create(int(device), ctypes.byref(h))
        if rc != 0:
            raise GpsError(f"gps_ctx_create(device={device}) failed: "
                           f"{self.lib.gps_last_error(None).decode()}")
        self.h = h
        self.device = device
        # which GP object's data the device currently holds, per kind ("full" / "fitc")
        self.resident = {}

    def check(self, rc, what):
        if rc == 0:
            return
        msg = self.lib.gps_last_error(self.h).decode()
        if rc > 0:
            raise NotPositiveDefinite(rc, f"{what}: {msg}")
        raise GpsError(f"{what} failed ({rc}): {msg}")

    def call(self, name, *args):
        self.check(getattr(self.lib, name)(self.h, *args), name)

    def close(self):
        if getattr(self, "h", None):
            self.lib.gps_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- profiling
    def prof(self, on=True):
        self.call("gps_prof_enable", 1 if on else 0)

    def prof_collect(self):
        import json
        buf = ctypes.create_string_buffer(1 << 16)
        self.call("gps_prof_collect", buf, len(buf))
        return json.loads(buf.value.decode())

    def phases(self, on=True):
        """Phase timing of the FITC forward on its production schedule (gps_phase_enable)."""
        self.call("gps_phase_enable", 1 if on else 0)

    def phase_collect(self):
        """{"phases": {name: {count, ms}}, "allreduce": [[bytes, ms], ...]} since the last
        collect (gps_phase_collect)."""
        import json
        buf = ctypes.create_string_buffer(1 << 20)
        self.call("gps_phase_collect", buf, len(buf))
        return json.loads(buf.value.decode())

    def set_overlap(self, on=True):
        """Run the factorisation's off-critical-path GEMMs on a second stream."""
        self.call("gps_ctx_set_option", GPS_OPT_OVERLAP, 1 if on else 0)

    def set_tiny_gemm(self, on=True):
        """The small kernel (16/32-blocks per wave, K split across a workgroup's waves) for
        the GEMMs at the bottom of the recursion (default) or the 64-tile split-K path
        (process-wide)."""
        self.call("gps_ctx_set_option", GPS_OPT_TINY_GEMM, 1 if on else 0)

    def set_gram_reg(self, on=True):
        """Gram kernels (process-wide): True / 2 (default) the d = 8, 16 builds on the matrix
        cores (the reference's expansion, centred), d = 1 on the register-resident kernel; 1 the
        register-resident direct-difference kernels (bitwise equal to 0); False / 0 the
        LDS-column kernel."""
        v = on if isinstance(on, int) and not isinstance(on, bool) else (2 if on else 0)
        self.call("gps_ctx_set_option", GPS_OPT_GRAM_REG, v)

    def set_graphs(self, on=True):
        """Replay the recursive factorisation from a captured hipGraph (default) or launch
        it eagerly."""
        self.call("gps_ctx_set_option", GPS_OPT_GRAPH, 1 if on else 0)

    def set_ar_chunks(self, chunks):
        """Sharded FITC: B's all-reduce in this many row blocks overlapped with the SYRK
        (GPS_OPT_AR_CHUNKS, default 4; 1 = one all-reduce after the SYRK)."""
        self.call("gps_ctx_set_option", GPS_OPT_AR_CHUNKS, int(chunks))

    def set_dag(self, on=True, tiles=None):
        """The persistent factorisation of the bottom diagonal blocks (GPS_OPT_DAG, default on)
        and its largest block in 128-tiles (GPS_OPT_DAG_TILES)."""
        self.call("gps_ctx_set_option", GPS_OPT_DAG, 1 if on else 0)
        if tiles is not None:
            self.call("gps_ctx_set_option", GPS_OPT_DAG_TILES, int(tiles))

    def set_pred_pre(self, on=True):
        """FITC: form the q_i = ||Lm^-1 k_i||^2 columns that need only the top-level Lm11^-1
        during Lm's factorisation (default), or the whole pass after it."""
        self.call("gps_ctx_set_option", GPS_OPT_PRED_PRE, 1 if on else 0)

    def synchronize(self):
        self.call("gps_ctx_synchronize")

    def stats(self):
        """{graphs, graph_cap, graph_overflow, device_bytes, graph_dropped, graph_evicted}
        (gps_ctx_stats)."""
        out = np.zeros(GPS_N_STATS, np.int64)
        rc = self.lib.gps_ctx_stats(self.h, out.ctypes.data_as(ctypes.c_void_p), GPS_N_STATS)
        self.check(0 if rc >= 0 else rc, "gps_ctx_stats")
        return dict(zip(("graphs", "graph_cap", "graph_overflow", "device_bytes", "graph_dropped",
                         "graph_evicted"), (int(v) for v in out)))

    def gemm_diag(self, desc, A, B, C=None, kscale=None, w=None, kr=None, out0=None, out1=None):
        """One internal GEMM launch on host arrays (gps_gemm_diag; diagnostics): C, out0 and out1
        are updated in place, the launch launch_gemm chose comes back as a dict (GEMM_PLAN_NAMES)."""
        plan = np.zeros(len(GEMM_PLAN_NAMES), np.int32)
        krp = None if kr is None else kr.ctypes.data_as(_PI)
        self.check(self.lib.gps_gemm_diag(self.h, ctypes.byref(desc), ptr(A), ptr(B), ptr(C),
                                          ptr(kscale), ptr(w), krp, ptr(out0), ptr(out1),
                                          plan.ctypes.data_as(_PI)), "gps_gemm_diag")
        return dict(zip(GEMM_PLAN_NAMES, (int(v) for v in plan)))

    def potrf_diag(self, A):
        """The factorisation as gps_potrf runs it, everything it wrote copied back whole
        (gps_potrf_diag; diagnostics): (L, Linv, logdiag, info, plan) with L and Linv the padded
        n_pad x n_pad squares, info 0 or the first non-PD minor (no exception), plan a dict
        (POTRF_PLAN_NAMES)."""
        A = f64(A)
        n = A.shape[0]
        npad = (n + 127) // 128 * 128
        L = np.full((npad, npad), np.nan)
        Li = np.full((npad, npad), np.nan)
        ld = np.full(npad, np.nan)
        info = np.full(1, -1, np.int32)
        plan = np.zeros(len(POTRF_PLAN_NAMES), np.int32)
        self.check(self.lib.gps_potrf_diag(self.h, n, ptr(A), A.shape[1], ptr(L), ptr(Li), ptr(ld),
                                           info.ctypes.data_as(_PI), plan.ctypes.data_as(_PI)),
                   "gps_potrf_diag")
        return L, Li, ld, int(info[0]), dict(zip(POTRF_PLAN_NAMES, (int(v) for v in plan)))

    def grad_terms_diag(self, which, obj, n, n_pad, ins, outs, scal=1.0, m_pad=0):
        """One per-point gradient-term launch on host arrays (gps_grad_terms_diag; diagnostics):
        ins / outs are the arrays in the header's order, None where one is absent; outs are
        written in place."""
        self.check(grad_terms_diag_raw(self.h, which, obj, n, n_pad, ins, outs, scal, m_pad),
                   "gps_grad_terms_diag")

    def vec_diag(self, which, dims, ins, outs, scal=()):
        """One vector-layer launch on host arrays (gps_vec_diag; diagnostics): dims / scal / ins /
        outs in the header's order, None where an array is absent; outs are written in place."""
        self.check(vec_diag_raw(self.h, which, dims, scal, ins, outs), "gps_vec_diag")

    def block_diag(self, which, dims, ins, outs, scal=()):
        """One launch of a block-LOO / energy-score / joint kernel on host arrays (gps_block_diag;
        diagnostics): dims / scal / ins / outs per `which` as tabulated in include/gpscore.h."""
        self.check(block_diag_raw(self.h, which, dims, scal, ins, outs), "gps_block_diag")

    def grad_contract_diag(self, X, inv_ell, sf2, Ainv, Mx, ld, alpha, v, a):
        """launch_grad_contract on host arrays (gps_grad_contract_diag; diagnostics): the
        passes x 18 block as the launcher writes it."""
        n, d = X.shape
        out = np.full(((d + 15) // 16, 18), np.nan)
        self.check(grad_contract_diag_raw(self.h, n, d, X, inv_ell, sf2, Ainv, Mx, ld, alpha, v, a,
                                          out), "gps_grad_contract_diag")
        return out

    def fitc_contract_diag(self, xr, xc, nc_pad, inv_ell, sf2, R=(), coef=(), rs=None,
                           pc=(0.0, 0.0), pv=(None, None), qv=(None, None)):
        """launch_fitc_grad_contract on host arrays (gps_fitc_contract_diag; diagnostics):
        (out [passes][17], zout [nc][d]).  R: up to four [nr][ldr] matrices (ldr their row
        length), rs: None or one entry (an array or None) per matrix."""
        (nr, d), nc = xr.shape, xc.shape[0]
        out = np.full(((d + 15) // 16, 17), np.nan)
        zout = np.full((nc, d), np.nan)
        self.check(fitc_contract_diag_raw(self.h, nr, nc, nc_pad, d, xr, xc, inv_ell, sf2, R, coef,
                                          rs, pc, pv, qv, out, zout), "gps_fitc_contract_diag")
        return out, zout

    def comm_info(self):
        """(nranks, rank, kind) of the context's communicator as the library sees it: RCCL's own
        ncclCommCount / ncclCommUserRank, the in-process group's, or (1, 0, "none")."""
        n, r, k = _c_int(), _c_int(), _c_int()
        self.call("gps_comm_info", ctypes.byref(n), ctypes.byref(r), ctypes.byref(k))
        return n.value, r.value, COMM_KINDS.get(k.value, str(k.value))

    def set_stream(self, stream_handle):
        self.call("gps_ctx_set_stream", _c_vp(stream_handle))


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        dev = int(os.environ.get("GPSCORE_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        _default_ctx = Context(dev)
    return _default_ctx
