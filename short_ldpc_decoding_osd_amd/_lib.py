"""ctypes binding of libldpcosd.so (C ABI: include/ldpc_osd.h).

There is deliberately no fallback: if the shared object is missing or a call fails the
wrapper raises -- the decoders only exist as HIP kernels.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# LDPC_OSD_LIB: another build of the same ABI (the host-only sanitizer build of `build.py --asan`, whose device entry
# points are stubs that fail)
LIB_PATH = os.environ.get("LDPC_OSD_LIB") or os.path.join(_HERE, "libldpcosd.so")

# every symbol include/ldpc_osd.h declares (tests check the list against the header)
SYMBOLS = (
    "ldpc_last_error", "ldpc_abi_version",
    "ldpc_code_from_alist", "ldpc_code_from_dense", "ldpc_code_destroy", "ldpc_code_dims",
    "ldpc_code_get_H", "ldpc_code_get_G", "ldpc_gf2elim_host", "ldpc_tep_table", "ldpc_tep_table_fs", "ldpc_osdl_pb_table", "ldpc_crc32c",
    "ldpc_ctx_create", "ldpc_ctx_destroy", "ldpc_ctx_nms_kernel", "ldpc_ctx_get_pb_tuning", "ldpc_ctx_set_pb_tuning",
    "ldpc_nms_decode", "ldpc_nms_traj_rows", "ldpc_nms_train_grad", "ldpc_eval_counts", "ldpc_compact", "ldpc_pack_bits", "ldpc_unpack_bits",
    "ldpc_gen_frames",
    "ldpc_osd_reserve", "ldpc_osd_reserve_stream", "ldpc_osd_release_stream", "ldpc_osd_index_errors", "ldpc_osd_ge", "ldpc_osd_front", "ldpc_osd_search", "ldpc_osd_decode", "ldpc_osd_tep_eval", "ldpc_osd_counts",
    "ldpc_osdx_supported", "ldpc_osdx_front", "ldpc_osdx_search", "ldpc_osdx_decode",
    "ldpc_osdx_fs_search", "ldpc_osdx_fs_decode", "ldpc_osdx_tep_eval", "ldpc_osdx_pb_search", "ldpc_osdx_pb_decode",
    "ldpc_osdw_supported", "ldpc_osdw_front", "ldpc_osdw_search", "ldpc_osdw_decode",
    "ldpc_osdw_fs_search", "ldpc_osdw_fs_decode", "ldpc_osdw_tep_eval", "ldpc_osdw_pb_search", "ldpc_osdw_pb_decode",
    "ldpc_osdl_supported", "ldpc_osdl_front", "ldpc_osdl_search", "ldpc_osdl_decode",
    "ldpc_osdl_fs_search", "ldpc_osdl_fs_decode", "ldpc_osdl_tep_eval", "ldpc_osdl_pb_search", "ldpc_osdl_pb_decode",
    "ldpc_hosd_pattern_teps", "ldpc_hosd_front", "ldpc_hosd_search", "ldpc_hosd_sliding",
    "ldpc_hosdx_supported", "ldpc_hosdx_front", "ldpc_hosdx_search", "ldpc_hosdx_sliding",
    "ldpc_hosdw_supported", "ldpc_hosdw_front", "ldpc_hosdw_search", "ldpc_hosdw_sliding",
    "ldpc_hosdl_supported", "ldpc_hosdl_pattern_teps", "ldpc_hosdl_front", "ldpc_hosdl_search", "ldpc_hosdl_sliding",
    "ldpc_dia_cnn", "ldpc_dia_cnn_grad",
    "ldpc_fcn_windows", "ldpc_fcn_grad",
    "ldpc_pipeline_run", "ldpc_pipeline_timing",
    "ldpc_osd_merge", "ldpc_family_pipeline_run", "ldpc_dlosd_pipeline_run",
)

NMS_AUTO, NMS_GENERIC, NMS_QC16 = 0, 1, 2
OSD_CONVENTIONAL, OSD_FS, OSD_PB = 0, 1, 2
# ldpc_osd_params.flags (LDPC_OSD_F_*)
OSD_F_TABLE_SCAN, OSD_F_PB_BLOCK, OSD_F_PB_REPLAY, OSD_F_READLANE_SCAN, OSD_F_PB_FRONT_INSIDE = 1, 2, 4, 8, 16


class OsdParams(C.Structure):
    _fields_ = [("order", C.c_int32), ("algo", C.c_int32), ("snr_db", C.c_float), ("fs_beta", C.c_float),
                ("fs_tau_e", C.c_float), ("fs_tau_psc", C.c_float), ("fs_reference_quirk", C.c_int32),
                ("flags", C.c_int32), ("d_aux", C.c_void_p), ("y_frames", C.c_int64)]


# ldpc_gen_params.flags (LDPC_GEN_F_*)
GEN_F_ALL_ZEROS, GEN_F_RAYLEIGH = 1, 2


class GenParams(C.Structure):
    """ldpc_gen_params of include/ldpc_osd.h (the frame generator's seed, first frame number and channel)."""
    _fields_ = [("seed", C.c_uint64), ("frame0", C.c_int64), ("sigma", C.c_float), ("mean", C.c_float),
                ("flags", C.c_uint32), ("fade_len", C.c_int32)]


class PbTuning(C.Structure):
    """ldpc_pb_tuning of include/ldpc_osd.h (PB-OSD hand-over schedule and chunk targets of a context)."""
    _fields_ = [(n, C.c_int32) for n in ("budget", "budget_s", "budget_m", "budget_l", "budget_xl", "t1", "t2", "t3",
                                         "late_min", "late_maxlen", "late_pct", "late_div", "handoff_maxlen")]


class Pipeline(C.Structure):
    """ldpc_pipeline of include/ldpc_osd.h (device pointers as integers)."""
    _fields_ = [("d_llr", C.c_void_p), ("B", C.c_int64), ("T", C.c_int32), ("nms_kernel", C.c_int32),
                ("alpha", C.POINTER(C.c_float)), ("w_in", C.c_float), ("w_out", C.c_float),
                ("d_soft", C.c_void_p), ("d_hard", C.c_void_p), ("d_fail", C.c_void_p),
                ("d_label_bits", C.c_void_p), ("d_nms_counts", C.c_void_p),
                ("osd_enable", C.c_int32), ("timing_slot", C.c_int32), ("osd", OsdParams),
                ("d_index", C.c_void_p), ("d_count", C.c_void_p), ("d_perm", C.c_void_p), ("d_parity", C.c_void_p),
                ("d_cw", C.c_void_p), ("d_metric", C.c_void_p), ("d_best", C.c_void_p), ("d_ntep", C.c_void_p),
                ("d_osd_counts", C.c_void_p)]


# ldpc_family_pipeline.family (LDPC_OSD_FAMILY_*) and the prefix of each family's entry points
OSD_FAMILY_AUTO, OSD_FAMILY_X, OSD_FAMILY_W, OSD_FAMILY_L = 0, 1, 2, 3
OSD_FAMILIES = {"osdx": OSD_FAMILY_X, "osdw": OSD_FAMILY_W, "osdl": OSD_FAMILY_L}


class FamilyPipeline(C.Structure):
    """ldpc_family_pipeline of include/ldpc_osd.h (device pointers as integers)."""
    _fields_ = [("d_llr", C.c_void_p), ("B", C.c_int64), ("T", C.c_int32), ("nms_kernel", C.c_int32),
                ("alpha", C.POINTER(C.c_float)), ("w_in", C.c_float), ("w_out", C.c_float),
                ("d_soft", C.c_void_p), ("d_hard", C.c_void_p), ("d_fail", C.c_void_p),
                ("d_label_bits", C.c_void_p), ("d_nms_counts", C.c_void_p),
                ("osd_enable", C.c_int32), ("timing_slot", C.c_int32), ("osd", OsdParams),
                ("family", C.c_int32), ("merge", C.c_int32),
                ("d_index", C.c_void_p), ("d_count", C.c_void_p), ("d_perm", C.c_void_p), ("d_parity", C.c_void_p),
                ("osd_capacity", C.c_int64),
                ("d_cw", C.c_void_p), ("d_metric", C.c_void_p), ("d_best", C.c_void_p), ("d_ntep", C.c_void_p),
                ("d_osd_counts", C.c_void_p), ("d_final_counts", C.c_void_p)]


# ldpc_dlosd_pipeline.family (LDPC_HOSD_FAMILY_*) and the prefix of each H-form family's entry points
HOSD_FAMILY_AUTO, HOSD_FAMILY_128, HOSD_FAMILY_X, HOSD_FAMILY_W, HOSD_FAMILY_L = 0, 1, 2, 3, 4
HOSD_FAMILIES = {"hosd": HOSD_FAMILY_128, "hosdx": HOSD_FAMILY_X, "hosdw": HOSD_FAMILY_W, "hosdl": HOSD_FAMILY_L}


class DlOsdPipeline(C.Structure):
    """ldpc_dlosd_pipeline of include/ldpc_osd.h (device pointers as integers)."""
    _fields_ = [("d_llr", C.c_void_p), ("B", C.c_int64), ("T", C.c_int32), ("nms_kernel", C.c_int32),
                ("alpha", C.POINTER(C.c_float)), ("w_in", C.c_float), ("w_out", C.c_float),
                ("d_soft", C.c_void_p), ("d_hard", C.c_void_p), ("d_fail", C.c_void_p),
                ("d_label_bits", C.c_void_p), ("d_nms_counts", C.c_void_p),
                ("osd_enable", C.c_int32), ("timing_slot", C.c_int32),
                ("family", C.c_int32), ("merge", C.c_int32),
                ("d_index", C.c_void_p), ("d_count", C.c_void_p), ("osd_capacity", C.c_int64),
                ("cnn_weights", C.POINTER(C.c_float)), ("fcn_weights", C.POINTER(C.c_float)),
                ("n_cnn_weights", C.c_int32), ("n_fcn_weights", C.c_int32),
                ("d_teps", C.c_void_p), ("d_block_off", C.c_void_p),
                ("nblk", C.c_int32), ("win", C.c_int32), ("group", C.c_int32), ("soft_margin", C.c_double),
                ("d_rows", C.c_void_p), ("d_order_llr", C.c_void_p), ("d_metric_llr", C.c_void_p), ("d_list_labels", C.c_void_p),
                ("d_lri", C.c_void_p), ("d_uidx", C.c_void_p), ("d_M", C.c_void_p), ("d_nswaps", C.c_void_p),
                ("d_deep_limit", C.c_void_p), ("d_global_min", C.c_void_p), ("d_truth", C.c_void_p), ("d_success", C.c_void_p),
                ("d_cw", C.c_void_p), ("d_metric", C.c_void_p), ("d_best", C.c_void_p), ("d_teps_evaluated", C.c_void_p),
                ("d_dl_counts", C.c_void_p), ("d_final_counts", C.c_void_p)]


TIMING_SLOTS = 64


class LdpcError(RuntimeError):
    pass


_lib = None


def load():
    """Load libldpcosd.so once; raise with build instructions if it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LdpcError(
            f"{LIB_PATH} is missing: build it with `python -m short_ldpc_decoding_osd_amd.build` "
            "(hipcc, --offload-arch=gfx950). There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    pi32, pi64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    sig = {
        "ldpc_last_error": (C.c_char_p, []),
        "ldpc_abi_version": (C.c_int, []),
        "ldpc_code_from_alist": (C.c_int, [C.c_char_p, C.POINTER(vp)]),
        "ldpc_code_from_dense": (C.c_int, [pi32, i32, i32, C.POINTER(vp)]),
        "ldpc_code_destroy": (None, [vp]),
        "ldpc_code_dims": (C.c_int, [vp, pi32, pi32, pi32, pi32]),
        "ldpc_code_get_H": (C.c_int, [vp, pi32]),
        "ldpc_code_get_G": (C.c_int, [vp, pi32]),
        "ldpc_gf2elim_host": (C.c_int, [pi32, i32, i32, pi32, pi32, pi32]),
        "ldpc_tep_table": (i64, [i32, i32, C.POINTER(C.c_uint8), pi64]),
        "ldpc_tep_table_fs": (i64, [i32, i32, C.POINTER(C.c_uint8)]),
        "ldpc_osdl_pb_table": (i64, [i32, i32, C.POINTER(C.c_double)]),
        "ldpc_crc32c": (C.c_uint32, [vp, C.c_uint64]),
        "ldpc_ctx_create": (C.c_int, [vp, i32, C.POINTER(vp)]),
        "ldpc_ctx_destroy": (None, [vp]),
        "ldpc_ctx_nms_kernel": (C.c_int, [vp]),
        "ldpc_ctx_get_pb_tuning": (C.c_int, [vp, C.POINTER(PbTuning)]),
        "ldpc_ctx_set_pb_tuning": (C.c_int, [vp, C.POINTER(PbTuning)]),
        # device entry points: device pointers travel as integers (tensor.data_ptr())
        "ldpc_nms_decode": (C.c_int, [vp, vp, i64, i32, C.POINTER(f32), f32, f32, vp, vp, vp, vp, i32, vp]),
        "ldpc_nms_traj_rows": (C.c_int, [vp, vp, vp, vp, i64, i32, C.POINTER(f32), f32, f32, vp, i32, vp]),
        "ldpc_nms_train_grad": (C.c_int, [vp, vp, vp, i64, i32, C.POINTER(f32), f32, f32, vp, vp, vp, vp, vp, vp, vp, vp]),
        "ldpc_eval_counts": (C.c_int, [vp, vp, vp, vp, i64, vp, vp]),
        "ldpc_compact": (C.c_int, [vp, vp, i64, vp, vp, vp]),
        "ldpc_pack_bits": (C.c_int, [vp, vp, i32, i64, vp, vp]),
        "ldpc_unpack_bits": (C.c_int, [vp, vp, i64, vp, i32, vp]),
        "ldpc_gen_frames": (C.c_int, [vp, C.POINTER(GenParams), i64, vp, vp, vp]),
        "ldpc_osd_reserve": (C.c_int, [vp, i64]),
        "ldpc_osd_reserve_stream": (C.c_int, [vp, i64, C.POINTER(OsdParams), vp]),
        "ldpc_osd_release_stream": (C.c_int, [vp, vp]),
        "ldpc_osd_index_errors": (C.c_int, [vp, pi64]),
        "ldpc_osd_ge": (C.c_int, [vp, vp, i64, vp, vp, vp, vp]),
        "ldpc_osd_front": (C.c_int, [vp, vp, vp, vp, i64, vp, vp, vp, vp]),
        "ldpc_osd_search": (C.c_int, [vp, vp, vp, vp, i64, vp, vp, C.POINTER(OsdParams), vp, vp, vp, vp, vp]),
        "ldpc_osd_decode": (C.c_int, [vp, vp, vp, vp, i64, C.POINTER(OsdParams), vp, vp, vp, vp, vp]),
        "ldpc_osd_tep_eval": (C.c_int, [vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp]),
        "ldpc_osd_counts": (C.c_int, [vp, vp, vp, vp, vp, vp, i64, vp, vp]),
        "ldpc_hosd_pattern_teps": (i64, [i32, pi32, pi32, C.POINTER(C.c_uint8)]),
        "ldpc_hosd_front": (C.c_int, [vp, vp, i64, vp, vp, vp, vp, vp]),
        "ldpc_hosd_search": (C.c_int, [vp, vp, vp, i64, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
        "ldpc_hosd_sliding": (C.c_int, [vp, vp, vp, i64, vp, vp, vp, vp, vp, i32, i32, C.c_double, C.POINTER(f32), i32, i32,
                                        vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "ldpc_hosdx_supported": (C.c_int, [vp]),
        "ldpc_hosdw_supported": (C.c_int, [vp]),
        "ldpc_hosdl_supported": (C.c_int, [vp]),
        "ldpc_hosdl_pattern_teps": (i64, [i32, pi32, pi32, C.POINTER(C.c_uint8)]),
        "ldpc_dia_cnn": (C.c_int, [vp, vp, i64, i32, C.POINTER(f32), i32, vp, vp]),
        "ldpc_dia_cnn_grad": (C.c_int, [vp, vp, vp, i64, i32, C.POINTER(f32), i32, vp, vp, vp, vp]),
        "ldpc_fcn_windows": (C.c_int, [vp, vp, vp, vp, i64, i32, i32, vp, vp, vp, vp]),
        "ldpc_fcn_grad": (C.c_int, [vp, vp, vp, vp, vp, i64, i32, C.POINTER(f32), i32, f32, vp, vp, vp, vp, vp, vp]),
        "ldpc_pipeline_run": (C.c_int, [vp, C.POINTER(Pipeline), vp]),
        "ldpc_pipeline_timing": (C.c_int, [vp, i32, C.POINTER(f32)]),
        "ldpc_osd_merge": (C.c_int, [vp, vp, vp, vp, i64, vp, vp, vp, vp]),
        "ldpc_family_pipeline_run": (C.c_int, [vp, C.POINTER(FamilyPipeline), vp]),
        "ldpc_dlosd_pipeline_run": (C.c_int, [vp, C.POINTER(DlOsdPipeline), vp]),
    }
    for op in ("front", "search", "sliding"):     # the any-shape, the wide and the long H-form family: the signatures of ldpc_hosd_*
        sig[f"ldpc_hosdx_{op}"] = sig[f"ldpc_hosdw_{op}"] = sig[f"ldpc_hosdl_{op}"] = sig[f"ldpc_hosd_{op}"]
    # the entry points that the any-shape and the high-rate family both have, under the same signatures
    for fam in ("osdx", "osdw"):
        sig.update({
            f"ldpc_{fam}_supported": (C.c_int, [vp]),
            f"ldpc_{fam}_front": (C.c_int, [vp, vp, vp, vp, i64, vp, vp, vp, vp]),
            f"ldpc_{fam}_search": (C.c_int, [vp, vp, vp, vp, i64, vp, vp, i32, vp, vp, vp, vp, vp]),
            f"ldpc_{fam}_decode": (C.c_int, [vp, vp, vp, vp, i64, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
            f"ldpc_{fam}_fs_search": (C.c_int, [vp, vp, vp, vp, i64, vp, vp, C.POINTER(OsdParams), vp, vp, vp, vp, vp]),
            f"ldpc_{fam}_fs_decode": (C.c_int, [vp, vp, vp, vp, i64, C.POINTER(OsdParams), vp, vp, vp, vp, vp, vp, vp, vp, vp]),
            f"ldpc_{fam}_tep_eval": (C.c_int, [vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp]),
            f"ldpc_{fam}_pb_search": (C.c_int, [vp, vp, vp, vp, i64, vp, vp, C.POINTER(OsdParams), vp, vp, vp, vp, vp]),
            f"ldpc_{fam}_pb_decode": (C.c_int, [vp, vp, vp, vp, i64, C.POINTER(OsdParams), vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        })
    # the long / low-rate family has all of these, under the signatures of the other two
    for op in ("supported", "front", "search", "decode", "fs_search", "fs_decode", "tep_eval", "pb_search", "pb_decode"):
        sig[f"ldpc_osdl_{op}"] = sig[f"ldpc_osdx_{op}"]
    for name in SYMBOLS:
        fn = getattr(L, name)  # AttributeError here = ABI/header drift, which must be loud
        fn.restype, fn.argtypes = sig[name]
    _lib = L
    return L


def check(rc, what=""):
    """Raise LdpcError for a negative status code."""
    if rc is not None and rc < 0:
        msg = load().ldpc_last_error()
        raise LdpcError(f"{what or 'libldpcosd'} failed ({rc}): {msg.decode() if msg else ''}")
    return rc
