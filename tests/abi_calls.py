"""Raw calls of the device entry points of include/ldpc_osd.h for the ABI-contract tests: every argument by the name the
header gives it, tensors as device pointers, an omitted argument as NULL / 0 -- so that any output can be left out,
which the Decoder methods do not allow.  ``call`` returns the status code instead of raising."""
import ctypes as C

import numpy as np
import torch

from short_ldpc_decoding_osd_amd import _lib

E_ARG = -1

# argument names between ctx and stream, in the header's order
SIGS = {
    "ldpc_nms_decode": ("d_llr", "B", "T", "alpha", "w_in", "w_out", "d_soft", "d_traj", "d_hard", "d_fail", "kernel"),
    "ldpc_nms_traj_rows": ("d_llr", "d_index", "d_count", "F", "T", "alpha", "w_in", "w_out", "d_rows", "kernel"),
    "ldpc_osd_ge": ("d_rows_in", "F", "d_rows_out", "d_swaps", "d_nswaps"),
    "ldpc_osd_front": ("d_y", "d_index", "d_count", "F", "d_perm", "d_parity", "d_nswaps"),
    "ldpc_osd_decode": ("d_y", "d_index", "d_count", "F", "params", "d_cw", "d_metric", "d_best", "d_ntep"),
    "ldpc_osd_search": ("d_y", "d_index", "d_count", "F", "d_perm", "d_parity", "params", "d_cw", "d_metric", "d_best",
                        "d_ntep"),
    "ldpc_osd_tep_eval": ("d_y", "d_index", "d_count", "F", "d_perm", "d_parity", "d_mask", "d_cw", "d_metric", "d_hd"),
    "ldpc_osd_counts": ("d_cw", "d_label_bits", "d_index", "d_count", "d_ntep", "F", "d_counts"),
    "ldpc_hosd_front": ("d_order_llr", "F", "d_lri", "d_uidx", "d_M", "d_nswaps"),
    "ldpc_hosd_search": ("d_order_llr", "d_metric_llr", "F", "d_lri", "d_uidx", "d_M", "d_teps", "d_block_off", "nblk",
                         "d_label_bits", "d_block_min", "d_block_arg", "d_truth", "d_cw", "d_metric", "d_best"),
    "ldpc_hosd_sliding": ("d_order_llr", "d_metric_llr", "F", "d_lri", "d_uidx", "d_M", "d_teps", "d_block_off", "nblk", "win",
                          "soft_margin", "fcn_weights", "n_weights", "group", "d_label_bits", "d_deep_limit", "d_global_min",
                          "d_truth", "d_success", "d_cw", "d_metric", "d_best", "d_teps_evaluated"),
}
# the G-form families (any shape, high rate, long / low rate) share their signatures
_FRONT_RESULTS = ("d_y", "d_index", "d_count", "F", "d_perm", "d_parity")
_SCAN_OUT = ("d_cw", "d_metric", "d_best", "d_ntep")
_DECODE_TAIL = ("d_perm", "d_parity") + _SCAN_OUT + ("d_label_bits", "d_counts")
for _fam in ("osdx", "osdw", "osdl"):
    SIGS[f"ldpc_{_fam}_front"] = SIGS["ldpc_osd_front"]
    SIGS[f"ldpc_{_fam}_search"] = _FRONT_RESULTS + ("order",) + _SCAN_OUT
    SIGS[f"ldpc_{_fam}_decode"] = ("d_y", "d_index", "d_count", "F", "order") + _DECODE_TAIL
    SIGS[f"ldpc_{_fam}_tep_eval"] = SIGS["ldpc_osd_tep_eval"]
    for _algo in ("fs", "pb"):
        SIGS[f"ldpc_{_fam}_{_algo}_search"] = _FRONT_RESULTS + ("params",) + _SCAN_OUT
        SIGS[f"ldpc_{_fam}_{_algo}_decode"] = ("d_y", "d_index", "d_count", "F", "params") + _DECODE_TAIL
_SCALARS = {"B": 0, "F": 0, "T": 0, "order": 0, "w_in": 1.0, "w_out": 1.0, "kernel": 0, "nblk": 0, "win": 0, "soft_margin": 0.0,
            "n_weights": 0, "group": 0}


def _arg(v):
    if isinstance(v, torch.Tensor):
        return v.data_ptr()
    if isinstance(v, np.ndarray):                       # host float arrays: alpha, fcn_weights
        assert v.dtype == np.float32 and v.flags.c_contiguous
        return v.ctypes.data_as(C.POINTER(C.c_float))
    if isinstance(v, _lib.OsdParams):
        return C.byref(v)
    return v


def call(dec, entry, **kw):
    """dec.L.<entry>(ctx, ..., stream) on torch's current stream.  Keyword names are the header's; the caller keeps the
    tensors, arrays and parameter blocks alive."""
    names = SIGS[entry]
    unknown = set(kw) - set(names)
    assert not unknown, (entry, unknown)
    args = [_arg(kw.get(n, _SCALARS.get(n))) for n in names]
    return getattr(dec.L, entry)(dec._ctx, *args, dec._stream())


def last_error(dec):
    return dec.L.ldpc_last_error().decode()


def run_pipeline(dec, p):
    """ldpc_pipeline_run on a _lib.Pipeline block (BatchPipeline._p, possibly with members set to None)."""
    return dec.L.ldpc_pipeline_run(dec._ctx, C.byref(p), dec._stream())


def params(order, algo=_lib.OSD_CONVENTIONAL, flags=0, snr_db=2.5, aux=None, y_frames=0):
    """ldpc_osd_params with the reference's FS constants."""
    return _lib.OsdParams(int(order), int(algo), float(snr_db), 0.1, 6.5, 30.0, 1, int(flags),
                          aux.data_ptr() if aux is not None else None, int(y_frames))


def alpha_array(alpha, T):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(alpha, dtype=np.float32), (max(T, 1),)))


# ---- sentinels: a value no kernel writes, per dtype
SENT = {torch.int64: 0x5A5A5A5A5A5A5A5A, torch.float32: -7.0, torch.int32: -7, torch.uint8: 0xEE,
        torch.int16: 0x6EEE}


def sentinel(dec, shape, dtype):
    return torch.full(shape, SENT[dtype], dtype=dtype, device=dec.device)


def untouched(t, start=0):
    """Rows start.. of t still hold the sentinel."""
    return bool((t[start:] == SENT[t.dtype]).all())


def same_bits(a, b):
    """Exact equality of two tensors, floats by their bit patterns."""
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return a.shape == b.shape and torch.equal(a, b)
