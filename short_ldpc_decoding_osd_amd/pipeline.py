"""One-call batch pipeline: NMS -> counters -> failure compaction -> OSD -> counters
(``ldpc_pipeline_run``).  This is the body of the reference drivers' batch loops
(ldpc_128_testing.py:117-131, then pb_testing.py / fs_testing.py per failed frame) executed as
seven kernel launches from ONE host call, with no device-to-host traffic in between.  All buffers are
allocated once; ``run()`` only enqueues work on torch's current stream.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .runtime import Decoder


class BatchPipeline:
    def __init__(self, dec: Decoder, B: int, T: int, alpha, osd_order=None, osd_algo=_lib.OSD_CONVENTIONAL, snr_db=0.0,
                 w_in=1.0, w_out=1.0, want_soft=True, keep_front=True, **osd_kw):
        self.dec, self.B, self.T = dec, int(B), int(T)
        e = dec.empty
        self.soft = e((B, dec.n), torch.float32) if want_soft else None
        self.hard = e((B, dec.words), torch.int64)
        self.fail = e((B,), torch.uint8)
        self._counts = torch.zeros(8, dtype=torch.int64, device=dec.device)   # one buffer: no torch op to gather them
        self.nms_counts, self.osd_counts = self._counts[:5], self._counts[5:]
        self._alpha = np.ascontiguousarray(np.broadcast_to(np.asarray(alpha, dtype=np.float32), (max(T, 1),)))
        p = _lib.Pipeline()
        p.B, p.T, p.nms_kernel = self.B, self.T, _lib.NMS_AUTO
        p.alpha = self._alpha.ctypes.data_as(C.POINTER(C.c_float))
        p.w_in, p.w_out = float(w_in), float(w_out)
        p.d_soft = self.soft.data_ptr() if want_soft else None
        p.d_hard, p.d_fail = self.hard.data_ptr(), self.fail.data_ptr()
        p.d_nms_counts = self.nms_counts.data_ptr()
        p.osd_enable, p.timing_slot = int(osd_order is not None), -1
        self.osd_order = osd_order
        if osd_order is not None:
            self.index, self.count = e((B,), torch.int32), e((1,), torch.int32)
            # keep_front: the front-end results (perm, P' rows) land in buffers of this object and the two
            # OSD kernels are timed separately; otherwise they go through the context's workspace
            self.perm = e((B, 128), torch.uint8) if keep_front else None
            self.parity = e((B, 64), torch.int64) if keep_front else None
            self.cw, self.metric = e((B, 2), torch.int64), e((B,), torch.float32)
            self.best, self.ntep = e((B,), torch.int32), e((B,), torch.int32)
            self.aux = torch.zeros((B, 4), dtype=torch.int32, device=dec.device) if osd_algo == _lib.OSD_PB else None
            p.osd = dec.osd_params(osd_order, osd_algo, snr_db=snr_db, aux=self.aux, **osd_kw)
            p.d_index, p.d_count = self.index.data_ptr(), self.count.data_ptr()
            p.d_perm = self.perm.data_ptr() if keep_front else None
            p.d_parity = self.parity.data_ptr() if keep_front else None
            p.d_cw, p.d_metric = self.cw.data_ptr(), self.metric.data_ptr()
            p.d_best, p.d_ntep = self.best.data_ptr(), self.ntep.data_ptr()
            p.d_osd_counts = self.osd_counts.data_ptr()
        self._p = p
        self._y = self._labels = None

    def bind(self, y, label_bits=None):
        """Attach the input batch ([B,n] f32) and optional packed labels ([B,words] int64)."""
        self.dec._chk(y, torch.float32, (self.dec.n,), "y")
        if y.shape[0] != self.B:
            raise ValueError(f"batch of {y.shape[0]} frames bound to a pipeline for {self.B}")
        self._y, self._labels = y, label_bits
        self._p.d_llr = y.data_ptr()
        self._p.d_label_bits = label_bits.data_ptr() if label_bits is not None else None
        return self

    def run(self, timing_slot=-1):
        if self._y is None:
            raise RuntimeError("bind() a batch first")
        self._p.timing_slot = int(timing_slot)
        _lib.check(self.dec.L.ldpc_pipeline_run(self.dec._ctx, C.byref(self._p), self.dec._stream()), "ldpc_pipeline_run")

    def timing(self, slot):
        """(nms_ms, osd_front_ms, osd_search_ms) of the run that used ``slot``; synchronise first."""
        ms = (C.c_float * 3)()
        _lib.check(self.dec.L.ldpc_pipeline_timing(self.dec._ctx, int(slot), ms), "ldpc_pipeline_timing")
        return tuple(float(v) for v in ms)

    def reset_counters(self):
        self._counts.zero_()

    def counters(self):
        """int64[8]: {frames, frame_err, bit_err, undetected, synd_fail, osd_frames, osd_wrong, teps}."""
        return self._counts


class FamilyPipeline:
    """``BatchPipeline`` for every code a G-form OSD family serves (``ldpc_family_pipeline_run``), with the decoder's final
    output: after ``run()`` ``hard`` holds the OSD codewords among the NMS decisions (``merge``).

    ``family``: ``"osdx"`` / ``"osdw"`` / ``"osdl"``, or None for the first of them that serves the code; ``.family`` is the
    prefix that was picked.  ``capacity``: the frames the OSD buffers hold (None: B); the OSD stage and the merge run on
    min(count, capacity) frames, ``count`` stays the number of syndrome failures.  ``perm`` and ``parity`` are in the
    family's layouts (``Decoder._osd_layout``).  Without ``osd_order`` this is the NMS-only pipeline, on any code."""

    def __init__(self, dec: Decoder, B: int, T: int, alpha, osd_order=None, osd_algo=_lib.OSD_CONVENTIONAL, snr_db=0.0,
                 family=None, capacity=None, merge=True, want_soft=True, w_in=1.0, w_out=1.0, **osd_kw):
        self.dec, self.B, self.T = dec, int(B), int(T)
        e = dec.empty
        self.soft = e((B, dec.n), torch.float32) if want_soft else None
        self.hard = e((B, dec.words), torch.int64)
        self.fail = e((B,), torch.uint8)
        self._counts = torch.zeros(12, dtype=torch.int64, device=dec.device)   # one buffer: no torch op to gather them
        self.nms_counts, self.osd_counts, self.final_counts = self._counts[:5], self._counts[5:8], self._counts[8:]
        self._alpha = np.ascontiguousarray(np.broadcast_to(np.asarray(alpha, dtype=np.float32), (max(T, 1),)))
        p = _lib.FamilyPipeline()
        p.B, p.T, p.nms_kernel = self.B, self.T, _lib.NMS_AUTO
        p.alpha = self._alpha.ctypes.data_as(C.POINTER(C.c_float))
        p.w_in, p.w_out = float(w_in), float(w_out)
        p.d_soft = self.soft.data_ptr() if want_soft else None
        p.d_hard, p.d_fail = self.hard.data_ptr(), self.fail.data_ptr()
        p.d_nms_counts = self.nms_counts.data_ptr()
        p.osd_enable, p.timing_slot = int(osd_order is not None), -1
        self.osd_order, self.family, self.capacity = osd_order, None, None
        if osd_order is not None:
            if family is not None and family not in _lib.OSD_FAMILIES:
                raise ValueError(f"family {family!r}: expected one of {sorted(_lib.OSD_FAMILIES)} or None")
            self.family = family if family is not None else dec.osd_family()
            self.capacity = cap = self.B if capacity is None else int(capacity)
            pdt, ptail, qtail, _ = dec._osd_layout(self.family)
            self.index, self.count = e((B,), torch.int32), e((1,), torch.int32)
            self.perm, self.parity = e((cap,) + ptail, pdt), e((cap,) + qtail, torch.int64)
            self.cw, self.metric = e((cap, dec.words), torch.int64), e((cap,), torch.float32)
            self.best, self.ntep = e((cap,), torch.int32), e((cap,), torch.int32)
            self.aux = torch.zeros((cap, 4), dtype=torch.int32, device=dec.device) if osd_algo == _lib.OSD_PB else None
            p.osd = dec.osd_params(osd_order, osd_algo, snr_db=snr_db, aux=self.aux, **osd_kw)
            p.family = _lib.OSD_FAMILY_AUTO if family is None else _lib.OSD_FAMILIES[family]
            p.merge, p.osd_capacity = int(bool(merge)), cap
            p.d_index, p.d_count = self.index.data_ptr(), self.count.data_ptr()
            p.d_perm, p.d_parity = self.perm.data_ptr(), self.parity.data_ptr()
            p.d_cw, p.d_metric = self.cw.data_ptr(), self.metric.data_ptr()
            p.d_best, p.d_ntep = self.best.data_ptr(), self.ntep.data_ptr()
            p.d_osd_counts, p.d_final_counts = self.osd_counts.data_ptr(), self.final_counts.data_ptr()
        self._p = p
        self._y = self._labels = None

    bind = BatchPipeline.bind
    timing = BatchPipeline.timing
    reset_counters = BatchPipeline.reset_counters

    def run(self, timing_slot=-1):
        if self._y is None:
            raise RuntimeError("bind() a batch first")
        self._p.timing_slot = int(timing_slot)
        _lib.check(self.dec.L.ldpc_family_pipeline_run(self.dec._ctx, C.byref(self._p), self.dec._stream()), "ldpc_family_pipeline_run")

    def counters(self):
        """int64[12]: the eight of ``BatchPipeline.counters``, then the merge's {merged, merged_wrong, bit_err_after,
        bit_err_before}.  End-to-end bit errors: counters[2] - counters[11] + counters[10]."""
        return self._counts


class DlOsdPipeline:
    """``FamilyPipeline``'s counterpart for the DL-OSD stage (``ldpc_dlosd_pipeline_run``): NMS, counters, compaction, then on the
    failures the trajectory rows and the bit-wise CNN (with ``cnn_weights``), the H-form front end, the sliding-window scan
    with its early stop, the stage counters and the merge into ``hard`` -- one host call, nothing read back in between.

    ``teps`` [Nt,4] u8 and ``block_off`` [nblk+1] int32 are device tensors as ``Decoder.hosd_sliding`` takes them;
    ``fcn_weights`` / ``cnn_weights`` are the packed f32 vectors of ``hosd_sliding`` / ``dia_cnn`` (None: no CNN, the ordering
    values are the channel values and ``rows`` / ``order_llr`` are not allocated).  ``family``: ``"hosd"`` / ``"hosdx"`` /
    ``"hosdw"`` / ``"hosdl"``, or None for what ``Decoder.hosd_stage_family()`` picks; ``.family`` is the prefix that was
    picked.  ``lri`` / ``uidx`` / ``M`` are in that family's layouts.  With ``teps=None`` the stage is off: the NMS-only pipeline,
    on any code (``family`` is then None).

    ``capacity``: the rows every list buffer holds (None: B); the stage and the merge run on min(count, capacity) frames and
    ``count`` stays the number of syndrome failures.  With a CNN the capacity decides the memory: ``rows`` alone is
    capacity x (T+1) x n floats -- at B = 131 072 frames of (128,64) and T = 12 that is 872 MB for capacity = B against 6.7 MB
    for the 1 000 rows that a 0.5 % failure rate needs with a margin, so size it from the failure rate and watch
    counters()[5] < counters()[4], which says that frames were left out."""

    def __init__(self, dec: Decoder, B: int, T: int, alpha, teps, block_off, win, soft_margin, fcn_weights, cnn_weights=None,
                 family=None, capacity=None, merge=True, want_soft=True, w_in=1.0, w_out=1.0, group=0):
        self.dec, self.B, self.T = dec, int(B), int(T)
        e = dec.empty
        self.soft = e((B, dec.n), torch.float32) if want_soft else None
        self.hard = e((B, dec.words), torch.int64)
        self.fail = e((B,), torch.uint8)
        self._counts = torch.zeros(15, dtype=torch.int64, device=dec.device)   # one buffer: no torch op to gather them
        self.nms_counts, self.dl_counts, self.final_counts = self._counts[:5], self._counts[5:11], self._counts[11:]
        self._alpha = np.ascontiguousarray(np.broadcast_to(np.asarray(alpha, dtype=np.float32), (max(T, 1),)))
        self.stage = teps is not None
        self.family = self.capacity = None
        if self.stage:
            if family is not None and family not in _lib.HOSD_FAMILIES:
                raise ValueError(f"family {family!r}: expected one of {sorted(_lib.HOSD_FAMILIES)} or None")
            if family is not None:
                self.family = family
            else:       # LDPC_HOSD_FAMILY_AUTO: hosd_stage_family() on every code a family serves; on a code none serves the
                        # library ends at the last family it tries, hosdl (the method names hosdw there: both refuse the code)
                self.family = "hosdl" if not (dec.hosdx_supported or dec.hosdw_supported) else dec.hosd_stage_family()
            dec._chk(teps, torch.uint8, (4,), "teps")
            if block_off.dtype != torch.int32 or block_off.device != dec.device or block_off.dim() != 1 or block_off.numel() < 1:
                raise ValueError("block_off: expected a 1-D int32 tensor [nblk+1] on the device")
            self.teps, self.block_off, self.win = teps, block_off, int(win)
            self._fcn = np.ascontiguousarray(np.asarray(fcn_weights, dtype=np.float32).reshape(-1))
            self._cnn = None if cnn_weights is None else np.ascontiguousarray(np.asarray(cnn_weights, dtype=np.float32).reshape(-1))
            self.capacity = cap = self.B if capacity is None else int(capacity)
            rows = max(cap, 1)
            if self.family == "hosdl":
                itail, mtail = dec._hosdl_layout()
                idt = torch.int16
            else:
                itail, mtail, idt = (128,), (128 if self.family == "hosdw" else 64,), torch.uint8
            self.index, self.count = e((B,), torch.int32), e((1,), torch.int32)
            self.rows = e((rows, T + 1, dec.n), torch.float32) if self._cnn is not None else None
            self.order_llr = e((rows, dec.n), torch.float32) if self._cnn is not None else None
            self.metric_llr, self.list_labels = e((rows, dec.n), torch.float32), e((rows, dec.words), torch.int64)
            self.lri, self.uidx, self.M = e((rows,) + itail, idt), e((rows,) + itail, idt), e((rows,) + mtail, torch.int64)
            self.nswaps, self.deep_limit = e((rows,), torch.int32), e((rows,), torch.int32)
            self.global_min, self.truth, self.success = e((rows,), torch.float32), e((rows,), torch.float32), e((rows,), torch.bool)
            self.cw, self.metric = e((rows, dec.words), torch.int64), e((rows,), torch.float32)
            self.best, self.teps_evaluated = e((rows,), torch.int32), e((rows,), torch.int32)
        p = _lib.DlOsdPipeline()
        p.B, p.T, p.nms_kernel = self.B, self.T, _lib.NMS_AUTO
        p.alpha = self._alpha.ctypes.data_as(C.POINTER(C.c_float))
        p.w_in, p.w_out = float(w_in), float(w_out)
        p.d_soft = self.soft.data_ptr() if want_soft else None
        p.d_hard, p.d_fail = self.hard.data_ptr(), self.fail.data_ptr()
        p.d_nms_counts = self.nms_counts.data_ptr()
        p.osd_enable, p.timing_slot = int(self.stage), -1
        if self.stage:
            p.family = _lib.HOSD_FAMILY_AUTO if family is None else _lib.HOSD_FAMILIES[family]
            p.merge, p.osd_capacity = int(bool(merge)), cap
            p.d_index, p.d_count = self.index.data_ptr(), self.count.data_ptr()
            if self._cnn is not None:
                p.cnn_weights, p.n_cnn_weights = self._cnn.ctypes.data_as(C.POINTER(C.c_float)), self._cnn.size
                p.d_rows, p.d_order_llr = self.rows.data_ptr(), self.order_llr.data_ptr()
            p.fcn_weights, p.n_fcn_weights = self._fcn.ctypes.data_as(C.POINTER(C.c_float)), self._fcn.size
            p.d_teps, p.d_block_off = teps.data_ptr(), block_off.data_ptr()
            p.nblk, p.win, p.group, p.soft_margin = block_off.numel() - 1, self.win, int(group), float(soft_margin)
            p.d_metric_llr, p.d_list_labels = self.metric_llr.data_ptr(), self.list_labels.data_ptr()
            p.d_lri, p.d_uidx, p.d_M, p.d_nswaps = self.lri.data_ptr(), self.uidx.data_ptr(), self.M.data_ptr(), self.nswaps.data_ptr()
            p.d_deep_limit, p.d_global_min = self.deep_limit.data_ptr(), self.global_min.data_ptr()
            p.d_truth, p.d_success = self.truth.data_ptr(), self.success.data_ptr()
            p.d_cw, p.d_metric = self.cw.data_ptr(), self.metric.data_ptr()
            p.d_best, p.d_teps_evaluated = self.best.data_ptr(), self.teps_evaluated.data_ptr()
            p.d_dl_counts, p.d_final_counts = self.dl_counts.data_ptr(), self.final_counts.data_ptr()
        self._p = p
        self._y = self._labels = None

    bind = BatchPipeline.bind
    timing = BatchPipeline.timing
    reset_counters = BatchPipeline.reset_counters

    def run(self, timing_slot=-1):
        if self._y is None:
            raise RuntimeError("bind() a batch first")
        self._p.timing_slot = int(timing_slot)
        _lib.check(self.dec.L.ldpc_dlosd_pipeline_run(self.dec._ctx, C.byref(self._p), self.dec._stream()), "ldpc_dlosd_pipeline_run")

    def counters(self):
        """int64[15]: the five NMS counters of ``BatchPipeline.counters``; the stage's {frames, success (global_min == truth),
        failure, windows (sum of deep_limit - win + 1), complexity (sum of block_off[deep_limit]), teps evaluated}; the merge's
        {merged, merged_wrong, bit_err_after, bit_err_before}.  End-to-end bit errors: counters[2] - counters[14] +
        counters[13]; end-to-end frame errors: counters[3] + counters[12]."""
        return self._counts
