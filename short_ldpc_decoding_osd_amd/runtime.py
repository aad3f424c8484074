"""Device runtime: a thin object around ``ldpc_ctx`` that takes torch tensors as device
buffers and hands their pointers to the C ABI (include/ldpc_osd.h).  PyTorch is plumbing
here (allocation, streams, torch.distributed) -- all arithmetic happens in the HIP kernels.

Packed bit words are carried as ``torch.int64`` tensors (bit v of a frame = bit v%64 of
word v//64); view them as uint64 on the NumPy side.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .fill_matrix_info import Code

COUNT_NAMES = ("frames", "frame_err", "bit_err", "undetected", "synd_fail")


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Decoder:
    """One per (code, GPU).  Every method is asynchronous on torch's current stream."""

    def __init__(self, code: Code | None = None, device=None):
        self.L = _lib.load()
        self.code = code if code is not None else Code()
        if not torch.cuda.is_available():
            raise _lib.LdpcError("no GPU visible to torch: the decoder has no CPU path")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else
                                   (device.index if isinstance(device, torch.device) else int(device)))
        self._ctx = C.c_void_p()
        _lib.check(self.L.ldpc_ctx_create(self.code._handle, self.device.index, C.byref(self._ctx)), "ldpc_ctx_create")
        self.n = self.code.check_matrix_column
        self.m = self.code.check_matrix_row
        self.k = self.code.k
        self.words = (self.n + 63) // 64
        self.nms_kernel = self.L.ldpc_ctx_nms_kernel(self._ctx)

    def __del__(self):
        ctx = getattr(self, "_ctx", None)
        if ctx is not None and ctx.value:
            self.L.ldpc_ctx_destroy(ctx)
            ctx.value = None

    # ------------------------------------------------------------------ helpers
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _chk(self, t, dtype, shape_tail, name):
        if not isinstance(t, torch.Tensor) or t.device != self.device:
            raise ValueError(f"{name}: expected a tensor on {self.device}")
        if t.dtype != dtype or not t.is_contiguous():
            raise ValueError(f"{name}: expected contiguous {dtype}, got {t.dtype} contiguous={t.is_contiguous()}")
        if tuple(t.shape[1:]) != tuple(shape_tail):
            raise ValueError(f"{name}: expected shape [*, {shape_tail}], got {tuple(t.shape)}")
        return t

    def empty(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.device)

    def _outputs(self, out, table):
        """``out`` (dict or None) as a dict with every key of ``table`` (name -> (shape, dtype, want)): a wanted output
        that is missing or None is allocated, one neither wanted nor given is None."""
        out = dict(out or {})
        for k, (shape, dtype, want) in table.items():
            if want and out.get(k) is None:
                out[k] = self.empty(shape, dtype)
            out.setdefault(k, None)
        return out

    def _osd_outputs(self, out, F):
        return self._outputs(out, {"cw": ((F, self.words), torch.int64, True), "metric": ((F,), torch.float32, True),
                                   "best": ((F,), torch.int32, True), "ntep": ((F,), torch.int32, True)})

    def _osd_frames(self, y, index, F):
        """The F rule of the calls that start from channel values: the frame list's length, else y's."""
        self._chk(y, torch.float32, (self.n,), "y")
        return (index.shape[0] if index is not None else y.shape[0]) if F is None else F

    # An OSD family is the prefix of its methods and library functions (``osd``: the (128,64) kernels, ``osdx``: any shape,
    # ``osdw``: high rate, ``osdl``: long / low rate) with the int64 words of a ``parity`` row and the shape tail of a
    # ``tep_eval`` mask.  ``osdl`` sizes its layouts by the code (``_osd_layout``).
    _OSD_PARITY_WORDS = {"osd": 64, "osdx": 64, "osdw": 128}
    _OSD_MASK_TAIL = {"osd": (), "osdx": (), "osdw": (2,)}

    def _osd_layout(self, fam):
        """(dtype of ``perm``, shape tail of ``perm``, shape tail of ``parity``, shape tail of a ``tep_eval`` mask) of the family
        on this code.  ``osdl``: perm [*, 64 ceil(n/64)] int16 (the library's u16), parity [*, 64 ceil(k/64)] int64 with one
        word per row, or [*, 64 ceil(k/64), ceil((n-k)/64)] with more, mask [*, ceil(k/64)]."""
        if fam != "osdl":
            return torch.uint8, (128,), (self._OSD_PARITY_WORDS[fam],), self._OSD_MASK_TAIL[fam]
        w, wp = (self.k + 63) // 64, (self.n - self.k + 63) // 64
        return torch.int16, (64 * self.words,), ((64 * w,) if wp == 1 else (64 * w, wp)), (w,)

    def _osd_call(self, fam, op, *args):
        """``ldpc_<fam>_<op>(ctx, *args, stream)``, checked."""
        name = f"ldpc_{fam}_{op}"
        _lib.check(getattr(self.L, name)(self._ctx, *args, self._stream()), name)

    def _osd_front_results(self, fam, y, perm, parity, F=None):
        """The checks of the calls that take front-end results (perm and parity in the layouts of ``_osd_layout``).  Returns F."""
        self._chk(y, torch.float32, (self.n,), "y")
        pdt, ptail, qtail, _ = self._osd_layout(fam)
        self._chk(perm, pdt, ptail, "perm")
        self._chk(parity, torch.int64, qtail, "parity")
        return perm.shape[0] if F is None else F

    def _osd_front(self, fam, y, index, count, F, out):
        """``<fam>_front``."""
        F = self._osd_frames(y, index, F)
        if out is not None:
            perm, parity, ns = out
        else:
            pdt, ptail, qtail, _ = self._osd_layout(fam)
            perm = self.empty((F,) + ptail, pdt)
            parity = self.empty((F,) + qtail, torch.int64)
            ns = self.empty((F,), torch.int32)
        self._osd_call(fam, "front", _ptr(y), _ptr(index), _ptr(count), F, _ptr(perm), _ptr(parity), _ptr(ns))
        return perm, parity, ns

    def _osd_tep_eval(self, fam, y, perm, parity, mask, index, count):
        """``<fam>_tep_eval``.  The kernel reads a mask row for every frame, so a shorter mask is refused here."""
        F = self._osd_front_results(fam, y, perm, parity)
        self._chk(mask, torch.int64, self._osd_layout(fam)[3], "mask")
        if mask.shape[0] < F:
            raise ValueError(f"mask: {mask.shape[0]} rows for {F} frames")
        out = dict(cw=self.empty((F, self.words), torch.int64), metric=self.empty((F,), torch.float32), hd=self.empty((F,), torch.int32))
        self._osd_call(fam, "tep_eval", _ptr(y), _ptr(index), _ptr(count), F, _ptr(perm), _ptr(parity), _ptr(mask), _ptr(out["cw"]),
                       _ptr(out["metric"]), _ptr(out["hd"]))
        return out

    def _osd_search(self, fam, op, y, perm, parity, arg, index, count, F, out):
        """``<fam>_<op>`` for the ``*search`` calls: a scan on front-end results.  ``arg``: the order, or the params by
        reference, as the library function takes it."""
        F = self._osd_front_results(fam, y, perm, parity, F)
        out = self._osd_outputs(out, F)
        self._osd_call(fam, op, _ptr(y), _ptr(index), _ptr(count), F, _ptr(perm), _ptr(parity), arg, _ptr(out["cw"]),
                       _ptr(out["metric"]), _ptr(out["best"]), _ptr(out["ntep"]))
        return out

    def _osd_decode(self, fam, op, y, arg, index, count, F, perm, parity, label_bits, counts, out):
        """``<fam>_<op>`` for the ``*decode`` calls: front end + scan through ``perm`` / ``parity``, which are checked when
        given, allocated when not, and returned in the dict.  F by the rule of ``_osd_frames``; ``arg`` as in ``_osd_search``."""
        F = self._osd_frames(y, index, F)
        pdt, ptail, qtail, _ = self._osd_layout(fam)
        perm = self.empty((F,) + ptail, pdt) if perm is None else self._chk(perm, pdt, ptail, "perm")
        parity = self.empty((F,) + qtail, torch.int64) if parity is None else self._chk(parity, torch.int64, qtail, "parity")
        out = self._osd_outputs(out, F)
        self._osd_call(fam, op, _ptr(y), _ptr(index), _ptr(count), F, arg, _ptr(perm), _ptr(parity), _ptr(out["cw"]),
                       _ptr(out["metric"]), _ptr(out["best"]), _ptr(out["ntep"]), _ptr(label_bits), _ptr(counts))
        out["perm"], out["parity"] = perm, parity
        return out

    def _hosd_args(self, order_llr, metric_llr, front, teps, block_off):
        """The checks hosd_search and hosd_sliding share.  Returns (lri, uidx, M, F, nblk)."""
        self._chk(order_llr, torch.float32, (self.n,), "order_llr")
        self._chk(metric_llr, torch.float32, (self.n,), "metric_llr")
        lri, uidx, M = front[:3]
        F = order_llr.shape[0]
        if metric_llr.shape[0] != F or lri.shape[0] != F:
            raise ValueError("order_llr, metric_llr and the front-end results must hold the same frames")
        self._chk(teps, torch.uint8, (4,), "teps")
        if block_off.dtype != torch.int32 or block_off.device != self.device or block_off.dim() != 1 or block_off.numel() < 1:
            raise ValueError("block_off: expected a 1-D int32 tensor [nblk+1] on the device")
        return lri, uidx, M, F, block_off.numel() - 1

    # ------------------------------------------------------------------ NMS
    def nms(self, llr, T, alpha, w_in=1.0, w_out=1.0, want_soft=True, want_traj=False, want_hard=True,
            want_fail=True, kernel=_lib.NMS_AUTO, out=None):
        """Normalised min-sum, T fixed iterations.  Returns dict(soft, traj, hard, fail) of
        tensors (None for outputs not requested).  ``out`` may carry preallocated tensors."""
        self._chk(llr, torch.float32, (self.n,), "llr")
        B = llr.shape[0]
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(alpha, dtype=np.float32), (max(T, 1),)))
        out = self._outputs(out, {"soft": ((B, self.n), torch.float32, want_soft), "traj": ((T, B, self.n), torch.float32, want_traj),
                                  "hard": ((B, self.words), torch.int64, want_hard), "fail": ((B,), torch.uint8, want_fail)})
        _lib.check(self.L.ldpc_nms_decode(self._ctx, _ptr(llr), B, T, a.ctypes.data_as(C.POINTER(C.c_float)),
                                          float(w_in), float(w_out), _ptr(out["soft"]), _ptr(out["traj"]),
                                          _ptr(out["hard"]), _ptr(out["fail"]), int(kernel), self._stream()),
                   "ldpc_nms_decode")
        return out

    def nms_traj_rows(self, llr, index, count, F, T, alpha, w_in=1.0, w_out=1.0, kernel=_lib.NMS_AUTO, out=None):
        """Rows of the listed frames only (collect_failed_output_selective, ms_test.py:55-64): [F, T+1, n] f32, row 0 the
        channel values, row t the posterior after iteration t.  ``index`` / ``count``: the list as ``compact`` wrote it;
        ``F``: how many rows to allocate for (the launch decodes min(count, F) frames)."""
        self._chk(llr, torch.float32, (self.n,), "llr")
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(alpha, dtype=np.float32), (max(T, 1),)))
        rows = out if out is not None else self.empty((max(int(F), 1), T + 1, self.n), torch.float32)
        _lib.check(self.L.ldpc_nms_traj_rows(self._ctx, _ptr(llr), _ptr(index), _ptr(count), int(F), T,
                                             a.ctypes.data_as(C.POINTER(C.c_float)), float(w_in), float(w_out), _ptr(rows),
                                             int(kernel), self._stream()), "ldpc_nms_traj_rows")
        return rows

    def nms_grad(self, llr, label_bits, T, alpha, w_in=1.0, w_out=1.0, want_loss=True, want_grad=True, want_sums=True,
                 want_traj=False, want_hard=False, want_fail=False, out=None):
        """Training step of NMS (ldpc_nms_train_grad): loss of Decoding_model (ms_decoder_dense.py:210-215) and its
        gradient with respect to the effective factors, forward and backward in one launch.  ``label_bits``: packed code
        bits [B, words] int64 (``pack_bits``).  Returns dict(loss [B] f32, grad [B, T+2] f32 = dL/dalpha_0..T-1,
        dL/dw_in, dL/dw_out, loss_sum [1] f64, grad_sum [T+2] f64, traj [T, B, n], hard, fail) -- None where not asked
        for; ``traj`` / ``hard`` / ``fail`` are ``nms``'s, bit for bit."""
        self._chk(llr, torch.float32, (self.n,), "llr")
        self._chk(label_bits, torch.int64, (self.words,), "label_bits")
        B = llr.shape[0]
        if label_bits.shape[0] != B:
            raise ValueError(f"label_bits: {label_bits.shape[0]} frames for {B} channel frames")
        a = np.asarray(alpha, dtype=np.float32)
        a = np.ascontiguousarray(np.broadcast_to(a, (max(T, 1),)) if T > 0 else np.zeros(1, np.float32))
        out = self._outputs(out, {"loss": ((B,), torch.float32, want_loss), "grad": ((B, T + 2), torch.float32, want_grad),
                                  "loss_sum": ((1,), torch.float64, want_sums), "grad_sum": ((T + 2,), torch.float64, want_sums),
                                  "traj": ((T, B, self.n), torch.float32, want_traj), "hard": ((B, self.words), torch.int64, want_hard),
                                  "fail": ((B,), torch.uint8, want_fail)})
        _lib.check(self.L.ldpc_nms_train_grad(self._ctx, _ptr(llr), _ptr(label_bits), B, T, a.ctypes.data_as(C.POINTER(C.c_float)),
                                              float(w_in), float(w_out), _ptr(out["loss"]), _ptr(out["grad"]),
                                              _ptr(out["loss_sum"]), _ptr(out["grad_sum"]), _ptr(out["traj"]),
                                              _ptr(out["hard"]), _ptr(out["fail"]), self._stream()), "ldpc_nms_train_grad")
        return out

    # ------------------------------------------------------------------ statistics / plumbing kernels
    def eval_counts(self, hard, label_bits, fail=None, counts=None):
        """counts[5] += {frames, frame_err, bit_err, undetected, synd_fail} (int64 tensor)."""
        self._chk(hard, torch.int64, (self.words,), "hard")
        self._chk(label_bits, torch.int64, (self.words,), "label_bits")
        if counts is None:
            counts = torch.zeros(5, dtype=torch.int64, device=self.device)
        _lib.check(self.L.ldpc_eval_counts(self._ctx, _ptr(hard), _ptr(label_bits), _ptr(fail), hard.shape[0],
                                           _ptr(counts), self._stream()), "ldpc_eval_counts")
        return counts

    def compact(self, flag, index=None, count=None):
        """Ascending indices of the non-zero flags.  Returns (index[B] int32, count[1] int32)."""
        self._chk(flag, torch.uint8, (), "flag")
        B = flag.shape[0]
        if index is None:
            index = self.empty((max(B, 1),), torch.int32)
        if count is None:
            count = self.empty((1,), torch.int32)
        _lib.check(self.L.ldpc_compact(self._ctx, _ptr(flag), B, _ptr(index), _ptr(count), self._stream()),
                   "ldpc_compact")
        return index, count

    def pack_bits(self, bits):
        """[B, n] 0/1 tensor (uint8 / int32 / int64) -> [B, words] packed int64."""
        es = {torch.uint8: 1, torch.int32: 4, torch.int64: 8}.get(bits.dtype)
        if es is None:
            raise ValueError(f"pack_bits: unsupported dtype {bits.dtype}")
        self._chk(bits, bits.dtype, (self.n,), "bits")
        words = self.empty((bits.shape[0], self.words), torch.int64)
        _lib.check(self.L.ldpc_pack_bits(self._ctx, _ptr(bits), es, bits.shape[0], _ptr(words), self._stream()),
                   "ldpc_pack_bits")
        return words

    def unpack_bits(self, words, dtype=torch.int64):
        es = {torch.uint8: 1, torch.int32: 4, torch.int64: 8}[dtype]
        self._chk(words, torch.int64, (self.words,), "words")
        bits = self.empty((words.shape[0], self.n), dtype)
        _lib.check(self.L.ldpc_unpack_bits(self._ctx, _ptr(words), words.shape[0], _ptr(bits), es, self._stream()),
                   "ldpc_unpack_bits")
        return bits

    # ------------------------------------------------------------------ frame generator
    def gen_sigma(self, snr_db):
        """sigma = sqrt(1 / (2 (k/n) 10^(snr/10))), as the reference computes it (data_generating.py:17)."""
        return float(np.sqrt(1. / (2 * (float(self.k) / float(self.n)) * 10 ** (snr_db / 10))))

    def gen_frames(self, B, *, seed, snr_db=None, sigma=None, mean=1.0, frame0=0, all_zeros=False, rayleigh=False, fade_len=16,
                   want_y=True, want_labels=True, out=None):
        """Frames ``frame0 .. frame0 + B - 1`` of the set ``seed`` (ldpc_gen_frames): random message . G, BPSK 0 -> +1,
        ``mean + sigma z`` (AWGN) or ``mean a + sigma z`` (``rayleigh``: one amplitude per ``fade_len`` consecutive samples
        of the set), in one launch.  Exactly one of ``snr_db`` (-> ``gen_sigma``) and ``sigma`` is given.  Frame i is a pure
        function of (seed, frame0 + i, the channel parameters): any split of a set into calls gives the same bits.
        Returns ``(y [B, n] f32, label_bits [B, words] int64)``; an output that is switched off is None and its buffer in
        ``out`` (dict: ``y``, ``label_bits``), if any, is not touched.  ``all_zeros``: zero labels, ``y`` unsigned."""
        if (snr_db is None) == (sigma is None):
            raise ValueError("gen_frames: give exactly one of snr_db and sigma")
        sigma = self.gen_sigma(snr_db) if sigma is None else float(sigma)
        B = int(B)
        out = self._outputs(out, {"y": ((B, self.n), torch.float32, want_y), "label_bits": ((B, self.words), torch.int64, want_labels)})
        y = self._chk(out["y"], torch.float32, (self.n,), "y") if want_y else None
        lab = self._chk(out["label_bits"], torch.int64, (self.words,), "label_bits") if want_labels else None
        for t, name in ((y, "y"), (lab, "label_bits")):
            if t is not None and t.shape[0] < B:
                raise ValueError(f"gen_frames: {name} holds {t.shape[0]} frames, {B} asked for")
        p = _lib.GenParams(int(seed) & 0xFFFFFFFFFFFFFFFF, int(frame0), sigma, float(mean),
                           (_lib.GEN_F_ALL_ZEROS if all_zeros else 0) | (_lib.GEN_F_RAYLEIGH if rayleigh else 0), int(fade_len))
        _lib.check(self.L.ldpc_gen_frames(self._ctx, C.byref(p), B, _ptr(y), _ptr(lab), self._stream()), "ldpc_gen_frames")
        return y, lab

    # ------------------------------------------------------------------ OSD
    def osd_reserve(self, max_frames):
        """Pre-size the OSD workspace (needed before capturing decode calls into a graph)."""
        _lib.check(self.L.ldpc_osd_reserve(self._ctx, int(max_frames)), "ldpc_osd_reserve")

    def osd_reserve_stream(self, max_frames, params=None):
        """Pre-size the OSD workspace of the CURRENT stream (instead of one eager call on it before a capture).
        ``params`` (osd_params(...)): also size what that search needs (PB-OSD lists and tables)."""
        _lib.check(self.L.ldpc_osd_reserve_stream(self._ctx, int(max_frames), C.byref(params) if params is not None else None,
                                                  self._stream()), "ldpc_osd_reserve_stream")

    def osd_release_stream(self, stream=None):
        """Free the OSD workspace of ``stream`` (default: the current stream).  The stream must be idle and graphs
        captured on it must not be replayed afterwards (include/ldpc_osd.h, 'Captured graphs')."""
        st = self._stream() if stream is None else C.c_void_p(stream.cuda_stream)
        _lib.check(self.L.ldpc_osd_release_stream(self._ctx, st), "ldpc_osd_release_stream")

    def pb_tuning(self):
        """The context's PB-OSD tuning (hand-over budgets, chunk targets) as a dict; see include/ldpc_osd.h."""
        t = _lib.PbTuning()
        _lib.check(self.L.ldpc_ctx_get_pb_tuning(self._ctx, C.byref(t)), "ldpc_ctx_get_pb_tuning")
        return {n: int(getattr(t, n)) for n, _ in _lib.PbTuning._fields_}

    def set_pb_tuning(self, **fields):
        """Change PB-OSD tuning fields of the context (no field: back to the defaults).  Results do not depend on them;
        applies to calls issued afterwards.  Returns the previous setting (a dict that can be passed back)."""
        prev = self.pb_tuning()
        if not fields:
            _lib.check(self.L.ldpc_ctx_set_pb_tuning(self._ctx, None), "ldpc_ctx_set_pb_tuning")
            return prev
        unknown = set(fields) - set(prev)
        if unknown:
            raise ValueError(f"unknown PB-OSD tuning field(s): {sorted(unknown)}")
        t = _lib.PbTuning(**{**prev, **{k: int(v) for k, v in fields.items()}})
        _lib.check(self.L.ldpc_ctx_set_pb_tuning(self._ctx, C.byref(t)), "ldpc_ctx_set_pb_tuning")
        return prev

    def osd_index_errors(self):
        """Out-of-range frame-list entries met by calls that carried ``y_frames`` (synchronises the device)."""
        n = C.c_int64(0)
        _lib.check(self.L.ldpc_osd_index_errors(self._ctx, C.byref(n)), "ldpc_osd_index_errors")
        return int(n.value)

    def osd_ge(self, rows):
        """Device GF(2) elimination of [F,64,2] packed matrices -> (reduced, swaps[F,64,2] u8, nswaps[F])."""
        self._chk(rows, torch.int64, (64, 2), "rows")
        F = rows.shape[0]
        red = self.empty((F, 64, 2), torch.int64)
        swaps = torch.zeros((F, 64, 2), dtype=torch.uint8, device=self.device)
        ns = self.empty((F,), torch.int32)
        _lib.check(self.L.ldpc_osd_ge(self._ctx, _ptr(rows), F, _ptr(red), _ptr(swaps), _ptr(ns), self._stream()),
                   "ldpc_osd_ge")
        return red, swaps, ns

    def osd_front(self, y, index=None, count=None, F=None, out=None):
        """Reliability sort + elimination + MRB bookkeeping.  Returns (perm[F,128] u8,
        parity[F,64] int64 rows of P', nswaps[F] int32); ``out`` may carry those three preallocated."""
        return self._osd_front("osd", y, index, count, F, out)

    def osd_params(self, order, algo=_lib.OSD_CONVENTIONAL, snr_db=0.0, fs_beta=0.1, fs_tau_e=6.5, fs_tau_psc=30.0,
                   fs_reference_quirk=1, aux=None, table_scan=False, pb_path=None, readlane_scan=False, y_frames=0,
                   pb_front_inside=False):
        """aux: optional int32 tensor [F,4] receiving the PB-OSD per-frame statistics;
        table_scan: use the table-driven conventional kernel also for order 2 (cross-check path);
        pb_path: None = staged PB-OSD kernels, "block" = every frame through the sorted-chunk kernel from its
        first TEP, "replay" = every frame through the literal list replay (cross-check paths);
        readlane_scan: conventional order 2 through the first register-resident kernel (triangular pairing by
        v_readlane) instead of the rotation-paired persistent one (cross-check path);
        y_frames: debug bound for caller-made frame lists (0 = off): entries of ``index`` outside [0, y_frames) are
        replaced by 0 and counted (``osd_index_errors``);
        pb_front_inside: PB-OSD through ``osd_decode`` with the front end inside the first PB kernel (nothing goes through a
        workspace: 43 % less HBM traffic for front end + head, 4-5 % more time).
        The keywords only set ``flags``; the library validates the combination (LdpcError)."""
        flags = ((_lib.OSD_F_TABLE_SCAN if table_scan else 0) | (_lib.OSD_F_READLANE_SCAN if readlane_scan else 0) |
                 {None: 0, "block": _lib.OSD_F_PB_BLOCK, "replay": _lib.OSD_F_PB_REPLAY}[pb_path] |
                 (_lib.OSD_F_PB_FRONT_INSIDE if pb_front_inside else 0))
        return _lib.OsdParams(int(order), int(algo), float(snr_db), float(fs_beta), float(fs_tau_e),
                              float(fs_tau_psc), int(fs_reference_quirk), flags,
                              aux.data_ptr() if aux is not None else None, int(y_frames))

    def osd_decode(self, y, order, algo=_lib.OSD_CONVENTIONAL, index=None, count=None, F=None, params=None, out=None):
        """OSD of the frames y[index[f]] (or y[f]).  Returns dict(cw[F,2] int64 original bit
        order, metric[F] f32, best[F] i32, ntep[F] i32)."""
        F = self._osd_frames(y, index, F)
        p = params if params is not None else self.osd_params(order, algo)
        out = self._osd_outputs(out, F)
        _lib.check(self.L.ldpc_osd_decode(self._ctx, _ptr(y), _ptr(index), _ptr(count), F, C.byref(p), _ptr(out["cw"]),
                                          _ptr(out["metric"]), _ptr(out["best"]), _ptr(out["ntep"]), self._stream()),
                   "ldpc_osd_decode")
        return out

    def osd_search(self, y, perm, parity, params, index=None, count=None, F=None, out=None):
        """Search only, on caller-supplied front-end results (perm [F,128] u8, parity [F,64] int64)."""
        return self._osd_search("osd", "search", y, perm, parity, C.byref(params), index, count, F, out)

    def osd_tep_eval(self, y, perm, parity, mask, index=None, count=None):
        """One given TEP per frame (mask [F] int64: bit p flips primed MRB position p) on front-end results.
        Returns dict(cw[F,2] int64 original bit order, metric[F] f32, hd[F] i32)."""
        return self._osd_tep_eval("osd", y, perm, parity, mask, index, count)

    # ------------------------------------------------------------------ OSD for short codes of any shape
    @property
    def osdx_supported(self):
        """Whether the ``osdx_*`` methods serve this code (1 <= k <= 64 and 1 <= n-k <= 64)."""
        return bool(self.L.ldpc_osdx_supported(self._ctx))

    def osdx_front(self, y, index=None, count=None, F=None, out=None):
        """``osd_front`` for any supported shape.  Returns (perm[F,128] u8: original bit at primed position p < n, MRB
        first, 0 beyond n; parity[F,64] int64: rows r < k of P', bits c < n-k, 0 elsewhere; nswaps[F] int32); ``out`` may
        carry those three preallocated (nswaps may be None)."""
        return self._osd_front("osdx", y, index, count, F, out)

    def osdx_search(self, y, perm, parity, order, index=None, count=None, F=None, out=None):
        """Conventional order-``order`` search on front-end results (perm [F,128] u8, parity [F,64] int64) of any supported
        shape.  Returns dict(cw[F,words] int64 original bit order, metric[F] f32, best[F] i32, ntep[F] i32)."""
        return self._osd_search("osdx", "search", y, perm, parity, int(order), index, count, F, out)

    def osdx_decode(self, y, order, index=None, count=None, F=None, perm=None, parity=None, label_bits=None, counts=None,
                    out=None):
        """Front end + conventional order-``order`` search of the frames y[index[f]] (or y[f]) for any supported shape, two
        launches through ``perm`` / ``parity`` (allocated when not given; returned in the dict).  With ``label_bits``
        ([*, words] int64, addressed through ``index``) and ``counts`` ([3] int64) the search accumulates
        counts += {frames, frames_wrong, teps_total}."""
        return self._osd_decode("osdx", "decode", y, int(order), index, count, F, perm, parity, label_bits, counts, out)

    # ------------------------------------------------------------------ OSD for high-rate short codes (k up to 127)
    @property
    def osdw_supported(self):
        """Whether the ``osdw_*`` methods serve this code (n <= 128 and 1 <= n-k <= 64)."""
        return bool(self.L.ldpc_osdw_supported(self._ctx))

    def osdw_front(self, y, index=None, count=None, F=None, out=None):
        """``osdx_front`` for every code with n <= 128 and 1 <= n-k <= 64.  Returns (perm[F,128] u8, parity[F,128] int64: rows
        r < k of P', bits c < n-k, 0 elsewhere; nswaps[F] int32); ``out`` may carry those three preallocated (nswaps may be
        None)."""
        return self._osd_front("osdw", y, index, count, F, out)

    def osdw_search(self, y, perm, parity, order, index=None, count=None, F=None, out=None):
        """Conventional order-``order`` search on the results of ``osdw_front`` (perm [F,128] u8, parity [F,128] int64).
        Returns the dict of ``osdx_search``."""
        return self._osd_search("osdw", "search", y, perm, parity, int(order), index, count, F, out)

    def osdw_decode(self, y, order, index=None, count=None, F=None, perm=None, parity=None, label_bits=None, counts=None,
                    out=None):
        """``osdx_decode`` for every code with n <= 128 and 1 <= n-k <= 64: front end + conventional order-``order`` search,
        two launches through ``perm`` [F,128] u8 / ``parity`` [F,128] int64 (allocated when not given; returned in the
        dict); ``label_bits`` / ``counts`` as there."""
        return self._osd_decode("osdw", "decode", y, int(order), index, count, F, perm, parity, label_bits, counts, out)

    def osdw_fs_search(self, y, perm, parity, params, index=None, count=None, F=None, out=None):
        """``osdx_fs_search`` for every code with n <= 128 and 1 <= n-k <= 64, on the results of ``osdw_front`` (perm [F,128]
        u8, parity [F,128] int64).  ``params`` and the returned dict as there."""
        return self._osd_search("osdw", "fs_search", y, perm, parity, C.byref(params), index, count, F, out)

    def osdw_fs_decode(self, y, params, index=None, count=None, F=None, perm=None, parity=None, label_bits=None, counts=None,
                       out=None):
        """``osdx_fs_decode`` for every code with n <= 128 and 1 <= n-k <= 64: ``osdw_decode`` with the search of
        ``osdw_fs_search``; ``perm`` [F,128] u8 / ``parity`` [F,128] int64 / ``label_bits`` / ``counts`` as there."""
        return self._osd_decode("osdw", "fs_decode", y, C.byref(params), index, count, F, perm, parity, label_bits, counts, out)

    def osdw_pb_search(self, y, perm, parity, params, index=None, count=None, F=None, out=None):
        """``osdx_pb_search`` for every code with n <= 128 and 1 <= n-k <= 64, on the results of ``osdw_front`` (perm [F,128]
        u8, parity [F,128] int64).  ``params`` (``osd_params(order, _lib.OSD_PB, snr_db=..., aux=...)``, order 0..min(3, k))
        and the returned dict as there."""
        return self._osd_search("osdw", "pb_search", y, perm, parity, C.byref(params), index, count, F, out)

    def osdw_pb_decode(self, y, params, index=None, count=None, F=None, perm=None, parity=None, label_bits=None, counts=None,
                       out=None):
        """``osdx_pb_decode`` for every code with n <= 128 and 1 <= n-k <= 64: ``osdw_decode`` with the search of
        ``osdw_pb_search``; ``perm`` [F,128] u8 / ``parity`` [F,128] int64 / ``label_bits`` / ``counts`` as there."""
        return self._osd_decode("osdw", "pb_decode", y, C.byref(params), index, count, F, perm, parity, label_bits, counts, out)

    def osdw_tep_eval(self, y, perm, parity, mask, index=None, count=None):
        """``osdx_tep_eval`` for every code with n <= 128 and 1 <= n-k <= 64, on the results of ``osdw_front`` (parity [F,128]
        int64).  mask [F,2] int64: bit p of word 0 flips primed MRB position p, bit p of word 1 position 64 + p; bits at or
        beyond k are ignored.  Returns dict(cw[F,words] int64 original bit order, metric[F] f32, hd[F] i32)."""
        return self._osd_tep_eval("osdw", y, perm, parity, mask, index, count)

    # ------------------------------------------------------------------ OSD for longer and low-rate codes (n <= 384, k, n-k <= 192)
    @property
    def osdl_supported(self):
        """Whether the ``osdl_*`` methods serve this code (n <= 384, 1 <= k <= 192 and 1 <= n-k <= 192)."""
        return bool(self.L.ldpc_osdl_supported(self._ctx))

    def osdl_front(self, y, index=None, count=None, F=None, out=None):
        """``osdx_front`` for every code with n <= 384, 1 <= k <= 192 and 1 <= n-k <= 192.  With S = ceil(n/64), W = ceil(k/64)
        and Wp = ceil((n-k)/64), returns (perm [F, 64 S] int16: original bit at primed position p < n, 0 beyond; parity
        [F, 64 W] int64 for Wp = 1, else [F, 64 W, Wp]: rows r < k of P', bit c of word w = P'[r][64 w + c], 0 elsewhere;
        nswaps [F] int32); ``out`` may carry those three preallocated (nswaps may be None)."""
        return self._osd_front("osdl", y, index, count, F, out)

    def osdl_search(self, y, perm, parity, order, index=None, count=None, F=None, out=None):
        """Conventional order-``order`` search on the results of ``osdl_front``.  Returns the dict of ``osdx_search``."""
        return self._osd_search("osdl", "search", y, perm, parity, int(order), index, count, F, out)

    def osdl_decode(self, y, order, index=None, count=None, F=None, perm=None, parity=None, label_bits=None, counts=None,
                    out=None):
        """``osdx_decode`` for every code with n <= 384, 1 <= k <= 192 and 1 <= n-k <= 192: front end + conventional
        order-``order`` search, two launches through ``perm`` / ``parity`` in the layouts of ``osdl_front`` (allocated when
        not given; returned in the dict); ``label_bits`` / ``counts`` as there."""
        return self._osd_decode("osdl", "decode", y, int(order), index, count, F, perm, parity, label_bits, counts, out)

    def osdl_fs_search(self, y, perm, parity, params, index=None, count=None, F=None, out=None):
        """``osdx_fs_search`` for every code with n <= 384, 1 <= k <= 192 and 1 <= n-k <= 192, on the results of
        ``osdl_front`` (its layouts)."""
        return self._osd_search("osdl", "fs_search", y, perm, parity, C.byref(params), index, count, F, out)

    def osdl_fs_decode(self, y, params, index=None, count=None, F=None, perm=None, parity=None, label_bits=None, counts=None,
                       out=None):
        """``osdx_fs_decode`` for every code with n <= 384, 1 <= k <= 192 and 1 <= n-k <= 192: ``osdl_decode`` with the
        search of ``osdl_fs_search``; ``perm`` / ``parity`` in the layouts of ``osdl_front``, ``label_bits`` / ``counts`` as there."""
        return self._osd_decode("osdl", "fs_decode", y, C.byref(params), index, count, F, perm, parity, label_bits, counts, out)

    def osdl_pb_search(self, y, perm, parity, params, index=None, count=None, F=None, out=None):
        """``osdx_pb_search`` for every code with n <= 384, 1 <= k <= 192 and 1 <= n-k <= 192, on the results of
        ``osdl_front`` (its layouts).  ``params`` (``osd_params(order, _lib.OSD_PB, snr_db=..., aux=...)``, order
        0..min(3, k)) and the returned dict as there."""
        return self._osd_search("osdl", "pb_search", y, perm, parity, C.byref(params), index, count, F, out)

    def osdl_pb_decode(self, y, params, index=None, count=None, F=None, perm=None, parity=None, label_bits=None, counts=None,
                       out=None):
        """``osdx_pb_decode`` for every code with n <= 384, 1 <= k <= 192 and 1 <= n-k <= 192: ``osdl_decode`` with the
        search of ``osdl_pb_search``; ``perm`` / ``parity`` in the layouts of ``osdl_front``, ``label_bits`` / ``counts`` as there."""
        return self._osd_decode("osdl", "pb_decode", y, C.byref(params), index, count, F, perm, parity, label_bits, counts, out)

    def osdl_tep_eval(self, y, perm, parity, mask, index=None, count=None):
        """``osdx_tep_eval`` for every code with n <= 384, 1 <= k <= 192 and 1 <= n-k <= 192, on the results of ``osdl_front``.
        mask [F, ceil(k/64)] int64: bit p of word w flips primed MRB position 64 w + p; bits at or beyond k are ignored.
        Returns dict(cw[F,words] int64 original bit order, metric[F] f32, hd[F] i32)."""
        return self._osd_tep_eval("osdl", y, perm, parity, mask, index, count)

    def osdx_fs_search(self, y, perm, parity, params, index=None, count=None, F=None, out=None):
        """FS-OSD on front-end results of any supported shape.  ``params``: ``osd_params(order, _lib.OSD_FS, fs_beta=...,
        fs_tau_e=..., fs_tau_psc=..., fs_reference_quirk=...)``, order 0..min(3, k).  Returns the dict of ``osdx_search``
        (best: rank in visit order, 0 = the all-zero TEP; ntep: num_teps)."""
        return self._osd_search("osdx", "fs_search", y, perm, parity, C.byref(params), index, count, F, out)

    def osdx_fs_decode(self, y, params, index=None, count=None, F=None, perm=None, parity=None, label_bits=None, counts=None,
                       out=None):
        """Front end + FS-OSD of the frames y[index[f]] (or y[f]) for any supported shape: ``osdx_decode`` with the search
        of ``osdx_fs_search``; ``perm`` / ``parity`` / ``label_bits`` / ``counts`` as there."""
        return self._osd_decode("osdx", "fs_decode", y, C.byref(params), index, count, F, perm, parity, label_bits, counts, out)

    def osdx_pb_search(self, y, perm, parity, params, index=None, count=None, F=None, out=None):
        """PB-OSD on front-end results of any supported shape.  ``params``: ``osd_params(order, _lib.OSD_PB, snr_db=...,
        aux=...)``, order 0..min(3, k); ``aux`` ([F, 4] int32, optional) receives {frontier comparisons, suc1, suc2, stop
        reason} per frame.  Returns the dict of ``osdx_search`` (best: rank in visit order, 0 = the all-zero TEP; ntep:
        cost_tep_num, or N_max when no rule fired)."""
        return self._osd_search("osdx", "pb_search", y, perm, parity, C.byref(params), index, count, F, out)

    def osdx_pb_decode(self, y, params, index=None, count=None, F=None, perm=None, parity=None, label_bits=None, counts=None,
                       out=None):
        """Front end + PB-OSD of the frames y[index[f]] (or y[f]) for any supported shape: ``osdx_decode`` with the search
        of ``osdx_pb_search``; ``perm`` / ``parity`` / ``label_bits`` / ``counts`` as there."""
        return self._osd_decode("osdx", "pb_decode", y, C.byref(params), index, count, F, perm, parity, label_bits, counts, out)

    def osdx_tep_eval(self, y, perm, parity, mask, index=None, count=None):
        """``osd_tep_eval`` for any supported shape (mask [F] int64: bit p < k flips primed MRB position p).
        Returns dict(cw[F,words] int64 original bit order, metric[F] f32, hd[F] i32)."""
        return self._osd_tep_eval("osdx", y, perm, parity, mask, index, count)

    # ------------------------------------------------------------------ H-form OSD (DL-OSD stage)
    @property
    def hosdx_supported(self):
        """Whether the H-form calls serve this code beyond (128,64) (``ldpc_hosdx_*``: 1 <= k <= 64 and an H of exactly
        n-k <= 64 rows)."""
        return bool(self.L.ldpc_hosdx_supported(self._ctx))

    @property
    def hosdw_supported(self):
        """Whether the wide H-form calls serve this code (``ldpc_hosdw_*``: n <= 128, an H of at most 127 rows as given, of
        rank n-k <= 64; k up to 127)."""
        return bool(self.L.ldpc_hosdw_supported(self._ctx))

    @property
    def hosdl_supported(self):
        """Whether the long H-form calls serve this code (``ldpc_hosdl_*``: n <= 384, an H of at most 192 rows as given, of
        rank n-k <= 192; k up to 192)."""
        return bool(self.L.ldpc_hosdl_supported(self._ctx))

    def hosd_stage_family(self):
        """The H-form family the DL-OSD stage runs on this code: ``"hosd"`` on (128,64), ``"hosdx"`` where
        ``hosdx_supported``, ``"hosdw"`` where ``hosdw_supported`` (high rate, or an H with redundant rows), ``"hosdl"``
        where only ``hosdl_supported`` holds (longer and low-rate codes), else ``"hosdw"``, which refuses the code.
        ``hosd_stage(op)`` is that family's ``front`` / ``search`` / ``sliding`` method."""
        if (self.n, self.k, self.m) == (128, 64, 64):
            return "hosd"
        if self.hosdx_supported:
            return "hosdx"
        return "hosdl" if not self.hosdw_supported and self.hosdl_supported else "hosdw"

    def hosd_stage(self, op):
        return getattr(self, f"{self.hosd_stage_family()}_{op}")

    def _hosd_fam(self):
        """The entry-point family of the H-form calls: the (128,64) kernels for that shape, the any-shape ones otherwise
        (which refuse what they do not serve)."""
        return "hosd" if (self.n, self.k, self.m) == (128, 64, 64) else "hosdx"

    def _hosdl_layout(self):
        """The long family's buffers: (index tail [64 S] int16, M tail [64 ceil(m/64), Wk] int64), m the rank of H."""
        m = self.n - self.k
        return (64 * self.words,), (64 * ((m + 63) // 64), (self.k + 63) // 64)

    def _hosd_M(self, fam, M, lri=None, uidx=None):
        """The wide family reads 128 words of M per frame, the long one its own layouts: front-end results of another family
        are refused here."""
        if fam == "hosdw" and tuple(M.shape[1:]) != (128,):
            raise ValueError(f"front: hosdw takes M [*, 128] (hosdw_front's), got {tuple(M.shape)}")
        if fam == "hosdl":
            itail, mtail = self._hosdl_layout()
            if tuple(M.shape[1:]) != mtail or M.dtype != torch.int64:
                raise ValueError(f"front: hosdl takes M [*, {mtail[0]}, {mtail[1]}] int64 (hosdl_front's), got {tuple(M.shape)}")
            for name, t in (("lri", lri), ("uidx", uidx)):
                if t.dtype != torch.int16 or tuple(t.shape[1:]) != itail:
                    raise ValueError(f"front: hosdl takes {name} [*, {itail[0]}] int16 (hosdl_front's), got {tuple(t.shape)} {t.dtype}")

    def _hosd_front(self, fam, order_llr):
        self._chk(order_llr, torch.float32, (self.n,), "order_llr")
        F = order_llr.shape[0]
        if fam == "hosdl":
            itail, mtail = self._hosdl_layout()
            lri, uidx = self.empty((F,) + itail, torch.int16), self.empty((F,) + itail, torch.int16)
            M = self.empty((F,) + mtail, torch.int64)
            ns = self.empty((F,), torch.int32)
            self._osd_call(fam, "front", _ptr(order_llr), F, _ptr(lri), _ptr(uidx), _ptr(M), _ptr(ns))
            return lri, uidx, M, ns
        lri = self.empty((F, 128), torch.uint8)
        uidx = self.empty((F, 128), torch.uint8)
        M = self.empty((F, 128 if fam == "hosdw" else 64), torch.int64)
        ns = self.empty((F,), torch.int32)
        self._osd_call(fam, "front", _ptr(order_llr), F, _ptr(lri), _ptr(uidx), _ptr(M), _ptr(ns))
        return lri, uidx, M, ns

    def _hosd_search(self, fam, order_llr, metric_llr, front, teps, block_off, label_bits, want_arg, want_best):
        lri, uidx, M, F, nblk = self._hosd_args(order_llr, metric_llr, front, teps, block_off)
        self._hosd_M(fam, M, lri, uidx)
        out = dict(block_min=self.empty((F, nblk), torch.float32),
                   block_arg=self.empty((F, nblk), torch.int32) if want_arg else None,
                   truth=self.empty((F,), torch.float32) if label_bits is not None else None,
                   cw=self.empty((F, self.words), torch.int64) if want_best else None,
                   metric=self.empty((F,), torch.float32) if want_best else None,
                   best=self.empty((F,), torch.int32) if want_best else None)
        self._osd_call(fam, "search", _ptr(order_llr), _ptr(metric_llr), F, _ptr(lri), _ptr(uidx), _ptr(M), _ptr(teps),
                       _ptr(block_off), nblk, _ptr(label_bits), _ptr(out["block_min"]), _ptr(out["block_arg"]),
                       _ptr(out["truth"]), _ptr(out["cw"]), _ptr(out["metric"]), _ptr(out["best"]))
        return out

    def _hosd_sliding(self, fam, order_llr, metric_llr, front, teps, block_off, win, soft_margin, fcn_weights, label_bits,
                      group, want_best):
        lri, uidx, M, F, nblk = self._hosd_args(order_llr, metric_llr, front, teps, block_off)
        self._hosd_M(fam, M, lri, uidx)
        w = np.ascontiguousarray(np.asarray(fcn_weights, dtype=np.float32).reshape(-1))
        lab = label_bits is not None
        out = dict(deep_limit=self.empty((F,), torch.int32), global_min=self.empty((F,), torch.float32),
                   truth=self.empty((F,), torch.float32) if lab else None,
                   success=self.empty((F,), torch.bool) if lab else None,
                   cw=self.empty((F, self.words), torch.int64) if want_best else None,
                   metric=self.empty((F,), torch.float32) if want_best else None,
                   best=self.empty((F,), torch.int32) if want_best else None,
                   teps=self.empty((F,), torch.int32))
        self._osd_call(fam, "sliding", _ptr(order_llr), _ptr(metric_llr), F, _ptr(lri), _ptr(uidx), _ptr(M), _ptr(teps),
                       _ptr(block_off), nblk, int(win), float(soft_margin), w.ctypes.data_as(C.POINTER(C.c_float)), w.size,
                       int(group), _ptr(label_bits), _ptr(out["deep_limit"]), _ptr(out["global_min"]), _ptr(out["truth"]),
                       _ptr(out["success"]), _ptr(out["cw"]), _ptr(out["metric"]), _ptr(out["best"]), _ptr(out["teps"]))
        return out

    def hosd_front(self, order_llr):
        """check_matrix_reorder + identify_mrb on [F,n] ordering values.  Returns (lri[F,128] u8, uidx[F,128] u8 -- entries
        at or beyond n are 0 --, M[F,64] int64 rows r < n-k of updated_M, bits j < k, 0 elsewhere, nswaps[F] int32).
        (128,64) runs ``ldpc_hosd_front``, every other shape ``ldpc_hosdx_front``."""
        return self._hosd_front(self._hosd_fam(), order_llr)

    def hosdx_front(self, order_llr):
        """``hosd_front`` through the any-shape kernels whatever the code (on (128,64) the same results)."""
        return self._hosd_front("hosdx", order_llr)

    def hosd_search(self, order_llr, metric_llr, front, teps, block_off, label_bits=None, want_arg=True, want_best=True):
        """Block minima over the TEP blocks ``teps[block_off[b]:block_off[b+1]]`` (device tensors: [Nt,4] u8,
        [nblk+1] int32).  Returns dict(block_min[F,nblk], block_arg, truth, cw[F,words], metric, best)."""
        return self._hosd_search(self._hosd_fam(), order_llr, metric_llr, front, teps, block_off, label_bits, want_arg, want_best)

    def hosdx_search(self, order_llr, metric_llr, front, teps, block_off, label_bits=None, want_arg=True, want_best=True):
        """``hosd_search`` through the any-shape kernels whatever the code."""
        return self._hosd_search("hosdx", order_llr, metric_llr, front, teps, block_off, label_bits, want_arg, want_best)

    def hosd_sliding(self, order_llr, metric_llr, front, teps, block_off, win, soft_margin, fcn_weights, label_bits=None,
                     group=0, want_best=True):
        """``hosd_search`` with the reference's sliding-window early stop: the blocks are scanned in groups of ``group``
        consecutive blocks (0 = the library's default; results do not depend on it) and a frame stops when the classifier
        (``fcn_weights``: dense1 [win+1,win+1] then dense2 [win+1,2], packed f32) fires with p1 > soft_margin.  Returns
        dict(deep_limit[F] int32, global_min[F], truth[F], success[F] bool, cw[F,words], metric[F], best[F] (first minimum
        over the blocks the reference evaluates), teps[F] int32 (TEPs scanned, speculative ones included))."""
        return self._hosd_sliding(self._hosd_fam(), order_llr, metric_llr, front, teps, block_off, win, soft_margin, fcn_weights,
                                  label_bits, group, want_best)

    def hosdx_sliding(self, order_llr, metric_llr, front, teps, block_off, win, soft_margin, fcn_weights, label_bits=None,
                      group=0, want_best=True):
        """``hosd_sliding`` through the any-shape kernels whatever the code."""
        return self._hosd_sliding("hosdx", order_llr, metric_llr, front, teps, block_off, win, soft_margin, fcn_weights,
                                  label_bits, group, want_best)

    def hosdw_front(self, order_llr):
        """``hosd_front`` through the wide kernels (``ldpc_hosdw_front``): M is [F,128] int64, entry r < n-k bits j = 0..63 of
        row r of updated_M, entry 64 + r bits j = 64..k-1, 0 elsewhere; the elimination deletes redundant rows of H as the
        reference does."""
        return self._hosd_front("hosdw", order_llr)

    def hosdw_search(self, order_llr, metric_llr, front, teps, block_off, label_bits=None, want_arg=True, want_best=True):
        """``hosd_search`` through the wide kernels on ``hosdw_front``'s results (TEP positions < k <= 127)."""
        return self._hosd_search("hosdw", order_llr, metric_llr, front, teps, block_off, label_bits, want_arg, want_best)

    def hosdw_sliding(self, order_llr, metric_llr, front, teps, block_off, win, soft_margin, fcn_weights, label_bits=None,
                      group=0, want_best=True):
        """``hosd_sliding`` through the wide kernels on ``hosdw_front``'s results."""
        return self._hosd_sliding("hosdw", order_llr, metric_llr, front, teps, block_off, win, soft_margin, fcn_weights,
                                  label_bits, group, want_best)

    def hosdl_front(self, order_llr):
        """``hosd_front`` through the long kernels (``ldpc_hosdl_front``): lri / uidx are [F, 64 S] int16 (S = ceil(n/64),
        entries at or beyond n are 0), M is [F, 64 ceil(m/64), ceil(k/64)] int64 (m = n-k: entry [r][w] bits j = 64w..64w+63
        of row r of updated_M, 0 elsewhere); the elimination deletes redundant rows of H as the reference does."""
        return self._hosd_front("hosdl", order_llr)

    def hosdl_search(self, order_llr, metric_llr, front, teps, block_off, label_bits=None, want_arg=True, want_best=True):
        """``hosd_search`` through the long kernels on ``hosdl_front``'s results (TEP positions < k <= 192)."""
        return self._hosd_search("hosdl", order_llr, metric_llr, front, teps, block_off, label_bits, want_arg, want_best)

    def hosdl_sliding(self, order_llr, metric_llr, front, teps, block_off, win, soft_margin, fcn_weights, label_bits=None,
                      group=0, want_best=True):
        """``hosd_sliding`` through the long kernels on ``hosdl_front``'s results."""
        return self._hosd_sliding("hosdl", order_llr, metric_llr, front, teps, block_off, win, soft_margin, fcn_weights,
                                  label_bits, group, want_best)

    def dia_cnn(self, rows, weights, out=None):
        """The bit-wise CNN (conv_bitwise) on retest rows ``[F, L, n]`` (or ``[F*L, n]`` with ``L`` taken from the
        weight count) -> refined values [F, n].  ``weights``: the packed f32 vector of ``nn_net.conv_bitwise.packed()``."""
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float32).reshape(-1))
        L = (w.size - 24 - 96 - 24 - 1) // 2 + 6
        if rows.dim() == 2:
            if rows.shape[0] % L:
                raise ValueError(f"rows: {rows.shape[0]} rows are not whole trajectories of {L}")
            rows = rows.reshape(rows.shape[0] // L, L, rows.shape[1])
        if rows.dtype != torch.float32 or rows.device != self.device or rows.dim() != 3 or rows.shape[2] != self.n \
                or not rows.is_contiguous():
            raise ValueError(f"rows: expected a contiguous float32 [F, L, {self.n}] tensor on {self.device}")
        F = rows.shape[0]
        out = self.empty((F, self.n), torch.float32) if out is None else out
        _lib.check(self.L.ldpc_dia_cnn(self._ctx, _ptr(rows), F, rows.shape[1], w.ctypes.data_as(C.POINTER(C.c_float)), w.size,
                                       _ptr(out), self._stream()), "ldpc_dia_cnn")
        return out

    def dia_cnn_grad(self, rows, label_bits, weights, want_out=False):
        """Training step of the bit-wise CNN (ldpc_dia_cnn_grad): the reference's loss (nn_training.py:293-297), summed
        over the frames and bits of ``rows`` [F, L, n], and its gradient with respect to every weight, in one call.
        ``label_bits``: packed code bits [F, words] int64 (``pack_bits``); ``weights``: as ``dia_cnn``.  Returns
        (loss_sum [1] f64, grad [n_weights] f64 in the packed order of the weights, out [F, n] f32 -- ``dia_cnn``'s, bit
        for bit -- or None)."""
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float32).reshape(-1))
        if rows.dtype != torch.float32 or rows.device != self.device or rows.dim() != 3 or rows.shape[2] != self.n \
                or not rows.is_contiguous():
            raise ValueError(f"rows: expected a contiguous float32 [F, L, {self.n}] tensor on {self.device}")
        self._chk(label_bits, torch.int64, (self.words,), "label_bits")
        F = rows.shape[0]
        if label_bits.shape[0] != F:
            raise ValueError(f"label_bits: {label_bits.shape[0]} frames for {F} frames of rows")
        make = torch.empty if F > 0 else torch.zeros      # (F = 0 writes nothing: the sums are 0)
        loss_sum = make((1,), dtype=torch.float64, device=self.device)
        grad = make((w.size,), dtype=torch.float64, device=self.device)
        out = self.empty((F, self.n), torch.float32) if want_out else None
        _lib.check(self.L.ldpc_dia_cnn_grad(self._ctx, _ptr(rows), _ptr(label_bits), F, rows.shape[1],
                                            w.ctypes.data_as(C.POINTER(C.c_float)), w.size, _ptr(out), _ptr(loss_sum), _ptr(grad),
                                            self._stream()), "ldpc_dia_cnn_grad")
        return loss_sum, grad, out

    # ------------------------------------------------------------------ training of the sliding-window classifier
    def _fcn_index(self, index, rows, name, check_index):
        """A 1-D int32 row list on the device; with ``check_index`` its range is checked (one synchronisation)."""
        if not isinstance(index, torch.Tensor) or index.device != self.device or index.dtype != torch.int32 \
                or index.dim() != 1 or not index.is_contiguous():
            raise ValueError(f"{name}: expected a contiguous 1-D int32 tensor on {self.device}")
        if check_index and index.numel():
            lo, hi = (int(v) for v in torch.aminmax(index))
            if lo < 0 or hi >= rows:
                raise ValueError(f"{name}: entries {lo}..{hi} outside the {rows} rows")
        return index

    def fcn_windows(self, block_min, success, index=None, win=5, check_index=True):
        """Training windows of the sliding-window classifier (ldpc_fcn_windows; reform_inputs of the reference's training
        stage).  ``block_min`` [F, nblk] f32: a search call's block minima; ``success`` [F] bool / uint8: the frame's
        overall minimum is the label's metric; ``index`` [R] int32 (optional): the kept frames, as ``compact`` writes them
        (pass ``index[:count]``).  Returns (inputs [(nblk-win+1)*R, win+1] f32: the ascending window then its position,
        window-major, row i*R + r; labels [(nblk-win+1)*R] uint8; class_count [2] int64: rows with label 0 / 1).
        ``check_index=False`` skips the range check of ``index`` (a synchronisation) where the list is valid by
        construction."""
        if not isinstance(block_min, torch.Tensor) or block_min.device != self.device or block_min.dtype != torch.float32 \
                or block_min.dim() != 2 or not block_min.is_contiguous():
            raise ValueError(f"block_min: expected a contiguous float32 [F, nblk] tensor on {self.device}")
        F, nblk = block_min.shape
        if not isinstance(success, torch.Tensor) or success.device != self.device or success.dtype not in (torch.bool, torch.uint8) \
                or tuple(success.shape) != (F,) or not success.is_contiguous():
            raise ValueError(f"success: expected a contiguous bool / uint8 [{F}] tensor on {self.device}")
        win = int(win)
        if not 1 <= win <= 15 or not win <= nblk <= 1024:
            raise ValueError(f"fcn_windows: win = {win}, nblk = {nblk}: 1 <= win <= 15 and win <= nblk <= 1024")
        R = F if index is None else self._fcn_index(index, F, "index", check_index).numel()
        rows = (nblk - win + 1) * R
        inputs = self.empty((rows, win + 1), torch.float32)
        labels = self.empty((rows,), torch.uint8)
        class_count = torch.zeros(2, dtype=torch.int64, device=self.device)      # (R = 0 writes nothing)
        _lib.check(self.L.ldpc_fcn_windows(self._ctx, _ptr(block_min), _ptr(success), _ptr(index), R, nblk, win, _ptr(inputs),
                                           _ptr(labels), _ptr(class_count), self._stream()), "ldpc_fcn_windows")
        return inputs, labels, class_count

    def fcn_grad(self, inputs, labels, weights, win, penalty, weight=None, index=None, want_p=False, want_grad=True,
                 check_index=True):
        """Training step of the sliding-window classifier (ldpc_fcn_grad): the reference's weighted, penalised
        cross-entropy (calculation_loss of its training stage) summed over the batch, its gradient with respect to both
        kernels, the weighted accuracy sums and the validation counts, in one call.  ``inputs`` [N, win+1] f32 and
        ``labels`` [N] uint8 as ``fcn_windows`` returns them; ``weights``: the packed f32 vector of
        ``nn_net.Predict_outlier_light.packed()``; ``weight`` [N] f32 (optional): the per-sample class weights;
        ``index`` [B] int32 (optional): the rows of the batch, in any order, repeats allowed (default: all N rows).
        Returns dict(loss_sum [1] f64, grad [n_weights] f64 in the packed order or None, acc [2] f64 = (sum of the weights
        where the prediction is right, sum of the weights), counts [3] int64 = (S, F1, F2), p [B, 2] f32 or None)."""
        win = int(win)
        if not 1 <= win <= 15:
            raise ValueError(f"fcn_grad: win = {win} outside 1..15")
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float32).reshape(-1))
        if w.size != (win + 1) ** 2 + 2 * (win + 1):
            raise ValueError(f"weights: {w.size} values, a window of {win} takes {(win + 1) ** 2 + 2 * (win + 1)}")
        if not isinstance(inputs, torch.Tensor) or inputs.dim() != 2:
            raise ValueError(f"inputs: expected a float32 [N, {win + 1}] tensor on {self.device}")
        self._chk(inputs, torch.float32, (win + 1,), "inputs")
        N = inputs.shape[0]
        self._chk(labels, torch.uint8, (), "labels")
        if labels.shape[0] != N:
            raise ValueError(f"labels: {labels.shape[0]} entries for {N} rows of inputs")
        if weight is not None:
            self._chk(weight, torch.float32, (), "weight")
            if weight.shape[0] != N:
                raise ValueError(f"weight: {weight.shape[0]} entries for {N} rows of inputs")
        B = N if index is None else self._fcn_index(index, N, "index", check_index).numel()
        make = torch.empty if B > 0 else torch.zeros      # (B = 0 writes nothing: the sums are 0)
        out = dict(loss_sum=make((1,), dtype=torch.float64, device=self.device),
                   grad=make((w.size,), dtype=torch.float64, device=self.device) if want_grad else None,
                   acc=make((2,), dtype=torch.float64, device=self.device),
                   counts=make((3,), dtype=torch.int64, device=self.device),
                   p=self.empty((B, 2), torch.float32) if want_p else None)
        _lib.check(self.L.ldpc_fcn_grad(self._ctx, _ptr(inputs), _ptr(labels), _ptr(weight), _ptr(index), B, win,
                                        w.ctypes.data_as(C.POINTER(C.c_float)), w.size, float(penalty), _ptr(out["p"]),
                                        _ptr(out["loss_sum"]), _ptr(out["grad"]), _ptr(out["acc"]), _ptr(out["counts"]),
                                        self._stream()), "ldpc_fcn_grad")
        return out

    def osd_counts(self, cw, label_bits, index=None, count=None, ntep=None, counts=None, F=None):
        """counts[3] += {frames, frames_wrong, teps_total}; labels are looked up through index."""
        F = cw.shape[0] if F is None else F
        if counts is None:
            counts = torch.zeros(3, dtype=torch.int64, device=self.device)
        _lib.check(self.L.ldpc_osd_counts(self._ctx, _ptr(cw), _ptr(label_bits), _ptr(index), _ptr(count), _ptr(ntep),
                                          F, _ptr(counts), self._stream()), "ldpc_osd_counts")
        return counts

    def osd_merge(self, cw, index, count, hard=None, label_bits=None, counts=None, F=None):
        """The OSD codewords back among the NMS decisions: hard[index[j]] = cw[j] for j < min(count, F), in place, and with
        ``label_bits`` counts[4] += {frames, frames_wrong, bit errors of cw, bit errors of the replaced rows of hard} (the last
        stays 0 without ``hard``).  ``counts`` is allocated when labels come without it.  Returns counts (None without labels)."""
        F = cw.shape[0] if F is None else F
        if counts is None and label_bits is not None:
            counts = torch.zeros(4, dtype=torch.int64, device=self.device)
        _lib.check(self.L.ldpc_osd_merge(self._ctx, _ptr(cw), _ptr(index), _ptr(count), F, _ptr(hard), _ptr(label_bits),
                                         _ptr(counts), self._stream()), "ldpc_osd_merge")
        return counts

    def osd_family(self):
        """The prefix of the G-form OSD family that serves this code: ``"osdx"`` where ``osdx_supported``, else ``"osdw"``, else
        ``"osdl"`` (which refuses the code where it does not serve it either): LDPC_OSD_FAMILY_AUTO."""
        return "osdx" if self.osdx_supported else "osdw" if self.osdw_supported else "osdl"


_default = {}


def default_decoder(code: Code, device=None) -> Decoder:
    """Decoder cache keyed by (code object, device) for the reference-style global-state API."""
    dev = torch.cuda.current_device() if device is None else int(device)
    key = (id(code), dev)
    if key not in _default:
        _default[key] = Decoder(code, dev)
    return _default[key]
