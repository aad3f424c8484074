"""Test helper: what the tests of the three G-form OSD families (ldpc_osdx_*: any shape with k <= 64, ldpc_osdw_*: high rate,
ldpc_osdl_*: long / low rate) share -- written once, so that every family is held to the same contract.

  Family         prefix, the ``needs`` sentence of its refusal, its layouts on a code (n, k), packers between the model's
                 (perm [n], [I | P']) and those layouts, split_masks for its tep_eval mask.  OSDX / OSDW / OSDL.
  CPU model      front_oracle (the C oracle's orc_osd_front in a family's layouts), self_check, h_systematic (H = [A | I]).
                 The scan oracle is osdx_model.scan_oracle, FS-OSD osdx_fs_model, PB-OSD osdx_pb_model: each serves any shape.
  calls          decoder (one cache), dev_front, sentinels, raw (tests/abi_calls.py: the header's argument names), fs_params,
                 pb_params
  assertions     assert_front (whole arrays, padding included, and nswaps), assert_scan / assert_fs / assert_pb / assert_same:
                 integers equal, floats by their bits
  contract       check_*: frame list and device count, nullable outputs and counters, subsets of the nullable outputs, frames
                 in turn beyond 65536 workgroups, bad arguments, refusal of unsupported shapes -- called from the tests in the family files

A new family's tests: add a ``Family`` entry, its codes (a model module with graph / make_code / frames) and its one-family tests.
"""
import functools

import numpy as np
import torch

from oracle import c_oracle, np_oracle
from tests import abi_calls as A
from tests.gpu_util import pack_np, to_dev, words_np


# ---------------------------------------------------------------------------------------------------------------------
# the families
# ---------------------------------------------------------------------------------------------------------------------
def pack_rows(bits, words):
    """[r, c <= 64 words] 0/1 -> [r, words] uint64: bit c % 64 of word c // 64."""
    bits = np.asarray(bits, dtype=np.uint8)
    pad = np.zeros((bits.shape[0], 64 * words - bits.shape[1]), np.uint8)
    return np.packbits(np.concatenate([bits, pad], axis=1), axis=1, bitorder="little").view(np.uint64).reshape(bits.shape[0], words)


def unpack_rows(words, cols):
    """The inverse of pack_rows: [r, words] uint64 -> [r, cols] 0/1."""
    words = np.ascontiguousarray(words, dtype=np.uint64)
    return np.unpackbits(words.view(np.uint8).reshape(words.shape[0], -1), axis=1, bitorder="little")[:, :cols]


class Family:
    """One G-form OSD family.  ``geometry(n, k)`` -> (entries of a perm row, rows of parity, words per parity row, words of a
    tep_eval mask or None for a scalar mask).  The model keeps the word axis of parity where ``word_axis`` (osdl: [64 W, Wp]
    always); the device layout drops it when a row is one word, as runtime.Decoder._osd_layout says."""

    def __init__(self, prefix, needs, limits, perm_np, perm_torch, geometry, word_axis):
        self.prefix, self.needs, self.limits = prefix, needs, limits
        self.perm_np, self.perm_torch, self.geometry, self.word_axis = perm_np, perm_torch, geometry, word_axis

    def __repr__(self):
        return self.prefix

    def serves(self, n, k):
        nmax, kmax, mmax = self.limits
        return n <= nmax and 1 <= k <= kmax and 1 <= n - k <= mmax

    def refusal(self, n, k):
        """The regular expression of the library's UNSUPPORTED message for an (n, k) code."""
        import re
        return rf"\(-5\).*{re.escape(self.needs)}; this code is \({n},{k}\)"

    # ---- layouts
    def layout(self, n, k):
        """(torch dtype of perm, shape tail of perm, shape tail of parity, shape tail of a tep_eval mask) on the device."""
        plen, rows, words, mwords = self.geometry(n, k)
        return self.perm_torch, (plen,), ((rows,) if words == 1 else (rows, words)), (() if mwords is None else (mwords,))

    def model_parity_tail(self, n, k):
        _, rows, words, _ = self.geometry(n, k)
        return (rows, words) if self.word_axis else (rows,)

    # ---- packers
    def pack_front(self, perm, Gp):
        """One frame's (perm [n], [I | P'] [k, n]) -> (perm row, parity rows) of the model, zero in the padding."""
        k, n = Gp.shape
        plen, rows, words, _ = self.geometry(n, k)
        p = np.zeros(plen, self.perm_np)
        p[:n] = perm
        q = np.zeros((rows, words), np.uint64)
        q[:k] = pack_rows(np.asarray(Gp)[:, k:], words)
        return p, (q if self.word_axis else q[:, 0])

    def unpack_front(self, p, q, n, k):
        """The inverse of pack_front -> (perm [n], P' [k, n-k])."""
        _, rows, words, _ = self.geometry(n, k)
        return np.asarray(p[:n], dtype=np.int64), unpack_rows(np.asarray(q).reshape(rows, words)[:k], n - k)

    def split_masks(self, masks, k):
        """Python-int masks (bit p = flip MRB position p) -> uint64 [F] + the mask tail of this family."""
        mwords = self.geometry(k + 1, k)[3]
        out = np.array([[(int(m) >> (64 * w)) & ((1 << 64) - 1) for w in range(mwords or 1)] for m in masks], dtype=np.uint64)
        return out.reshape(len(masks), mwords or 1) if mwords else out.reshape(len(masks))


def _ceil64(v):
    return (v + 63) // 64


OSDX = Family("osdx", "the any-shape OSD kernels need 1 <= k <= 64 and 1 <= n-k <= 64", (128, 64, 64), np.uint8, torch.uint8,
              lambda n, k: (128, 64, 1, None), False)
OSDW = Family("osdw", "the high-rate OSD kernels need 1 <= n-k <= 64 and n <= 128", (128, 127, 64), np.uint8, torch.uint8,
              lambda n, k: (128, 128, 1, 2), False)
OSDL = Family("osdl", "the long / low-rate OSD kernels need n <= 384, 1 <= k <= 192 and 1 <= n-k <= 192", (384, 192, 192),
              np.uint16, torch.int16, lambda n, k: (64 * _ceil64(n), 64 * _ceil64(k), _ceil64(n - k), _ceil64(k)), True)
FAMILIES = {f.prefix: f for f in (OSDX, OSDW, OSDL)}


# ---------------------------------------------------------------------------------------------------------------------
# the CPU model every family shares
# ---------------------------------------------------------------------------------------------------------------------
def front_oracle(G, y, fam, swaps=False):
    """The C oracle's general orc_osd_front, frame by frame -> (perm, parity, nswaps [F] i32, Gp list) in the model layouts of
    ``fam``: entries beyond n, rows beyond k and bits beyond n-k are zero.  ``swaps``: a fifth member, the recorded exchanges
    [(a, b), ...] per frame."""
    G = np.asarray(G)
    k, n = G.shape
    y = np.asarray(y, dtype=np.float32)
    plen = fam.geometry(n, k)[0]
    perm = np.zeros((len(y), plen), fam.perm_np)
    parity = np.zeros((len(y),) + fam.model_parity_tail(n, k), np.uint64)
    ns = np.zeros(len(y), np.int32)
    Gps, sws = [], []
    for f, row in enumerate(y):
        p, Gp, sw = c_oracle.osd_front(G, row)
        assert np.array_equal(Gp[:, :k], np.eye(k, dtype=np.int32))
        perm[f], parity[f] = fam.pack_front(p, Gp)
        ns[f] = len(sw)
        Gps.append(Gp.astype(np.int64))
        sws.append(list(sw))
    return (perm, parity, ns, Gps, sws) if swaps else (perm, parity, ns, Gps)


def self_check(model, name, order=1, frames_=3, seed=5):
    """On ``frames_`` frames at 1.5 dB of the code ``name`` of a model module (its graph and frames): the two front-end
    oracles agree, and osdx_model.scan_frame's vectorised costs equal np_oracle.convention_osd's at ``order``, bit for bit."""
    from tests import osdx_model
    G = model.graph(name)[1]
    y, labels = model.frames(name, 1.5, frames_, seed)
    for row, lab in zip(y, labels):
        yp, labp, Gp, perm, _ = np_oracle.swapped_info(row, lab, G)
        ref = np_oracle.convention_osd(yp, labp, Gp, order)
        cost, cand = osdx_model.scan_frame(yp, Gp, order)
        assert np.array_equal(cost.view(np.uint32), ref["costs"].view(np.uint32))
        assert int(np.argmin(cost)) == ref["best_index"] and np.array_equal(cand[ref["best_index"]], ref["codeword"])
        p_c, Gp_c, _ = c_oracle.osd_front(G, row)
        assert np.array_equal(p_c, perm) and np.array_equal(Gp_c, Gp)
    return True


def h_systematic(n, k, colw=3):
    """-> (H, G) with H = [A | I_m] from default_rng(5): column c of A gets min(m, colw) ones."""
    rng = np.random.default_rng(5)
    m = n - k
    A = np.zeros((m, k), np.int64)
    for c in range(k):
        A[rng.choice(m, size=min(m, colw), replace=False), c] = 1
    H = np.concatenate([A, np.eye(m, dtype=np.int64)], axis=1)
    G = np_oracle.generator_from_H(H)
    assert G.shape == (k, n)
    return H, G


# ---------------------------------------------------------------------------------------------------------------------
# calls
# ---------------------------------------------------------------------------------------------------------------------
_decoders = {}


OWN_SHAPES = {(80, 121): "array_121_80", (130, 321): "s321_130", (192, 384): "wl384"}     # (k, n) -> the family's own code


@functools.lru_cache(maxsize=None)
def shape_graph(k, n):
    """(H, G) of a code of shape (k, n) to hold the context of caller-made front-end results (the searches never read G): a
    family's own code of that shape, else H = [A | I] of h_systematic."""
    if (k, n) in OWN_SHAPES:
        from tests import osdl_model
        return osdl_model.graph(OWN_SHAPES[(k, n)])
    return h_systematic(n, k)


def decoder(code, graph=shape_graph):
    """One context per code, shared by every test file: a name some model module knows (osdl_model.make_code resolves them
    all), or a tuple -- a shape (k, n), or whatever ``graph(*code)`` -> (H, G) takes."""
    key = code if graph is shape_graph else (code, graph)
    if key not in _decoders:
        from short_ldpc_decoding_osd_amd import Code
        from short_ldpc_decoding_osd_amd.runtime import Decoder
        from tests import osdl_model
        _decoders[key] = Decoder(Code(H=graph(*code)[0]) if isinstance(code, tuple) else osdl_model.make_code(code))
    return _decoders[key]


def tiny_case():
    """A (6,2) code, where weight class 3 does not exist, and 64 frames at 0 dB -> (context, G, y)."""
    if "tiny" not in _decoders:
        from short_ldpc_decoding_osd_amd import Code
        from short_ldpc_decoding_osd_amd.runtime import Decoder
        H = np.array([[1, 1, 0, 1, 0, 0], [0, 1, 1, 0, 1, 0], [1, 0, 1, 0, 0, 1], [1, 1, 1, 1, 1, 0]], dtype=np.int64)
        code = Code(H=H)
        assert code.k == 2
        _decoders["tiny"] = Decoder(code)
    dec = _decoders["tiny"]
    G = np.asarray(dec.code.G)
    return dec, G, np_oracle.make_frames(G, 0.0, 64, np.random.default_rng(9))[0]


def dev_front(perm, parity, dec, fam):
    """The model's perm and parity as the device tensors of the binding."""
    tail = fam.layout(dec.n, dec.k)[2]
    perm, parity = np.ascontiguousarray(perm), np.ascontiguousarray(parity)
    return (to_dev(perm.view(np.int16) if fam.perm_np == np.uint16 else perm, dec),
            to_dev(parity.view(np.int64).reshape((len(perm),) + tail), dec))


def new_aux(dec, F):
    return A.sentinel(dec, (F, 4), torch.int32)


def sentinels(dec, fam, F, aux=False):
    """Every buffer of a call in the family's layouts, filled with values no kernel writes (abi_calls.SENT)."""
    pdt, ptail, qtail, _ = fam.layout(dec.n, dec.k)
    bufs = dict(perm=A.sentinel(dec, (F,) + ptail, pdt), parity=A.sentinel(dec, (F,) + qtail, torch.int64),
                cw=A.sentinel(dec, (F, dec.words), torch.int64), metric=A.sentinel(dec, (F,), torch.float32),
                best=A.sentinel(dec, (F,), torch.int32), ntep=A.sentinel(dec, (F,), torch.int32))
    if aux:
        bufs["aux"] = new_aux(dec, F)
    return bufs


def assert_untouched(bufs, clean, start=0):
    for k in bufs:
        if bufs[k] is not None:
            assert torch.equal(bufs[k][start:], clean[k][start:]), k


def raw(dec, fam, op, bufs=None, **kw):
    """ldpc_<fam>_<op> through abi_calls.call: the status code.  ``bufs``: perm / parity / cw / metric / best / ntep / hd / mask
    tensors (None or missing: NULL) under their d_ names; every other argument by the header's name."""
    entry = f"ldpc_{fam.prefix}_{op}"
    for key, t in (bufs or {}).items():
        if "d_" + key in A.SIGS[entry]:
            kw.setdefault("d_" + key, t)
    return A.call(dec, entry, **kw)


def _arg(entry, arg):
    return {"order" if "order" in A.SIGS[entry] else "params": arg}


def raw_decode(dec, fam, op, yd, index, count, F, arg, bufs, label=None, counts=None):
    """ldpc_<fam>_<op> for the *decode calls; ``arg``: the order, or the parameter block (None: NULL)."""
    return raw(dec, fam, op, bufs, d_y=yd, d_index=index, d_count=count, F=F, d_label_bits=label, d_counts=counts,
               **_arg(f"ldpc_{fam.prefix}_{op}", arg))


def raw_search(dec, fam, op, yd, F, arg, bufs):
    """ldpc_<fam>_<op> for the *search calls on the front-end results in ``bufs``, without a frame list."""
    return raw(dec, fam, op, bufs, d_y=yd, F=F, **_arg(f"ldpc_{fam.prefix}_{op}", arg))


def raw_tep_eval(dec, fam, yd, F, perm, parity, mask, cw, metric, hd):
    return raw(dec, fam, "tep_eval", d_y=yd, F=F, d_perm=perm, d_parity=parity, d_mask=mask, d_cw=cw, d_metric=metric, d_hd=hd)


def fs_params(dec, order, s, quirk, **kw):
    from short_ldpc_decoding_osd_amd import _lib
    return dec.osd_params(order, _lib.OSD_FS, fs_beta=s[0], fs_tau_e=s[1], fs_tau_psc=s[2], fs_reference_quirk=quirk, **kw)


def pb_params(dec, order, snr_db, aux=None, **kw):
    from short_ldpc_decoding_osd_amd import _lib
    return dec.osd_params(order, _lib.OSD_PB, snr_db=snr_db, aux=aux, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# assertions: integers equal, floats by their bits
# ---------------------------------------------------------------------------------------------------------------------
def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _bits(a):
    a = _np(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_front(fam, dec, perm, parity, front, nswaps=None, rows=slice(None)):
    """perm and parity as whole arrays -- the padding included: the oracle's arrays are zero there -- against the rows ``rows``
    of a front_oracle result, and nswaps when given."""
    n, k = dec.n, dec.k
    pdt, ptail, qtail, _ = fam.layout(n, k)
    assert perm.dtype == pdt and tuple(perm.shape[1:]) == ptail, ("perm", perm.dtype, tuple(perm.shape))
    assert parity.dtype == torch.int64 and tuple(parity.shape[1:]) == qtail, ("parity", parity.dtype, tuple(parity.shape))
    got_p = _np(perm).view(fam.perm_np)
    got_q = words_np(parity).reshape((-1,) + fam.model_parity_tail(n, k))
    assert np.array_equal(got_p, front[0][rows]), "perm"
    assert np.array_equal(got_q, front[1][rows]), "parity"
    if nswaps is not None:
        assert np.array_equal(_np(nswaps), front[2][rows]), "nswaps"


def assert_outputs(out, ref, sl=slice(None), pick=None, where="", keys=("cw", "metric", "best", "ntep")):
    """``keys`` of ``out`` (tensors) against the model's arrays ``ref``, rows ``sl``.  ``pick``: the model's frames that the
    outputs hold, in order (a frame list)."""
    for key in keys:
        want = np.asarray(ref[key])
        want = want if pick is None else want[np.asarray(pick)]
        got = words_np(out[key]) if key == "cw" else _np(out[key])
        assert got.dtype == want.dtype, (where, key, got.dtype, want.dtype)
        assert np.array_equal(_bits(got)[sl], _bits(want)[sl]), (where, key)


def assert_scan(out, ref, F=None, where=""):
    """cw, metric, best, ntep of the first F frames."""
    assert_outputs(out, ref, slice(0, F), where=where)


def fs_view(ref, quirk):
    """A Batch.fs result as the outputs of one quirk mode: cw, metric, best, ntep."""
    key = "ref" if quirk else "hit"
    return dict(cw=ref["cw_" + key], metric=ref["metric_" + key], best=ref["best_" + key], ntep=ref["ntep"])


def assert_fs(out, ref, quirk, sl=slice(None), where=""):
    assert_outputs(out, fs_view(ref, quirk), sl, where=where)


def assert_pb(out, aux, ref, sl=slice(None), pick=None, where=""):
    """cw, metric, best, ntep and, where ``aux`` is given, the four aux columns."""
    assert_outputs(out, ref, sl, pick, where)
    if aux is not None:
        assert_outputs(dict(aux=aux), ref, sl, pick, where, keys=("aux",))


def assert_same(got, want, keys, where=""):
    """Two sets of device outputs: same dtype, same shape, same bits."""
    for key in keys:
        assert A.same_bits(got[key], want[key]) and got[key].dtype == want[key].dtype, (where, key)


# ---------------------------------------------------------------------------------------------------------------------
# the contract every family's decode / search entry points keep, written once.  ``op``: "decode", "fs_decode", "pb_decode" (and
# the matching search); ``case``: dict(dec, yd, index, count, nf, rows: the model's frames the list names, in order, ref: the
# model's outputs (cw, metric, best, ntep and, for PB, aux), front: the front_oracle result, labels [frames, n] and
# label_rows: the labels' rows of the listed frames, arg: bufs -> the order or the parameter block of the call).
# ---------------------------------------------------------------------------------------------------------------------
def _case_keys(case):
    return ("cw", "metric", "best", "ntep") + (("aux",) if "aux" in case["ref"] else ())


def check_frame_list(fam, op, case, which):
    """The device-side count against the capacity F: min(count, F) frames are written, nothing at or beyond."""
    dec, nf = case["dec"], case["nf"]
    F = {"smaller": nf + 13, "equal": nf, "larger": nf - 9}[which]
    done = min(nf, F)
    keys = _case_keys(case)
    bufs = sentinels(dec, fam, nf + 13, aux="aux" in keys)
    clean = {k: v.clone() for k, v in bufs.items()}
    assert raw_decode(dec, fam, op, case["yd"], case["index"], case["count"], F, case["arg"](bufs), bufs) == 0
    torch.cuda.synchronize()
    rows = np.asarray(case["rows"])[:done]
    assert_outputs({k: bufs[k][:done] for k in keys}, case["ref"], pick=rows, keys=keys)
    assert_front(fam, dec, bufs["perm"][:done], bufs["parity"][:done], case["front"], rows=rows)
    assert_untouched(bufs, clean, done)


def check_nullable(fam, op, case, off):
    """``off``: "none", or the outputs left NULL joined by "+" (metric, best, ntep, aux, counts, label).  The others are written
    as ever; the fused counters move only with d_counts and d_label_bits, teps_total only with d_ntep."""
    dec, nf, ref, rows = case["dec"], case["nf"], case["ref"], np.asarray(case["rows"])
    keys = _case_keys(case)
    label = to_dev(pack_np(case["labels"]).view(np.int64), dec)
    bufs = sentinels(dec, fam, nf, aux="aux" in keys)
    counts = torch.tensor([5, 6, 7], dtype=torch.int64, device=dec.device)
    gone = off.split("+")
    for key in gone:
        if key in bufs:
            bufs[key] = None
    assert raw_decode(dec, fam, op, case["yd"], case["index"], case["count"], nf, case["arg"](bufs), bufs,
                      None if "label" in gone else label, None if "counts" in gone else counts) == 0
    torch.cuda.synchronize()
    assert_outputs(bufs, ref, pick=rows, where=off, keys=[k for k in keys if k not in gone])
    assert_front(fam, dec, bufs["perm"], bufs["parity"], case["front"], rows=rows)
    wrong = int(np.any(ref["cw"][rows] != pack_np(case["labels"][case["label_rows"]]), axis=1).sum())
    if case.get("some_wrong", True):                          # premises of the inputs, where the family's case states them
        assert 0 < wrong < nf
    assert len(set(ref["ntep"][rows].tolist())) > case.get("distinct_ntep", 0)
    teps = 0 if "ntep" in gone else int(ref["ntep"][rows].astype(np.int64).sum())
    assert counts.cpu().tolist() == ([5, 6, 7] if "counts" in gone or "label" in gone else [5 + nf, 6 + wrong, 7 + teps])


def check_nullable_subsets(fam, op, case, mask, F=12):
    """PB search: metric, best, ntep and aux, each of the 14 proper non-empty subsets present, the others NULL."""
    dec, ref, front = case["dec"], case["ref"], case["front"]
    names = ("metric", "best", "ntep", "aux")
    bufs = sentinels(dec, fam, F, aux=True)
    bufs["perm"], bufs["parity"] = dev_front(front[0][:F], front[1][:F], dec, fam)
    for b, key in enumerate(names):
        if not (mask >> b) & 1:
            bufs[key] = None
    assert raw_search(dec, fam, op, case["yd"], F, case["arg"](bufs), bufs) == 0
    torch.cuda.synchronize()
    assert_outputs(bufs, ref, slice(0, F), where=mask, keys=["cw"] + [k for k in names if bufs[k] is not None])


def check_frames_in_turn(fam, dec, y, decode, model, extra=300, distinct_ntep=0):
    """More frames than the grid's 65536 workgroups: wavefront b decodes frame b and then frame 65536 + b.  ``decode(yd)`` ->
    the outputs of a *decode call; ``model(frames)`` -> (front_oracle result, outputs).  The frames that share a wavefront are
    checked against the model, all of them against the same frames in split launches."""
    F = 65536 + extra
    assert len(y) == F
    yd = to_dev(y, dec)
    out, head, tail = decode(yd), decode(yd[:65536].contiguous()), decode(yd[65536:].contiguous())
    torch.cuda.synchronize()
    for k in ("perm", "parity", "cw", "metric", "best", "ntep"):
        assert torch.equal(out[k][:65536], head[k]) and torch.equal(out[k][65536:], tail[k]), k
    for sl in (slice(0, extra), slice(65536, F)):
        front, ref = model(y[sl])
        assert len(set(ref["ntep"].tolist())) > distinct_ntep          # premise: the frames of a wavefront differ in their scans
        assert_outputs({k: out[k][sl] for k in ("cw", "metric", "best", "ntep")}, ref)
        assert_front(fam, dec, out["perm"][sl], out["parity"][sl], front)


def check_bad_arguments(fam, algo, dec, yd, bufs, make, good, mask=None):
    """``algo``: "fs" or "pb".  Every parameter block the family's <algo>_search / <algo>_decode must refuse (``make(order, **kw)``
    builds the family's block), every required pointer as NULL, a negative F, and F == 0, which is LDPC_OK without a launch;
    with ``mask`` (FS) the same for tep_eval.  Each refusal is LDPC_E_ARG under the entry point's own name.  The caller
    checks afterwards that ``bufs`` is untouched."""
    from short_ldpc_decoding_osd_amd import _lib
    import pytest
    F, pre = len(yd), f"ldpc_{fam.prefix}_{algo}_"
    search, decode = getattr(dec, f"{fam.prefix}_{algo}_search"), getattr(dec, f"{fam.prefix}_{algo}_decode")
    other = {"fs": (_lib.OSD_PB, 2), "pb": (_lib.OSD_FS, 1)}[algo]
    bad = [(dec.osd_params(2, _lib.OSD_CONVENTIONAL), rf"algo 0 is not LDPC_OSD_{algo.upper()}"),
           (dec.osd_params(2, other[0]), rf"algo {other[1]} is not LDPC_OSD_{algo.upper()}"),
           (make(4), r"order 4 outside 0\.\.3"), (make(-1), r"order -1 outside 0\.\.3"),
           (make(2, table_scan=True), r"flags 0x1 are not served here"), (make(2, y_frames=4), r"y_frames 4 is not served here")]
    if algo == "fs":
        bad.append((make(2, aux=torch.zeros((F, 4), dtype=torch.int32, device=dec.device)), r"d_aux is not served here"))
    else:
        bad.append((make(2, pb_path="replay"), r"flags 0x4 are not served here"))
    for p, why in bad:
        with pytest.raises(_lib.LdpcError, match=r"\(-1\).*" + pre + "decode: " + why):
            decode(yd, p, perm=bufs["perm"], parity=bufs["parity"], out=bufs)
        with pytest.raises(_lib.LdpcError, match=r"\(-1\).*" + pre + "search: " + why):
            search(yd, bufs["perm"], bufs["parity"], p, out=bufs)

    def refused(rc, who, why):
        assert rc == A.E_ARG and f"{who}: {why}" in A.last_error(dec), (who, why, rc, A.last_error(dec))
    for missing in ("cw", "perm", "parity"):
        refused(raw_decode(dec, fam, algo + "_decode", yd, None, None, F, good, {**bufs, missing: None}), pre + "decode", f"d_{missing} is NULL")
        refused(raw_search(dec, fam, algo + "_search", yd, F, good, {**bufs, missing: None}), pre + "search", f"d_{missing} is NULL")
    refused(raw_decode(dec, fam, algo + "_decode", None, None, None, F, good, bufs), pre + "decode", "d_y is NULL")
    refused(raw_search(dec, fam, algo + "_search", None, F, good, bufs), pre + "search", "d_y is NULL")
    refused(raw_decode(dec, fam, algo + "_decode", yd, None, None, F, None, bufs), pre + "decode", "params is NULL")
    refused(raw_search(dec, fam, algo + "_search", yd, F, None, bufs), pre + "search", "params is NULL")
    refused(raw_decode(dec, fam, algo + "_decode", yd, None, None, -1, good, bufs), pre + "decode", "bad arguments")
    refused(raw_search(dec, fam, algo + "_search", yd, -1, good, bufs), pre + "search", "bad arguments")
    assert raw_decode(dec, fam, algo + "_decode", yd, None, None, 0, good, {}) == 0          # F == 0: LDPC_OK, no launch
    assert raw_search(dec, fam, algo + "_search", yd, 0, good, {}) == 0
    if mask is not None:
        for missing in ("y", "perm", "parity", "mask", "cw"):
            a = dict(y=yd, perm=bufs["perm"], parity=bufs["parity"], mask=mask, cw=bufs["cw"])
            a[missing] = None
            refused(raw_tep_eval(dec, fam, a["y"], F, a["perm"], a["parity"], a["mask"], a["cw"], None, None),
                    f"ldpc_{fam.prefix}_tep_eval", f"d_{missing} is NULL")
        assert raw_tep_eval(dec, fam, None, 0, None, None, None, None, None, None) == 0


def check_unsupported(fam, dec, y, calls):
    """A code the family refuses: every call of ``calls`` (op -> bufs -> the call through the binding) raises UNSUPPORTED under
    its own name with the family's sentence and the code's shape, and nothing is written."""
    from short_ldpc_decoding_osd_amd import _lib
    import pytest
    assert not fam.serves(dec.n, dec.k) and not getattr(dec, fam.prefix + "_supported")
    bufs = sentinels(dec, fam, len(y), aux=True)
    clean = {k: v.clone() for k, v in bufs.items()}
    for op, call in calls.items():
        with pytest.raises(_lib.LdpcError, match=rf"ldpc_{fam.prefix}_{op} .*" + fam.refusal(dec.n, dec.k)):
            call(bufs)
    torch.cuda.synchronize()
    assert_untouched(bufs, clean)
