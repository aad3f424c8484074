"""-m gpu: the long / low-rate OSD entry points (ldpc_osdl_*) on structured front-end results and at the shape edges no tested
code has -- the pairs and codes of tests/osdl_shapes.py, bit for bit against the CPU models (osdx_model.scan_oracle,
osdx_fs_model.Batch, osdl_pb_model.pb, osdl_model.front_oracle), which tests/test_osdl_shapes_host.py holds to the reference
restatements and whose premises it asserts.  Integers compare equal, floats as uint32.

  1  every search on caller-made (perm, P') pairs of the LONG shapes: zero, equal, all-ones, unit and rank-one rows of P', float
     and grid magnitudes, perm = identity with sorted y' and a random perm with unsorted y' (conventional search and one TEP only)
  2  the SHORT shapes, which the older families serve as well: every output equals ldpc_osdw_* / ldpc_osdx_pb_search's
  3  the six magnitude extremes through the calls of 1
  4  non-zero padding of perm and P': ignored by every search entry point; a device-side count below F
  5  structured codes (zero columns, repeated columns, a rank-one parity part of G) through the device front end and the decodes
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from short_ldpc_decoding_osd_amd import _lib
from tests import osd_family as OF
from tests import osd_shapes as S
from tests import osdl_model, osdl_pb_model
from tests import osdl_shapes as LS
from tests import osdw_fs_model as W
from tests import osdx_fs_model as M
from tests.gpu_util import to_dev
from tests.osd_family import fs_params, new_aux

pytestmark = pytest.mark.gpu
LONG_CASES = [(k, n, name) for k, n in LS.LONG for name in LS.STRUCTURES]
SHORT_CASES = [(k, n, name) for k, n in LS.SHORT for name in LS.STRUCTURES]
CODE_CASES = [(k, n, name) for k, n in LS.CODE_SHAPES for name in LS.CODE_STRUCTURES]
LONG_PAIRS = (("float", "sorted"), ("grid", "sorted"), ("float", "unsorted"))
SCAN_KEYS = ("cw", "metric", "best", "ntep")
FAM = OF.OSDL
_REF = {}


def _graph(k, n, name):
    return LS.context_graph(k, n) if name is None else LS.code(k, n, name)[:2]


def decoder(k, n, name=None):
    """A context of the shape (a plain H = [A | I] code: the searches never read G), or of the structured code ``name``."""
    dec = OF.decoder((k, n, name), _graph)
    assert np.array_equal(dec.code.G, _graph(k, n, name)[1]) and (dec.code.k, dec.code.check_matrix_column) == (k, n)
    assert dec.osdl_supported and dec.osdw_supported == (n <= 128 and n - k <= 64) and dec.osdx_supported == (k <= 64 and n - k <= 64)
    return dec


def ref(kind, c, *args):
    """One model result per (case, search, parameters), shared by the tests and left unchanged.  (errstate: the extremes
    overflow float32 sums to +inf, and all-zero parity magnitudes give 0 / 0 in PB's beta, on purpose.)"""
    key = (kind, c["k"], c["n"], c["name"], c["mode"], c["form"]) + args
    if key not in _REF:
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            if kind == "batch":
                _REF[key] = M.Batch(c["y"], c["perm"], c["Gps"])
            elif kind == "conv":
                F = LS.conv_frames(c["k"], args[0], len(c["y"]))
                _REF[key] = osdl_model.scan_oracle(c["G"], c["y"][:F], args[0], LS.front_of(c))
            elif kind == "fs_batch":
                Fs = LS.fs_pb_frames(c["k"], len(c["y"]))
                _REF[key] = M.Batch(c["y"][:Fs], c["perm"][:Fs], c["Gps"][:Fs])
            elif kind == "fs":
                _REF[key] = ref("fs_batch", c).fs(LS.fs_order(c["k"]), *args)
            elif kind == "pb":
                Fs = LS.fs_pb_frames(c["k"], len(c["y"]))
                _REF[key] = osdl_pb_model.pb(c["y"][:Fs], c["perm"][:Fs], c["Gps"][:Fs], min(2, c["k"]), args[0])
            elif kind == "masks":
                _REF[key] = LS.tep_masks(c, np.random.default_rng(77))
            elif kind == "tep":
                _REF[key] = ref("batch", c).one_tep(ref("masks", c)[args[0]])
    return _REF[key]


def assert_scan(out, want, tag):
    OF.assert_scan(out, want, len(want["best"]), tag)


def assert_fs(out, want, quirk, tag):
    assert_scan(out, OF.fs_view(want, quirk), tag)


def assert_same(a, b, tag, keys=SCAN_KEYS):
    OF.assert_same(a, b, keys, tag)


def dev_front(perm, parity, dec):
    return OF.dev_front(perm, parity, dec, FAM)


def run_searches(dec, c, padding=False):
    """Every ldpc_osdl_* search call the case is defined for -> {(call, parameters...): output dict}; PB results carry ``aux``."""
    k, F = c["k"], len(c["y"])
    yd = to_dev(np.array(c["y"]), dec)
    perm, parity = dev_front(*(LS.dirty(c) if padding else (c["perm"], c["parity"])), dec)
    out = {}
    for order in range(4):
        Fo = LS.conv_frames(k, order, F)
        if Fo:
            out["search", order] = dec.osdl_search(yd, perm[:Fo], parity[:Fo], order)
    for i, masks in enumerate(ref("masks", c)):
        out["tep_eval", i] = dec.osdl_tep_eval(yd, perm, parity, to_dev(LS.split_masks(masks, k).view(np.int64), dec))
    if c["form"] == "sorted":
        Fs = LS.fs_pb_frames(k, F)
        for s in LS.fs_sets(k, c["n"]):
            for quirk in (1, 0):
                out["fs_search", s, quirk] = dec.osdl_fs_search(yd, perm[:Fs], parity[:Fs], fs_params(dec, LS.fs_order(k), s, quirk))
        for snr in LS.PB_SNRS:
            aux = new_aux(dec, Fs)
            r = dec.osdl_pb_search(yd, perm[:Fs], parity[:Fs], dec.osd_params(min(2, k), _lib.OSD_PB, snr_db=snr, aux=aux))
            out["pb_search", snr] = dict(r, aux=aux)
    torch.cuda.synchronize()
    return out


def _check_conv(c, args, got, tag):
    assert_scan(got, ref("conv", c, args[0]), tag)


def _check_tep(c, args, got, tag):
    OF.assert_outputs(got, ref("tep", c, args[0]), where=tag, keys=("cw", "metric", "hd"))


def _check_fs(c, args, got, tag):
    assert_fs(got, ref("fs", c, *args[0]), args[1], tag)


def _check_pb(c, args, got, tag):
    OF.assert_pb(got, got["aux"], ref("pb", c, args[0]), where=tag)


# the calls of run_searches: (checker against the model, outputs compared between runs)
CALLS = {"search": (_check_conv, SCAN_KEYS), "tep_eval": (_check_tep, ("cw", "metric", "hd")),
         "fs_search": (_check_fs, SCAN_KEYS), "pb_search": (_check_pb, SCAN_KEYS + ("aux",))}


def check_against_models(c, out):
    tag = (c["k"], c["n"], c["name"], c["mode"], c["form"])
    assert len(out) == (4 if LS.conv_frames(c["k"], 3, 2) else 3) + 7 + (8 if c["form"] == "sorted" else 0)
    for key, got in out.items():
        CALLS[key[0]][0](c, key[1:], got, tag + key)


# ---------------------------------------------------------------------------------------------------------------------
# 1: searches on caller-made pairs of the LONG shapes, per shape and structure
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,n,name", LONG_CASES)
def test_searches_on_pairs(k, n, name):
    dec = decoder(k, n)
    assert not dec.osdw_supported and not dec.osdx_supported
    for mode, form in LONG_PAIRS:
        c = LS.pair(k, n, name, mode, form)
        masks = ref("masks", c)
        assert max(max(m) for m in masks) >> k == 0
        if name == "zero_rows" and k >= 3:
            assert all(m != 0 for m in masks[5])             # premise: a TEP over zero rows of P' only
        if name in ("equal_rows", "rank_one") and LS.equal_row_groups(k, n, name):
            assert all(bin(m).count("1") > 1 for m in masks[6])   # premise: a TEP over a group of equal rows
        check_against_models(c, run_searches(dec, c))


# ---------------------------------------------------------------------------------------------------------------------
# 2: the SHORT shapes beside the older families
# ---------------------------------------------------------------------------------------------------------------------
def run_older(dec, c, old):
    """The calls of run_searches on the same frames through ldpc_osdw_* (PB: ldpc_osdx_pb_search where k <= 64), keyed alike.
    ``old``: the osd_shapes.pair of the case, in the older layouts."""
    k, F = c["k"], len(c["y"])
    yd = to_dev(np.array(old["y"]), dec)
    perm, p128 = to_dev(np.array(old["perm"]), dec), to_dev(np.array(old["parity128"]).view(np.int64), dec)
    out = {}
    for order in range(4):
        Fo = LS.conv_frames(k, order, F)
        if Fo:
            out["search", order] = dec.osdw_search(yd, perm[:Fo], p128[:Fo], order)
    for i, masks in enumerate(ref("masks", c)):
        out["tep_eval", i] = dec.osdw_tep_eval(yd, perm, p128, to_dev(W.split_masks(masks).view(np.int64), dec))
    if c["form"] == "sorted":
        for s in LS.fs_sets(k, c["n"]):
            for quirk in (1, 0):
                out["fs_search", s, quirk] = dec.osdw_fs_search(yd, perm, p128, fs_params(dec, LS.fs_order(k), s, quirk))
        for snr in LS.PB_SNRS:
            aux = new_aux(dec, F)
            p = dec.osd_params(min(2, k), _lib.OSD_PB, snr_db=snr, aux=aux)
            r = (dec.osdx_pb_search(yd, perm, to_dev(np.array(old["parity64"]).view(np.int64), dec), p) if k <= 64 else
                 dec.osdw_pb_search(yd, perm, p128, p))
            out["pb_search", snr] = dict(r, aux=aux)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("k,n,name", SHORT_CASES)
def test_short_shapes_equal_the_older_family(k, n, name):
    """The pairs of osd_shapes.pair (float and grid, both forms) re-packed into the osdl layouts: every output of every
    ldpc_osdl_* search call equals that of ldpc_osdw_* on the same device, which tests/test_gpu_osd_shapes.py holds to the
    models on exactly these inputs.  n-k = 1, 8, 16, 17 and k = 1, 2 through the FS and PB kernels of this family."""
    dec = decoder(k, n)
    for mode in S.MODES:
        for form in S.FORMS:
            c, old = LS.pair(k, n, name, mode, form), S.pair(k, n, name, mode, form)
            assert np.array_equal(c["y"], old["y"]) and np.array_equal(c["perm"][:, :n], old["perm"][:, :n])
            got, want = run_searches(dec, c), run_older(dec, c, old)
            assert got.keys() == want.keys() and len(got) == (4 if k <= 64 else 3) + 7 + (8 if form == "sorted" else 0)
            for key in got:
                assert_same(got[key], want[key], (k, n, name, mode, form) + key, CALLS[key[0]][1])


# ---------------------------------------------------------------------------------------------------------------------
# 3: magnitude extremes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random_dense", "equal_rows"])
@pytest.mark.parametrize("k,n", LS.LONG)
def test_magnitude_extremes(k, n, name):
    dec = decoder(k, n)
    for form in LS.FORMS:
        c = LS.pair(k, n, name, "extreme", form)
        assert len(c["y"]) == 6
        check_against_models(c, run_searches(dec, c))


# ---------------------------------------------------------------------------------------------------------------------
# 4: non-zero padding is ignored
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,n", LS.LONG)
def test_padding_of_the_inputs_is_ignored(k, n):
    """perm entries at or beyond n set to 0xEEEE, parity rows at or beyond k all ones, bits at or beyond n-k set in every word:
    every output on the pairs of part 1, ldpc_osdl_pb_search's aux among them, equals the clean run's.  ((128,256), (192,320) and
    (192,384) have no padding; LS.dirty asserts that every other shape's inputs did change.)"""
    dec = decoder(k, n)
    for name in LS.STRUCTURES:
        for mode, form in LONG_PAIRS:
            c = LS.pair(k, n, name, mode, form)
            clean, dirty = run_searches(dec, c), run_searches(dec, c, padding=True)
            assert clean.keys() == dirty.keys()
            for key in clean:
                assert_same(dirty[key], clean[key], (k, n, name, mode, form) + key, CALLS[key[0]][1])


def _sentinels(dec, F):
    """The outputs of the search calls (no perm / parity: they are inputs here) and hd."""
    b = OF.sentinels(dec, FAM, F, aux=True)
    return dict({k: b[k] for k in SCAN_KEYS + ("aux",)}, hd=OF.A.sentinel(dec, (F,), torch.int32))


@pytest.mark.parametrize("k,n", [(65, 129), (192, 384)])
def test_padding_through_raw_calls_with_sentinels(k, n):
    """The padded pairs through every C search entry point of the family with a device-side count below F: the frames below the
    count equal the models, nothing at or beyond it is written, and no output the call does not have."""
    dec = decoder(k, n)
    c = LS.pair(k, n, "equal_rows", "grid")
    F = len(c["y"])
    done = LS.conv_frames(k, 2, F) if k >= 100 else F - 2
    assert 0 < done < F
    yd = to_dev(np.array(c["y"]), dec)
    perm, parity = dev_front(*LS.dirty(c), dec)
    count = to_dev(np.array([done], np.int32), dec)
    s = LS.fs_sets(k, n)[0]
    order = LS.fs_order(k)
    front = dict(d_y=yd, d_count=count, F=F, d_perm=perm, d_parity=parity)
    conv = ref("conv", c, 2)
    fs = OF.fs_view(ref("fs", c, *s), 1)
    tep = ref("tep", c, 3)
    md = to_dev(LS.split_masks(ref("masks", c)[3], k).view(np.int64), dec)
    fsp, runs = fs_params(dec, order, s, 1), []

    def run(name, want, keys, call):
        b = _sentinels(dec, F)
        assert call(b) == 0, (name, dec.L.ldpc_last_error())
        runs.append((name, b, {key: want[key] for key in keys}))

    run("osdl_search", conv, SCAN_KEYS, lambda b: OF.raw(dec, FAM, "search", b, order=2, **front))
    run("osdl_fs_search", fs, SCAN_KEYS, lambda b: OF.raw(dec, FAM, "fs_search", b, params=fsp, **front))
    run("osdl_tep_eval", tep, ("cw", "metric", "hd"), lambda b: OF.raw(dec, FAM, "tep_eval", b, d_mask=md, **front))

    def pb_call(b):
        return OF.raw(dec, FAM, "pb_search", b, params=dec.osd_params(order, _lib.OSD_PB, snr_db=1.0, aux=b["aux"]), **front)
    run("osdl_pb_search", ref("pb", c, 1.0), SCAN_KEYS + ("aux",), pb_call)
    torch.cuda.synchronize()
    clean = _sentinels(dec, F)
    assert len(runs) == 4
    for name, b, want in runs:
        OF.assert_outputs(b, want, slice(0, done), where=name, keys=tuple(want))
        for key in b:
            lo = done if key in want else 0                  # an output the call does not have stays untouched altogether
            assert torch.equal(b[key][lo:], clean[key][lo:]), (name, key)


# ---------------------------------------------------------------------------------------------------------------------
# 5: structured codes through the device front end
# ---------------------------------------------------------------------------------------------------------------------
def assert_front(got, want, k, n, rows=slice(None)):
    """perm, parity and nswaps against the oracle, whose arrays are zero in the padding."""
    OF.assert_front(FAM, SimpleNamespace(n=n, k=k), got[0], got[1], want, got[2], rows)


def decode_frames(k):
    """The FS and PB decodes run on the first 8 frames at k >= 100 (the CPU models take about 0.3 s per frame there), else on
    all 24."""
    return 8 if k >= 100 else LS.CODE_FRAMES


def code_ref(kind, k, n, name, mode, *args):
    """The models of a structured code's decodes on the oracle's front, one result per (code, mode, search), shared."""
    key = ("code", kind, k, n, name, mode) + args
    if key not in _REF:
        cc = LS.code_case(k, n, name, mode)
        Fd = LS.CODE_FRAMES if kind == "conv" else decode_frames(k)
        y, front = cc["y"][:Fd], tuple(part[:Fd] for part in cc["front"][:4])
        if kind == "conv":
            _REF[key] = osdl_model.scan_oracle(cc["G"], y, 1, front)
        elif kind == "fs":
            _REF[key] = M.Batch(y, front[0], front[3]).fs(LS.fs_order(k), *LS.fs_sets(k, n)[0])
        elif kind == "pb":
            _REF[key] = osdl_pb_model.pb(y, front[0], front[3], 2, args[0])
    return _REF[key]


@pytest.mark.parametrize("mode", LS.MODES)
@pytest.mark.parametrize("k,n,name", CODE_CASES)
def test_structured_codes_through_the_front_end(k, n, name, mode):
    """A code whose G has zero columns, repeated columns or a rank-one parity part: ldpc_osdl_front on 24 frames against the
    oracle (grid mode: sort ties meet zero and repeated columns), prefilled outputs: the padding is written as zero; and
    ldpc_osdl_decode at order 1 against front + search and against the model on the oracle's front."""
    dec = decoder(k, n, name)
    cc = LS.code_case(k, n, name, mode)
    y, front = cc["y"], cc["front"]
    F = len(y)
    assert F == LS.CODE_FRAMES
    yd = to_dev(y, dec)
    S_, W_, Wp = LS.layout(k, n)
    perm = torch.full((F, 64 * S_), 0x6EEE, dtype=torch.int16, device=dec.device)
    parity = torch.full((F, 64 * W_) + ((Wp,) if Wp > 1 else ()), -1, dtype=torch.int64, device=dec.device)
    ns = torch.full((F,), -7, dtype=torch.int32, device=dec.device)
    got = dec.osdl_front(yd, out=(perm, parity, ns))
    torch.cuda.synchronize()
    assert_front(got, front, k, n)
    conv = code_ref("conv", k, n, name, mode)
    only = dec.osdl_search(yd, got[0], got[1], 1)
    full = dec.osdl_decode(yd, 1)
    torch.cuda.synchronize()
    tag = (k, n, name, mode)
    assert_scan(only, conv, tag + ("front + search",))
    assert_scan(full, conv, tag + ("decode",))
    assert_same(full, only, tag)
    assert_front((full["perm"], full["parity"], None), front, k, n)


@pytest.mark.parametrize("k,n,name", CODE_CASES)
def test_structured_codes_through_fs_and_pb_decode(k, n, name):
    """ldpc_osdl_fs_decode on the first parameter set, in both quirk modes, and ldpc_osdl_pb_decode at order 2 and 1.0 dB (aux
    included) on the float frames of the structured codes (``decode_frames``), against the models on the oracle's front."""
    dec = decoder(k, n, name)
    cc = LS.code_case(k, n, name, "float")
    Fd = decode_frames(k)
    yd = to_dev(cc["y"][:Fd], dec)
    front = cc["front"]
    rows = slice(0, Fd)
    fs, s = code_ref("fs", k, n, name, "float"), LS.fs_sets(k, n)[0]
    for quirk in (1, 0):
        out = dec.osdl_fs_decode(yd, fs_params(dec, LS.fs_order(k), s, quirk))
        torch.cuda.synchronize()
        assert_fs(out, fs, quirk, (k, n, name, "fs_decode", quirk))
        assert_front((out["perm"], out["parity"], None), front, k, n, rows)
    want = code_ref("pb", k, n, name, "float", 1.0)
    aux = new_aux(dec, Fd)
    out = dec.osdl_pb_decode(yd, dec.osd_params(2, _lib.OSD_PB, snr_db=1.0, aux=aux))
    torch.cuda.synchronize()
    assert_scan(out, want, (k, n, name, "pb_decode"))
    assert np.array_equal(aux.cpu().numpy(), want["aux"]), (k, n, name)
    assert_front((out["perm"], out["parity"], None), front, k, n, rows)
