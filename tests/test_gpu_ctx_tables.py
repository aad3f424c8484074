"""-m gpu: a context owns ONE set of OSD tables (G columns, conventional TEP table, FS visit-order table), built with the
context and freed with it, and both OSD families -- the (128,64) kernels behind ``osd_*`` and the any-shape kernels behind
``osdx_*`` -- read it.  Per code: every family the code has is run on one decoder, the decoder is destroyed, a second one is
created, and the second must return the same bits; a code without tables must be refused with the same texts both times.
On CCSDS the two families also take turns on one context, and every turn must repeat the family's first answer."""
import numpy as np
import pytest
import torch

from short_ldpc_decoding_osd_amd import _lib
from tests import osdx_model
from tests.gpu_util import to_dev

pytestmark = pytest.mark.gpu
FRAMES = 8
OSD_TEXT = r"\(-5\).*OSD kernels need an \(n=128, k=64\) code; this one is \({n},{k}\)"
OSDX_TEXT = r"\(-5\).*1 <= k <= 64 and 1 <= n-k <= 64.*\({n},{k}\)"
# code -> n, k within the any-shape bounds or beyond them, which families serve it: osd_*, osdx_*
CODES = {"ccsds": (128, True, True, True), "short": (40, True, False, True), "wimax_1056": (1056, False, False, False)}


def make_decoder(name):
    from short_ldpc_decoding_osd_amd.runtime import Decoder
    return Decoder(osdx_model.make_code(name))


def destroy(dec):
    torch.cuda.synchronize()
    dec.__del__()          # ldpc_ctx_destroy now, not whenever the collector runs
    assert not dec._ctx.value


def bits(out):
    """Every tensor of a result dict as raw bytes (a float compares by its bits)."""
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().tobytes() for k, v in out.items() if v is not None}


def osd_fs(dec, yd):
    return bits(dec.osd_decode(yd, 2, params=dec.osd_params(2, _lib.OSD_FS)))


def osd_conv(dec, yd):
    return bits(dec.osd_decode(yd, 2))


def osdx_fs(dec, yd):
    return bits(dec.osdx_fs_decode(yd, dec.osd_params(2, _lib.OSD_FS)))


def osdx_conv(dec, yd):
    return bits(dec.osdx_decode(yd, 1))


def refusals(dec, yd, osd, osdx):
    """The families that do not serve the code refuse, each with its own text."""
    if not osd:
        text = OSD_TEXT.format(n=dec.n, k=dec.k)
        with pytest.raises(_lib.LdpcError, match=text):
            dec.osd_decode(yd, 2)
        with pytest.raises(_lib.LdpcError, match=text):
            dec.osd_decode(yd, 2, params=dec.osd_params(2, _lib.OSD_FS))
    if not osdx:
        text = OSDX_TEXT.format(n=dec.n, k=dec.k)
        with pytest.raises(_lib.LdpcError, match=text):
            dec.osdx_decode(yd, 1)
        with pytest.raises(_lib.LdpcError, match=text):
            dec.osdx_fs_decode(yd, dec.osd_params(2, _lib.OSD_FS))


def run_families(dec, yd, osd, osdx):
    assert dec.osdx_supported is osdx
    res = {}
    if osd:
        res["osd_conv"], res["osd_fs"] = osd_conv(dec, yd), osd_fs(dec, yd)
    if osdx:
        res["osdx_conv"], res["osdx_fs"] = osdx_conv(dec, yd), osdx_fs(dec, yd)
    refusals(dec, yd, osd, osdx)
    return res


@pytest.mark.parametrize("name", list(CODES))
def test_a_second_context_of_the_code_repeats_the_first(name):
    n, within, osd, osdx = CODES[name]
    y, _ = osdx_model.frames(name, 1.0, FRAMES, 7)
    first = make_decoder(name)
    assert first.n == n and (1 <= first.k <= 64 and 1 <= n - first.k <= 64) is within
    a = run_families(first, to_dev(y, first), osd, osdx)
    destroy(first)
    second = make_decoder(name)
    b = run_families(second, to_dev(y, second), osd, osdx)
    destroy(second)
    assert a.keys() == b.keys() and len(a) == 2 * (osd + osdx)
    for call in a:
        assert a[call].keys() == b[call].keys() >= {"cw", "metric", "best", "ntep"}, call
        for key in a[call]:
            assert a[call][key] == b[call][key], (call, key)
    # premise: the searches were searches -- somewhere a scan went beyond the order-0 candidate and chose another one
    for call in a:
        ntep, best = (np.frombuffer(a[call][key], np.int32) for key in ("ntep", "best"))
        assert ntep.size == FRAMES and ntep.max() > 1 and best.max() > 0, call


def test_the_two_families_take_turns_on_one_context():
    dec = make_decoder("ccsds")
    y, _ = osdx_model.frames("ccsds", 1.0, FRAMES, 7)
    yd = to_dev(y, dec)
    turns = (osd_fs, osdx_fs, osd_conv, osdx_conv)
    first = [f(dec, yd) for f in turns]
    for _ in range(2):
        for f, want in zip(turns, first):
            assert f(dec, yd) == want, f.__name__
    # the FS scans of the two families read the same table: same codewords, metrics, ranks and counts
    for key in ("cw", "metric", "best", "ntep"):
        assert first[0][key] == first[1][key], key
    destroy(dec)
