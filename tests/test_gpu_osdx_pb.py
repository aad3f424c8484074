"""-m gpu: PB-OSD for short codes of any shape (ldpc_osdx_pb_search / _pb_decode) -- bit-exact against the model of
tests/osdx_pb_model.py on (96,48), (121,60), the zoo's `short` (40,17) and `thin` (24,11) and CCSDS (128,64), and against the
specialised PB routes on CCSDS.  The inputs and the branches they reach are those tests/test_osdx_pb_host.py asserts on the CPU."""
import numpy as np
import pytest
import torch

from short_ldpc_decoding_osd_amd import _lib
from tests import nms_graphs, osdx_model
from tests import osd_family as OF
from tests import osdx_pb_model as M
from tests.gpu_util import pack_np, to_dev
from tests.osd_family import assert_pb, decoder, new_aux, pb_params

pytestmark = pytest.mark.gpu
FAM = OF.OSDX
KEYS = ("cw", "metric", "best", "ntep", "aux")


def assert_front(perm, parity, front, dec, pick=slice(None)):
    OF.assert_front(FAM, dec, perm, parity, front, rows=pick)


def _sentinels(dec, F):
    return OF.sentinels(dec, FAM, F, aux=True)


def _raw_decode(dec, *args, **kw):
    return OF.raw_decode(dec, FAM, "pb_decode", *args, **kw)


def _raw_search(dec, *args):
    return OF.raw_search(dec, FAM, "pb_search", *args)


# ---------------------------------------------------------------------------------------------------------------------
# 1: parity with the model, every set, both routes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,i", M.CASES)
def test_pb_matches_the_model(name, i):
    dec = decoder(name)
    y, _, front, order, snr_db, ref = M.case(name, i)
    yd = to_dev(y, dec)
    aux1, aux2 = new_aux(dec, len(y)), new_aux(dec, len(y))
    full = dec.osdx_pb_decode(yd, pb_params(dec, order, snr_db, aux1))
    out = dec.osdx_pb_search(yd, to_dev(front[0], dec), to_dev(front[1].view(np.int64), dec), pb_params(dec, order, snr_db, aux2))
    torch.cuda.synchronize()
    assert_front(full["perm"], full["parity"], front, dec)
    assert_pb(full, aux1, ref, where="decode")
    assert_pb(out, aux2, ref, where="search")


# ---------------------------------------------------------------------------------------------------------------------
# 2: (128,64) through the any-shape kernel equals the specialised routes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(M.SETS["ccsds"])))
def test_ccsds_equals_the_specialised_pb_routes(i):
    dec = decoder("ccsds")
    y, _, _, order, snr_db, ref = M.case("ccsds", i)
    yd = to_dev(y, dec)
    perm, parity, _ = dec.osd_front(yd)
    aux = new_aux(dec, len(y))
    got = dec.osdx_pb_search(yd, perm, parity, pb_params(dec, order, snr_db, aux))
    torch.cuda.synchronize()
    assert_pb(got, aux, ref)
    for path in (None, "replay"):
        aux_w = new_aux(dec, len(y))
        want = dec.osd_search(yd, perm, parity, pb_params(dec, order, snr_db, aux_w, pb_path=path))
        torch.cuda.synchronize()
        for key in ("cw", "best", "ntep"):
            assert torch.equal(got[key], want[key]), (path, key)
        assert torch.equal(got["metric"].view(torch.int32), want["metric"].view(torch.int32)), path
        assert torch.equal(aux, aux_w), path


# ---------------------------------------------------------------------------------------------------------------------
# 3: equal magnitudes on the MRB: the visit order is the insertion order
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,order,levels", [("short", 3, 1), ("short", 3, 2), ("array_121_60", 2, 1), ("array_121_60", 2, 2)])
def test_equal_magnitudes(name, order, levels):
    dec = decoder(name)
    c = M.equal_magnitudes(name, order, levels)
    aux = new_aux(dec, len(c["y"]))
    out = dec.osdx_pb_search(to_dev(c["y"], dec), to_dev(c["perm"], dec), to_dev(c["parity"].view(np.int64), dec),
                             pb_params(dec, order, c["snr_db"], aux))
    torch.cuda.synchronize()
    assert_pb(out, aux, c["model"])


# ---------------------------------------------------------------------------------------------------------------------
# 4, 5: frame lists, device-side counts, nullable outputs, counters
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def listed():
    """ldpc_96_48, the 96 frames of set 1 (order 2, both stop rules): a list of 40 of them with repeats, not ascending."""
    dec = decoder("ldpc_96_48")
    y, cw, front, order, snr_db, ref = M.case("ldpc_96_48", 1)
    rng = np.random.default_rng(17)
    idx = np.concatenate([rng.integers(0, len(y), 30), [95, 60, 60, 33, 9, 9, 9, 2, 0, 0]]).astype(np.int32)
    nf = len(idx)
    assert len(set(idx.tolist())) < nf and np.any(np.diff(idx) < 0)
    assert len(set(ref["aux"][idx, 3].tolist())) == 2 and len(set(ref["ntep"][idx].tolist())) > 3
    return dict(dec=dec, yd=to_dev(y, dec), labels=cw, label_rows=idx, index=to_dev(idx, dec),
                count=to_dev(np.array([nf], np.int32), dec), nf=nf, rows=idx, ref=ref, front=front, order=order, snr_db=snr_db,
                arg=lambda bufs: pb_params(dec, order, snr_db, bufs["aux"]))


@pytest.mark.parametrize("which", ["smaller", "equal", "larger"])
def test_frame_list_and_device_count(listed, which):
    OF.check_frame_list(FAM, "pb_decode", listed, which)


@pytest.mark.parametrize("off", ["metric", "best", "ntep", "aux", "counts", "label"])
def test_nullable_outputs_and_counters(listed, off):
    OF.check_nullable(FAM, "pb_decode", listed, off)


# ---------------------------------------------------------------------------------------------------------------------
# 6: several frames per wavefront
# ---------------------------------------------------------------------------------------------------------------------
def test_one_wavefront_decodes_several_frames_in_turn():
    """More frames than the grid's 65536 workgroups: wavefront b decodes frame b and then frame 65536 + b.  Four distinct
    frames are tiled through d_index so that a wavefront meets a full scan (834 TEPs) and then a search that stops at its first
    TEP, or the other way round: what a frame leaves in the frontier slots, the chunk minima or the CDF table must not reach the
    next one."""
    dec = decoder("short")
    y, labels, ref = M.in_turn("short", 3, 1.0)
    assert ref["ntep"].tolist() == [834, 834, 1, 1] and ref["aux"][:, 3].tolist() == [0, 0, 1, 1]
    extra = 300
    F = 65536 + extra
    f = np.arange(F)
    # frame f < 65536: full scan for even f, one-TEP stop for odd f; frame 65536 + b: the other kind than frame b
    kind = np.where(f < 65536, f & 1, 1 - (f & 1))
    idx = (2 * kind + ((f >> 1) & 1)).astype(np.int32)
    assert {(a < 2, b < 2) for a, b in zip(idx[:extra].tolist(), idx[65536:].tolist())} == {(True, False), (False, True)}
    aux = new_aux(dec, F)
    label = to_dev(pack_np(labels).view(np.int64), dec)
    counts = torch.zeros(3, dtype=torch.int64, device=dec.device)
    out = dec.osdx_pb_decode(to_dev(y, dec), pb_params(dec, 3, 1.0, aux), index=to_dev(idx, dec), F=F, label_bits=label, counts=counts)
    torch.cuda.synchronize()
    pick = torch.from_numpy(idx.astype(np.int64)).to(dec.device)
    want = dict(cw=to_dev(ref["cw"].view(np.int64), dec), metric=to_dev(ref["metric"], dec), best=to_dev(ref["best"], dec),
                ntep=to_dev(ref["ntep"], dec), aux=to_dev(ref["aux"], dec))
    got = dict(out, aux=aux)
    for k in KEYS:
        a, b = got[k], want[k][pick]
        if k == "metric":
            a, b = a.view(torch.int32), b.view(torch.int32)
        assert torch.equal(a, b), k
    wrong = np.any(ref["cw"] != pack_np(labels), axis=1)[idx]
    assert counts.cpu().tolist() == [F, int(wrong.sum()), int(ref["ntep"][idx].astype(np.int64).sum())]


# ---------------------------------------------------------------------------------------------------------------------
# 7: refusals
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wimax_1056", "wide"])
def test_unsupported_shapes_are_refused(name):
    dec = decoder(name)
    yd = to_dev(nms_graphs.frames(name, 2.0, 4, 1)[0], dec)
    OF.check_unsupported(FAM, dec, yd, {
        "pb_search": lambda b: dec.osdx_pb_search(yd, b["perm"], b["parity"], pb_params(dec, 1, 1.0, b["aux"]), out=b),
        "pb_decode": lambda b: dec.osdx_pb_decode(yd, pb_params(dec, 1, 1.0, b["aux"]), perm=b["perm"], parity=b["parity"], out=b)})


def test_bad_arguments_and_shapes():
    dec = decoder("ldpc_96_48")
    y, _ = osdx_model.frames("ldpc_96_48", 1.5, 4, 2)
    yd = to_dev(y, dec)
    bufs = _sentinels(dec, 4)
    clean = {k: v.clone() for k, v in bufs.items()}
    good = pb_params(dec, 2, 1.5, bufs["aux"])
    OF.check_bad_arguments(FAM, "pb", dec, yd, bufs, lambda order, **kw: pb_params(dec, order, 1.5, **kw), good)
    old = r"\(-5\).*OSD kernels need an \(n=128, k=64\) code; this one is \(96,48\)"
    with pytest.raises(_lib.LdpcError, match=old):                         # the (128,64) entry points keep their refusal
        dec.osd_decode(yd, 2, params=good)
    with pytest.raises(_lib.LdpcError, match=old):
        dec.osd_search(yd, bufs["perm"], bufs["parity"], good, out=bufs)
    torch.cuda.synchronize()
    OF.assert_untouched(bufs, clean)


def test_order_is_bounded_by_k():
    """A (6,2) code: weight class 3 does not exist, so order 3 is refused; order 2 visits {1}, {0}, {0, 1} at most."""
    dec, G, y = OF.tiny_case()
    yd = to_dev(y, dec)
    bufs = _sentinels(dec, 64)
    clean = {k: v.clone() for k, v in bufs.items()}
    with pytest.raises(_lib.LdpcError, match=r"\(-1\).*ldpc_osdx_pb_decode: order 3 outside 0\.\.2"):
        dec.osdx_pb_decode(yd, pb_params(dec, 3, 0.0), perm=bufs["perm"], parity=bufs["parity"], out=bufs)
    torch.cuda.synchronize()
    OF.assert_untouched(bufs, clean)
    front = osdx_model.front_oracle(G, y)
    for order in (0, 1, 2):
        ref = M.pb(y, front[0], front[3], order, 0.0)
        aux = new_aux(dec, 64)
        out = dec.osdx_pb_decode(yd, pb_params(dec, order, 0.0, aux))
        torch.cuda.synchronize()
        assert_pb(out, aux, ref, where=f"order {order}")
        if order == 0:
            assert ref["ntep"].tolist() == [1] * 64 and not ref["aux"].any()


# ---------------------------------------------------------------------------------------------------------------------
# 8: graph capture
# ---------------------------------------------------------------------------------------------------------------------
def test_pb_decode_is_graph_capturable():
    dec = decoder("ldpc_96_48")
    F = 16
    a, b = M.case("ldpc_96_48", 1), M.case("ldpc_96_48", 3)               # the same order and snr_db: one set of parameters
    assert (a[3], a[4]) == (b[3], b[4])
    bufs = _sentinels(dec, F)
    p = pb_params(dec, a[3], a[4], bufs["aux"])
    ybuf = torch.zeros((F, dec.n), dtype=torch.float32, device=dec.device)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):               # no eager call first: the entry point holds no per-stream state
        dec.osdx_pb_decode(ybuf, p, perm=bufs["perm"], parity=bufs["parity"], out=bufs)   # front end, then search: one chain
    for y, front, ref in ((a[0][:F], a[2], a[5]), (b[0], b[2], b[5])):
        ybuf.copy_(to_dev(y, dec))
        graph.replay()
        torch.cuda.synchronize()
        assert_front(bufs["perm"], bufs["parity"], front, dec, slice(0, F))
        assert_pb(bufs, bufs["aux"], ref, slice(0, F), np.arange(F))
