"""-m gpu: FS-OSD and the one-TEP primitive for short codes of any shape (ldpc_osdx_fs_search / _fs_decode / _tep_eval) --
bit-exact against the vectorised model of tests/osdx_fs_model.py on (96,48), (121,60), the zoo's `short` (40,17) and `thin`
(24,11) and CCSDS (128,64), and against the specialised osd_fs_kernel / osd_tep_eval_kernel on CCSDS.  The inputs and the
branches they reach are those tests/test_osdx_fs_host.py asserts on the CPU."""
import numpy as np
import pytest
import torch

from short_ldpc_decoding_osd_amd import _lib
from tests import osd_family as OF
from tests import osdx_fs_model as M
from tests import nms_graphs, osdx_model
from tests.gpu_util import to_dev, words_np
from tests.osd_family import assert_fs, decoder, fs_params

pytestmark = pytest.mark.gpu
ALPHA0 = 0.669435
FAM = OF.OSDX


def assert_front(perm, parity, front, dec):
    OF.assert_front(FAM, dec, perm, parity, front)


def _sentinels(dec, F):
    return OF.sentinels(dec, FAM, F)


def _raw_decode(dec, *args, **kw):
    return OF.raw_decode(dec, FAM, "fs_decode", *args, **kw)


def _raw_search(dec, *args):
    return OF.raw_search(dec, FAM, "fs_search", *args)


# ---------------------------------------------------------------------------------------------------------------------
# 1: parity with the model, every parameter set, both quirks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,order3", [(n, False) for n in osdx_model.CODES] + [("ldpc_96_48", True)])
def test_fs_matches_the_model(name, order3):
    dec = decoder(name)
    y, _, front, _, order, sets, refs = M.parity_case(name, order3)
    yd = to_dev(y, dec)
    for s, ref in zip(sets, refs):
        for quirk in (1, 0):
            p = fs_params(dec, order, s, quirk)
            full = dec.osdx_fs_decode(yd, p)
            out = dec.osdx_fs_search(yd, full["perm"], full["parity"], p)
            torch.cuda.synchronize()
            assert_front(full["perm"], full["parity"], front, dec)
            assert_fs(full, ref, quirk, where=f"decode {s} quirk {quirk}")
            assert_fs(out, ref, quirk, where=f"search {s} quirk {quirk}")
    # premise: somewhere the two quirk answers differ, so both modes were told apart
    assert any((r["best_ref"] != r["best_hit"]).any() for r in refs)


# ---------------------------------------------------------------------------------------------------------------------
# 2: a planted stop in class 3 at a chosen rank, on caller-made front-end results
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,n,which", M.PLANTED)
def test_planted_stop_in_class_3(k, n, which):
    dec = decoder(M.PLANTED_CODE[k])
    assert (dec.k, dec.n) == (k, n)
    case = M.planted(k, n, which)
    order, *s = case["params"]
    ref = case["batch"].fs(order, *s)
    at = 1 + k + k * (k - 1) // 2 + case["rank"]
    assert ref["best_hit"][0] == at and ref["ntep"][0] == at + 1
    yd, perm = to_dev(case["y"], dec), to_dev(case["perm"], dec)
    parity = to_dev(case["parity"].view(np.int64), dec)
    for quirk in (1, 0):
        out = dec.osdx_fs_search(yd, perm, parity, fs_params(dec, order, s, quirk))
        torch.cuda.synchronize()
        assert_fs(out, ref, quirk, where=f"quirk {quirk}")
        assert int(out["ntep"].cpu()[0]) == at + 1
        if not quirk:
            assert int(out["best"].cpu()[0]) == at           # the stop at exactly the FS rank of {a, b, c}


# ---------------------------------------------------------------------------------------------------------------------
# 3: (128,64) through the any-shape kernel equals osd_fs_kernel
# ---------------------------------------------------------------------------------------------------------------------
def test_ccsds_equals_the_specialised_fs_kernel():
    dec = decoder("ccsds")
    y, _, _, _, order, sets, refs = M.parity_case("ccsds")
    yd = to_dev(y, dec)
    perm, parity, _ = dec.osd_front(yd)
    for s, ref in zip(sets, refs):
        for quirk in (1, 0):
            p = fs_params(dec, order, s, quirk)
            got = dec.osdx_fs_search(yd, perm, parity, p)
            want = dec.osd_search(yd, perm, parity, p)
            torch.cuda.synchronize()
            for key in ("cw", "best", "ntep"):
                assert torch.equal(got[key], want[key]), (s, quirk, key)
            assert torch.equal(got["metric"].view(torch.int32), want["metric"].view(torch.int32))
            assert_fs(got, ref, quirk)


# ---------------------------------------------------------------------------------------------------------------------
# 4: one given TEP per frame
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", osdx_model.CODES)
def test_tep_eval_matches_the_model(name):
    dec = decoder(name)
    F = 48
    y, _, front, b = M.batch(name, M.PARITY[name][0], 192, 7)
    rng = np.random.default_rng(3)
    masks = np.zeros(F, np.uint64)
    for f in range(F):                                         # weights 0..5, eight frames each
        for pos in rng.choice(dec.k, f % 6, replace=False):
            masks[f] |= np.uint64(1) << np.uint64(pos)
    ref = b.one_tep(masks)                                     # the first F frames of the batch
    yd = to_dev(y[:F], dec)
    perm, parity = to_dev(front[0][:F], dec), to_dev(front[1][:F].view(np.int64), dec)
    md = to_dev(masks.view(np.int64), dec)
    out = dec.osdx_tep_eval(yd, perm, parity, md)
    torch.cuda.synchronize()
    assert np.array_equal(words_np(out["cw"]), ref["cw"])
    assert np.array_equal(out["metric"].cpu().numpy().view(np.uint32), ref["metric"].view(np.uint32))
    assert np.array_equal(out["hd"].cpu().numpy(), ref["hd"])
    if name == "ccsds":
        old = dec.osd_tep_eval(yd, perm, parity, md)
        torch.cuda.synchronize()
        assert torch.equal(out["cw"], old["cw"]) and torch.equal(out["hd"], old["hd"])
        assert torch.equal(out["metric"].view(torch.int32), old["metric"].view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------
# 5: frame lists, device-side counts, nullable outputs, counters, several frames per wavefront, refusals, graph capture
# ---------------------------------------------------------------------------------------------------------------------
LISTED_SET = (0.02, 10.5, 30)


@pytest.fixture(scope="module")
def listed():
    """array_121_60: 600 frames at 2.0 dB through NMS and ldpc_compact; the model of the listed frames at order 2."""
    dec = decoder("array_121_60")
    G = osdx_model.graph("array_121_60")[1]
    y, cw = osdx_model.frames("array_121_60", 2.0, 600, 21)
    yd = to_dev(y, dec)
    res = dec.nms(yd, 10, ALPHA0)
    index, count = dec.compact(res["fail"])
    torch.cuda.synchronize()
    nf = int(count.cpu()[0])
    idx = index[:nf].cpu().numpy()
    assert 40 < nf < 600 and np.all(np.diff(idx) > 0)
    front = osdx_model.front_oracle(G, y[idx])
    ref = M.Batch(y[idx], front[0], front[3]).fs(2, *LISTED_SET)
    assert ref["hit"].any() and not ref["hit"].all()
    p = fs_params(dec, 2, LISTED_SET, 1)
    return dict(dec=dec, y=y, yd=yd, labels=cw, label_rows=idx, index=index, count=count, nf=nf, rows=np.arange(nf),
                ref=OF.fs_view(ref, 1), front=front, arg=lambda bufs: p, distinct_ntep=3)


@pytest.mark.parametrize("which", ["smaller", "equal", "larger"])
def test_frame_list_and_device_count(listed, which):
    OF.check_frame_list(FAM, "fs_decode", listed, which)


@pytest.mark.parametrize("off", ["metric", "best", "ntep", "counts", "label"])
def test_nullable_outputs_and_counters(listed, off):
    OF.check_nullable(FAM, "fs_decode", listed, off)


def test_one_wavefront_decodes_several_frames_in_turn():
    """More frames than the grid's 65536 workgroups: wavefront b decodes frame b and then frame 65536 + b.  The frames that
    share a wavefront are checked against the model, all of them against the same frames decoded one per wavefront."""
    name, s = "thin", (0.0, 3.5, 5)
    dec = decoder(name)
    G = osdx_model.graph(name)[1]
    p = fs_params(dec, 3, s, 1)

    def model(ys):
        front = osdx_model.front_oracle(G, ys)
        return front, OF.fs_view(M.Batch(ys, front[0], front[3]).fs(3, *s), 1)
    OF.check_frames_in_turn(FAM, dec, osdx_model.frames(name, 0.0, 65536 + 300, 31)[0], lambda yd: dec.osdx_fs_decode(yd, p), model,
                            distinct_ntep=3)


@pytest.mark.parametrize("name", ["wimax_1056", "wide"])
def test_unsupported_shapes_are_refused(name):
    dec = decoder(name)
    yd = to_dev(nms_graphs.frames(name, 2.0, 4, 1)[0], dec)
    p = fs_params(dec, 1, (0.1, 4.5, 30), 1)
    mask = torch.zeros(4, dtype=torch.int64, device=dec.device)
    OF.check_unsupported(FAM, dec, yd, {
        "fs_search": lambda b: dec.osdx_fs_search(yd, b["perm"], b["parity"], p, out=b),
        "fs_decode": lambda b: dec.osdx_fs_decode(yd, p, perm=b["perm"], parity=b["parity"], out=b),
        "tep_eval": lambda b: dec.osdx_tep_eval(yd, b["perm"], b["parity"], mask)})


def test_bad_arguments_are_refused_and_the_old_entry_points_keep_their_refusal(monkeypatch):
    dec = decoder("ldpc_96_48")
    y, _ = osdx_model.frames("ldpc_96_48", 1.5, 4, 2)
    yd = to_dev(y, dec)
    bufs = _sentinels(dec, 4)
    clean = {k: v.clone() for k, v in bufs.items()}
    s = (0.1, 4.5, 30)
    good = fs_params(dec, 2, s, 1)
    mask = torch.zeros(4, dtype=torch.int64, device=dec.device)
    OF.check_bad_arguments(FAM, "fs", dec, yd, bufs, lambda order, **kw: fs_params(dec, order, s, 1, **kw), good, mask)
    old = r"\(-5\).*OSD kernels need an \(n=128, k=64\) code; this one is \(96,48\)"
    with pytest.raises(_lib.LdpcError, match=old):
        dec.osd_decode(yd, 2, params=good)
    with pytest.raises(_lib.LdpcError, match=old):
        dec.osd_search(yd, bufs["perm"], bufs["parity"], good, out=bufs)
    with pytest.raises(_lib.LdpcError, match=old):
        dec.osd_tep_eval(yd, bufs["perm"], bufs["parity"], mask)
    torch.cuda.synchronize()
    OF.assert_untouched(bufs, clean)
    # a mask with fewer rows than frames (the kernels read a row per frame) is refused before any launch: every call of the
    # library asks for the stream
    ccsds = decoder("ccsds")
    yc = to_dev(osdx_model.frames("ccsds", 1.5, 4, 2)[0], ccsds)
    perm, parity, _ = ccsds.osd_front(yc)
    torch.cuda.synchronize()

    def no_launch():
        raise AssertionError("a launch was prepared")
    monkeypatch.setattr(ccsds, "_stream", no_launch)
    for tep_eval in (ccsds.osdx_tep_eval, ccsds.osd_tep_eval):
        with pytest.raises(ValueError, match="mask: 3 rows for 4 frames"):
            tep_eval(yc, perm, parity, mask[:3])


def test_order_is_bounded_by_k():
    """A (6,2) code: weight class 3 does not exist, so order 3 is refused; order 2 scans the single pair."""
    dec, G, y = OF.tiny_case()
    yd = to_dev(y, dec)
    bufs = _sentinels(dec, 64)
    clean = {k: v.clone() for k, v in bufs.items()}
    s = (0.0, 1.5, 30)
    with pytest.raises(_lib.LdpcError, match=r"\(-1\).*ldpc_osdx_fs_decode: order 3 outside 0\.\.2"):
        dec.osdx_fs_decode(yd, fs_params(dec, 3, s, 1), perm=bufs["perm"], parity=bufs["parity"], out=bufs)
    torch.cuda.synchronize()
    OF.assert_untouched(bufs, clean)
    front = osdx_model.front_oracle(G, y)
    ref = M.Batch(y, front[0], front[3]).fs(2, *s)
    assert (ref["depth"] == 2).any() and ref["hit"].any()
    for quirk in (1, 0):
        out = dec.osdx_fs_decode(yd, fs_params(dec, 2, s, quirk))
        torch.cuda.synchronize()
        assert_fs(out, ref, quirk)


def test_fs_decode_is_graph_capturable():
    dec = decoder("array_121_60")
    F = 96
    p = fs_params(dec, 2, LISTED_SET, 1)
    ys = [osdx_model.frames("array_121_60", 1.5, F, s)[0] for s in (41, 42, 43)]
    bufs = _sentinels(dec, F)
    ybuf = to_dev(ys[0], dec)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):               # no eager call first: the entry point holds no per-stream state
        dec.osdx_fs_decode(ybuf, p, perm=bufs["perm"], parity=bufs["parity"], out=bufs)
    G = osdx_model.graph("array_121_60")[1]
    for y in ys[1:]:
        ybuf.copy_(to_dev(y, dec))
        graph.replay()
        torch.cuda.synchronize()
        front = osdx_model.front_oracle(G, y)
        assert_front(bufs["perm"], bufs["parity"], front, dec)
        assert_fs(bufs, M.Batch(y, front[0], front[3]).fs(2, *LISTED_SET), 1)
