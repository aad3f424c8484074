"""-m gpu: FS-OSD and the one-TEP primitive for high-rate short codes (ldpc_osdw_fs_search / _fs_decode / _tep_eval: n <= 128,
1 <= n-k <= 64, k up to 127) -- bit-exact against the model of tests/osdx_fs_model.py on (121,80), the synthetic (128,96) and
(128,65) and the zoo's deg65 (80,74), and against ldpc_osdx_fs_* / _tep_eval on CCSDS (128,64) and (121,60).  The inputs and the
branches they reach are those tests/test_osdw_fs_host.py asserts on the CPU.  Floats compare by their bits."""
import numpy as np
import pytest
import torch

from short_ldpc_decoding_osd_amd import _lib
from tests import nms_graphs, osdw_model, osdx_model
from tests import osd_family as OF
from tests import osdw_fs_model as W
from tests import osdx_fs_model as M
from tests.gpu_util import to_dev, words_np
from tests.osd_family import assert_fs, assert_same, decoder, fs_params

pytestmark = pytest.mark.gpu
ALPHA0 = 0.669435
FAM = OF.OSDW


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
@pytest.mark.parametrize("name", list(W.PARITY))
def test_fs_matches_the_model(name):
    dec = decoder(name)
    assert dec.k > 64 and dec.osdw_supported and not dec.osdx_supported
    y, _, front, _, order, sets, refs = W.parity_case(name)
    yd = to_dev(y, dec)
    operm, oparity = to_dev(front[0], dec), to_dev(front[1].view(np.int64), dec)
    for s, ref in zip(sets, refs):
        for quirk in (1, 0):
            p = fs_params(dec, order, s, quirk)
            full = dec.osdw_fs_decode(yd, p)
            out = dec.osdw_fs_search(yd, operm, oparity, p)          # on the oracle's front-end results
            torch.cuda.synchronize()
            assert_front(full["perm"], full["parity"], front, dec)
            assert_fs(full, ref, quirk, where=f"decode {s} quirk {quirk}")
            assert_fs(out, ref, quirk, where=f"search {s} quirk {quirk}")
    if name != "deg65":      # premise: somewhere the two quirk answers differ, so both modes were told apart
        assert any((r["best_ref"] != r["best_hit"]).any() for r in refs)


# ---------------------------------------------------------------------------------------------------------------------
# 2: a planted stop in class 3 at a chosen rank, on caller-made front-end results
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,n,which", W.PLANTED)
def test_planted_stop_in_class_3(k, n, which):
    dec = decoder((k, n))
    assert (dec.k, dec.n) == (k, n)
    case = W.planted(k, n, which)
    order, *s = case["params"]
    ref = case["batch"].fs(order, *s)
    at = 1 + k + k * (k - 1) // 2 + case["rank"]
    assert ref["best_hit"][0] == at and ref["ntep"][0] == at + 1
    yd, perm = to_dev(case["y"], dec), to_dev(case["perm"], dec)
    parity = to_dev(case["parity"].view(np.int64), dec)
    assert tuple(parity.shape) == (1, 128)
    for quirk in (1, 0):
        out = dec.osdw_fs_search(yd, perm, parity, fs_params(dec, order, s, quirk))
        torch.cuda.synchronize()
        assert_fs(out, ref, quirk, where=f"quirk {quirk}")
        assert int(out["ntep"].cpu()[0]) == at + 1
        if not quirk:
            assert int(out["best"].cpu()[0]) == at           # the stop at exactly the FS rank of {a, b, c}


# ---------------------------------------------------------------------------------------------------------------------
# 3: k <= 64 through the new family equals ldpc_osdx_fs_* / _tep_eval
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", osdw_model.NARROW)
def test_narrow_codes_equal_the_any_shape_kernels(name):
    dec = decoder(name)
    assert dec.osdx_supported and dec.osdw_supported
    snr, order, sets = M.PARITY[name]
    y, _ = osdx_model.frames(name, snr, 192, 7)
    yd = to_dev(y, dec)
    moved = False
    for s in sets:
        for quirk in (1, 0):
            p = fs_params(dec, order, s, quirk)
            got, want = dec.osdw_fs_decode(yd, p), dec.osdx_fs_decode(yd, p)
            again = dec.osdw_fs_search(yd, got["perm"], got["parity"], p)
            torch.cuda.synchronize()
            assert_same(got, want, ("cw", "metric", "best", "ntep", "perm"), (s, quirk))
            assert_same(again, want, ("cw", "metric", "best", "ntep"), (s, quirk))
            assert torch.equal(got["parity"][:, :64], want["parity"]) and not got["parity"][:, 64:].any()
            moved |= int(got["best"].max()) > 0 and len(set(got["ntep"].cpu().tolist())) > 3
    assert moved                                             # premise: the searches were searches
    # one TEP: word 1 of the mask is ignored
    rng = np.random.default_rng(3)
    masks = np.zeros(192, np.uint64)
    for f in range(192):                                     # weights 0..5
        for pos in rng.choice(dec.k, f % 6, replace=False):
            masks[f] |= np.uint64(1) << np.uint64(pos)
    two = np.stack([masks, rng.integers(0, 2**63, 192, dtype=np.int64).view(np.uint64) | np.uint64(1)], axis=1)
    got = dec.osdw_tep_eval(yd, got["perm"], got["parity"], to_dev(two.view(np.int64), dec))
    want = dec.osdx_tep_eval(yd, want["perm"], want["parity"], to_dev(masks.view(np.int64), dec))
    torch.cuda.synchronize()
    assert_same(got, want, ("cw", "metric", "hd"))


# ---------------------------------------------------------------------------------------------------------------------
# 4: one given TEP per frame
# ---------------------------------------------------------------------------------------------------------------------
def _tep_masks(k, F, rng):
    """Python-int masks of weight f % 5 (0..4), the first frames with chosen supports: position k-1 alone, a support across
    position 64, wholly below, wholly at or above it (as far as k allows)."""
    masks = []
    for f in range(F):
        sup = rng.choice(k, f % 5, replace=False).tolist()
        masks.append(sum(1 << int(p) for p in sup))
    above = list(range(64, min(k, 68)))
    masks[0] = 0
    masks[1] = 1 << (k - 1)
    masks[2] = (1 << 63) | (1 << 64)
    masks[3] = (1 << 0) | (1 << 31) | (1 << 32) | (1 << 63)
    masks[4] = sum(1 << p for p in above)
    masks[5] = (1 << 5) | (1 << 62) | (1 << (k - 1))
    return masks


def _raw_tep_eval(dec, yd, *args):
    return OF.raw_tep_eval(dec, FAM, yd, yd.shape[0], *args)


@pytest.mark.parametrize("name", ["array_121_80", "s128_96", "s128_65", "deg65"])
def test_tep_eval_matches_the_model(name):
    dec = decoder(name)
    F, k = 48, dec.k
    y, _, front, b = W.batch(name, W.PARITY[name][0])
    masks = _tep_masks(k, F, np.random.default_rng(3))
    assert {bin(m).count("1") for m in masks} >= {0, 1, 2, 3, 4}
    ref = b.one_tep(masks)                                    # the first F frames of the batch
    beyond = ((1 << 128) - 1) ^ ((1 << k) - 1)                # every bit at or beyond k: ignored by the kernel
    dirty = [m | (beyond if f % 2 else 0) for f, m in enumerate(masks)]
    assert k < 128 and any(d != m for d, m in zip(dirty, masks))
    md = to_dev(W.split_masks(dirty).view(np.int64), dec)
    assert tuple(md.shape) == (F, 2)
    yd = to_dev(y[:F], dec)
    perm, parity = to_dev(front[0][:F], dec), to_dev(front[1][:F].view(np.int64), dec)
    out = dec.osdw_tep_eval(yd, perm, parity, md)
    torch.cuda.synchronize()
    assert np.array_equal(words_np(out["cw"]), ref["cw"])
    assert np.array_equal(out["metric"].cpu().numpy().view(np.uint32), ref["metric"].view(np.uint32))
    assert np.array_equal(out["hd"].cpu().numpy(), ref["hd"])
    for off in ("metric", "hd"):                              # nullable, each on its own
        cw = torch.full((F, dec.words), -1, dtype=torch.int64, device=dec.device)
        metric = None if off == "metric" else torch.full((F,), -5.0, dtype=torch.float32, device=dec.device)
        hd = None if off == "hd" else torch.full((F,), -9, dtype=torch.int32, device=dec.device)
        assert _raw_tep_eval(dec, yd, perm, parity, md, cw, metric, hd) == 0
        torch.cuda.synchronize()
        assert torch.equal(cw, out["cw"])
        if metric is not None:
            assert torch.equal(metric.view(torch.int32), out["metric"].view(torch.int32))
        if hd is not None:
            assert torch.equal(hd, out["hd"])


# ---------------------------------------------------------------------------------------------------------------------
# 5: frame lists, device-side counts, nullable outputs, counters, several frames per wavefront, graph capture
# ---------------------------------------------------------------------------------------------------------------------
LISTED_SET = (0.02, 8.5, 30)


@pytest.fixture(scope="module")
def listed():
    """array_121_80: 600 frames at 3.0 dB through NMS and ldpc_compact; the model of the listed frames at order 2."""
    dec = decoder("array_121_80")
    G = osdw_model.graph("array_121_80")[1]
    y, cw = osdw_model.frames("array_121_80", 3.0, 600, 21)
    yd = to_dev(y, dec)
    res = dec.nms(yd, 10, ALPHA0)
    index, count = dec.compact(res["fail"])
    torch.cuda.synchronize()
    nf = int(count.cpu()[0])
    idx = index[:nf].cpu().numpy()
    assert 40 < nf < 600 and np.all(np.diff(idx) > 0)
    front = osdw_model.front_oracle(G, y[idx])
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
    name, s = "s70_66", (0.0, 1.5, 3)
    dec = decoder(name)
    G = osdw_model.graph(name)[1]
    p = fs_params(dec, 2, s, 1)

    def model(ys):
        front = osdw_model.front_oracle(G, ys)
        return front, OF.fs_view(M.Batch(ys, front[0], front[3]).fs(2, *s), 1)
    OF.check_frames_in_turn(FAM, dec, osdw_model.frames(name, 1.5, 65536 + 300, 31)[0], lambda yd: dec.osdw_fs_decode(yd, p), model,
                            distinct_ntep=3)


def test_fs_decode_is_graph_capturable():
    dec = decoder("array_121_80")
    F = 96
    p = fs_params(dec, 2, LISTED_SET, 1)
    ys = [osdw_model.frames("array_121_80", 2.0, F, s)[0] for s in (41, 42, 43)]
    bufs = _sentinels(dec, F)
    ybuf = to_dev(ys[0], dec)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):               # no eager call first: the entry point holds no per-stream state
        dec.osdw_fs_decode(ybuf, p, perm=bufs["perm"], parity=bufs["parity"], out=bufs)
    G = osdw_model.graph("array_121_80")[1]
    for y in ys[1:]:
        ybuf.copy_(to_dev(y, dec))
        graph.replay()
        torch.cuda.synchronize()
        front = osdw_model.front_oracle(G, y)
        assert_front(bufs["perm"], bufs["parity"], front, dec)
        assert_fs(bufs, M.Batch(y, front[0], front[3]).fs(2, *LISTED_SET), 1)


# ---------------------------------------------------------------------------------------------------------------------
# 6: refusals launch nothing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wimax_1056", "wide"])
def test_unsupported_shapes_are_refused(name):
    dec = decoder(name)
    assert dec.n > 128 or dec.n - dec.k > 64
    yd = to_dev(nms_graphs.frames(name, 2.0, 4, 1)[0], dec)
    p = fs_params(dec, 1, (0.1, 4.5, 30), 1)
    mask = torch.zeros((4, 2), dtype=torch.int64, device=dec.device)
    OF.check_unsupported(FAM, dec, yd, {
        "fs_search": lambda b: dec.osdw_fs_search(yd, b["perm"], b["parity"], p, out=b),
        "fs_decode": lambda b: dec.osdw_fs_decode(yd, p, perm=b["perm"], parity=b["parity"], out=b),
        "tep_eval": lambda b: dec.osdw_tep_eval(yd, b["perm"], b["parity"], mask)})


def test_bad_arguments_are_refused_and_the_any_shape_family_keeps_its_refusal():
    dec = decoder("array_121_80")
    y, _ = osdw_model.frames("array_121_80", 1.5, 4, 2)
    yd = to_dev(y, dec)
    bufs = _sentinels(dec, 4)
    clean = {k: v.clone() for k, v in bufs.items()}
    s = (0.1, 4.5, 30)
    good = fs_params(dec, 2, s, 1)
    mask = torch.zeros((4, 2), dtype=torch.int64, device=dec.device)
    OF.check_bad_arguments(FAM, "fs", dec, yd, bufs, lambda order, **kw: fs_params(dec, order, s, 1, **kw), good, mask)
    # the any-shape family still refuses this code, in its own words
    old = {k: v for k, v in bufs.items() if k not in ("perm", "parity")}
    parity64 = bufs["parity"][:, :64].contiguous()
    mask1 = torch.zeros(4, dtype=torch.int64, device=dec.device)
    osdx = r"\(-5\).*the any-shape OSD kernels need 1 <= k <= 64 and 1 <= n-k <= 64; this code is \(121,80\)"
    with pytest.raises(_lib.LdpcError, match=osdx):
        dec.osdx_fs_search(yd, bufs["perm"], parity64, good, out=old)
    with pytest.raises(_lib.LdpcError, match=osdx):
        dec.osdx_fs_decode(yd, good, perm=bufs["perm"], parity=parity64, out=old)
    with pytest.raises(_lib.LdpcError, match=osdx):
        dec.osdx_tep_eval(yd, bufs["perm"], parity64, mask1)
    torch.cuda.synchronize()
    OF.assert_untouched(bufs, clean)
    assert OF.A.untouched(parity64)


def test_order_is_bounded_by_k():
    """A (6,2) code: weight class 3 does not exist, so order 3 is refused; order 2 scans the single pair."""
    dec, G, y = OF.tiny_case()
    yd = to_dev(y, dec)
    bufs = _sentinels(dec, 64)
    clean = {k: v.clone() for k, v in bufs.items()}
    s = (0.0, 1.5, 30)
    with pytest.raises(_lib.LdpcError, match=r"\(-1\).*ldpc_osdw_fs_decode: order 3 outside 0\.\.2"):
        dec.osdw_fs_decode(yd, fs_params(dec, 3, s, 1), perm=bufs["perm"], parity=bufs["parity"], out=bufs)
    with pytest.raises(_lib.LdpcError, match=r"\(-1\).*ldpc_osdw_fs_search: order 3 outside 0\.\.2"):
        dec.osdw_fs_search(yd, bufs["perm"], bufs["parity"], fs_params(dec, 3, s, 1), out=bufs)
    torch.cuda.synchronize()
    OF.assert_untouched(bufs, clean)
    front = osdw_model.front_oracle(G, y)
    ref = M.Batch(y, front[0], front[3]).fs(2, *s)
    assert (ref["depth"] == 2).any() and ref["hit"].any()
    for quirk in (1, 0):
        out = dec.osdw_fs_decode(yd, fs_params(dec, 2, s, quirk))
        torch.cuda.synchronize()
        assert_fs(out, ref, quirk)
