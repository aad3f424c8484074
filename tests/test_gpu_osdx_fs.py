"""-m gpu: FS-OSD and the one-TEP primitive for short codes of any shape (ldpc_osdx_fs_search / _fs_decode / _tep_eval) --
bit-exact against the vectorised model of tests/osdx_fs_model.py on (96,48), (121,60), the zoo's `short` (40,17) and `thin`
(24,11) and CCSDS (128,64), and against the specialised osd_fs_kernel / osd_tep_eval_kernel on CCSDS.  The inputs and the
branches they reach are those tests/test_osdx_fs_host.py asserts on the CPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from short_ldpc_decoding_osd_amd import _lib
from tests import nms_graphs, osdx_model
from tests import osdx_fs_model as M
from tests.gpu_util import pack_np, to_dev, words_np

pytestmark = pytest.mark.gpu
ALPHA0 = 0.669435
_decoders = {}


def decoder(name):
    if name not in _decoders:
        from short_ldpc_decoding_osd_amd.runtime import Decoder
        _decoders[name] = Decoder(nms_graphs.make_code(name) if name in nms_graphs.NAMES else osdx_model.make_code(name))
    return _decoders[name]


def fs_params(dec, order, s, quirk, **kw):
    return dec.osd_params(order, _lib.OSD_FS, fs_beta=s[0], fs_tau_e=s[1], fs_tau_psc=s[2], fs_reference_quirk=quirk, **kw)


def assert_fs(out, ref, quirk, sl=slice(None), where=""):
    """Every output bit for bit: cw, metric as uint32, best, ntep."""
    key = "ref" if quirk else "hit"
    assert np.array_equal(words_np(out["cw"])[sl], ref["cw_" + key][sl]), where
    assert np.array_equal(out["metric"].cpu().numpy().view(np.uint32)[sl], ref["metric_" + key].view(np.uint32)[sl]), where
    assert np.array_equal(out["best"].cpu().numpy()[sl], ref["best_" + key][sl]), where
    assert np.array_equal(out["ntep"].cpu().numpy()[sl], ref["ntep"][sl]), where


def assert_front(perm, parity, front, n, k):
    assert np.array_equal(perm.cpu().numpy()[:, :n], front[0][:, :n])
    assert np.array_equal(words_np(parity)[:, :k], front[1][:, :k])


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
            assert_front(full["perm"], full["parity"], front, dec.n, dec.k)
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


def _sentinels(dec, F):
    return dict(perm=torch.full((F, 128), 0xEE, dtype=torch.uint8, device=dec.device),
                parity=torch.full((F, 64), -1, dtype=torch.int64, device=dec.device),
                cw=torch.full((F, dec.words), -1, dtype=torch.int64, device=dec.device),
                metric=torch.full((F,), -5.0, dtype=torch.float32, device=dec.device),
                best=torch.full((F,), -9, dtype=torch.int32, device=dec.device),
                ntep=torch.full((F,), -9, dtype=torch.int32, device=dec.device))


_p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731


def _raw_decode(dec, yd, index, count, F, params, bufs, label=None, counts=None):
    return dec.L.ldpc_osdx_fs_decode(dec._ctx, _p(yd), _p(index), _p(count), F, C.byref(params) if params is not None else None,
                                     _p(bufs.get("perm")), _p(bufs.get("parity")), _p(bufs.get("cw")), _p(bufs.get("metric")),
                                     _p(bufs.get("best")), _p(bufs.get("ntep")), _p(label), _p(counts), dec._stream())


def _raw_search(dec, yd, F, params, bufs):
    return dec.L.ldpc_osdx_fs_search(dec._ctx, _p(yd), None, None, F, _p(bufs.get("perm")), _p(bufs.get("parity")),
                                     C.byref(params) if params is not None else None, _p(bufs.get("cw")), _p(bufs.get("metric")),
                                     _p(bufs.get("best")), _p(bufs.get("ntep")), dec._stream())


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
    return dict(dec=dec, y=y, yd=yd, labels=cw, index=index, count=count, nf=nf, idx=idx, ref=ref,
                params=fs_params(dec, 2, LISTED_SET, 1))


@pytest.mark.parametrize("which", ["smaller", "equal", "larger"])
def test_frame_list_and_device_count(listed, which):
    dec, nf = listed["dec"], listed["nf"]
    F = {"smaller": nf + 13, "equal": nf, "larger": nf - 9}[which]       # the device count against the capacity F
    done = min(nf, F)
    bufs = _sentinels(dec, nf + 13)
    clean = {k: v.clone() for k, v in bufs.items()}
    assert _raw_decode(dec, listed["yd"], listed["index"], listed["count"], F, listed["params"], bufs) == 0
    torch.cuda.synchronize()
    assert_fs(bufs, listed["ref"], 1, slice(0, done))
    for k in bufs:                                                       # nothing at or beyond min(count, F)
        assert torch.equal(bufs[k][done:], clean[k][done:]), k


@pytest.mark.parametrize("off", ["metric", "best", "ntep", "counts", "label"])
def test_nullable_outputs_and_counters(listed, off):
    dec, nf, ref = listed["dec"], listed["nf"], listed["ref"]
    label = to_dev(pack_np(listed["labels"]).view(np.int64), dec)
    bufs = _sentinels(dec, nf)
    counts = torch.tensor([5, 6, 7], dtype=torch.int64, device=dec.device)
    if off in bufs:
        bufs[off] = None
    assert _raw_decode(dec, listed["yd"], listed["index"], listed["count"], nf, listed["params"], bufs,
                       None if off == "label" else label, None if off == "counts" else counts) == 0
    torch.cuda.synchronize()
    assert np.array_equal(words_np(bufs["cw"]), ref["cw_ref"])
    if off != "metric":
        assert np.array_equal(bufs["metric"].cpu().numpy().view(np.uint32), ref["metric_ref"].view(np.uint32))
    if off != "best":
        assert np.array_equal(bufs["best"].cpu().numpy(), ref["best_ref"])
    if off != "ntep":
        assert np.array_equal(bufs["ntep"].cpu().numpy(), ref["ntep"])
    # the counters, recomputed on the host: teps_total is the sum of the per-frame ntep
    wrong = int(np.any(ref["cw_ref"] != pack_np(listed["labels"][listed["idx"]]), axis=1).sum())
    assert 0 < wrong < nf and len(set(ref["ntep"].tolist())) > 3
    want = [5, 6, 7] if off in ("counts", "label") else [5 + nf, 6 + wrong, 7 + (0 if off == "ntep" else int(ref["ntep"].sum()))]
    assert counts.cpu().tolist() == want


def test_one_wavefront_decodes_several_frames_in_turn():
    """More frames than the grid's 65536 workgroups: wavefront b decodes frame b and then frame 65536 + b.  The frames that
    share a wavefront are checked against the model, all of them against the same frames decoded one per wavefront."""
    dec = decoder("thin")
    G = osdx_model.graph("thin")[1]
    extra, s = 300, (0.0, 3.5, 5)
    F = 65536 + extra
    y, _ = osdx_model.frames("thin", 0.0, F, 31)
    yd = to_dev(y, dec)
    p = fs_params(dec, 3, s, 1)
    out = dec.osdx_fs_decode(yd, p)
    head = dec.osdx_fs_decode(yd[:65536].contiguous(), p)
    tail = dec.osdx_fs_decode(yd[65536:].contiguous(), p)
    torch.cuda.synchronize()
    for k in ("perm", "parity", "cw", "metric", "best", "ntep"):
        assert torch.equal(out[k][:65536], head[k]) and torch.equal(out[k][65536:], tail[k]), k
    for sl in (slice(0, extra), slice(65536, F)):
        front = osdx_model.front_oracle(G, y[sl])
        ref = M.Batch(y[sl], front[0], front[3]).fs(3, *s)
        assert len(set(ref["ntep"].tolist())) > 3            # premise: the frames of a wavefront differ in their scans
        assert_fs({k: out[k][sl] for k in ("cw", "metric", "best", "ntep")}, ref, 1)


@pytest.mark.parametrize("name", ["wimax_1056", "wide"])
def test_unsupported_shapes_are_refused(name):
    dec = decoder(name)
    y, _ = nms_graphs.frames(name, 2.0, 4, 1)
    yd = to_dev(y, dec)
    bufs = _sentinels(dec, 4)
    clean = {k: v.clone() for k, v in bufs.items()}
    p = fs_params(dec, 1, (0.1, 4.5, 30), 1)
    mask = torch.zeros(4, dtype=torch.int64, device=dec.device)
    msg = rf"\(-5\).*1 <= k <= 64 and 1 <= n-k <= 64.*\({dec.n},{dec.k}\)"
    with pytest.raises(_lib.LdpcError, match=msg):
        dec.osdx_fs_search(yd, bufs["perm"], bufs["parity"], p, out=bufs)
    with pytest.raises(_lib.LdpcError, match=msg):
        dec.osdx_fs_decode(yd, p, perm=bufs["perm"], parity=bufs["parity"], out=bufs)
    with pytest.raises(_lib.LdpcError, match=msg):
        dec.osdx_tep_eval(yd, bufs["perm"], bufs["parity"], mask)
    torch.cuda.synchronize()
    for k in bufs:
        assert torch.equal(bufs[k], clean[k]), k


def test_bad_arguments_are_refused_and_the_old_entry_points_keep_their_refusal(monkeypatch):
    dec = decoder("ldpc_96_48")
    y, _ = osdx_model.frames("ldpc_96_48", 1.5, 4, 2)
    yd = to_dev(y, dec)
    bufs = _sentinels(dec, 4)
    clean = {k: v.clone() for k, v in bufs.items()}
    s = (0.1, 4.5, 30)
    good = fs_params(dec, 2, s, 1)
    aux = torch.zeros((4, 4), dtype=torch.int32, device=dec.device)
    mask = torch.zeros(4, dtype=torch.int64, device=dec.device)
    bad = [(dec.osd_params(2, _lib.OSD_CONVENTIONAL), r"algo 0 is not LDPC_OSD_FS"),
           (dec.osd_params(2, _lib.OSD_PB), r"algo 2 is not LDPC_OSD_FS"),
           (fs_params(dec, 4, s, 1), r"order 4 outside 0\.\.3"),
           (fs_params(dec, -1, s, 1), r"order -1 outside 0\.\.3"),
           (fs_params(dec, 2, s, 1, table_scan=True), r"flags 0x1 are not served here"),
           (fs_params(dec, 2, s, 1, aux=aux), r"d_aux is not served here"),
           (fs_params(dec, 2, s, 1, y_frames=4), r"y_frames 4 is not served here")]
    for p, why in bad:
        with pytest.raises(_lib.LdpcError, match=r"\(-1\).*ldpc_osdx_fs_decode: " + why):
            dec.osdx_fs_decode(yd, p, perm=bufs["perm"], parity=bufs["parity"], out=bufs)
        with pytest.raises(_lib.LdpcError, match=r"\(-1\).*ldpc_osdx_fs_search: " + why):
            dec.osdx_fs_search(yd, bufs["perm"], bufs["parity"], p, out=bufs)
    for missing in ("cw", "perm", "parity"):
        assert _raw_decode(dec, yd, None, None, 4, good, {**bufs, missing: None}) == -1
        assert f"ldpc_osdx_fs_decode: d_{missing} is NULL".encode() in dec.L.ldpc_last_error()
        assert _raw_search(dec, yd, 4, good, {**bufs, missing: None}) == -1
        assert f"ldpc_osdx_fs_search: d_{missing} is NULL".encode() in dec.L.ldpc_last_error()
    assert _raw_decode(dec, None, None, None, 4, good, bufs) == -1 and b"ldpc_osdx_fs_decode: d_y is NULL" in dec.L.ldpc_last_error()
    assert _raw_decode(dec, yd, None, None, 4, None, bufs) == -1 and b"ldpc_osdx_fs_decode: params is NULL" in dec.L.ldpc_last_error()
    assert _raw_search(dec, yd, 4, None, bufs) == -1 and b"ldpc_osdx_fs_search: params is NULL" in dec.L.ldpc_last_error()
    for missing in ("y", "perm", "parity", "mask", "cw"):
        a = dict(y=yd, perm=bufs["perm"], parity=bufs["parity"], mask=mask, cw=bufs["cw"])
        a[missing] = None
        assert dec.L.ldpc_osdx_tep_eval(dec._ctx, _p(a["y"]), None, None, 4, _p(a["perm"]), _p(a["parity"]), _p(a["mask"]),
                                        _p(a["cw"]), None, None, dec._stream()) == -1
        assert f"ldpc_osdx_tep_eval: d_{missing} is NULL".encode() in dec.L.ldpc_last_error()
    assert _raw_decode(dec, yd, None, None, 0, good, {}) == 0              # F == 0: LDPC_OK, no launch
    assert _raw_search(dec, yd, 0, good, {}) == 0
    assert dec.L.ldpc_osdx_tep_eval(dec._ctx, None, None, None, 0, None, None, None, None, None, None, dec._stream()) == 0
    old = r"\(-5\).*OSD kernels need an \(n=128, k=64\) code; this one is \(96,48\)"
    with pytest.raises(_lib.LdpcError, match=old):
        dec.osd_decode(yd, 2, params=good)
    with pytest.raises(_lib.LdpcError, match=old):
        dec.osd_search(yd, bufs["perm"], bufs["parity"], good, out=bufs)
    with pytest.raises(_lib.LdpcError, match=old):
        dec.osd_tep_eval(yd, bufs["perm"], bufs["parity"], mask)
    torch.cuda.synchronize()
    for k in bufs:
        assert torch.equal(bufs[k], clean[k]), k
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
    from short_ldpc_decoding_osd_amd import Code
    from short_ldpc_decoding_osd_amd.runtime import Decoder
    H = np.array([[1, 1, 0, 1, 0, 0], [0, 1, 1, 0, 1, 0], [1, 0, 1, 0, 0, 1], [1, 1, 1, 1, 1, 0]], dtype=np.int64)
    code = Code(H=H)
    assert code.k == 2
    dec = Decoder(code)
    G = np.asarray(code.G)
    from oracle import np_oracle
    y, _ = np_oracle.make_frames(G, 0.0, 64, np.random.default_rng(9))
    yd = to_dev(y, dec)
    bufs = _sentinels(dec, 64)
    clean = {k: v.clone() for k, v in bufs.items()}
    s = (0.0, 1.5, 30)
    with pytest.raises(_lib.LdpcError, match=r"\(-1\).*ldpc_osdx_fs_decode: order 3 outside 0\.\.2"):
        dec.osdx_fs_decode(yd, fs_params(dec, 3, s, 1), perm=bufs["perm"], parity=bufs["parity"], out=bufs)
    torch.cuda.synchronize()
    for k in bufs:
        assert torch.equal(bufs[k], clean[k]), k
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
        assert_front(bufs["perm"], bufs["parity"], front, dec.n, dec.k)
        assert_fs(bufs, M.Batch(y, front[0], front[3]).fs(2, *LISTED_SET), 1)
