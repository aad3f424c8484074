"""-m gpu: OSD for short codes of any shape (ldpc_osdx_front / _search / _decode) -- bit-exact against the CPU oracles of
tests/osdx_model.py on (96,48), (121,60), the zoo's `short` (40,17) and `thin` (24,11), and against the specialised kernels
on the CCSDS (128,64) code."""
import numpy as np
import pytest
import torch

from oracle import np_oracle
from short_ldpc_decoding_osd_amd import _lib
from tests import nms_graphs, osdx_model
from tests import osd_family as OF
from tests.gpu_util import pack_np, to_dev, words_np
from tests.osd_family import assert_scan, decoder

pytestmark = pytest.mark.gpu
ALPHA0 = 0.669435
_front, _scan = {}, {}


def front_case(name):
    """256 frames at 1.0 dB and their front-end oracle (computed once)."""
    if name not in _front:
        y, _ = osdx_model.frames(name, 1.0, 256, 1)
        _front[name] = (y, osdx_model.front_oracle(osdx_model.graph(name)[1], y))
    return _front[name]


def scan_case(name, order, F=64):
    """F frames at 1.5 dB, their front-end oracle and scan oracle (computed once)."""
    key = (name, order, F)
    if key not in _scan:
        G = osdx_model.graph(name)[1]
        y, cw = osdx_model.frames(name, 1.5, F, 11)
        front = osdx_model.front_oracle(G, y)
        _scan[key] = (y, cw, front, osdx_model.scan_oracle(G, y, order, front))
    return _scan[key]


FAM = OF.OSDX


def assert_front(got, want, dec):
    """(perm, parity, nswaps) of a front-end call against a front_oracle result."""
    OF.assert_front(FAM, dec, got[0], got[1], want, got[2])


def _sentinels(dec, F):
    return OF.sentinels(dec, FAM, F)


def _raw_decode(dec, *args, **kw):
    return OF.raw_decode(dec, FAM, "decode", *args, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# 1, 2: the front end
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", osdx_model.CODES)
def test_front_end_matches_oracle(name):
    dec = decoder(name)
    y, want = front_case(name)
    ns_o = want[2]
    assert (ns_o == 0).any() and (ns_o >= 3).any()           # premise: frames without an exchange and frames with chains
    assert dec.osdx_supported
    perm = torch.full((256, 128), 0xEE, dtype=torch.uint8, device=dec.device)
    parity = torch.full((256, 64), -1, dtype=torch.int64, device=dec.device)
    ns = torch.full((256,), -7, dtype=torch.int32, device=dec.device)
    got = dec.osdx_front(to_dev(y, dec), out=(perm, parity, ns))
    torch.cuda.synchronize()
    assert_front(got, want, dec)


def awkward_frames(G):
    """The cases of test_front_end_ties_and_zeros and test_front_end_saturated_inputs (tests/test_gpu_osd.py), resized to n."""
    n = G.shape[1]
    rng = np.random.default_rng(12)
    y, _ = np_oracle.make_frames(G, 2.5, 24, rng)
    y[0] = 1.0                               # all equal
    y[1] = np.where(np.arange(n) % 2, -0.5, 0.5)
    y[2, :n // 2] = 0.0                      # zeros (reliability 0) in the first half
    y[3] = np.round(y[3] * 4) / 4            # quantised: many duplicates
    y[4, 10] = -y[4, 20]
    y[5] = -0.0
    y[6] *= 40.0
    y[7] *= 1e-3
    y[8, n - 19] = 1e30                      # one outlier: every other value lands in one sort bucket
    y[9, 5], y[9, n - 28] = np.inf, -np.inf
    y[10] *= 1e-41                           # denormals
    y[11, 3] = 3.0e38
    z, _ = np_oracle.make_frames(G, 2.5, 8, np.random.default_rng(77))
    z = np.clip(z, -1.0, 1.0)                # saturated: most keys in ONE bucket, an exact zero in the lowest
    z[:, 5] = 0.0
    z[1, n - 1] = 0.0                        # the smallest real key: (|0.0| bits, 127 - (n - 1)), just above the padded ones
    z[2] = np.clip(z[2] * 8, -1.0, 1.0)
    z[2, 5] = 0.0
    z[3] = 1.0
    z[3, n - 1] = 0.0
    z[4] = np.where(rng.random(n) < 0.52, 1.0, z[4] * 0.01).astype(np.float32)
    z[5] = 0.0                               # every key ties with the padding's magnitude
    return np.concatenate([y, z]).astype(np.float32)


@pytest.mark.parametrize("name", ["ldpc_96_48", "array_121_60"])
def test_front_end_awkward_inputs(name):
    dec = decoder(name)
    G = osdx_model.graph(name)[1]
    y = awkward_frames(G)
    got = dec.osdx_front(to_dev(y, dec))
    torch.cuda.synchronize()
    perm = got[0].cpu().numpy()
    assert all(sorted(p[:dec.n]) == list(range(dec.n)) for p in perm.tolist())
    assert_front(got, osdx_model.front_oracle(G, y), dec)


def test_scan_without_a_finite_cost_flips_nothing():
    """Order 1 on frames whose every cost is +inf: the scan holds no candidate -- best = 0x7FFFFFFF, the metric +inf and no MRB
    flip: the codeword words are the hard decisions.  (ldpc_osdl_search takes the first TEP there: tests/test_gpu_osdl.py.)"""
    dec = decoder("short")
    G = osdx_model.graph("short")[1]
    y = osdx_model.saturated_frames(G)
    with np.errstate(over="ignore"):
        ref = osdx_model.scan_oracle(G, y, 1)
    assert np.isposinf(ref["metric"]).all() and (ref["ties"] == ref["ntep"]).all()    # premise: every cost is +inf
    assert not ref["best"].any()                                 # (np.argmin names the first TEP there; these kernels name none)
    hard = pack_np((y < 0).astype(np.uint8))                     # nothing flipped, no discrepancy taken over: the hard decisions of y
    for out in (dec.osdx_decode(to_dev(y, dec), 1), dec.osdx_search(to_dev(y, dec), *dec.osdx_front(to_dev(y, dec))[:2], 1)):
        torch.cuda.synchronize()
        assert np.array_equal(words_np(out["cw"]), hard)
        assert np.isposinf(out["metric"].cpu().numpy()).all()
        assert (out["best"].cpu().numpy() == 0x7FFFFFFF).all()
        assert np.array_equal(out["ntep"].cpu().numpy(), ref["ntep"])


# ---------------------------------------------------------------------------------------------------------------------
# 3, 4: the scan
# ---------------------------------------------------------------------------------------------------------------------
SCAN_CASES = [(name, order, 64) for name in osdx_model.SMALL for order in (0, 1, 2)] + [("short", 3, 64), ("ldpc_96_48", 3, 8)]


@pytest.mark.parametrize("name,order,F", SCAN_CASES)
def test_scan_matches_oracle(name, order, F):
    dec = decoder(name)
    y, _, front, ref = scan_case(name, order, F)
    if order >= 1:
        assert ref["weight"].max() >= 1                      # premise: some winner is no order-0 candidate
    yd = to_dev(y, dec)
    fr = dec.osdx_front(yd)
    torch.cuda.synchronize()
    assert_front(fr, front, dec)                    # the search runs on oracle-checked front-end results
    out = dec.osdx_search(yd, fr[0], fr[1], order)
    full = dec.osdx_decode(yd, order)
    torch.cuda.synchronize()
    assert_scan(out, ref)
    assert_scan(full, ref)
    assert_front((full["perm"], full["parity"], fr[2]), front, dec)


def test_argmin_ties_go_to_the_first_minimum():
    dec = decoder("ldpc_96_48")
    G = osdx_model.graph("ldpc_96_48")[1]
    y, _ = nms_graphs.frames("ldpc_96_48", 1.5, 32, 1, quantise=True)
    ref = osdx_model.scan_oracle(G, y, 2)
    assert (ref["ties"] > 1).any()                           # premise: two TEPs share the minimum in some frame
    out = dec.osdx_decode(to_dev(y, dec), 2)
    torch.cuda.synchronize()
    assert_scan(out, ref)


# ---------------------------------------------------------------------------------------------------------------------
# 5: (128,64) through the any-shape route equals the specialised kernels
# ---------------------------------------------------------------------------------------------------------------------
def test_ccsds_equals_the_specialised_kernels():
    dec = decoder("ccsds")
    y, _ = osdx_model.frames("ccsds", 2.0, 512, 3)
    yd = to_dev(y, dec)
    a, b = dec.osdx_front(yd), dec.osd_front(yd)
    torch.cuda.synchronize()
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    for order in range(4):
        got = dec.osdx_decode(yd, order)
        refs = [dec.osd_decode(yd, order)]
        if order == 2:                                       # the default is the rotation-paired kernel; and the table scan
            refs.append(dec.osd_decode(yd, 2, params=dec.osd_params(2, table_scan=True)))
        torch.cuda.synchronize()
        for ref in refs:
            assert torch.equal(got["cw"], ref["cw"]) and torch.equal(got["best"], ref["best"])
            assert torch.equal(got["ntep"], ref["ntep"])
            assert torch.equal(got["metric"].view(torch.int32), ref["metric"].view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------
# 6: frame lists, device-side counts, nullable outputs, counters
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def listed():
    """array_121_60: 600 frames at 2.0 dB through NMS and ldpc_compact; the oracle of the listed frames at order 1."""
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
    return dict(dec=dec, y=y, yd=yd, labels=cw, label_rows=idx, index=index, count=count, nf=nf, rows=np.arange(nf), front=front,
                ref=osdx_model.scan_oracle(G, y[idx], 1, front), arg=lambda bufs: 1)


@pytest.mark.parametrize("which", ["smaller", "equal", "larger"])
def test_frame_list_and_device_count(listed, which):
    OF.check_frame_list(FAM, "decode", listed, which)


@pytest.mark.parametrize("off", ["metric", "best", "ntep", "counts", "label"])
def test_nullable_outputs_and_counters(listed, off):
    OF.check_nullable(FAM, "decode", listed, off)


def test_one_wavefront_decodes_several_frames_in_turn():
    """More frames than the grid's 65536 workgroups: wavefront b decodes frame b and then frame 65536 + b.  The frames that
    share a wavefront are checked against the oracle, all of them against the same frames decoded one per wavefront."""
    name = "thin"
    dec = decoder(name)
    G = osdx_model.graph(name)[1]

    def model(ys):
        front = osdx_model.front_oracle(G, ys)
        return front, osdx_model.scan_oracle(G, ys, 1, front)
    OF.check_frames_in_turn(FAM, dec, osdx_model.frames(name, 1.5, 65536 + 300, 31)[0], lambda yd: dec.osdx_decode(yd, 1), model)


# ---------------------------------------------------------------------------------------------------------------------
# 7: refusals launch nothing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wimax_1056", "wide"])
def test_unsupported_shapes_are_refused(name):
    dec = decoder(name)
    yd = to_dev(nms_graphs.frames(name, 2.0, 4, 1)[0], dec)
    OF.check_unsupported(FAM, dec, yd, {
        "front": lambda b: dec.osdx_front(yd, out=(b["perm"], b["parity"], None)),
        "search": lambda b: dec.osdx_search(yd, b["perm"], b["parity"], 1, out=b),
        "decode": lambda b: dec.osdx_decode(yd, 1, perm=b["perm"], parity=b["parity"], out=b)})


def test_bad_arguments_are_refused_and_the_old_entry_points_keep_their_refusal():
    dec = decoder("ldpc_96_48")
    y, _ = osdx_model.frames("ldpc_96_48", 1.5, 4, 2)
    yd = to_dev(y, dec)
    bufs = _sentinels(dec, 4)
    clean = {k: v.clone() for k, v in bufs.items()}
    with pytest.raises(_lib.LdpcError, match=r"\(-1\).*ldpc_osdx_decode: order 4 outside 0\.\.3"):
        dec.osdx_decode(yd, 4, perm=bufs["perm"], parity=bufs["parity"], out=bufs)
    with pytest.raises(_lib.LdpcError, match=r"\(-1\).*ldpc_osdx_search: order -1 outside 0\.\.3"):
        dec.osdx_search(yd, bufs["perm"], bufs["parity"], -1, out=bufs)
    assert _raw_decode(dec, yd, None, None, 4, 1, dict(bufs, cw=None)) == -1
    assert b"ldpc_osdx_decode: d_cw is NULL" in dec.L.ldpc_last_error()
    assert _raw_decode(dec, yd, None, None, 4, 1, dict(bufs, perm=None)) == -1
    assert b"ldpc_osdx_decode: d_perm is NULL" in dec.L.ldpc_last_error()
    assert _raw_decode(dec, yd, None, None, 0, 1, {}) == 0                 # F == 0: LDPC_OK, no launch
    with pytest.raises(_lib.LdpcError, match=r"\(-5\).*OSD kernels need an \(n=128, k=64\) code; this one is \(96,48\)"):
        dec.osd_decode(yd, 2)
    with pytest.raises(_lib.LdpcError, match=r"\(-5\).*OSD kernels need an \(n=128, k=64\) code; this one is \(96,48\)"):
        dec.osd_front(yd)
    torch.cuda.synchronize()
    OF.assert_untouched(bufs, clean)


# ---------------------------------------------------------------------------------------------------------------------
# 8: graph capture
# ---------------------------------------------------------------------------------------------------------------------
def test_decode_is_graph_capturable():
    dec = decoder("array_121_60")
    F = 96
    ys = [osdx_model.frames("array_121_60", 1.5, F, s)[0] for s in (41, 42, 43)]
    want = []
    for y in ys[1:]:
        o = dec.osdx_decode(to_dev(y, dec), 2)
        torch.cuda.synchronize()
        want.append({k: v.clone() for k, v in o.items()})
    ybuf = to_dev(ys[0], dec)
    bufs = _sentinels(dec, F)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):               # no eager call first: the entry point holds no per-stream state
        dec.osdx_decode(ybuf, 2, perm=bufs["perm"], parity=bufs["parity"], out=bufs)
    for y, ref in zip(ys[1:], want):
        ybuf.copy_(to_dev(y, dec))
        graph.replay()
        torch.cuda.synchronize()
        for k in ("perm", "parity", "cw", "metric", "best", "ntep"):
            assert torch.equal(bufs[k], ref[k]), k
