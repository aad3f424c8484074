"""-m gpu: OSD for high-rate short codes (ldpc_osdw_front / _search / _decode: n <= 128, 1 <= n-k <= 64, k up to 127) --
bit-exact against the CPU oracles of tests/osdw_model.py on (121,80), the zoo's deg65 (80,74) and four synthetic codes with
k = 65, 96, 124 and 66, and against ldpc_osdx_* on CCSDS (128,64) and (121,60).  Floats compare by their bits."""
import numpy as np
import pytest
import torch

from oracle import np_oracle
from short_ldpc_decoding_osd_amd import _lib
from tests import nms_graphs, osdw_model, osdx_model
from tests import osd_family as OF
from tests.gpu_util import pack_np, to_dev, words_np
from tests.osd_family import assert_scan, decoder

pytestmark = pytest.mark.gpu
ALPHA0 = 0.669435
_front, _scan = {}, {}

# The classes of column exchanges the 256 front-end frames must hold, per code: frames without an exchange, frames with three or
# more, recorded exchanges (a, b) with the pivot step a in the first / second word of the row map and the partner b in the
# first slot, in the second slot inside the MRB, and in the parity part.  (The counts the CPU oracle gives; a zero is a class
# the code cannot produce.)
EXCHANGES = {
    "array_121_80": dict(frames_0=59, frames_ge3=73, most=14, a_lt64=15, a_ge64=530, b_lt64=8, b_mid=264, b_gek=273),
    "deg65": dict(frames_0=0, frames_ge3=234, most=14, a_lt64=458, a_ge64=1073, b_lt64=202, b_mid=687, b_gek=642),
    "s128_65": dict(frames_0=0, frames_ge3=256, most=38, a_lt64=5694, a_ge64=247, b_lt64=3590, b_mid=141, b_gek=2210),
    "s128_96": dict(frames_0=2, frames_ge3=246, most=32, a_lt64=74, a_ge64=2239, b_lt64=44, b_mid=1419, b_gek=850),
    "s128_124": dict(frames_0=24, frames_ge3=98, most=6, a_lt64=0, a_ge64=559, b_lt64=0, b_mid=229, b_gek=330),
    "s70_66": dict(frames_0=20, frames_ge3=155, most=15, a_lt64=628, a_ge64=288, b_lt64=417, b_mid=195, b_gek=304),
}
SEARCHED = ("array_121_80", "s128_65", "s128_96")      # the codes whose order-2 winners have every weight


def front_case(name):
    """256 frames at 1.0 dB and their front-end oracle with the recorded exchanges (computed once)."""
    if name not in _front:
        y, _ = osdw_model.frames(name, 1.0, 256, 1)
        _front[name] = (y, osdw_model.front_oracle(osdw_model.graph(name)[1], y, swaps=True))
    return _front[name]


def scan_case(name, order, F):
    """F frames at 1.5 dB, their front-end oracle and scan oracle (computed once)."""
    key = (name, order, F)
    if key not in _scan:
        G = osdw_model.graph(name)[1]
        y, cw = osdw_model.frames(name, 1.5, F, 11)
        front = osdw_model.front_oracle(G, y)
        _scan[key] = (y, cw, front, osdx_model.scan_oracle(G, y, order, front))
    return _scan[key]


FAM = OF.OSDW


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
@pytest.mark.parametrize("name", osdw_model.CODES)
def test_front_end_matches_oracle(name):
    dec = decoder(name)
    y, want = front_case(name)
    if name in EXCHANGES:                                    # premises: the paths a two-word elimination can get wrong
        cls = osdw_model.exchange_classes(dec.k, want[2], want[4])
        for key, count in EXCHANGES[name].items():
            assert (cls[key] > 0) == (count > 0), (key, cls[key], count)
        if name == "array_121_80":
            assert all(v > 0 for v in cls.values()), cls
        assert dec.k > 64 and not dec.osdx_supported
    assert dec.osdw_supported
    b = _sentinels(dec, 256)
    ns = torch.full((256,), -7, dtype=torch.int32, device=dec.device)
    got = dec.osdw_front(to_dev(y, dec), out=(b["perm"], b["parity"], ns))
    torch.cuda.synchronize()
    assert_front(got, want, dec)


def awkward_frames(G):
    """The frames of awkward_frames in tests/test_gpu_osdx.py: all-equal, zeros, -0.0, quantised, +-inf, denormals, 3e38,
    saturated."""
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


@pytest.mark.parametrize("name", ["array_121_80", "s70_66"])
def test_front_end_awkward_inputs(name):
    dec = decoder(name)
    G = osdw_model.graph(name)[1]
    y = awkward_frames(G)
    got = dec.osdw_front(to_dev(y, dec))
    torch.cuda.synchronize()
    perm = got[0].cpu().numpy()
    assert all(sorted(p[:dec.n]) == list(range(dec.n)) for p in perm.tolist())
    assert_front(got, osdw_model.front_oracle(G, y), dec)


def test_scan_without_a_finite_cost_flips_nothing():
    """Order 1 on frames whose every cost is +inf (osdx_model.saturated_frames): the scan holds no candidate --
    best = 0x7FFFFFFF, the metric +inf and no MRB flip: the codeword words are the hard decisions.  (ldpc_osdl_search takes
    the first TEP there: tests/test_gpu_osdl.py.)"""
    dec = decoder("short")
    G = osdw_model.graph("short")[1]
    y = osdx_model.saturated_frames(G)
    with np.errstate(over="ignore"):
        ref = osdx_model.scan_oracle(G, y, 1, osdw_model.front_oracle(G, y))
    assert np.isposinf(ref["metric"]).all() and (ref["ties"] == ref["ntep"]).all()    # premise: every cost is +inf
    assert not ref["best"].any()                                 # (np.argmin names the first TEP there; these kernels name none)
    hard = pack_np((y < 0).astype(np.uint8))                     # nothing flipped, no discrepancy taken over: the hard decisions of y
    for out in (dec.osdw_decode(to_dev(y, dec), 1), dec.osdw_search(to_dev(y, dec), *dec.osdw_front(to_dev(y, dec))[:2], 1)):
        torch.cuda.synchronize()
        assert np.array_equal(words_np(out["cw"]), hard)
        assert np.isposinf(out["metric"].cpu().numpy()).all()
        assert (out["best"].cpu().numpy() == 0x7FFFFFFF).all()
        assert np.array_equal(out["ntep"].cpu().numpy(), ref["ntep"])


# ---------------------------------------------------------------------------------------------------------------------
# 3, 4: the scan
# ---------------------------------------------------------------------------------------------------------------------
# (s128_124 stays at order <= 2: its order-3 table has 317 875 TEPs, about 9 s per frame on the CPU oracle)
SCAN_CASES = [(name, order, 32) for name in osdw_model.CODES for order in (0, 1, 2)] + [("array_121_80", 3, 4), ("s70_66", 3, 4)]


@pytest.mark.parametrize("name,order,F", SCAN_CASES)
def test_scan_matches_oracle(name, order, F):
    dec = decoder(name)
    y, _, front, ref = scan_case(name, order, F)
    if order == 2 and name in SEARCHED:                      # premises: winners of every weight, flips in either word
        E = osdx_model.tep_matrix(dec.k, 2)
        flipped = [np.flatnonzero(E[b]) for b in ref["best"]]
        assert (ref["weight"] == 1).any() and (ref["weight"] == 2).any()
        assert any((p >= 64).any() for p in flipped) and any((p < 64).any() for p in flipped)
    yd = to_dev(y, dec)
    fr = dec.osdw_front(yd)
    torch.cuda.synchronize()
    assert_front(fr, front, dec)                    # the search runs on oracle-checked front-end results
    out = dec.osdw_search(yd, fr[0], fr[1], order)
    full = dec.osdw_decode(yd, order)
    torch.cuda.synchronize()
    assert_scan(out, ref)
    assert_scan(full, ref)
    assert_front((full["perm"], full["parity"], fr[2]), front, dec)


def test_argmin_ties_go_to_the_first_minimum():
    dec = decoder("array_121_80")
    G = osdw_model.graph("array_121_80")[1]
    y, _ = osdw_model.frames("array_121_80", 1.5, 32, 1)
    y = (np.round(y * 2) / 2).astype(np.float32)             # as nms_graphs.frames(..., quantise=True)
    y[:, ::17] = 0.0
    front = osdw_model.front_oracle(G, y)
    ref = osdx_model.scan_oracle(G, y, 2, front)
    assert (ref["ties"] > 1).any()                           # premise: two TEPs share the minimum in some frame
    out = dec.osdw_decode(to_dev(y, dec), 2)
    torch.cuda.synchronize()
    assert_scan(out, ref)


# ---------------------------------------------------------------------------------------------------------------------
# 5: k <= 64 through the new family equals ldpc_osdx_*
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", osdw_model.NARROW)
def test_narrow_codes_equal_the_any_shape_kernels(name):
    dec = decoder(name)
    assert dec.osdx_supported and dec.osdw_supported
    y, _ = osdw_model.frames(name, 2.0, 512, 3)
    yd = to_dev(y, dec)
    a, b = dec.osdw_front(yd), dec.osdx_front(yd)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
    assert torch.equal(a[1][:, :64], b[1]) and not a[1][:, 64:].any()
    for order in range(4):
        got, ref = dec.osdw_decode(yd, order), dec.osdx_decode(yd, order)
        torch.cuda.synchronize()
        assert torch.equal(got["cw"], ref["cw"]) and torch.equal(got["best"], ref["best"])
        assert torch.equal(got["ntep"], ref["ntep"]) and torch.equal(got["perm"], ref["perm"])
        assert torch.equal(got["metric"].view(torch.int32), ref["metric"].view(torch.int32))
        assert torch.equal(got["parity"][:, :64], ref["parity"])
        if order:
            assert int(got["best"].max()) > 0                # premise: some winner is no order-0 candidate


# ---------------------------------------------------------------------------------------------------------------------
# 6: frame lists, device-side counts, nullable outputs, counters
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def listed():
    """array_121_80: 600 frames at 3.0 dB through NMS and ldpc_compact; the oracle of the listed frames at order 1."""
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
    return dict(dec=dec, y=y, yd=yd, labels=cw, label_rows=idx, index=index, count=count, nf=nf, rows=np.arange(nf), front=front,
                ref=osdx_model.scan_oracle(G, y[idx], 1, front), arg=lambda bufs: 1)


@pytest.mark.parametrize("which", ["smaller", "equal", "larger"])
def test_frame_list_and_device_count(listed, which):
    OF.check_frame_list(FAM, "decode", listed, which)


@pytest.mark.parametrize("off", ["metric", "best", "ntep", "counts", "label"])
def test_nullable_outputs_and_counters(listed, off):
    OF.check_nullable(FAM, "decode", listed, off)


# ---------------------------------------------------------------------------------------------------------------------
# 7: frames in turn
# ---------------------------------------------------------------------------------------------------------------------
def test_one_wavefront_decodes_several_frames_in_turn():
    """More frames than the grid's 65536 workgroups: wavefront b decodes frame b and then frame 65536 + b.  The frames that
    share a wavefront are checked against the oracle, all of them against the same frames decoded one per wavefront."""
    name = "s70_66"
    dec = decoder(name)
    G = osdw_model.graph(name)[1]

    def model(ys):
        front = osdw_model.front_oracle(G, ys)
        return front, osdx_model.scan_oracle(G, ys, 1, front)
    OF.check_frames_in_turn(FAM, dec, osdw_model.frames(name, 1.5, 65536 + 300, 31)[0], lambda yd: dec.osdw_decode(yd, 1), model)


# ---------------------------------------------------------------------------------------------------------------------
# 8: refusals launch nothing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wimax_1056", "wide"])
def test_unsupported_shapes_are_refused(name):
    dec = decoder(name)
    yd = to_dev(nms_graphs.frames(name, 2.0, 4, 1)[0], dec)
    OF.check_unsupported(FAM, dec, yd, {
        "front": lambda b: dec.osdw_front(yd, out=(b["perm"], b["parity"], None)),
        "search": lambda b: dec.osdw_search(yd, b["perm"], b["parity"], 1, out=b),
        "decode": lambda b: dec.osdw_decode(yd, 1, perm=b["perm"], parity=b["parity"], out=b)})


def test_bad_arguments_are_refused_and_the_old_families_keep_their_refusal():
    dec = decoder("array_121_80")
    y, _ = osdw_model.frames("array_121_80", 1.5, 4, 2)
    yd = to_dev(y, dec)
    bufs = _sentinels(dec, 4)
    clean = {k: v.clone() for k, v in bufs.items()}
    with pytest.raises(_lib.LdpcError, match=r"\(-1\).*ldpc_osdw_decode: order 4 outside 0\.\.3"):
        dec.osdw_decode(yd, 4, perm=bufs["perm"], parity=bufs["parity"], out=bufs)
    with pytest.raises(_lib.LdpcError, match=r"\(-1\).*ldpc_osdw_search: order -1 outside 0\.\.3"):
        dec.osdw_search(yd, bufs["perm"], bufs["parity"], -1, out=bufs)
    assert _raw_decode(dec, yd, None, None, 4, 1, dict(bufs, cw=None)) == -1
    assert b"ldpc_osdw_decode: d_cw is NULL" in dec.L.ldpc_last_error()
    assert _raw_decode(dec, yd, None, None, 4, 1, dict(bufs, perm=None)) == -1
    assert b"ldpc_osdw_decode: d_perm is NULL" in dec.L.ldpc_last_error()
    assert _raw_decode(dec, yd, None, None, 0, 1, {}) == 0                 # F == 0: LDPC_OK, no launch
    assert not dec.osdx_supported
    old = {k: v for k, v in bufs.items() if k not in ("perm", "parity")}
    perm64, parity64 = bufs["perm"], bufs["parity"][:, :64].contiguous()
    with pytest.raises(_lib.LdpcError, match=r"\(-5\).*1 <= k <= 64 and 1 <= n-k <= 64.*\(121,80\)"):
        dec.osdx_decode(yd, 1, perm=perm64, parity=parity64, out=old)
    with pytest.raises(_lib.LdpcError, match=r"\(-5\).*OSD kernels need an \(n=128, k=64\) code; this one is \(121,80\)"):
        dec.osd_decode(yd, 2)
    torch.cuda.synchronize()
    OF.assert_untouched(bufs, clean)
    assert OF.A.untouched(parity64)


# ---------------------------------------------------------------------------------------------------------------------
# 9: a second context repeats the first; graph capture
# ---------------------------------------------------------------------------------------------------------------------
def test_a_second_context_of_the_code_repeats_the_first():
    from short_ldpc_decoding_osd_amd.runtime import Decoder
    y, _ = osdw_model.frames("array_121_80", 1.0, 8, 7)
    runs = []
    for _ in range(2):
        dec = Decoder(osdw_model.make_code("array_121_80"))
        assert dec.osdw_supported and not dec.osdx_supported
        out = dec.osdw_decode(to_dev(y, dec), 2)
        torch.cuda.synchronize()
        runs.append({k: v.cpu().numpy().tobytes() for k, v in out.items()})
        dec.__del__()          # ldpc_ctx_destroy now, not whenever the collector runs
        assert not dec._ctx.value
    assert runs[0].keys() == runs[1].keys() >= {"cw", "metric", "best", "ntep", "perm", "parity"}
    for key in runs[0]:
        assert runs[0][key] == runs[1][key], key
    ntep, best = (np.frombuffer(runs[0][key], np.int32) for key in ("ntep", "best"))
    assert ntep.size == 8 and ntep.max() > 1 and best.max() > 0          # premise: the searches were searches


def test_decode_is_graph_capturable():
    dec = decoder("array_121_80")
    F = 96
    ys = [osdw_model.frames("array_121_80", 1.5, F, s)[0] for s in (41, 42, 43)]
    want = []
    for y in ys[1:]:
        o = dec.osdw_decode(to_dev(y, dec), 2)
        torch.cuda.synchronize()
        want.append({k: v.clone() for k, v in o.items()})
    ybuf = to_dev(ys[0], dec)
    bufs = _sentinels(dec, F)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):               # no eager call first: the entry point holds no per-stream state
        dec.osdw_decode(ybuf, 2, perm=bufs["perm"], parity=bufs["parity"], out=bufs)
    for y, ref in zip(ys[1:], want):
        ybuf.copy_(to_dev(y, dec))
        graph.replay()
        torch.cuda.synchronize()
        for k in ("perm", "parity", "cw", "metric", "best", "ntep"):
            assert torch.equal(bufs[k], ref[k]), k
