"""-m gpu: OSD for longer and low-rate codes (ldpc_osdl_front / _search / _decode: n <= 384, 1 <= k <= 192, 1 <= n-k <= 192) --
bit-exact against the CPU oracles of tests/osdl_model.py on the reference's (384,192) code and six synthetic codes, and against
ldpc_osdx_* / ldpc_osdw_* on four codes those families serve as well.  Floats compare by their bits.  The premises of the
inputs (which paths of the elimination they take) are asserted on the CPU in tests/test_osdl_host.py."""
import numpy as np
import pytest
import torch

from short_ldpc_decoding_osd_amd import _lib
from tests import osd_family as OF
from tests import osdl_model
from tests.gpu_util import to_dev
from tests.osd_family import assert_scan, decoder

pytestmark = pytest.mark.gpu
_scan = {}
OUTS = ("perm", "parity", "cw", "metric", "best", "ntep")
FAM = OF.OSDL


def layout(dec):
    """Shape tails of perm and parity."""
    return FAM.layout(dec.n, dec.k)[1:3]


def filled(dec, F):
    """Every buffer of a call, prefilled with values no kernel writes."""
    return OF.sentinels(dec, FAM, F)


def assert_front(got, want, dec, rows=slice(None)):
    """(perm, parity, nswaps or None) of the frames ``rows`` against a front_oracle result."""
    OF.assert_front(FAM, dec, got[0][rows], got[1][rows], want, None if got[2] is None else got[2][rows], rows)


def _raw_decode(dec, *args, **kw):
    return OF.raw_decode(dec, FAM, "decode", *args, **kw)


def subset(front, rows):
    perm, parity, ns, Gps = front[:4]
    return perm[rows], parity[rows], ns[rows], [Gps[int(r)] for r in rows]


def scan_case(name, order, rows):
    """The frames ``rows`` of the code's front-end case, their front-end oracle and their scan oracle (computed once)."""
    key = (name, order, tuple(int(r) for r in rows))
    if key not in _scan:
        y, front = osdl_model.front_case(name)
        rows = np.asarray(rows)
        sub = subset(front, rows)
        _scan[key] = (np.ascontiguousarray(y[rows]), sub, osdl_model.scan_oracle(osdl_model.graph(name)[1], y[rows], order, sub))
    return _scan[key]


def order2_rows(name):
    """wl384: two natural frames, a dependent-set frame, a last-step frame and the all-equal and half-zero frames (6 <= 8);
    every other code: its 32 natural frames, the two all-equal frames, the half-zero and the all-zero frame."""
    F = len(osdl_model.front_case(name)[0])
    if name == "wl384":
        return [0, 1, 48 + 1, F - 7, F - 6, F - 4]
    return list(range(32)) + [F - 6, F - 5, F - 4, F - 3]


def check_search_and_decode(name, order, rows):
    dec = decoder(name)
    y, front, ref = scan_case(name, order, rows)
    yd = to_dev(y, dec)
    fr = dec.osdl_front(yd)
    torch.cuda.synchronize()
    assert_front(fr, front, dec)                                   # the search runs on oracle-checked front-end results
    out = dec.osdl_search(yd, fr[0], fr[1], order)
    full = dec.osdl_decode(yd, order)                              # _decode equals _front followed by _search
    torch.cuda.synchronize()
    assert_scan(out, ref)
    assert_scan(full, ref)
    assert_front((full["perm"], full["parity"], None), front, dec)
    return ref


# ---------------------------------------------------------------------------------------------------------------------
# 1: the front end against the C oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", osdl_model.SERVED)
def test_front_end_matches_oracle(name):
    dec = decoder(name)
    y, want = osdl_model.front_case(name)
    assert dec.osdl_supported
    if name in osdl_model.NEW:
        assert not dec.osdx_supported and not dec.osdw_supported
    F = len(y)
    b = filled(dec, F)
    ns = OF.A.sentinel(dec, (F,), torch.int32)
    got = dec.osdl_front(to_dev(y, dec), out=(b["perm"], b["parity"], ns))
    torch.cuda.synchronize()
    assert (tuple(got[0].shape[1:]), tuple(got[1].shape[1:])) == layout(dec)
    perm = got[0].cpu().numpy().view(np.uint16)
    assert all(sorted(p[:dec.n]) == list(range(dec.n)) for p in perm.tolist())
    assert not perm[:, dec.n:].any()                                # the padded entries are written, as zero
    assert_front(got, want, dec)
    assert (want[2] >= 0).all()
    # without nswaps: the same perm and parity
    again = dec.osdl_front(to_dev(y, dec), out=(filled(dec, F)["perm"], filled(dec, F)["parity"], None))
    torch.cuda.synchronize()
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])


# ---------------------------------------------------------------------------------------------------------------------
# 2: the search against the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("name", osdl_model.SERVED)
def test_orders_0_and_1_match_oracle_on_every_front_end_frame(name, order):
    F = len(osdl_model.front_case(name)[0])
    ref = check_search_and_decode(name, order, range(F))
    assert np.isinf(ref["metric"][-2])                              # premise: the saturated frame overflows the metric to +inf
    if (name, order) == ("s100_20", 1):                             # every cost is +inf there: the first TEP wins, as np.argmin has it
        assert ref["ties"][-2] == ref["ntep"][-2] and ref["best"][-2] == 0
    if order == 1:                                                  # premises: a search, and minima shared by many TEPs
        assert (ref["weight"] == 1).any() and (ref["ties"][-6:] > 1).any() and ref["ties"][-3] == ref["ntep"][-3]


@pytest.mark.parametrize("name", osdl_model.SERVED)
def test_order_2_matches_oracle(name):
    ref = check_search_and_decode(name, 2, order2_rows(name))
    assert (ref["ties"] > 1).any()                                  # premise: the first-minimum rule decided a frame
    if decoder(name).k > 1:
        assert (ref["weight"] == 2).any()                           # premise: a winner beyond order 1


@pytest.mark.parametrize("name", ["s100_20", "s193_1"])
def test_order_3_matches_oracle(name):
    F = len(osdl_model.front_case(name)[0])
    ref = check_search_and_decode(name, 3, range(F))
    assert int(ref["ntep"][0]) == {"s100_20": 1351, "s193_1": 2}[name]          # (k = 1: the table ends at weight 1)


# ---------------------------------------------------------------------------------------------------------------------
# 3: the search on inputs the front end cannot produce
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,order", [("s321_130", 1), ("s100_20", 2), ("s193_1", 1), ("array_121_80", 1)])
def test_search_ignores_the_padding(name, order):
    dec = decoder(name)
    n, k, S, W, Wp = osdl_model.shape(name)
    rows = list(range(8)) + [len(osdl_model.front_case(name)[0]) - 6]
    y, front, ref = scan_case(name, order, rows)
    perm, parity = front[0].copy(), front[1].copy()
    assert 64 * S > n or 64 * W > k or 64 * Wp > n - k
    perm[:, n:] = 0xFFFF                                            # entries >= n in the padding
    parity[:, k:, :] = ~np.uint64(0)                                # rows >= k
    if (n - k) % 64:
        parity[:, :, Wp - 1] |= ~np.uint64(0) << np.uint64((n - k) % 64)        # bits >= n-k
    yd = to_dev(y, dec)
    pd = to_dev(perm.view(np.int16), dec)
    qd = to_dev(parity.view(np.int64).reshape((len(rows),) + layout(dec)[1]), dec)
    out = dec.osdl_search(yd, pd, qd, order)
    torch.cuda.synchronize()
    assert_scan(out, ref)


# ---------------------------------------------------------------------------------------------------------------------
# 4: decode, compaction and counts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def listed():
    """s200_100: a shuffled subset of its front-end frames as the frame list, a device-side count below the list's length, and
    the order-1 oracle of the listed frames."""
    name = "s200_100"
    dec = decoder(name)
    y, _ = osdl_model.front_case(name)
    _, labels = osdl_model.frames(name, 1.5, 32, 1)                 # the codewords of the 32 natural frames
    rng = np.random.default_rng(4)
    idx = rng.permutation(32)[:20].astype(np.int32)
    assert not np.all(np.diff(idx) > 0)
    nf = 13
    _, front, ref = scan_case(name, 1, idx[:nf])
    return dict(dec=dec, yd=to_dev(y, dec), labels=labels, label_rows=idx[:nf], index=to_dev(idx, dec), idx=idx, nf=nf, rows=np.arange(nf),
                front=front, ref=ref, count=to_dev(np.array([nf], np.int32), dec), arg=lambda bufs: 1)


def test_frame_list_and_device_count(listed):
    dec, nf = listed["dec"], listed["nf"]
    F = len(listed["idx"])
    for cap in (F, nf, nf - 4):                                     # the device count against the capacity F
        done = min(nf, cap)
        bufs = filled(dec, F)
        assert _raw_decode(dec, listed["yd"], listed["index"], listed["count"], cap, 1, bufs) == 0
        torch.cuda.synchronize()
        assert_scan(bufs, listed["ref"], done)
        assert_front((bufs["perm"], bufs["parity"], None), listed["front"], dec, slice(0, done))
        for k in OUTS:                                              # nothing at or beyond min(count, F)
            assert OF.A.untouched(bufs[k], done), (cap, k)


@pytest.mark.parametrize("off", ["none", "metric", "best", "ntep", "counts", "label"])
def test_nullable_outputs_and_counters(listed, off):
    OF.check_nullable(FAM, "decode", listed, off)


def test_more_frames_than_workgroups():
    """The 32 natural frames of s128_32 tiled to F = 70 001 at order 1: the grid has 65 536 workgroups, so 4 465 wavefronts
    decode two frames in turn.  Every output of every frame equals the tiled oracle result."""
    name, F = "s128_32", 70001
    dec = decoder(name)
    y, front, ref = scan_case(name, 1, range(32))
    reps = -(-F // 32)
    tile = lambda a: np.concatenate([a] * reps)[:F]                 # noqa: E731
    out = dec.osdl_decode(to_dev(tile(y), dec), 1)
    torch.cuda.synchronize()
    assert_scan(out, {k: tile(ref[k]) for k in ("cw", "metric", "best", "ntep")})
    assert_front((out["perm"], out["parity"], None), (tile(front[0]), tile(front[1])), dec)


# ---------------------------------------------------------------------------------------------------------------------
# 5: beside the older families
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", osdl_model.CROSS)
def test_equals_the_older_family(name):
    dec = decoder(name)
    fam = "osdx" if dec.osdx_supported else "osdw"
    assert fam == {"ccsds": "osdx", "ldpc_96_48": "osdx", "array_121_80": "osdw", "s128_96": "osdw"}[name] and dec.osdl_supported
    y, _ = osdl_model.frames(name, 1.5, 256, 3)
    yd = to_dev(y, dec)
    a, b = dec.osdl_front(yd), getattr(dec, fam + "_front")(yd)
    torch.cuda.synchronize()
    assert torch.equal(a[0].to(torch.int32), b[0].to(torch.int32)) and torch.equal(a[2], b[2])
    assert a[1].shape == b[1].shape and a[1].cpu().numpy().tobytes() == b[1].cpu().numpy().tobytes()
    for order, F in ((0, 256), (1, 256), (2, 256)) + (((3, 8),) if name == "ccsds" else ()):
        got = dec.osdl_decode(yd[:F].contiguous(), order)
        ref = getattr(dec, fam + "_decode")(yd[:F].contiguous(), order)
        torch.cuda.synchronize()
        assert torch.equal(got["cw"], ref["cw"]) and torch.equal(got["best"], ref["best"]) and torch.equal(got["ntep"], ref["ntep"])
        assert torch.equal(got["metric"].view(torch.int32), ref["metric"].view(torch.int32))
        assert torch.equal(got["perm"].to(torch.int32), ref["perm"].to(torch.int32))
        assert got["parity"].cpu().numpy().tobytes() == ref["parity"].cpu().numpy().tobytes()
        only = dec.osdl_search(yd[:F].contiguous(), got["perm"], got["parity"], order)
        torch.cuda.synchronize()
        assert torch.equal(only["cw"], ref["cw"]) and torch.equal(only["best"], ref["best"])
        if order:
            assert int(got["best"].max()) > 0                       # premise: some winner is no order-0 candidate


# ---------------------------------------------------------------------------------------------------------------------
# 6: refusals launch nothing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wimax_1056"] + list(osdl_model.REFUSED))
def test_unsupported_shapes_are_refused(name):
    dec = decoder(name)
    assert not dec.osdl_supported and not dec.osdx_supported and not dec.osdw_supported
    assert (dec.n, dec.k) == {"wimax_1056": (1056, 880), "s385_193": (385, 193), "s384_193": (384, 193), "s384_191": (384, 191)}[name]
    yd = to_dev(osdl_model.frames(name, 2.0, 4, 1)[0], dec)
    OF.check_unsupported(FAM, dec, yd, {
        "front": lambda b: dec.osdl_front(yd, out=(b["perm"], b["parity"], None)),
        "search": lambda b: dec.osdl_search(yd, b["perm"], b["parity"], 1, out=b),
        "decode": lambda b: dec.osdl_decode(yd, 1, perm=b["perm"], parity=b["parity"], out=b)})


def test_bad_arguments_are_refused():
    dec = decoder("s100_20")
    y, _ = osdl_model.frames("s100_20", 1.5, 4, 2)
    yd = to_dev(y, dec)
    bufs = filled(dec, 4)
    with pytest.raises(_lib.LdpcError, match=r"\(-1\).*ldpc_osdl_decode: order 4 outside 0\.\.3"):
        dec.osdl_decode(yd, 4, perm=bufs["perm"], parity=bufs["parity"], out=bufs)
    with pytest.raises(_lib.LdpcError, match=r"\(-1\).*ldpc_osdl_search: order -1 outside 0\.\.3"):
        dec.osdl_search(yd, bufs["perm"], bufs["parity"], -1, out=bufs)
    for missing in ("cw", "perm", "parity"):
        assert _raw_decode(dec, yd, None, None, 4, 1, dict(bufs, **{missing: None})) == -1
        assert f"ldpc_osdl_decode: d_{missing} is NULL".encode() in dec.L.ldpc_last_error()
    assert _raw_decode(dec, None, None, None, 4, 1, bufs) == -1
    assert b"ldpc_osdl_decode: d_y is NULL" in dec.L.ldpc_last_error()
    front = lambda y_, perm, parity: OF.raw(dec, FAM, "front", d_y=y_, F=4, d_perm=perm, d_parity=parity)   # noqa: E731
    search = lambda y_, perm, parity, cw: OF.raw(dec, FAM, "search", d_y=y_, F=4, d_perm=perm, d_parity=parity, order=1, d_cw=cw)   # noqa: E731
    for call, args, who in ((front, (None, bufs["perm"], bufs["parity"]), "ldpc_osdl_front: d_y"),
                            (front, (yd, None, bufs["parity"]), "ldpc_osdl_front: d_perm"),
                            (front, (yd, bufs["perm"], None), "ldpc_osdl_front: d_parity"),
                            (search, (None, bufs["perm"], bufs["parity"], bufs["cw"]), "ldpc_osdl_search: d_y"),
                            (search, (yd, None, bufs["parity"], bufs["cw"]), "ldpc_osdl_search: d_perm"),
                            (search, (yd, bufs["perm"], None, bufs["cw"]), "ldpc_osdl_search: d_parity"),
                            (search, (yd, bufs["perm"], bufs["parity"], None), "ldpc_osdl_search: d_cw")):
        assert call(*args) == -1
        assert f"{who} is NULL".encode() in dec.L.ldpc_last_error()
    assert _raw_decode(dec, yd, None, None, 0, 1, {}) == 0                 # F == 0: LDPC_OK, no launch
    assert OF.raw(dec, FAM, "front", F=0) == 0
    assert OF.raw(dec, FAM, "search", F=0, order=1) == 0
    # the older families keep their refusal of this code
    with pytest.raises(_lib.LdpcError, match=r"\(-5\).*1 <= k <= 64 and 1 <= n-k <= 64.*\(100,20\)"):
        dec.osdx_decode(yd, 1)
    with pytest.raises(_lib.LdpcError, match=r"\(-5\).*1 <= n-k <= 64 and n <= 128.*\(100,20\)"):
        dec.osdw_decode(yd, 1)
    torch.cuda.synchronize()
    for k in OUTS:
        assert OF.A.untouched(bufs[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# 7: streams and capture
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wl384", "s128_32"])
def test_side_stream_and_graph_replay(name):
    dec = decoder(name)
    y, front, ref = scan_case(name, 1, range(32))
    yd = to_dev(y, dec)
    eager = dec.osdl_decode(yd, 1)
    torch.cuda.synchronize()
    assert_scan(eager, ref)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = dec.osdl_decode(yd, 1)
    side.synchronize()
    for k in OUTS:
        assert torch.equal(other[k], eager[k]), k
    bufs = filled(dec, 32)
    ybuf = torch.zeros_like(yd)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):                  # no eager call first: the entry point holds no per-stream state
        dec.osdl_decode(ybuf, 1, perm=bufs["perm"], parity=bufs["parity"], out=bufs)
    ybuf.copy_(yd)
    graph.replay()
    torch.cuda.synchronize()
    for k in OUTS:
        assert torch.equal(bufs[k], eager[k]), k
