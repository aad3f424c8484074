"""-m gpu: OSD for longer and low-rate codes (ldpc_osdl_front / _search / _decode: n <= 384, 1 <= k <= 192, 1 <= n-k <= 192) --
bit-exact against the CPU oracles of tests/osdl_model.py on the reference's (384,192) code and six synthetic codes, and against
ldpc_osdx_* / ldpc_osdw_* on four codes those families serve as well.  Floats compare by their bits.  The premises of the
inputs (which paths of the elimination they take) are asserted on the CPU in tests/test_osdl_host.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from short_ldpc_decoding_osd_amd import _lib
from tests import osdl_model, osdx_model
from tests.gpu_util import pack_np, to_dev, words_np

pytestmark = pytest.mark.gpu
_decoders, _scan = {}, {}
OUTS = ("perm", "parity", "cw", "metric", "best", "ntep")
NEEDS = r"n <= 384, 1 <= k <= 192 and 1 <= n-k <= 192"


def decoder(name):
    if name not in _decoders:
        from short_ldpc_decoding_osd_amd.runtime import Decoder
        _decoders[name] = Decoder(osdl_model.make_code(name))
    return _decoders[name]


def layout(dec):
    S, W, Wp = dec.words, (dec.k + 63) // 64, (dec.n - dec.k + 63) // 64
    return (64 * S,), ((64 * W,) if Wp == 1 else (64 * W, Wp))


def filled(dec, F, value=7):
    """Every buffer of a call, prefilled."""
    ptail, qtail = layout(dec)
    mk = lambda shape, dt: torch.full(shape, value, dtype=dt, device=dec.device)      # noqa: E731
    return dict(perm=mk((F,) + ptail, torch.int16), parity=mk((F,) + qtail, torch.int64), cw=mk((F, dec.words), torch.int64),
                metric=mk((F,), torch.float32), best=mk((F,), torch.int32), ntep=mk((F,), torch.int32))


def front_np(perm, parity, dec):
    """Device front-end results in the oracle's types: perm [F, 64 S] u16, parity [F, 64 W, Wp] u64."""
    W, Wp = (dec.k + 63) // 64, (dec.n - dec.k + 63) // 64
    return perm.cpu().numpy().view(np.uint16), words_np(parity).reshape(-1, 64 * W, Wp)


def assert_front(got, want, dec, rows=slice(None)):
    """perm, parity (padding included: the oracle's arrays are zero there) and nswaps."""
    perm, parity = front_np(got[0], got[1], dec)
    assert np.array_equal(perm[rows], want[0][rows])
    assert np.array_equal(parity[rows], want[1][rows])
    if got[2] is not None:
        assert np.array_equal(got[2].cpu().numpy()[rows], want[2][rows])


def assert_scan(out, ref, F=None):
    sl = slice(0, F)
    assert np.array_equal(words_np(out["cw"])[sl], ref["cw"][sl])
    assert np.array_equal(out["metric"].cpu().numpy().view(np.uint32)[sl], ref["metric"].view(np.uint32)[sl])
    assert np.array_equal(out["best"].cpu().numpy()[sl], ref["best"][sl])
    assert np.array_equal(out["ntep"].cpu().numpy()[sl], ref["ntep"][sl])


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
    b = filled(dec, F, -1)
    ns = torch.full((F,), -7, dtype=torch.int32, device=dec.device)
    got = dec.osdl_front(to_dev(y, dec), out=(b["perm"], b["parity"], ns))
    torch.cuda.synchronize()
    assert (tuple(got[0].shape[1:]), tuple(got[1].shape[1:])) == layout(dec)
    perm = front_np(got[0], got[1], dec)[0]
    assert all(sorted(p[:dec.n]) == list(range(dec.n)) for p in perm.tolist())
    assert not perm[:, dec.n:].any()                                # the padded entries are written, as zero
    assert_front(got, want, dec)
    assert (want[2] >= 0).all()
    # without nswaps: the same perm and parity
    again = dec.osdl_front(to_dev(y, dec), out=(filled(dec, F, -1)["perm"], filled(dec, F, -1)["parity"], None))
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
def _raw_decode(dec, yd, index, count, F, order, bufs, label=None, counts=None):
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    return dec.L.ldpc_osdl_decode(dec._ctx, p(yd), p(index), p(count), F, order, p(bufs.get("perm")), p(bufs.get("parity")),
                                  p(bufs.get("cw")), p(bufs.get("metric")), p(bufs.get("best")), p(bufs.get("ntep")),
                                  p(label), p(counts), dec._stream())


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
    return dict(dec=dec, yd=to_dev(y, dec), labels=labels, index=to_dev(idx, dec), idx=idx, nf=nf, front=front, ref=ref,
                count=to_dev(np.array([nf], np.int32), dec))


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
            assert bool((bufs[k][done:] == 7).all()), (cap, k)


@pytest.mark.parametrize("off", ["none", "metric", "best", "ntep", "counts", "label"])
def test_nullable_outputs_and_counters(listed, off):
    dec, nf, ref = listed["dec"], listed["nf"], listed["ref"]
    label = to_dev(pack_np(listed["labels"]).view(np.int64), dec)
    bufs = filled(dec, nf)
    counts = torch.tensor([5, 6, 7], dtype=torch.int64, device=dec.device)
    if off in bufs:
        bufs[off] = None
    assert _raw_decode(dec, listed["yd"], listed["index"], listed["count"], nf, 1, bufs,
                       None if off == "label" else label, None if off == "counts" else counts) == 0
    torch.cuda.synchronize()
    assert np.array_equal(words_np(bufs["cw"]), ref["cw"])
    if off != "metric":
        assert np.array_equal(bufs["metric"].cpu().numpy().view(np.uint32), ref["metric"].view(np.uint32))
    if off != "best":
        assert np.array_equal(bufs["best"].cpu().numpy(), ref["best"])
    if off != "ntep":
        assert np.array_equal(bufs["ntep"].cpu().numpy(), ref["ntep"])
    # the counters, recomputed on the host from cw, the labels of the listed frames and ntep
    wrong = int(np.any(ref["cw"] != pack_np(listed["labels"][listed["idx"][:nf]]), axis=1).sum())
    assert 0 < wrong < nf
    want = [5, 6, 7] if off in ("counts", "label") else [5 + nf, 6 + wrong, 7 + (0 if off == "ntep" else int(ref["ntep"].sum()))]
    assert counts.cpu().tolist() == want


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
    y, _ = osdl_model.frames(name, 2.0, 4, 1)
    yd = to_dev(y, dec)
    bufs = filled(dec, 4)
    msg = rf"\(-5\).*{NEEDS}.*\({dec.n},{dec.k}\)"
    with pytest.raises(_lib.LdpcError, match=msg):
        dec.osdl_front(yd, out=(bufs["perm"], bufs["parity"], None))
    with pytest.raises(_lib.LdpcError, match=msg):
        dec.osdl_search(yd, bufs["perm"], bufs["parity"], 1, out=bufs)
    with pytest.raises(_lib.LdpcError, match=msg):
        dec.osdl_decode(yd, 1, perm=bufs["perm"], parity=bufs["parity"], out=bufs)
    torch.cuda.synchronize()
    for k in OUTS:
        assert bool((bufs[k] == 7).all()), k


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
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    front = lambda y_, perm, parity: dec.L.ldpc_osdl_front(dec._ctx, p(y_), None, None, 4, p(perm), p(parity), None, dec._stream())   # noqa: E731
    search = lambda y_, perm, parity, cw: dec.L.ldpc_osdl_search(dec._ctx, p(y_), None, None, 4, p(perm), p(parity), 1, p(cw), None,   # noqa: E731
                                                                 None, None, dec._stream())
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
    assert dec.L.ldpc_osdl_front(dec._ctx, None, None, None, 0, None, None, None, dec._stream()) == 0
    assert dec.L.ldpc_osdl_search(dec._ctx, None, None, None, 0, None, None, 1, None, None, None, None, dec._stream()) == 0
    # the older families keep their refusal of this code
    with pytest.raises(_lib.LdpcError, match=r"\(-5\).*1 <= k <= 64 and 1 <= n-k <= 64.*\(100,20\)"):
        dec.osdx_decode(yd, 1)
    with pytest.raises(_lib.LdpcError, match=r"\(-5\).*1 <= n-k <= 64 and n <= 128.*\(100,20\)"):
        dec.osdw_decode(yd, 1)
    torch.cuda.synchronize()
    for k in OUTS:
        assert bool((bufs[k] == 7).all()), k


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
