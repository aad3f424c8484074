"""-m gpu: PB-OSD for longer and low-rate codes (ldpc_osdl_pb_search / _pb_decode: n <= 384, 1 <= k <= 192, 1 <= n-k <= 192)
-- bit-exact against the model of tests/osdl_pb_model.py on the wimax-like (384,192) code and the synthetic codes of
tests/osdl_model.py, on full scans and first-TEP stops that one wavefront decodes in turn in every slot tier of the kernel,
just above each tier boundary, on tied reliability sums, and against ldpc_osdx_pb_* / ldpc_osdw_pb_* on the codes an older
family serves as well.  The inputs and what they reach are those tests/test_osdl_pb_host.py asserts on the CPU.  Integers
compare equal, floats by their bits."""
import numpy as np
import pytest
import torch

from short_ldpc_decoding_osd_amd import _lib
from tests import osd_family as OF
from tests import osdl_model
from tests import osdl_pb_model as LP
from tests.gpu_util import pack_np, to_dev
from tests.osd_family import assert_pb, assert_same, decoder, new_aux, pb_params

pytestmark = pytest.mark.gpu
FAM = OF.OSDL
KEYS = ("cw", "metric", "best", "ntep", "aux")


def dev_front(perm, parity, dec):
    return OF.dev_front(perm, parity, dec, FAM)



def assert_front(perm, parity, front, dec, pick=slice(None)):
    OF.assert_front(FAM, dec, perm, parity, front, rows=pick)


def sentinels(dec, F):
    return OF.sentinels(dec, FAM, F, aux=True)


def _raw_decode(dec, *args, **kw):
    return OF.raw_decode(dec, FAM, "pb_decode", *args, **kw)


def _raw_search(dec, *args):
    return OF.raw_search(dec, FAM, "pb_search", *args)


def check_against_model(dec, y, front, order, snr_db, ref, where=""):
    """search on the oracle's front, decode, search on the decode's own front."""
    F = len(y)
    yd = to_dev(y, dec)
    operm, oparity = dev_front(front[0], front[1], dec)
    aux1, aux2, aux3 = new_aux(dec, F), new_aux(dec, F), new_aux(dec, F)
    out = dec.osdl_pb_search(yd, operm, oparity, pb_params(dec, order, snr_db, aux1))
    full = dec.osdl_pb_decode(yd, pb_params(dec, order, snr_db, aux2))
    again = dec.osdl_pb_search(yd, full["perm"], full["parity"], pb_params(dec, order, snr_db, aux3))
    torch.cuda.synchronize()
    assert_pb(out, aux1, ref, where=(where, "search"))
    assert_front(full["perm"], full["parity"], front, dec)
    assert_pb(full, aux2, ref, where=(where, "decode"))
    assert_pb(again, aux3, ref, where=(where, "search on the decode's front"))


# ---------------------------------------------------------------------------------------------------------------------
# 1: natural frames
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(LP.NATURAL)))
def test_pb_matches_the_model_on_natural_frames(i):
    name = LP.NATURAL[i][0]
    dec = decoder(name)
    assert dec.osdl_supported and not dec.osdx_supported and not dec.osdw_supported
    y, _, front, order, snr_db, ref = LP.natural(i)
    check_against_model(dec, y, front, order, snr_db, ref, LP.NATURAL[i])


# ---------------------------------------------------------------------------------------------------------------------
# 2: full scans and first-TEP stops in turn on one wavefront, in every slot tier
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("code", LP.IN_TURN, ids=str)
def test_one_wavefront_decodes_loud_and_quiet_frames_in_turn(code, order):
    """The grid of a call follows its frame count, so a wavefront decodes frames in turn only beyond the 65536 workgroups of
    the grid: wavefront b < 64 decodes frame b and then frame 65536 + b.  Four distinct frames -- two loud ones (a full
    order-2 scan; at order 3 a stop on the first weight-3 TEP with every weight-3 run live) and two quiet ones (a stop at the
    first TEP) -- are tiled through d_index so that such a wavefront meets a long search and then a first-TEP stop, or the other
    way round, or two of a kind: what a frame leaves in the frontier slots, the chunk minima, the high-water mark of the
    emptying or the CDF table must not reach the next one.  (Frames 64..65535 are first-TEP stops.)"""
    dec = decoder(code)
    y, labels, front, ref = LP.in_turn(code, order)
    assert ref["ntep"][2:].tolist() == [1, 1] and ref["ntep"][0] == ref["ntep"][1] > 500
    assert order == 2 or ref["peak"][0] == (dec.k - 1) * (dec.k - 2) // 2
    check_against_model(dec, y, front, order, LP.LOUD_SNR_DB, ref, (code, order))      # the four frames, a wavefront each
    extra = 64
    F = 65536 + extra
    f = np.arange(F)
    b = f & 65535
    # wavefront b < 64: (first, second) kind by b mod 4 = (long, stop), (stop, long), (long, long), (stop, stop)
    first = np.array([0, 1, 0, 1])[b & 3]
    second = np.array([1, 0, 0, 1])[b & 3]
    kind = np.where(f < 65536, np.where(b < extra, first, 1), second)      # 0: long search, 1: first-TEP stop
    idx = (2 * kind + ((f >> 2) & 1)).astype(np.int32)
    assert {(int(kind[i]), int(kind[65536 + i])) for i in range(extra)} == {(0, 1), (1, 0), (0, 0), (1, 1)}
    aux = new_aux(dec, F)
    label = to_dev(pack_np(labels).view(np.int64), dec)
    counts = torch.zeros(3, dtype=torch.int64, device=dec.device)
    out = dec.osdl_pb_decode(to_dev(y, dec), pb_params(dec, order, LP.LOUD_SNR_DB, aux), index=to_dev(idx, dec), F=F, label_bits=label,
                             counts=counts)
    torch.cuda.synchronize()
    pick = torch.from_numpy(idx.astype(np.int64)).to(dec.device)
    want = dict(cw=to_dev(ref["cw"].view(np.int64), dec), metric=to_dev(ref["metric"], dec), best=to_dev(ref["best"], dec),
                ntep=to_dev(ref["ntep"], dec), aux=to_dev(ref["aux"], dec))
    got = dict(out, aux=aux)
    for k in KEYS:
        a, b_ = got[k], want[k][pick]
        if k == "metric":
            a, b_ = a.view(torch.int32), b_.view(torch.int32)
        assert torch.equal(a, b_), k
    wrong = np.any(ref["cw"] != pack_np(labels), axis=1)[idx]
    assert counts.cpu().tolist() == [F, int(wrong.sum()), int(ref["ntep"][idx].astype(np.int64).sum())]


# ---------------------------------------------------------------------------------------------------------------------
# 3: one order-3 frame just above each tier boundary, every weight-3 run of that k live
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code", LP.TIER_FRAMES, ids=str)
def test_order_3_frame_just_above_a_tier_boundary(code):
    dec = decoder(code)
    y, _, front, ref = LP.in_turn(code, 3, 1, 0)
    check_against_model(dec, y, front, 3, LP.LOUD_SNR_DB, ref, code)


# ---------------------------------------------------------------------------------------------------------------------
# 4: ties: the visit order is the insertion order, across slots and chunks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,n,order,levels,F", LP.EQUAL)
def test_equal_magnitudes(k, n, order, levels, F):
    dec = decoder((k, n))
    c = LP.equal_magnitudes(k, n, order, levels, F)
    aux = new_aux(dec, F)
    perm, parity = dev_front(c["perm"], c["parity"], dec)
    out = dec.osdl_pb_search(to_dev(c["y"], dec), perm, parity, pb_params(dec, order, c["snr_db"], aux))
    torch.cuda.synchronize()
    assert_pb(out, aux, c["model"], where=(k, n, order, levels))


@pytest.mark.parametrize("i,F", LP.QUANTISED)
def test_quantised_inputs(i, F):
    dec = decoder(LP.NATURAL[i][0])
    y, _, front, order, snr_db, ref = LP.natural(i, True)
    check_against_model(dec, y, front, order, snr_db, ref, ("quantised", LP.NATURAL[i]))


# ---------------------------------------------------------------------------------------------------------------------
# 5: one search, three prefixes: a code an older family serves gives the same outputs through this one
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("name", osdl_model.CROSS)
def test_equals_the_older_family(name, order):
    dec = decoder(name)
    fam = "osdx" if dec.osdx_supported else "osdw"
    assert fam == {"ccsds": "osdx", "ldpc_96_48": "osdx", "array_121_80": "osdw", "s128_96": "osdw"}[name] and dec.osdl_supported
    F = 48
    snr = {"ccsds": 1.5, "ldpc_96_48": 1.5, "array_121_80": 2.0, "s128_96": 1.0}[name]
    y, _ = osdl_model.frames(name, snr, F, 7)
    yd = to_dev(y, dec)
    a1, a2, a3 = new_aux(dec, F), new_aux(dec, F), new_aux(dec, F)
    got = dec.osdl_pb_decode(yd, pb_params(dec, order, snr, a1))
    want = getattr(dec, fam + "_pb_decode")(yd, pb_params(dec, order, snr, a2))
    again = dec.osdl_pb_search(yd, got["perm"], got["parity"], pb_params(dec, order, snr, a3))
    torch.cuda.synchronize()
    assert_same(dict(got, aux=a1), dict(want, aux=a2), KEYS, (name, order))
    assert_same(dict(again, aux=a3), dict(want, aux=a2), KEYS, (name, order))
    assert torch.equal(got["perm"].to(torch.int32), want["perm"].to(torch.int32))        # value for value
    assert int(got["best"].max()) > 0 and len(set(got["ntep"].cpu().tolist())) > 3      # premise: the searches were searches


# ---------------------------------------------------------------------------------------------------------------------
# 6: frame lists, device-side counts, nullable outputs, counters
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def listed():
    """wl384, the 12 frames of NATURAL[0] (order 2, both stop rules, three first-TEP stops): a list of 20 of them with repeats,
    not ascending."""
    dec = decoder("wl384")
    y, cw, front, order, snr_db, ref = LP.natural(0)
    rng = np.random.default_rng(17)
    idx = np.concatenate([rng.integers(0, len(y), 12), [11, 3, 3, 6, 9, 9, 2, 0]]).astype(np.int32)
    nf = len(idx)
    assert len(set(idx.tolist())) < nf and np.any(np.diff(idx) < 0)
    assert len(set(ref["aux"][idx, 3].tolist())) == 2 and len(set(ref["ntep"][idx].tolist())) > 3
    return dict(dec=dec, yd=to_dev(y, dec), labels=cw, label_rows=idx, index=to_dev(idx, dec),
                count=to_dev(np.array([nf], np.int32), dec), nf=nf, rows=idx, ref=ref, front=front, order=order, snr_db=snr_db,
                arg=lambda bufs: pb_params(dec, order, snr_db, bufs["aux"]), some_wrong=False)


@pytest.mark.parametrize("which", ["smaller", "equal", "larger"])
def test_frame_list_and_device_count(listed, which):
    OF.check_frame_list(FAM, "pb_decode", listed, which)


@pytest.mark.parametrize("off", ["none", "metric", "best", "ntep", "aux", "counts", "label", "metric+best+ntep+aux"])
def test_nullable_outputs_and_counters(listed, off):
    OF.check_nullable(FAM, "pb_decode", listed, off)


@pytest.mark.parametrize("mask", range(1, 15))
def test_every_subset_of_the_nullable_outputs_through_the_search(listed, mask):
    """metric, best, ntep and aux: each of the 14 proper non-empty subsets present, the others NULL (all and none: above)."""
    OF.check_nullable_subsets(FAM, "pb_search", listed, mask)


# ---------------------------------------------------------------------------------------------------------------------
# 7: refusals launch nothing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wimax_1056"] + list(osdl_model.REFUSED))
def test_unsupported_shapes_are_refused(name):
    dec = decoder(name)
    assert not dec.osdx_supported and not dec.osdw_supported
    yd = to_dev(osdl_model.frames(name, 2.0, 4, 1)[0], dec)
    OF.check_unsupported(FAM, dec, yd, {
        "pb_search": lambda b: dec.osdl_pb_search(yd, b["perm"], b["parity"], pb_params(dec, 1, 1.0, b["aux"]), out=b),
        "pb_decode": lambda b: dec.osdl_pb_decode(yd, pb_params(dec, 1, 1.0, b["aux"]), perm=b["perm"], parity=b["parity"], out=b)})


def test_bad_arguments_are_refused_and_the_older_families_keep_their_refusal():
    name = "s200_100"
    dec = decoder(name)
    y, _ = osdl_model.frames(name, 1.5, 4, 2)
    yd = to_dev(y, dec)
    bufs = sentinels(dec, 4)
    clean = {k: v.clone() for k, v in bufs.items()}
    good = pb_params(dec, 2, 1.5, bufs["aux"])
    OF.check_bad_arguments(FAM, "pb", dec, yd, bufs, lambda order, **kw: pb_params(dec, order, 1.5, **kw), good)
    # the older families still refuse this code, in their own words
    old = {k: v for k, v in bufs.items() if k not in ("perm", "parity")}
    perm8, par64, par128 = (OF.A.sentinel(dec, (4, w), dt) for w, dt in ((128, torch.uint8), (64, torch.int64), (128, torch.int64)))
    osdx = r"\(-5\).*the any-shape OSD kernels need 1 <= k <= 64 and 1 <= n-k <= 64; this code is \(200,100\)"
    osdw = r"\(-5\).*the high-rate OSD kernels need 1 <= n-k <= 64 and n <= 128; this code is \(200,100\)"
    with pytest.raises(_lib.LdpcError, match=osdx):
        dec.osdx_pb_search(yd, perm8, par64, good, out=old)
    with pytest.raises(_lib.LdpcError, match=osdx):
        dec.osdx_pb_decode(yd, good, perm=perm8, parity=par64, out=old)
    with pytest.raises(_lib.LdpcError, match=osdw):
        dec.osdw_pb_search(yd, perm8, par128, good, out=old)
    with pytest.raises(_lib.LdpcError, match=osdw):
        dec.osdw_pb_decode(yd, good, perm=perm8, parity=par128, out=old)
    torch.cuda.synchronize()
    OF.assert_untouched(bufs, clean)
    assert OF.A.untouched(perm8) and OF.A.untouched(par64) and OF.A.untouched(par128)


def test_order_is_bounded_by_k():
    """s193_1 (k = 1): weight class 2 does not exist, so order 2 is refused; order 1 visits the single position (NATURAL[7])."""
    name = "s193_1"
    dec = decoder(name)
    assert dec.k == 1
    y, _, front, order, snr_db, ref = LP.natural(7)
    yd = to_dev(y, dec)
    bufs = sentinels(dec, len(y))
    clean = {k: v.clone() for k, v in bufs.items()}
    with pytest.raises(_lib.LdpcError, match=r"\(-1\).*ldpc_osdl_pb_decode: order 2 outside 0\.\.1"):
        dec.osdl_pb_decode(yd, pb_params(dec, 2, 0.0), perm=bufs["perm"], parity=bufs["parity"], out=bufs)
    with pytest.raises(_lib.LdpcError, match=r"\(-1\).*ldpc_osdl_pb_search: order 2 outside 0\.\.1"):
        dec.osdl_pb_search(yd, bufs["perm"], bufs["parity"], pb_params(dec, 2, 0.0), out=bufs)
    torch.cuda.synchronize()
    OF.assert_untouched(bufs, clean)
    ref0 = LP.pb(y, front[0], front[3], 0, snr_db)
    aux = new_aux(dec, len(y))
    out = dec.osdl_pb_decode(yd, pb_params(dec, 0, snr_db, aux))
    torch.cuda.synchronize()
    assert_pb(out, aux, ref0, where="order 0")
    assert ref0["ntep"].tolist() == [1] * len(y) and not ref0["aux"].any()


# ---------------------------------------------------------------------------------------------------------------------
# 8: graph capture
# ---------------------------------------------------------------------------------------------------------------------
def test_pb_decode_is_graph_capturable():
    dec = decoder("wl384")
    F = 8
    a, b = LP.natural(0), LP.natural(2)                         # the frames at 2.0 dB and at 1.0 dB, order 2
    order, snr_db = a[3], a[4]
    assert b[3] == order
    bufs = sentinels(dec, F)
    p = pb_params(dec, order, snr_db, bufs["aux"])
    ybuf = torch.zeros((F, dec.n), dtype=torch.float32, device=dec.device)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):               # no eager call first: the entry point holds no per-stream state
        dec.osdl_pb_decode(ybuf, p, perm=bufs["perm"], parity=bufs["parity"], out=bufs)   # front end, then search: one chain
    for y in (a[0][:F], b[0][:F]):
        ybuf.copy_(to_dev(y, dec))
        graph.replay()
        torch.cuda.synchronize()
        eager_aux = new_aux(dec, F)
        eager = dec.osdl_pb_decode(to_dev(y, dec), pb_params(dec, order, snr_db, eager_aux))
        torch.cuda.synchronize()
        assert_same(dict(bufs), dict(eager, aux=eager_aux), KEYS + ("perm", "parity"))
    assert_pb(bufs, bufs["aux"], LP.pb(b[0][:F], b[2][0][:F], b[2][3][:F], order, snr_db))
