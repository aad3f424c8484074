"""-m gpu: the order-2 OSD stage after the trim of its wave reductions and per-frame serial work (DPP-fused reductions,
the unsigned-minimum form of wave_min_f32, bucket_scale by reciprocal, the scalar-prefix below_mask, the rotation direction as
a template parameter), bit for bit against the C oracle through ldpc_osd_front, ldpc_osd_search and ldpc_osd_decode.

What each group is for:
  frame counts   1, 2, 65, 300 frames on both order-2 routes: fewer frames than the grid, and the three-deep frame pipeline of
                 the rotation scan with one, two and several trips.
  edge frames    each changed helper at an edge: all magnitudes equal (one bucket, nmax = 128), all zero (m = 0: the scale
                 is +inf), one FLT_MAX among small values (the reciprocal is denormal), denormals only (the reciprocal
                 overflows), quantised values (ties), frames without a column exchange (below_mask is skipped) and frames
                 crafted to exchange at the word borders of the membership mask.
  winners        the best TEP owned by lane 0, lane 63 and a lane of each 16-lane row (the row_bcast steps of the reductions
                 and the read of lane 63), and equal metrics in lanes of different rows (the tie goes to the lower table rank).
  FS, PB         one ldpc_osd_search each at 64 frames: they pick up the new reductions; their own suites cover the rest.

The rotation direction is probed when the context is made and no entry point lets a caller choose it, so both instantiations
cannot be run on one device: the tests rely on the probe's direction.  The winner pairs are chosen so that lanes 0 and 63
own one of them under either direction.

On the mask indices: position 0 never leaves the MRB (column 0 of G is non-zero, so step 0 always finds its pivot) and
position 127 never enters it (the columns outside any hyperplane are the support of a codeword, at least 14 of them, so
rank 64 is reached by position 114 at the latest); x = 0 and x = 127 are arguments of below_mask in every frame with an
exchange (idx1 of lane 0, idx2 of lane 63).  The crafted frames exchange at 31, 32, 63 and 64, asserted from the oracle's
exchange records."""
import numpy as np
import pytest
import torch

from oracle import c_oracle, np_oracle
from tests import osd_adversary as A
from tests import osd_generators as Z
from tests.gpu_util import pack_np, to_dev, words_np
from tests.test_gpu_osd_generators import check_fs, check_pb, fs_run, pb_run

pytestmark = pytest.mark.gpu
F32 = np.float32
FLT_MAX = np.finfo(F32).max
_CACHE = {}


@pytest.fixture(scope="module")
def dec():
    from short_ldpc_decoding_osd_amd import Code
    from short_ldpc_decoding_osd_amd.runtime import Decoder
    return Decoder(Code())


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def natural(dec):
    """300 frames at 2.5 dB with the oracle's front end and order-2 result: computed once, shared, left unchanged."""
    if "natural" not in _CACHE:
        y, cw = np_oracle.make_frames(dec.code.G, 2.5, 300, np.random.default_rng(7301))
        _CACHE["natural"] = (y, cw, Z.front(dec.code.G, y), c_oracle.conv_osd(dec.code.G, y, cw, 2))
    return _CACHE["natural"]


def check_front(dec, yd, front):
    perm, Gp, ns = front
    dperm, dparity, dns = dec.osd_front(yd)
    torch.cuda.synchronize()
    assert np.array_equal(dperm.cpu().numpy().astype(np.int32), perm)
    assert np.array_equal(words_np(dparity), Z.pack_rows(Gp[:, :, 64:]))
    assert np.array_equal(dns.cpu().numpy(), ns)
    return dperm, dparity


def check_result(out, r, n, tag):
    assert np.array_equal(out["best"].cpu().numpy(), r["best"][:n]), tag
    assert np.array_equal(words_np(out["cw"]), pack_np(r["codeword"][:n])), tag
    assert np.array_equal(u32(out["metric"].cpu().numpy()), u32(r["metric"][:n])), tag
    assert (out["ntep"].cpu().numpy() == 2081).all(), tag


def check_both_routes(dec, y, front, r, tag):
    """ldpc_osd_front against the oracle's front end, then front + ldpc_osd_search (osd_search2r_kernel) and ldpc_osd_decode
    (osd_fused2r_kernel) against the oracle's order-2 result."""
    n = len(y)
    yd = to_dev(y, dec)
    dperm, dparity = check_front(dec, yd, tuple(a[:n] for a in front))
    scan = dec.osd_search(yd, dperm, dparity, dec.osd_params(2))
    fused = dec.osd_decode(yd, 2)
    torch.cuda.synchronize()
    check_result(scan, r, n, tag + ("search",))
    check_result(fused, r, n, tag + ("fused",))


@pytest.mark.parametrize("frames", [1, 2, 65, 300])
def test_frame_counts(dec, frames):
    y, cw, front, r = natural(dec)
    check_both_routes(dec, np.array(y[:frames]), front, r, (frames,))


# ---------------------------------------------------------------------------------------------------------- edge frames
def _exchange_frames(dec, y):
    """Frames that must exchange at sorted positions 31, 32 and 63: the support of a row of H (a dependent set of columns of G)
    laid on the positions t - w + 1 .. t of the reliability order, so column t lies in the span of the columns before it."""
    G, H = np.asarray(dec.code.G), np.asarray(dec.code.H)
    rng = np.random.default_rng(7305)
    out = []
    for f, t in enumerate((31, 32, 63, 31, 32, 63)):
        sup = rng.permutation(np.flatnonzero(H[f]))
        rest = rng.permutation(np.setdiff1d(np.arange(128), sup))
        order = np.concatenate([rest[:t + 1 - len(sup)], sup, rest[t + 1 - len(sup):]])
        out.append(A.frame_along(order, y[f], True))
    return np.stack(out)


def edge_sets(dec):
    if "edge" in _CACHE:
        return _CACHE["edge"]
    G = dec.code.G
    y, cw, front, _ = natural(dec)
    rng = np.random.default_rng(7302)
    sign = np.where(np.signbit(y), F32(-1.0), F32(1.0))
    sets = {}
    sets["all_equal"] = (sign[:8] * F32(1.0), cw[:8])
    sets["all_zero"] = (np.concatenate([np.zeros((1, 128), F32), -np.zeros((1, 128), F32), (sign[:2] * F32(0.0))]), cw[:4])
    big = (y[:8] * F32(1e-3)).astype(F32)
    for f in range(8):
        big[f, (0, 63, 64, 127, 17, 90, 5, 100)[f]] = FLT_MAX if f % 2 else -FLT_MAX
    sets["one_flt_max"] = (big, cw[:8])
    den = rng.integers(1, 40, size=(8, 128)).astype(np.uint32).view(F32)             # 1..39 units of 2^-149, many ties
    sets["denormals"] = ((sign[:8] * den).astype(F32), cw[:8])
    sets["quantised"] = (Z.to_grid(y[:24], 2.0), cw[:24])
    none = np.flatnonzero(front[2] == 0)[:8]
    assert len(none) == 8
    sets["no_exchange"] = (np.array(y[none]), cw[none])
    sets["mask_borders"] = (_exchange_frames(dec, y), cw[:6])
    out = {}
    for name, (ys, cs) in sets.items():
        ys = np.ascontiguousarray(ys, dtype=F32)
        out[name] = (ys, cs, Z.front(G, ys), c_oracle.conv_osd(G, ys, cs, 2))
    _CACHE["edge"] = out
    return out


EDGES = ("all_equal", "all_zero", "one_flt_max", "denormals", "quantised", "no_exchange", "mask_borders")


@pytest.mark.parametrize("name", EDGES)
def test_edge_frames(dec, name):
    y, cw, front, r = edge_sets(dec)[name]
    perm, Gp, ns = front
    # the premises, from the oracle and the inputs alone
    if name == "all_equal":
        assert (np.abs(y) == 1.0).all()
    elif name == "all_zero":
        assert (y == 0).all() and np.signbit(y).any() and not np.signbit(y).all()
    elif name == "one_flt_max":
        assert ((np.abs(y) == FLT_MAX).sum(axis=1) == 1).all() and np.isfinite(r["metric"]).all()
    elif name == "denormals":
        assert (np.abs(y) < np.finfo(F32).tiny).all() and (y != 0).all()
    elif name == "quantised":
        assert np.array([len(np.unique(np.abs(row))) for row in y]).max() <= 16
    elif name == "no_exchange":
        assert not ns.any()
    elif name == "mask_borders":
        seen = set()
        for row in y:
            seen |= {i for pair in c_oracle.osd_front(dec.code.G, row)[2] for i in pair}
        assert {31, 32, 63, 64} <= seen
    check_both_routes(dec, y, front, r, (name,))


# -------------------------------------------------------------------------------------------------------------- winners
TIE_LANES = (3, 19, 35, 51)                           # one lane of each 16-lane row
WIN_SINGLES = (0, 63, 5, 21, 37, 53)                  # lane 0, lane 63, one lane of each 16-lane row
WIN_PAIRS = ((0, 1), (0, 63), (62, 63), (7, 20), (24, 40), (33, 50), (49, 60))


def _winner_parity():
    """Dense random P' (so [I | P'] needs no exchange when the MRB is the more reliable half) with the rows TIE_LANES equal."""
    P = np.random.default_rng(7303).integers(0, 2, size=(64, 64))
    for l in TIE_LANES[1:]:
        P[l] = P[TIE_LANES[0]]
    return P


def _run_direct(dec, P, yp, cw):
    """(perm = identity, P') to ldpc_osd_search; the oracle on G = [I | P'], whose front end must be the identity."""
    G = np.concatenate([np.eye(64, dtype=np.int64), P], axis=1)
    for row in yp:
        perm, Gp, sw = c_oracle.osd_front(G, row)
        assert np.array_equal(perm, np.arange(128)) and not sw
    r = c_oracle.conv_osd(G, yp, cw, 2)
    F = len(yp)
    perm = to_dev(np.tile(np.arange(128, dtype=np.uint8), (F, 1)), dec)
    parity = to_dev(np.tile(Z.pack_rows(P).view(np.int64), (F, 1)), dec)
    out = dec.osd_search(to_dev(yp, dec), perm, parity, dec.osd_params(2))
    torch.cuda.synchronize()
    check_result(out, r, F, ("direct",))
    return r


def test_winner_lanes(dec):
    """The all-zero codeword with one or two wrong MRB bits: every position 1.0 (MRB) / 0.5 (parity), so the front end is the
    identity; the order-0 candidate then differs in ~32 parity positions (~16) and the TEP on the wrong bits costs 1 or 2.
    TEP {l} belongs to lane l; pair {a, b} to lane a or b, by the rotation direction."""
    P = _winner_parity()
    sup = [(l,) for l in WIN_SINGLES] + list(WIN_PAIRS)
    yp = np.tile(np.concatenate([np.full(64, 1.0, F32), np.full(64, 0.5, F32)]), (len(sup), 1))
    for f, s in enumerate(sup):
        yp[f, list(s)] = -1.0
    r = _run_direct(dec, P, yp, np.zeros((len(sup), 128), np.int64))
    n1 = len(WIN_SINGLES)
    assert np.array_equal(r["best"][:n1], 64 - np.array(WIN_SINGLES))                  # rank({p}) = 64 - p
    assert (r["best"][n1:] >= 65).all()                                                  # an order-2 TEP
    assert np.array_equal(r["metric"], np.array([1.0] * n1 + [2.0] * len(WIN_PAIRS), F32))
    assert not r["codeword"].any()


def test_equal_metrics_across_lanes(dec):
    """Codeword = row a of [I | P'] for a in TIE_LANES, received with MRB bit a wrong and nothing else: the rows TIE_LANES of
    P' are equal and the MRB magnitudes too, so the TEPs {3}, {19}, {35}, {51} -- four lanes, one in each 16-lane row -- all
    cost exactly 1.0 and the lowest table rank, 64 - 51, wins whichever row was sent."""
    P = _winner_parity()
    F = len(TIE_LANES)
    cw = np.zeros((F, 128), np.int64)
    yp = np.tile(np.concatenate([np.full(64, 1.0, F32), np.full(64, 0.5, F32)]), (F, 1))
    for f, a in enumerate(TIE_LANES):
        cw[f, a] = 1
        cw[f, 64:] = P[a]
        yp[f, 64:][P[a] == 1] = -0.5
    r = _run_direct(dec, P, yp, cw)
    assert (r["best"] == 64 - TIE_LANES[-1]).all() and (r["metric"] == 1.0).all()


# --------------------------------------------------------------------------------------------------------------- FS, PB
def test_fs_and_pb_search(dec):
    y, cw, front, _ = natural(dec)
    G, y, cw = dec.code.G, np.array(y[:64]), cw[:64]
    yd = to_dev(y, dec)
    dperm, dparity = check_front(dec, yd, tuple(a[:64] for a in front))
    th = (0.1, 6.5, 30.0)
    check_fs(fs_run(dec, (yd, dperm, dparity), 2, th, 1), c_oracle.fs_osd(G, y, cw, 2, *th), 1, ("fs",))
    out, aux = pb_run(dec, (yd, dperm, dparity), 2, 2.5, {})
    check_pb(out, aux, c_oracle.pb_osd(G, y, cw, 2, 2.5), ("pb",))
