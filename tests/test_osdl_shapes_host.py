"""CPU: the premises of tests/test_gpu_osdl_shapes.py, from the models alone, and the models held to the reference restatements
of oracle/np_oracle.py on the very pairs the GPU test searches (tests/osdl_shapes.py): a drift of a generator or of a model shows
up here, not as a silently weaker GPU test."""
import numpy as np
import pytest

from oracle import np_oracle
from tests import osd_shapes as S
from tests import osdl_model, osdl_pb_model
from tests import osdl_shapes as LS
from tests import osdx_fs_model as M
from tests.gpu_util import pack_np

F32 = np.float32
bits32 = lambda a: np.asarray(a, dtype=F32).reshape(-1).view(np.uint32)      # noqa: E731
CROSS_FRAMES = 2
_CONV = {}


def conv(c, order):
    """osdl_model.scan_oracle on the frames the GPU test runs at this order (LS.conv_frames), computed once."""
    key = (c["k"], c["n"], c["name"], c["mode"], c["form"], order)
    if key not in _CONV:
        F = LS.conv_frames(c["k"], order, len(c["y"]))
        _CONV[key] = osdl_model.scan_oracle(c["G"], c["y"][:F], order, LS.front_of(c)) if F else None
    return _CONV[key]


def test_shapes_are_the_specified_ones():
    assert LS.LONG == ((2, 194), (64, 129), (65, 129), (63, 191), (128, 256), (129, 258), (100, 257), (192, 320), (192, 193),
                       (191, 383), (192, 384))
    assert LS.SHORT == S.SHAPES and LS.STRUCTURES == S.STRUCTURES and len(LS.STRUCTURES) == 6
    lay = {}
    for k, n in LS.LONG:
        assert osdl_model.served(n, k) and not (n <= 128 and n - k <= 64) and not (k <= 64 and n - k <= 64), (k, n)
        lay[k, n] = LS.layout(k, n)
    assert {v[2] for v in lay.values()} == {1, 2, 3} and {v[1] for v in lay.values()} == {1, 2, 3}
    assert {v[0] for v in lay.values()} >= {3, 4, 5, 6}                       # both odd slot counts the host rounds up
    # the edges each shape is there for
    assert lay[2, 194] == (4, 1, 3) and 194 - 2 == 192
    assert lay[64, 129] == (3, 1, 2) and 129 - 64 == 65 and lay[65, 129] == (3, 2, 1) and 129 - 65 == 64
    assert lay[63, 191] == (3, 1, 2) and 191 - 63 == 128
    assert lay[128, 256] == (4, 2, 2) and lay[129, 258] == (5, 3, 3) and 258 - 129 == 129
    assert lay[100, 257] == (5, 2, 3) and 257 % 64 == 1
    assert lay[192, 320] == (5, 3, 2) and lay[192, 193] == (4, 3, 1) and lay[191, 383] == (6, 3, 3) == lay[192, 384]
    assert {k for k, n in LS.LONG if n > 128} >= {64, 65, 128, 129} and {n - k for k, n in LS.LONG} >= {1, 64, 65, 128, 129, 192}
    assert {n for k, n in LS.LONG} >= {129, 257, 320}
    for k, n in LS.SHORT:
        assert osdl_model.served(n, k)
    assert {n - k for k, n in LS.SHORT} >= {1, 8, 16, 17} and {k for k, n in LS.SHORT} >= {1, 2}
    assert LS.CODE_SHAPES == ((65, 129), (40, 200), (128, 256), (130, 321), (192, 193), (192, 384))
    assert LS.CODE_STRUCTURES == ("zero_cols", "equal_cols", "rank_one", "identity") and (LS.CODE_FRAMES, LS.CODE_SNR) == (24, 1.0)
    # the frame counts of the conventional scan
    assert [LS.conv_frames(k, o, 6) for k in (64, 65, 99, 100, 149, 150) for o in range(4)] == [
        6, 6, 6, 2, 6, 6, 6, 0, 6, 6, 6, 0, 6, 6, 2, 0, 6, 6, 2, 0, 6, 6, 1, 0]
    assert [LS.fs_pb_frames(k, 6) for k in (1, 149, 150, 192)] == [6, 6, 2, 2] and max(k for k, _ in LS.SHORT) < 150


@pytest.mark.parametrize("form", LS.FORMS)
def test_pair_forms(form):
    for k, n in LS.LONG:
        c = LS.pair(k, n, "equal_rows", "grid", form)
        S_, W, Wp = LS.layout(k, n)
        F = len(c["y"])
        assert F == LS.LONG_FRAMES == 6
        assert c["perm"].shape == (F, 64 * S_) and c["perm"].dtype == np.uint16
        assert c["parity"].shape == (F, 64 * W, Wp) and c["parity"].dtype == np.uint64
        p = c["perm"][:, :n].astype(np.int64)
        assert all(sorted(r) == list(range(n)) for r in p.tolist()) and not c["perm"][:, n:].any()
        assert np.array_equal(np.take_along_axis(c["y"], p, axis=1), c["yp"])
        assert np.array_equal(np.take_along_axis(c["cw"], p, axis=1), c["cwp"])
        assert not (c["cwp"][:, :k].dot(c["G"]) % 2 != c["cwp"]).any()         # the labels are codewords of [I | P']
        for f in range(F):
            q, P = osdl_model.unpack_front(c["perm"][f], c["parity"][f], n, k)
            assert np.array_equal(P, S.parity(k, n, "equal_rows")) and np.array_equal(q, p[f])
        assert not c["parity"][:, k:].any()
        if (n - k) % 64:
            assert not (c["parity"][:, :, Wp - 1] >> np.uint64((n - k) % 64)).any()
        if form == "sorted":
            assert (p == np.arange(n)).all() and (np.diff(np.abs(c["yp"]), axis=1) <= 0).all()
            assert (np.abs(c["yp"]) * 2 == np.round(np.abs(c["yp"]) * 2)).all() and (np.abs(c["yp"]) >= 0.5).all()
        else:
            assert (p != np.arange(n)).any() and (np.diff(np.abs(c["yp"]), axis=1) > 0).any()
        perm, par = LS.dirty(c)                                                # (asserts that something changed, where it can)
        assert LS.has_padding(k, n) == ((k, n) not in ((128, 256), (192, 320), (192, 384)))
        assert (perm[:, n:] == 0xEEEE).all() and (par[:, k:] == ~np.uint64(0)).all()
        live = osdl_model.pack_rows(np.ones((1, n - k), np.uint8), Wp)[0]      # bits < n-k of every word
        assert np.array_equal(par[:, :k] & live, c["parity"][:, :k]) and (par[:, :k] | live == ~np.uint64(0)).all()
        assert np.array_equal(perm[:, :n], c["perm"][:, :n])


def test_short_pairs_are_the_older_pairs_repacked():
    for k, n in LS.SHORT:
        for form in LS.FORMS:
            c, old = LS.pair(k, n, "ones_row", "float", form), S.pair(k, n, "ones_row", "float", form)
            assert len(c["y"]) == S.FRAMES and np.array_equal(c["y"], old["y"]) and np.array_equal(c["yp"], old["yp"])
            assert np.array_equal(c["perm"][:, :n], old["perm"][:, :n]) and c["perm"].shape[1] == 64 * ((n + 63) // 64)
            W = (k + 63) // 64
            assert c["parity"].shape == (S.FRAMES, 64 * W, 1) and np.array_equal(c["parity"][:, :, 0], old["parity128"][:, :64 * W])
            rng = lambda: np.random.default_rng(77)                            # noqa: E731
            assert LS.tep_masks(c, rng()) == S.tep_masks(old, rng())


def test_tep_masks_span_the_row_words_and_reach_zero_and_equal_rows():
    """The seven mask lists of every LONG shape: bits below k only; over the zero rows alone; over a group of equal rows,
    which every equal_rows and rank_one P' has but rank_one at (2,194) (one non-zero row); supports in every row word."""
    for k, n in LS.LONG:
        spans = set()
        for name in LS.STRUCTURES:
            masks = LS.tep_masks(LS.pair(k, n, name, "float"), np.random.default_rng(77))
            assert len(masks) == 7 and all(len(m) == 6 for m in masks) and max(max(m) for m in masks) >> k == 0
            assert [bin(m[0]).count("1") for m in masks[:5]] == [min(w, k) for w in range(5)]
            if name == "zero_rows" and k >= 3:
                zr = sum(1 << r for r in S.zero_rows_of(k))              # (n-k = 1: other rows of P' are zero as well)
                P = S.parity(k, n, name)
                assert all(m & zr == zr and not any(P[p].any() for p in range(k) if (m >> p) & 1) for m in masks[5])
            if name in ("equal_rows", "rank_one"):
                assert LS.equal_row_groups(k, n, name) == ((k, n, name) != (2, 194, "rank_one"))
                if LS.equal_row_groups(k, n, name):
                    assert all(bin(m).count("1") > 1 for m in masks[6])
            spans |= {tuple(sorted({p >> 6 for p in range(k) if (m >> p) & 1})) for ms in masks for m in ms}
        W = (k + 63) // 64
        assert {w for s in spans for w in s} == set(range(W)) and (W < 3 or (0, 1, 2) in spans)
        assert LS.split_masks([(1 << k) - 1], k).shape == (1, W)


def test_extremes_are_finite_and_of_six_kinds():
    for k, n in ((2, 194), (65, 129), (192, 384)):
        c = LS.pair(k, n, "random_dense", "extreme")
        y = c["y"]
        assert len(y) == 6 and np.isfinite(y).all()
        assert np.isfinite(np.abs(y).sum(axis=1, dtype=F32)).all()
        assert (np.abs(y[:1]) < 1e-37).all() and (np.abs(y[1:2]) == 0.75).all() and (y[2:3] == 0).any()
        assert (np.abs(y[3:4]) <= 1).all() and (np.abs(y[4:5]) == F32(1e30)).sum() == 1
        assert (np.abs(y[5:]) > 2.0 ** 50).any()


@pytest.mark.parametrize("k,n", LS.LONG)
def test_models_equal_the_numpy_oracle(k, n):
    """On the sorted float random_dense pair of the shape, bit for bit: osdx_model.scan_oracle against np_oracle.convention_osd
    at order 2, Batch.fs against np_oracle.fs_osd_frame on every parameter set (both quirk answers), osdl_pb_model.pb against
    np_oracle.pb_osd_frame (NumPy's exp, SciPy's binom.cdf) at 1.0 and 2.5 dB: index, counts, stop rule, metric bits, codeword."""
    c = LS.pair(k, n, "random_dense", "float")
    F = min(CROSS_FRAMES, LS.conv_frames(k, 2, len(c["y"])))
    got = conv(c, 2)
    for f in range(F):
        ref = np_oracle.convention_osd(c["yp"][f], c["cwp"][f], c["G"], 2)
        assert got["best"][f] == ref["best_index"] and got["ntep"][f] == ref["teps_size"], f
        assert bits32(got["metric"][f])[0] == bits32(ref["metric"])[0], f
        assert np.array_equal(got["cw"][f], pack_np(ref["codeword"][None])[0]), f          # perm is the identity
    order = LS.fs_order(k)
    b = M.Batch(c["y"][:CROSS_FRAMES], c["perm"][:CROSS_FRAMES], c["Gps"][:CROSS_FRAMES])
    for s in LS.fs_sets(k, n):
        assert bits32(M.beta_term(s[0], n, k))[0] == bits32(F32(s[0] * (n - k)))[0], s
        r = b.fs(order, *s)
        for f in range(CROSS_FRAMES):
            ref = np_oracle.fs_osd_frame(c["yp"][f], c["cwp"][f], c["G"], order, *s)
            assert r["ntep"][f] == ref["num_teps"], (s, f)
            assert bits32(r["metric_ref"][f])[0] == bits32(ref["metric_ref"])[0], (s, f)
            assert np.array_equal(r["cw_ref"][f], pack_np(ref["codeword_ref"][None])[0]), (s, f)
            assert bool(r["hit"][f]) == (ref["codeword_hit"] is not None), (s, f)
            if r["hit"][f]:
                assert bits32(r["metric_hit"][f])[0] == bits32(ref["metric_hit"])[0], (s, f)
                assert np.array_equal(r["cw_hit"][f], pack_np(ref["codeword_hit"][None])[0]), (s, f)
    # PB: the oracle calls NumPy's exp and SciPy's binom.cdf where the model and the kernels call deterministic float routines;
    # as in tests/test_osd_shapes_host.py the two may part where a stop probability sits within float rounding of its
    # threshold.  That happens on one of the 22 frames here ((191,383) at 1.0 dB: rule 1 fires one TEP later in the model, 8486
    # against 8485).  Such a frame must show exactly that -- the same rule, one TEP apart, the same winner, metric and
    # codeword -- and at most one frame of a shape may.
    moved = 0
    for f, snr in enumerate(LS.PB_SNRS):
        r = osdl_pb_model.pb(c["y"][f:f + 1], c["perm"][f:f + 1], c["Gps"][f:f + 1], min(2, k), snr)
        with np.errstate(over="ignore", divide="ignore"):
            ref = np_oracle.pb_osd_frame(c["yp"][f], None, c["G"], min(2, k), snr)
        got = (int(r["ntep"][0]), int(r["best"][0]), int(r["aux"][0, 0]), int(r["aux"][0, 3]))
        want = (ref["num_teps"], ref["best_index"], ref["comparisons"], ref["stop"])
        print((k, n), snr, "model", got, "oracle", want)
        if got != want:
            moved += 1
            assert abs(got[0] - want[0]) == 1 and abs(got[2] - want[2]) <= 2 and got[1] == want[1] and got[3] == want[3] == 1, snr
        assert bits32(r["metric"][0])[0] == bits32(ref["metric"])[0], snr
        assert np.array_equal(r["cw"][0], pack_np(ref["codeword"][None])[0]), snr
    assert moved <= 1 and (moved == 0 or (k, n) == (191, 383))


@pytest.mark.parametrize("k,n", LS.LONG)
def test_ties_and_zero_words(k, n):
    """On the frames and at the orders the GPU test scans.  Grid pairs with equal_rows and with rank_one P': a frame where two
    TEPs share the minimal cost.  zero_rows pairs of a shape with WP >= 2: a frame whose winner has a discrepancy that is zero
    in a whole word."""
    for name in ("equal_rows", "rank_one"):
        c = LS.pair(k, n, name, "grid", "sorted")
        ties = sum(int((conv(c, order)["ties"] > 1).sum()) for order in range(4) if conv(c, order) is not None)
        print((k, n), name, "grid frames (per order) with ties:", ties)
        assert ties >= 1, name
    if LS.layout(k, n)[2] < 2:
        return
    if k < 3:
        # (2,194): zero_rows clears rows where k >= 3 only, so this P' is random; a winner would need 64 hard decisions of the
        # parity part to agree with one of 4 random candidates
        assert S.zero_rows_of(k) == () and S.parity(k, n, "zero_rows").any(axis=1).all()
        return
    assert not S.parity(k, n, "zero_rows")[list(S.zero_rows_of(k))].any()
    found = []
    for mode, form in (("float", "sorted"), ("grid", "sorted"), ("float", "unsorted")):
        c = LS.pair(k, n, "zero_rows", mode, form)
        for order in range(4):
            r = conv(c, order)
            for f in range(len(r["best"]) if r is not None else 0):
                found += [(mode, form, order, f, q) for q, w in enumerate(LS.winner_discrepancy_words(c, r, f)) if not w.any()]
    print((k, n), "winners with an all-zero discrepancy word:", found[:6])
    assert found


@pytest.mark.parametrize("k,n", LS.CODE_SHAPES)
def test_structured_codes(k, n):
    """The codes are what they are said to be, and the exchanges of their 24 float and 24 grid frames, as the C oracle records
    them, over the four structures together: a pivot step without a pivot in every row word the shape has, a partner in every
    slot from that of position k-1 to the last one that holds a position, and frames with three exchanges and more."""
    S_, W, _ = LS.layout(k, n)
    words, slots, ge3 = set(), set(), 0
    for name in LS.CODE_STRUCTURES:
        H, G, pi = LS.code(k, n, name)
        assert G.shape == (k, n) and not (H.dot(G.T) % 2).any() and int(H.sum(axis=1).max()) <= LS.MAX_CHECK_DEGREE == 65
        P = LS.code_parity(k, n, name)
        zero, rep = int((~G.any(axis=0)).sum()), n - len({tuple(col) for col in G.T})
        if name == "zero_cols":
            assert not P[:, ::3].any() and zero >= len(range(0, n - k, 3))      # a zero column of P' is a check on one bit
        if name == "equal_cols":
            assert all(np.array_equal(P[:, 2 * i], P[:, 2 * i + 1]) for i in range((n - k) // 2)) and (rep >= (n - k) // 2)
        if name == "rank_one":
            assert len({tuple(r) for r in P if r.any()}) == 1
        if name == "identity":
            assert all(P[r].sum() == (0 if (k > 64 * (n - k) and r >= 64) else 1) for r in range(k))
        for mode in LS.MODES:
            cc = LS.code_case(k, n, name, mode)
            assert len(cc["y"]) == LS.CODE_FRAMES and all(g.shape == (k, n) for g in cc["front"][3])
            assert cc["front"][0].shape == (24, 64 * S_) and (cc["front"][2] >= 0).all()
            cls = cc["classes"]
            print((k, n), name, mode, cls)
            words |= set(cls["words"])
            slots |= set(cls["slots"])
            ge3 += cls["frames_ge3"]
            assert all(s >= a for a, s in cls["pairs"])
    assert words == set(range(W))
    assert slots >= set(range((k - 1) >> 6, ((n - 1) >> 6) + 1)), slots       # no slot of any of these shapes is out of reach
    assert ge3 >= 1
