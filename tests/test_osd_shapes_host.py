"""CPU: the premises of tests/test_gpu_osd_shapes.py, from the models alone, and the models held to the reference restatements
of oracle/np_oracle.py on the very pairs the GPU test searches (tests/osd_shapes.py): a drift of a generator or of a model shows
up here, not as a silently weaker GPU test."""
import numpy as np
import pytest

from oracle import np_oracle
from tests import osd_shapes as S
from tests import osdx_fs_model as M
from tests import osdx_model, osdx_pb_model
from tests.gpu_util import pack_np

F32 = np.float32
bits32 = lambda a: np.asarray(a, dtype=F32).reshape(-1).view(np.uint32)      # noqa: E731
CROSS_FRAMES = 4

# The column exchanges of the structured codes (64 frames at 1.0 dB, float mode), as the CPU oracle counts them: the longest chain
# of one frame and the recorded exchanges (a, b) by the word of the pivot step a and by where the partner b lies.
EXCHANGES = {
    (70, 87, "zero_cols"): dict(most=31, a_lt64=1086, a_ge64=299, b_lt64=796, b_mid=269, b_gek=320),
    (70, 87, "equal_cols"): dict(most=25, a_lt64=719, a_ge64=295, b_lt64=441, b_mid=228, b_gek=345),
    (70, 87, "rank_one"): dict(most=35, a_lt64=1337, a_ge64=314, b_lt64=582, b_mid=245, b_gek=824),
    (96, 128, "zero_cols"): dict(most=50, a_lt64=1056, a_ge64=1341, b_lt64=730, b_mid=1148, b_gek=519),
    (96, 128, "equal_cols"): dict(most=45, a_lt64=667, a_ge64=1325, b_lt64=409, b_mid=978, b_gek=605),
    (96, 128, "rank_one"): dict(most=53, a_lt64=1380, a_ge64=1416, b_lt64=396, b_mid=921, b_gek=1479),
    (100, 108, "zero_cols"): dict(most=21, a_lt64=274, a_ge64=622, b_lt64=151, b_mid=519, b_gek=226),
    (100, 108, "equal_cols"): dict(most=21, a_lt64=146, a_ge64=571, b_lt64=50, b_mid=408, b_gek=259),
    (100, 108, "rank_one"): dict(most=24, a_lt64=312, a_ge64=810, b_lt64=93, b_mid=617, b_gek=412),
}
# FS tags of Batch.fs over every pair case and parameter set of a shape (sorted form, float and grid, order min(2, k))
FS_TAGS = ("zero", "bound1", "bound2", "full", "hit1", "hit2", "hit_after_improvement", "psc_blocked")
_FS = {}


def fs_results(k, n):
    """[(case, set, Batch.fs result)] of the shape, computed once."""
    if (k, n) not in _FS:
        out = []
        for name in S.STRUCTURES:
            for mode in S.MODES:
                c = S.pair(k, n, name, mode)
                b = M.Batch(c["y"], c["perm"], c["Gps"])
                out += [(c, s, b.fs(S.fs_order(k), *s)) for s in S.fs_sets(k, n)]
        _FS[k, n] = out
    return _FS[k, n]


def test_shapes_and_structures_are_the_specified_ones():
    assert {n - k for k, n in S.SHAPES} >= {1, 8, 16, 17} and {k for k, n in S.SHAPES} >= {1, 2, 64, 65, 127}
    assert {n for k, n in S.SHAPES} >= {64, 65} and all(k <= 64 for k, _ in S.BOTH) and all(k > 64 for k, _ in S.WIDE)
    for k, n in S.SHAPES:
        assert 1 <= n - k <= 64 and n <= 128
        m = n - k
        P = {name: S.parity(k, n, name) for name in S.STRUCTURES}
        assert all(p.shape == (k, m) for p in P.values())
        assert not P["zero_rows"][list(S.zero_rows_of(k))].any() and (k < 3 or len(S.zero_rows_of(k)) == 3)
        assert all(np.array_equal(P["equal_rows"][2 * i], P["equal_rows"][2 * i + 1]) for i in range(k // 2))
        assert P["ones_row"][0].all()
        assert all(P["identity"][r, r % m] == 1 and P["identity"][r].sum() == 1 for r in range(k))
        rows = {tuple(r) for r in P["rank_one"] if r.any()}
        assert len(rows) == 1
        if k >= 4:
            h = k // 2
            assert np.array_equal(P["ones_row"][h], 1 - P["ones_row"][1])


@pytest.mark.parametrize("form", S.FORMS)
def test_pair_forms(form):
    for k, n in ((2, 10), (64, 65), (127, 128)):
        c = S.pair(k, n, "equal_rows", "grid", form)
        p = c["perm"][:, :n].astype(np.int64)
        assert all(sorted(r) == list(range(n)) for r in p.tolist()) and not c["perm"][:, n:].any()
        assert np.array_equal(np.take_along_axis(c["y"], p, axis=1), c["yp"])
        assert np.array_equal(np.take_along_axis(c["cw"], p, axis=1), c["cwp"])
        assert not (c["cwp"][:, :k].dot(c["G"]) % 2 != c["cwp"]).any()         # the labels are codewords of [I | P']
        assert c["parity128"].shape == (len(c["y"]), 128) and not c["parity128"][:, k:].any()
        assert (c["parity64"] is None) == (k > 64)
        if k <= 64:
            assert np.array_equal(c["parity64"], c["parity128"][:, :64])
        if n - k < 64:
            assert not (c["parity128"] >> np.uint64(n - k)).any()
        if form == "sorted":
            assert (p == np.arange(n)).all() and (np.diff(np.abs(c["yp"]), axis=1) <= 0).all()
            assert (np.abs(c["yp"]) * 2 == np.round(np.abs(c["yp"]) * 2)).all() and (np.abs(c["yp"]) >= 0.5).all()
        else:
            assert (p != np.arange(n)).any() and (np.diff(np.abs(c["yp"]), axis=1) > 0).any()
        perm, p64, p128 = S.dirty(c)
        assert (perm[:, n:] == 0xEE).all() and (p128[:, k:] == ~np.uint64(0)).all()
        assert np.array_equal(p128[:, :k] & np.uint64((1 << (n - k)) - 1), c["parity128"][:, :k])


def test_extremes_are_finite_and_of_six_kinds():
    for k, n in ((2, 10), (64, 65), (127, 128)):
        c = S.pair(k, n, "random_dense", "extreme")
        y = c["y"]
        assert len(y) == S.FRAMES and np.isfinite(y).all()
        assert np.isfinite(np.abs(y).sum(axis=1, dtype=F32)).all()
        q = S.FRAMES // 6
        assert (np.abs(y[:q]) < 1e-37).all() and (np.abs(y[q:2 * q]) == 0.75).all() and (y[2 * q:3 * q] == 0).any()
        assert (np.abs(y[3 * q:4 * q]) <= 1).all() and (np.abs(y[4 * q:5 * q]) == F32(1e30)).sum() == q
        assert (np.abs(y[5 * q:]) > 2.0 ** 50).any()


@pytest.mark.parametrize("k,n", S.SHAPES)
def test_conventional_model_equals_the_numpy_oracle(k, n):
    """osdx_model.scan_oracle against np_oracle.convention_osd on the sorted form: index, metric bits, codeword.  Order 2 on four
    frames per (structure, mode), which at k >= 100 are more than the GPU test searches at that order."""
    runs = ((2, CROSS_FRAMES),)
    for name in S.STRUCTURES:
        for mode in S.MODES:
            c = S.pair(k, n, name, mode)
            for order, F in runs:
                got = osdx_model.scan_oracle(c["G"], c["y"][:F], order, S.front_of(c))
                for f in range(F):
                    ref = np_oracle.convention_osd(c["yp"][f], c["cwp"][f], c["G"], order)
                    tag = (name, mode, order, f)
                    assert got["best"][f] == ref["best_index"] and got["ntep"][f] == ref["teps_size"], tag
                    assert bits32(got["metric"][f])[0] == bits32(ref["metric"])[0], tag
                    assert np.array_equal(got["cw"][f], pack_np(ref["codeword"][None])[0]), tag   # perm is the identity


@pytest.mark.parametrize("k,n", S.SHAPES)
def test_fs_model_equals_the_numpy_oracle(k, n):
    """Batch.fs against np_oracle.fs_osd_frame on the sorted form, every parameter set, four frames per case: num_teps, both
    quirk answers.  The betas are dyadic, so the model's beta term is the reference's rounding; asserted."""
    order = S.fs_order(k)
    for beta, _, _ in S.fs_sets(k, n):
        assert bits32(M.beta_term(beta, n, k))[0] == bits32(F32(beta * (n - k)))[0], beta
    for c, s, r in fs_results(k, n):
        for f in range(CROSS_FRAMES):
            ref = np_oracle.fs_osd_frame(c["yp"][f], c["cwp"][f], c["G"], order, *s)
            tag = (c["name"], c["mode"], s, f)
            assert r["ntep"][f] == ref["num_teps"], tag
            assert bits32(r["metric_ref"][f])[0] == bits32(ref["metric_ref"])[0], tag
            assert np.array_equal(r["cw_ref"][f], pack_np(ref["codeword_ref"][None])[0]), tag
            assert bool(r["hit"][f]) == (ref["codeword_hit"] is not None), tag
            if r["hit"][f]:
                assert bits32(r["metric_hit"][f])[0] == bits32(ref["metric_hit"])[0], tag
                assert np.array_equal(r["cw_hit"][f], pack_np(ref["codeword_hit"][None])[0]), tag


@pytest.mark.parametrize("k,n", S.BOTH)
def test_pb_model_agrees_with_the_numpy_oracle(k, n):
    """osdx_pb_model.pb against np_oracle.pb_osd_frame (libm's exp, SciPy's binom.cdf) on the sorted form, four frames per case,
    the snr_db alternating: as in tests/test_osdx_pb_host.py a frame may differ only where a decision sits within float rounding
    of a threshold, at most 2 % of the shape's frames."""
    order = min(2, k)
    differ = total = 0
    for name in S.STRUCTURES:
        for mode in S.MODES:
            c = S.pair(k, n, name, mode)
            for i, snr in enumerate(S.PB_SNRS):
                sel = np.arange(i, CROSS_FRAMES, len(S.PB_SNRS))
                r = osdx_pb_model.pb(c["y"][sel], c["perm"][sel], c["Gps"], order, snr)
                for j, f in enumerate(sel):
                    with np.errstate(over="ignore", divide="ignore"):
                        ref = np_oracle.pb_osd_frame(c["yp"][f], None, c["G"], order, snr)
                    got = (int(r["ntep"][j]), int(r["best"][j]), int(r["aux"][j, 0]), int(r["aux"][j, 3]))
                    differ += got != (ref["num_teps"], ref["best_index"], ref["comparisons"], ref["stop"])
                    total += 1
    print((k, n), "frames that differ:", differ, "of", total)
    assert differ <= 0.02 * total


@pytest.mark.parametrize("k,n", [s for s in S.SHAPES if s[1] - s[0] >= 7 and s[0] >= 2])
def test_winner_weights_and_grid_ties(k, n):
    """Over the shape's cases (both forms) at order 2: a winner of each weight 0..min(2, k), and in grid mode a frame where two
    TEPs share the minimum."""
    F = 3 if k >= 100 else S.FRAMES
    weights, ties = set(), 0
    for name in S.STRUCTURES:
        for mode in S.MODES:
            for form in S.FORMS:
                c = S.pair(k, n, name, mode, form)
                r = osdx_model.scan_oracle(c["G"], c["y"][:F], 2, S.front_of(c))
                weights |= set(r["weight"].tolist())
                ties += int((r["ties"] > 1).sum()) if mode == "grid" else 0
    print((k, n), sorted(weights), "grid frames with ties:", ties)
    assert weights >= set(range(min(2, k) + 1)) and ties >= 1


def test_fs_tags_per_family():
    """Every tag of FS_TAGS on a shape with k <= 64 and on one with k > 64, hit_late on one with k > 64."""
    narrow, wide = {}, {}
    for k, n in S.SHAPES:
        counts = M.tag_counts([r for _, _, r in fs_results(k, n)])
        print((k, n), sorted(counts.items()))
        for t, v in counts.items():
            side = narrow if k <= 64 else wide
            side[t] = side.get(t, 0) + v
    for t in FS_TAGS:
        assert narrow.get(t, 0) >= 1 and wide.get(t, 0) >= 1, t
    assert wide.get("hit_late", 0) >= 1
    # the n-k = 1 shapes stop at the all-zero TEP or at the first bound; k = 1 reaches psc_blocked
    for k, n in ((64, 65), (65, 66), (127, 128)):
        assert set(M.tag_counts([r for _, _, r in fs_results(k, n)])) == {"zero", "bound1"}
    assert M.tag_counts([r for _, _, r in fs_results(1, 65)]).get("psc_blocked", 0) >= 1


@pytest.mark.parametrize("k,n", S.CODE_SHAPES)
def test_structured_codes(k, n):
    for name in S.CODE_STRUCTURES:
        H, G, pi = S.code(k, n, name)
        assert G.shape == (k, n) and not (H.dot(G.T) % 2).any() and int(H.sum(axis=1).max()) <= S.MAX_CHECK_DEGREE
        P = S.code_parity(k, n, name)
        zero, rep = int((~G.any(axis=0)).sum()), n - len({tuple(c) for c in G.T})
        if name == "zero_cols":
            assert not P[:, ::3].any() and zero >= len(range(0, n - k, 3))      # a zero column of P' is a check on one bit
        if name == "equal_cols":
            assert all(np.array_equal(P[:, 2 * i], P[:, 2 * i + 1]) for i in range((n - k) // 2)) and (rep >= (n - k) // 2)
        if name == "rank_one":
            assert len({tuple(r) for r in P if r.any()}) == 1
        for mode in S.MODES:
            c = S.code_case(k, n, name, mode)
            assert len(c["y"]) == S.CODE_FRAMES and all(g.shape == (k, n) for g in c["front"][3])
        cls = S.code_case(k, n, name)["classes"]
        print((k, n), name, cls)
        if (k, n, name) in EXCHANGES:
            want = EXCHANGES[k, n, name]
            assert {key: cls[key] for key in want} == want
            assert all(cls[key] > 0 for key in ("a_lt64", "a_ge64", "b_lt64", "b_mid", "b_gek"))
            assert cls["most"] >= (40 if (k, n) == (96, 128) else 20)


def test_every_specified_structured_code_has_its_counts():
    shapes = ((70, 87), (96, 128), (100, 108))
    assert set(EXCHANGES) == {(k, n, s) for k, n in shapes for s in ("zero_cols", "equal_cols", "rank_one")}
