"""CPU: tests/hosd_layouts.py against the frame models it is built from, the named block layouts, and the coverage conditions
the GPU tests of tests/test_gpu_sliding_layouts.py rely on -- all of them on the model alone, so that no GPU test can pass
vacuously."""
import re

import numpy as np
import pytest

from oracle import np_oracle
from tests import dlosd_model as DM
from tests import hosd_layouts as HL
from tests import hosdw_model as WM
from tests import hosdx_model as HM

LARGE = ("ccsds", "96_48", "121_80")
CALLED = {"ccsds": 38, "96_48": 30, "121_80": 24}     # reversed-table cases in which the calls average is asserted, at least


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ------------------------------------------------------------------------------------- the helper against the frame models
@pytest.mark.parametrize("kind", HL.KINDS)
@pytest.mark.parametrize("name", sorted(HL.CODES))
def test_helper_equals_the_frame_model_on_the_natural_blocks(name, kind):
    family, H, G, m = HL.code(name)
    x, y, cw = HL.frames(name, kind)
    assert (H.shape[1], G.shape[0]) == {"ccsds": (128, 64), "96_48": (96, 48), "5_12": (12, 5), "121_80": (121, 80)}[name]
    blocks = list(HL.natural_blocks(G.shape[0]))
    frame = {"hosd": np_oracle.hosd_frame, "hosdx": HM.hosdx_frame, "hosdw": lambda *a: WM.hosdw_frame(*a, m)}[family]
    c = HL.costs(name, kind, "natural")
    off = HL.layout("natural", c["cost"].shape[1], 1, c["sizes"])
    assert np.array_equal(off, np.insert(np.cumsum([len(E) for E in blocks]), 0, 0)) and (np.diff(off) == 0).any()
    assert len(x) == HL.FRAMES == 32
    for f in range(len(x)):
        want = frame(x[f], y[f], cw[f], H, blocks)
        bmin, barg = HL.layout_minima(c["cost"][f], off)
        assert np.array_equal(bits(bmin), bits(want["block_min"])) and np.array_equal(barg, want["block_arg"]), f
        assert bits(np.float32(c["truth"][f])) == bits(np.float32(want["truth"])), f
        best, metric = HL.best_before(c["cost"][f], off, len(blocks))
        assert best == want["best_index"] and bits(np.float32(metric)) == bits(np.float32(want["metric"])), f
        assert np.array_equal(HL.codeword(c["tc"][f], best), want["codeword"]), f
        # a scan that stops after ``deep`` blocks: the frame model on the first blocks
        deep = 3 + f % (len(blocks) - 3)
        part = frame(x[f], y[f], cw[f], H, blocks[:deep])
        best, metric = HL.best_before(c["cost"][f], off, deep)
        assert best == part["best_index"] and np.array_equal(HL.codeword(c["tc"][f], best), part["codeword"]), (f, deep)


def test_layout_minima_on_empty_blocks_and_ties():
    cost = np.array([3, 1, 1, 2, 0.5, 0.5, 7], np.float32)
    bmin, barg = HL.layout_minima(cost, [0, 0, 0, 3, 3, 4, 7, 7])
    assert bmin.tolist() == [np.inf, np.inf, 1.0, np.inf, 2.0, 0.5, np.inf] and barg.tolist() == [-1, -1, 1, -1, 3, 4, -1]
    assert HL.best_before(cost, [0, 0, 0, 3, 3, 4, 7, 7], 2) == (-1, np.inf) and HL.best_before(cost, [0, 3, 7], 1)[0] == 1
    assert HL.group_end(np.array([0, 2, 4, 6, 8, 9]), 3, 2) == (4, 8) and HL.group_end(np.array([0, 2, 4, 6, 8, 9]), 5, 2) == (5, 9)
    assert HL.group_end(np.array([0, 2, 4, 6, 8, 9]), 1, 7) == (5, 9) and HL.group_end(np.array([1, 2, 4]), 1, 1) == (1, 1)


LOOKUP = [(name, kind, which, lay, win) for name in sorted(HL.CODES) for kind, which, lay, win in (
    ("grid", "reversed", "b128", 4), ("float", "natural", "empties", 3), ("grid", "reversed", "singles", 15),
    ("float", "reversed", "random", 8), ("grid", "natural", "b16", 1), ("float", "reversed", "empties", 15),
    ("grid", "natural", "big_small", 8), ("float", "natural", "plus_one", 11))]


@pytest.mark.parametrize("name,kind,which,lay,win", LOOKUP)
def test_decide_with_the_window_table_equals_the_plain_classifier(name, kind, which, lay, win):
    """``decide`` answering from ``window_table`` against np_oracle.sliding_window_decide under dlosd_model.Classifier itself,
    window by window, on every frame, under the very weights and margins the GPU tests use: the same depth, minimum, success,
    calls, near count and windows seen, and the same p1 bits for every window the plain classifier saw."""
    c = HL.costs(name, kind, which)
    off, bmin, _ = HL.minima(name, kind, which, lay, win)
    used = [HL.stopping_case(name, kind, which, lay, win)] + list(HL.dense_cases(name, kind, which, lay, win).values())
    for case in used:
        d = win + 1
        w1, w2 = case["w"][:d * d].reshape(d, d), case["w"][d * d:].reshape(d, 2)
        tab = HL.window_table(bmin, w1, w2, win)
        for f in range(HL.FRAMES):
            plain = HL.decide(bmin[f], c["truth"][f], w1, w2, win, case["margin"], off, trace=True)
            want = (case["deep_limit"][f], bits(case["global_min"][f:f + 1])[0], bool(case["success"][f]), case["calls"][f])
            assert (plain[0], bits(np.float32(plain[1])), plain[2], plain[3]) == want, (case["margin"], f)
            assert plain[5] == case["seen"][f] and plain[4] == 0
            net = DM.Classifier(w1, w2)
            ok, windows, _, g = np_oracle.sliding_window_decide(bmin[f], c["truth"][f], net, win, case["margin"], off)
            assert (windows + win - 1, bool(ok), len(net.p1)) == (plain[0], plain[2], plain[3])
            assert np.array_equal(bits(np.array(net.p1, np.float32)), bits(tab[0][f, plain[5]].astype(np.float32))), (case["margin"], f)


# ---------------------------------------------------------------------------------------------------------- the layouts
@pytest.mark.parametrize("name", sorted(HL.CODES))
def test_layouts_are_valid_and_hold_what_they_are_named_for(name):
    k = HL.code(name)[2].shape[0]
    E, sizes = HL.table(k, "natural")
    N = len(E)
    assert N == 1 + k + k * (k - 1) // 2 <= 3241 and E.sum(1).max() == 2 and not E[0].any() and not HL.table(k, "reversed")[0][-1].any()
    for lay in HL.LAYOUTS:
        for win in HL.widths(lay):
            off = HL.layout(lay, N, win, sizes)
            nblk = len(off) - 1
            assert off[0] == 0 and off[-1] == N and (np.diff(off) >= 0).all() and 1 <= nblk <= HL.MAX_BLOCKS, (lay, win)
            size = np.diff(off)
            if lay == "exact":
                assert nblk == win
            elif lay == "plus_one":
                assert nblk == win + 1
            elif lay in ("b16", "b128", "b129", "b1024"):
                assert nblk == min(int(lay[1:]), N) and size.min() >= 1 and size.max() - size.min() <= 1
            elif lay == "singles":
                assert nblk == min(N, 1024) and (size[:-1] == 1).all()
            elif lay == "big_small" and N >= 1511:
                assert size[:3].tolist() == [257, 513, 700] and (size[3:43] == 1).all() and nblk == 44
            elif lay == "empties":
                empty = "".join("e" if s == 0 else "x" for s in size)
                runs = [len(r) for r in empty.replace("x", " ").split()]
                assert runs == [2, win, win + 2, 2] and empty.startswith("ee") and empty.endswith("ee") and nblk >= win + 4
                first = empty.index("x")
                assert empty.index("e", first) - first < max(win, 2)       # fewer blocks than a window before the first run
                if N > 256:        # the TEP at the run of win + 2 empty blocks is no multiple of a thread's run: a run crosses it
                    cut = off[[r.start() for r in re.finditer("e+", empty)][2]]
                    assert all(cut % per for per in (-(-N // 256), -(-N // 256) | 1)), (win, cut)
            elif lay == "random":
                assert nblk == 200 and (size == 0).sum() >= 5
    assert N != 16 or len(HL.layout("singles", N, 15)) - 1 == 16               # (5,12): nblk = 16 for win = 15
    valid = {(lay, win) for lay in HL.LAYOUTS for win in HL.widths(lay) if len(HL.layout(lay, N, win, sizes)) - 1 >= win}
    missing = {(lay, win) for lay in HL.LAYOUTS for win in HL.widths(lay)} - valid
    assert missing == {("natural", 15)}                                        # the order-2 path has ten blocks


def test_groups_and_light_tables():
    assert HL.groups(1, 30) == (0, 1, 7, 30, 35) and HL.groups(8, 16) == (0, 1, 7, 16, 21) and HL.groups(5, 200) == (0, 1, 4, 7, 200, 205)
    for k in (64, 80):
        light = HL.light_table(k, 2304)[:2081]
        assert len(HL.light_table(k, 2304)) == 2304 and len(HL.light_table(k, 2305)) == 2305 and light.sum(1).max() == 2
        assert np.array_equal(HL.light_table(k, 2305)[2081:], light[:224]) and light[:k + 1].sum() == k
        heavy = HL.light_table(k, "heavy")
        assert len(heavy) == 2082 and heavy[-1].sum() == 3 and heavy[-1, k - 1] == 1 and np.array_equal(heavy[:-1], light)


# ------------------------------------------------------------------------------------------------ coverage of the inputs
@pytest.mark.parametrize("which", HL.TABLES)
@pytest.mark.parametrize("name", sorted(HL.CODES))
def test_coverage_conditions_hold_on_the_model(name, which):
    depths15, ties, saturated, counted, required, called = {}, {kind: 0 for kind in HL.KINDS}, 0, 0, 0, 0
    for kind in HL.KINDS:
        for lay in HL.LAYOUTS:
            for win, tag, case in HL.cases(name, kind, which, lay):
                counted += len(HL.groups(win, len(case["off"]) - 1))
                nblk, deep = len(case["off"]) - 1, case["deep_limit"]
                off, bmin, _ = HL.minima(name, kind, which, lay, win)
                assert case["near"] == 0 and (deep >= win).all() and (deep <= nblk).all(), (kind, lay, win, tag)
                ties[kind] += sum(HL.skip_rule_ties(case, bmin, win))
                if tag == "stop":
                    assert case["a"] in HL.SCALES, (kind, lay, win)
                    if HL.spread_required(name, lay, nblk, win):
                        assert case["spread"] and HL.depth_spread(case, win), (kind, lay, win, case["a"], sorted(set(deep.tolist())))
                        required += 1
                    if HL.calls_required(name, which, lay, win):
                        assert case["calls"].mean() >= 4, (kind, lay, win, case["a"], case["calls"].mean())
                        called += 1
                    if win == 15:
                        depths15.setdefault(lay, set()).update(deep.tolist())
                    if lay == "empties":
                        seen = HL.infinite_windows(case, bmin, win)
                        assert all(a and b and c for a, b, c in seen), (kind, win)
                        assert win > 2 or all(np.isinf(bmin[f, :win]).all() and s[0] == 0 for f, s in enumerate(case["seen"]))
                elif tag == "dense1.0":
                    assert (deep == nblk).all() and (case["calls"] >= 1).all()
                elif tag == "dense-1.0":          # stops at the first decision whose p1 is a number
                    for f, seen in enumerate(case["seen"]):
                        p = case["p1"][f, seen]
                        assert np.isnan(p[:-1]).all() and (not np.isnan(p[-1]) or deep[f] == nblk), (kind, lay, win, f)
                elif tag == "dense0.0":           # a window saturated to p1 == 0 exactly does not stop
                    for f, seen in enumerate(case["seen"]):
                        p = case["p1"][f, seen]
                        saturated += int((p[:-1] == 0.0).sum())
                        assert ((p[:-1] == 0.0) | np.isnan(p[:-1])).all() and (p[-1] > 0.0 or deep[f] == nblk), (kind, lay, win, f)
    assert saturated > 0 and ties["grid"] > 0, (saturated, ties)
    assert name == "5_12" or (required == 56 and (which != "reversed" or called >= CALLED[name])), (required, called)
    print(f"{name} {which}: {counted} (layout, win, classifier, margin, group) cases per entry point; tied skip-rule decisions "
          f"{ties}; windows saturated to p1 == 0 passed over {saturated}; deep_limit at win = 15 per layout "
          f"{ {lay: sorted(v) for lay, v in depths15.items()} }; depth spread asserted in {required} cases, the calls average in {called}")


def test_where_the_spread_is_required():
    """``spread_required`` from the shape alone: every layout with nblk >= win + 4 but ``empties`` and ``big_small``, on the
    three larger codes, with at least eight depths strictly between win and nblk."""
    want = {"natural": (1,), "b16": tuple(range(1, 8)), "b128": HL.SOME_WINS, "b129": HL.SOME_WINS, "b1024": HL.SOME_WINS,
            "singles": HL.SOME_WINS, "random": HL.SOME_WINS, "exact": (), "plus_one": (), "big_small": (), "empties": ()}
    for name in LARGE:
        k = HL.code(name)[2].shape[0]
        E, sizes = HL.table(k, "natural")
        for lay in HL.LAYOUTS:
            got = tuple(win for win in HL.widths(lay) if HL.spread_required(name, lay, len(HL.layout(lay, len(E), win, sizes)) - 1, win))
            assert got == want[lay], (name, lay, got)
    assert not HL.spread_required("5_12", "b16", 16, 1)
    bmin = np.array([[5, 7, 5, 9, 4, np.inf, 4, 3]], np.float32)
    assert HL.decisions_offered(bmin, 2).tolist() == [5] and HL.decisions_offered(bmin, 7).tolist() == [2]
