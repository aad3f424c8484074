"""-m gpu: the sliding-window scan (ldpc_hosd_sliding / ldpc_hosdx_sliding / ldpc_hosdw_sliding) and the block search at every
window width from 1 to 15 and on block layouts the order paths never produce, against the NumPy model of tests/hosd_layouts.py
(the oracle's order, elimination, cost, window loop and classifier, sliced by layout).  Every comparison is array_equal on bit
patterns.

Layouts over one table of all TEPs of weight <= 2 (natural order and reversed), as functions of (N, win):
  natural    the order patterns' own ten blocks (one of them empty)
  exact      nblk == win: a single decision                  plus_one   nblk == win + 1: two
  b16 b128 b129 b1024   even cuts: the first group holds up to 15 blocks; 128 against 129 blocks picks the search's form;
             1024 is the LDS key limit
  singles    one TEP per block (the last one takes what is left past 1024 blocks)
  big_small  blocks of 257, 513 and 700 TEPs (two and more TEPs per thread in one group), then 40 one-TEP blocks, then the rest
  empties    two empty blocks first and last (a first window that holds +inf: a NaN classifier output and `NaN > margin`), a
             run of win empty blocks (a window of +inf only, which the skip rule's `inf > global_min` passes over; for
             win <= 2 the first window is one and the classifier sees it), a run of win + 2 that a thread's run of TEPs crosses
  random     199 seeded cuts with repeated cut points
Classifiers: the scaled stopping classifier z1 - z0 = a k / nblk - 0.3 min(window) at margin 0.9 (a of hosd_layouts.SCALES, chosen
per case on the model so that the stops spread over the path)
and dense random weights at margins 0.5, 0.0 (a window saturated to p1 == 0 exactly does not stop), 1.0 (never stops) and -1.0
(stops at the first decision whose p1 is a number).  Groups 0, 1, win - 1, 7, nblk, nblk + 5: the results do not depend on the
group, d_teps_evaluated is the end of the first group that reaches deep_limit.  tests/test_hosd_layouts_host.py asserts on the
model what these inputs cover; nothing is launched for a case the model has not cleared (no output within 1e-6 of a margin).
"""
import numpy as np
import pytest
import torch

from tests import hosd_layouts as HL
from tests import hosdx_model as HM
from tests.gpu_util import to_dev

pytestmark = pytest.mark.gpu

ENTRIES = [("ccsds", "hosd"), ("ccsds", "hosdx"), ("ccsds", "hosdw"), ("96_48", "hosdx"), ("5_12", "hosdx"), ("121_80", "hosdw")]
SLIDE_KEYS = ("deep_limit", "global_min", "success", "truth", "cw", "metric", "best")
SEARCH_KEYS = ("block_min", "block_arg", "truth", "cw", "metric", "best")
_decoders, _inputs, _fronts = {}, {}, {}


def decoder(name):
    from short_ldpc_decoding_osd_amd import Code
    from short_ldpc_decoding_osd_amd.runtime import Decoder
    if name not in _decoders:
        path = HL.CODES[name][1]
        _decoders[name] = Decoder(Code(path) if path else Code(H=np.array(HL.code(name)[1])))
        assert (_decoders[name].n, _decoders[name].k) == (HL.code(name)[1].shape[1], HL.code(name)[2].shape[0])
    return _decoders[name]


def frames_on_device(name, kind):
    dec = decoder(name)
    if (name, kind) not in _inputs:
        x, y, cw = HL.frames(name, kind)
        _inputs[name, kind] = dict(x=to_dev(np.array(x), dec), y=to_dev(np.array(y), dec),
                                   lab=to_dev(HM.pack_cw(np.asarray(cw)).view(np.int64), dec))
    return _inputs[name, kind]


def front(name, kind, fam):
    if (name, kind, fam) not in _fronts:
        _fronts[name, kind, fam] = getattr(decoder(name), fam + "_front")(frames_on_device(name, kind)["x"])[:3]
    return _fronts[name, kind, fam]


def bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def search_model(cost, truth, tc, off):
    """The search call on a layout: block minima and arguments, the label's metric, the first minimum and its codeword."""
    mm = [HL.layout_minima(row, off) for row in cost]
    best = [HL.best_before(row, off, len(off) - 1) for row in cost]
    return dict(block_min=np.stack([a for a, _ in mm]), block_arg=np.stack([b for _, b in mm]).astype(np.int32),
                truth=np.asarray(truth, np.float32), best=np.array([b[0] for b in best], np.int32),
                metric=np.array([b[1] for b in best], np.float32),
                cw=HM.pack_cw(np.stack([HL.codeword(tc[f], best[f][0]) for f in range(len(cost))])))


def check_search(dec, fam, d, fr, teps_d, off, want, what):
    off_d = to_dev(np.asarray(off, np.int32), dec)
    got = getattr(dec, fam + "_search")(d["x"], d["y"], fr, teps_d, off_d, label_bits=d["lab"])
    for key in SEARCH_KEYS:
        assert np.array_equal(bits(got[key]), bits(want[key])), (key, what)


@pytest.mark.parametrize("lay", HL.LAYOUTS)
@pytest.mark.parametrize("which", HL.TABLES)
@pytest.mark.parametrize("kind", HL.KINDS)
@pytest.mark.parametrize("name,fam", ENTRIES)
def test_sliding_scan_and_search_on_a_layout(name, fam, kind, which, lay):
    dec, d, fr = decoder(name), frames_on_device(name, kind), front(name, kind, fam)
    c = HL.costs(name, kind, which)
    N = c["cost"].shape[1]
    teps_d = to_dev(HM.teps_of(c["E"]), dec)
    assert name != "121_80" or int(HM.teps_of(c["E"])[:, :2].max()) == 79
    sliding = getattr(dec, fam + "_sliding")
    searched, cases = {}, HL.cases(name, kind, which, lay)
    assert len(cases) == 5 * sum(1 for win in HL.widths(lay) if (lay, win) != ("natural", 15))
    for win, tag, case in cases:
        off = case["off"]
        nblk, key = len(off) - 1, off.tobytes()
        if key not in searched:                 # the same layout through the search call: the sliding call's block minima
            off_m, bmin, barg = HL.minima(name, kind, which, lay, win)
            assert np.array_equal(off_m, off)
            searched[key] = to_dev(off.astype(np.int32), dec)
            check_search(dec, fam, d, fr, teps_d, off, search_model(c["cost"], c["truth"], c["tc"], off), (lay, win))
        assert case["near"] == 0 and (tag != "stop" or case["a"] in HL.SCALES)
        groups = HL.groups(win, nblk)
        outs = [sliding(d["x"], d["y"], fr, teps_d, searched[key], win, case["margin"], case["w"], label_bits=d["lab"], group=g)
                for g in groups]
        for k in SLIDE_KEYS:
            got = bits(torch.stack([o[k] for o in outs]))
            want = bits(case[k])
            for i, g in enumerate(groups):
                assert np.array_equal(got[i], want), (k, lay, win, tag, g)
        teps = torch.stack([o["teps"] for o in outs]).cpu().numpy()
        for i, g in enumerate(groups):
            if g > 0:
                want = np.array([HL.group_end(off, deep, g)[1] for deep in case["deep_limit"]], np.int32)
                assert np.array_equal(teps[i], want), (lay, win, tag, g)
            else:
                assert (off[case["deep_limit"]] - off[0] <= teps[i]).all() and (teps[i] <= N).all(), (lay, win, tag)


@pytest.mark.parametrize("which", [2304, 2305, "heavy"])
@pytest.mark.parametrize("name,fam", [e for e in ENTRIES if e[0] in ("ccsds", "121_80")])
def test_search_at_the_edges_of_the_per_thread_run_form(name, fam, which):
    """ldpc_hosd*_search takes the per-thread-run form for ntep <= 2304, nblk <= 128 and no TEP of weight 3, the work-item form
    otherwise: the light table (2081 TEPs of weight <= 2) padded with its own first TEPs to 2304 and to 2305 TEPs -- every
    repeat ties with its original, the lower index wins --, and the light table with one weight-3 TEP appended, each in 16,
    128 and 129 blocks."""
    dec = decoder(name)
    family, H, G, m = HL.code(name)
    E = HL.light_table(G.shape[0], which)
    teps = HM.teps_of(E)
    assert len(E) == (2082 if which == "heavy" else which) and int(teps[:, 3].max()) == (3 if which == "heavy" else 2)
    teps_d = to_dev(teps, dec)
    for kind in HL.KINDS:
        d, fr = frames_on_device(name, kind), front(name, kind, fam)
        x, y, cw = HL.frames(name, kind)
        tc = [HL.tep_costs(family, x[f], y[f], cw[f], H, E, m) for f in range(len(x))]
        cost, truth = np.stack([t["cost"] for t in tc]), [t["truth"] for t in tc]
        if which != "heavy":                      # the repeats do tie with the minimum, in a later block
            assert sum(1 for row in cost if int(np.argmin(row)) < which - 2081) >= 8
            assert np.array_equal(cost[:, 2081:], cost[:, :which - 2081])
        for nblk in (16, 128, 129):
            off = (np.arange(nblk + 1, dtype=np.int64) * len(E)) // nblk
            check_search(dec, fam, d, fr, teps_d, off, search_model(cost, truth, tc, off), (kind, nblk))
