"""Test helper: the inputs of the PB-OSD tests of the high-rate family (ldpc_osdw_pb_search / _pb_decode).  The CPU model is
tests/osdx_pb_model.py, which serves any k as it is; here are the codes, frames and parameter sets, the front-end results in the
osdw layouts (parity [F,128]), ``equal_magnitudes`` bound to those layouts, this family's ``in_turn`` frames, the shape edges
and the largest frontier.  tests/test_osdw_pb_host.py asserts the coverage of these inputs without a GPU."""
import functools

import numpy as np

from tests import osd_shapes as S
from tests import osd_family as OF
from tests import osdw_fs_model, osdw_model
from tests import osdx_pb_model as M

F32 = np.float32
pb, quantise, tag_counts, frontier_bound = M.pb, M.quantise, M.tag_counts, M.frontier_bound

# code -> [(frames at dB, snr_db, order, frames, quantised)], all from osdw_model.frames(code, dB, frames, 7)
SETS = {
    "array_121_80": [(1.0, 1.0, 2, 48, False), (0.0, 30.0, 2, 8, True), (2.0, 2.0, 3, 16, False)],
    "s128_96": [(1.0, 1.0, 2, 24, False)],
    "s128_65": [(0.0, -4.0, 2, 8, False)],
    "s128_124": [(5.0, 5.0, 2, 8, False)],
    "deg65": [(4.0, 4.0, 3, 2, False)],
    "s70_66": [(4.0, 4.0, 3, 2, False)],
}
CASES = [(name, i) for name in SETS for i in range(len(SETS[name]))]
EVERY_TAG = ("stop0", "stop1", "stop2", "improved", "tie", "late_improvement")

# the slot tiers of osdw_pb_kernel at order 3 (ldpc_osdw_pb.h): 2048 slots serve k <= 64, 4096 k <= 91, 8064 k <= 127
TIER_SLOTS = (2048, 4096, 8064)


slots3, tier = M.slots3, functools.partial(M.tier, slots=TIER_SLOTS)


@functools.lru_cache(maxsize=None)
def case(name, i):
    """-> (y, labels, front oracle in the osdw layouts, order, snr_db, model result) of set i of ``name``, computed once."""
    snr, snr_db, order, F, quant = SETS[name][i]
    G = osdw_model.graph(name)[1]
    y, cw = osdw_model.frames(name, snr, F, 7)
    if quant:
        y = quantise(y)
    y = np.ascontiguousarray(y, dtype=F32)
    front = osdw_model.front_oracle(G, y)
    return y, cw, front, order, snr_db, pb(y, front[0], front[3], order, snr_db)


def winner_spans(name, i):
    """The set of osdw_fs_model.span() values over the winners (rank > 0) of set i of ``name``, with their counts."""
    y, _, front, order, snr_db, r = case(name, i)
    n = y.shape[1]
    out = {}
    for f in range(len(y)):
        if r["best"][f]:
            p = front[0][f, :n].astype(np.int64)
            sup = M.pb_frame(y[f][p], front[3][f], order, snr_db)["support"]
            s = osdw_fs_model.span(sup)
            out[s] = out.get(s, 0) + 1
    return out


# ------------------------------------------------------------------------------------------------------------ shape edges
def edge_frames(k):
    """Frames of a pair the shape-edge test decodes: all 12, at k >= 100 (up to 8129 TEPs per frame in the model) the first 3,
    one per SNR of osd_shapes.SNRS."""
    return 3 if k >= 100 else S.FRAMES


@functools.lru_cache(maxsize=None)
def edge(k, n, name, mode, snr_db):
    """-> (pair, frames, model) of osd_shapes.pair(k, n, name, mode, "sorted") at order 2."""
    c = S.pair(k, n, name, mode, "sorted")
    F = edge_frames(k)
    with np.errstate(invalid="ignore"):                       # (all-zero parity magnitudes: 0 / 0 in beta, which then is 0)
        return c, F, pb(c["y"][:F], c["perm"][:F], c["Gps"][:F], 2, snr_db)


# one order-3 frame just above each tier boundary (k = 65 and k = 92) and the largest frontier (k = 127): (k, n, snr_db)
TIER_FRAMES = ((65, 66, 2.5), (92, 100, 2.5))
LARGEST = (127, 128, 2.5)


@functools.lru_cache(maxsize=None)
def order3_frame(k, n, snr_db):
    """Frame 0 of pair(k, n, "random_dense", "float") at order 3 -> (pair, model)."""
    c = S.pair(k, n, "random_dense", "float", "sorted")
    return c, pb(c["y"][:1], c["perm"][:1], c["Gps"][:1], 3, snr_db)


# --------------------------------------------------------------------------------------------------------- insertion order
EQUAL = ((80, 121, 2, 1, 3), (80, 121, 2, 2, 3), (67, 100, 3, 1, 1))      # (k, n, order, levels, frames)


def equal_magnitudes(k, n, order, levels, F, seed=11):
    """osdx_pb_model.equal_magnitudes_in with two-word parity [F, 128]."""
    return M.equal_magnitudes_in(OF.OSDW, k, n, order, levels, F, seed)


# ---------------------------------------------------------------------------------------------------------- frames in turn
IN_TURN = ("s128_96", 1.0)                                   # code, snr_db


@functools.lru_cache(maxsize=None)
def in_turn(order=2):
    """The construction of osdx_pb_model.in_turn on s128_96 (k = 96, n - k = 32; at order 3 the 8064-slot tier of the kernel, 72
    chunks: two chunk minima per lane), decoded with snr_db = 1: four distinct
    frames, two that no rule stops and two that stop at the first TEP.  All four are noiseless codewords, so the all-zero TEP
    costs 0.0, nothing improves on it (the success rule never runs) and beta = 0: the promising sum is w1 cdfA[0] + w2 cdfH[0]
    with cdfH[0] = 2^-32.
      loud   |y| = 1.574 (1 +- 5 %), c4 |y| ~ -5: q_p ~ 0.0067, cdfA[0] ~ 0.8, spl ~ 0.52, niu ~ 0.977, so the threshold is
             ~ 4.5e-6 and the sum of a weight-2 TEP ~ e^-10 * 0.42 = 1.9e-5: at order 2 every one of the 4657 TEPs is visited.  At
             order 3 the first weight-3 TEP (e^-15) stops the search after all of the lighter ones, with the frontier full.
      quiet  |y| = 0.02: q_p ~ 1/2, niu ~ 0 and the threshold, 2.9e-5 at order 2, lies far above the sum ~ 2^-32.
    -> (y [4, n], labels [4, n], front oracle, model of the four)."""
    name, snr_db = IN_TURN
    G = osdw_model.graph(name)[1]
    _, cw0 = osdw_model.frames(name, 1.0, 4, 7)
    rng = np.random.default_rng(3)
    amp = np.concatenate([F32(1.574) * (1.0 + rng.uniform(-0.05, 0.05, (2, G.shape[1]))), np.full((2, G.shape[1]), 0.02)]).astype(F32)
    y = np.ascontiguousarray(amp * (F32(1.0) - F32(2.0) * cw0.astype(F32)), dtype=F32)
    front = osdw_model.front_oracle(G, y)
    return y, cw0, front, pb(y, front[0], front[3], order, snr_db)
