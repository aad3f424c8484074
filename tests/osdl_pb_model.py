"""Test helper: the inputs of tests/test_gpu_osdl_pb.py in the osdl layouts (tests/test_osdl_pb_host.py asserts their premises
without a GPU): natural and quantised frames, loud and quiet noiseless frames per slot tier, equal magnitudes.  The CPU model is
tests/osdx_pb_model.py (``pb``), which serves any (k, n); this module owns no arithmetic.
"""
import functools

import numpy as np

from tests import osd_family as OF
from tests import osdl_model
from tests import osdx_pb_model as M

F32 = np.float32
det_expf, binom_cdf, quantise, tag_counts, frontier_bound = M.det_expf, M.binom_cdf, M.quantise, M.tag_counts, M.frontier_bound


pb, pb_frame = M.pb, M.pb_frame


def span(sup):
    """The MRB words a support lies in, ascending, one entry per position: (1, 2), (1, 1), ..."""
    return tuple(p >> 6 for p in sup)


# ---------------------------------------------------------------------------------------------------------------------
# the slot tiers of osdl_pb_kernel at order 3 (ldpc_osdl_pb.h): 2048 slots serve k <= 64, 4096 k <= 91, 8064 k <= 127 and
# 18 368 k <= 192; orders <= 2 take 192 slots
# ---------------------------------------------------------------------------------------------------------------------
TIER_SLOTS = (2048, 4096, 8064, 18368)


slots3, tier = M.slots3, functools.partial(M.tier, slots=TIER_SLOTS)


# ---------------------------------------------------------------------------------------------------------------------
# codes: the named ones of osdl_model, or a shape (k, n): osd_family.shape_graph
# ---------------------------------------------------------------------------------------------------------------------
def graph(code):
    """-> (H, G) of a name of osdl_model or of a shape (k, n)."""
    return OF.shape_graph(*code) if isinstance(code, tuple) else osdl_model.graph(code)


# ---------------------------------------------------------------------------------------------------------------------
# 1: natural frames, all from osdl_model.frames(code, dB, frames, 7), decoded with snr_db = the channel's
# ---------------------------------------------------------------------------------------------------------------------
# (code, dB, order, frames)
NATURAL = (("wl384", 2.0, 2, 12), ("wl384", 2.0, 3, 6), ("wl384", 1.0, 2, 8), ("s200_100", 1.0, 3, 8), ("s128_32", 0.0, 3, 12),
           ("s100_20", 0.0, 3, 8), ("s321_130", 1.0, 2, 8), ("s193_1", 0.0, 1, 8), ("s256_192", 3.0, 2, 8), ("s256_192", 1.0, 2, 8))
SEED = 7


@functools.lru_cache(maxsize=None)
def natural(i, quant=False):
    """-> (y, labels, front oracle in the osdl layouts, order, snr_db, model result) of NATURAL[i], computed once and shared;
    ``quant``: the same frames quantised (osdx_pb_model.quantise)."""
    name, snr, order, F = NATURAL[i]
    G = osdl_model.graph(name)[1]
    y, cw = osdl_model.frames(name, snr, F, SEED)
    if quant:
        y = quantise(y)
    y = np.ascontiguousarray(y, dtype=F32)
    front = osdl_model.front_oracle(G, y)
    return y, cw, front, order, snr, pb(y, front[0], front[3], order, snr)


# quantised inputs: reliability sums tie massively.  s200_100: k = 100, WP = 2; wl384: k = 192, WP = 3.  (index into NATURAL, frames)
QUANTISED = ((3, 4), (0, 4))


# ---------------------------------------------------------------------------------------------------------------------
# 2: loud and quiet noiseless frames
# ---------------------------------------------------------------------------------------------------------------------
LOUD_AMP, QUIET_AMP, LOUD_SNR_DB = 6.0 / 3.1773, 0.02, 1.0
IN_TURN = ("wl384", (100, 200), (80, 150), (32, 128))       # the top tier and one code per lower tier (8064, 4096, 2048 slots)
TIER_FRAMES = ((65, 130), (92, 150), (128, 320))           # one order-3 frame just above each tier boundary: WP = 2, 1, 3


@functools.lru_cache(maxsize=None)
def in_turn(code, order, loud=2, quiet=2):
    """Noiseless codewords of ``code`` decoded with snr_db = 1: ``loud`` frames with |y| = 6.0 / 3.1773 (1 +- 1 %) and ``quiet``
    ones with |y| = 0.02.  The all-zero TEP costs 0.0, nothing improves on it and beta = 0.  Loud: at order 2 no rule stops the
    search, every TEP is visited; at order 3 the first weight-3 TEP stops it by rule 1, after all of the lighter ones, with
    (k-1)(k-2)/2 weight-3 runs live: every weight-3 slot k needs has been written.  Quiet: q ~ 1/2, the search stops at its
    first TEP.  -> (y, labels, front oracle, model)."""
    G = graph(code)[1]
    n = G.shape[1]
    rng = np.random.default_rng(3)
    msg = rng.integers(0, 2, (loud + quiet, G.shape[0]))
    cw = (msg @ G % 2).astype(np.uint8)
    amp = np.concatenate([LOUD_AMP * (1.0 + rng.uniform(-0.01, 0.01, (loud, n))), np.full((quiet, n), QUIET_AMP)]).astype(F32)
    y = np.ascontiguousarray(amp * (F32(1.0) - F32(2.0) * cw.astype(F32)), dtype=F32)
    front = osdl_model.front_oracle(G, y)
    return y, cw, front, pb(y, front[0], front[3], order, LOUD_SNR_DB)


# ---------------------------------------------------------------------------------------------------------------------
# 4: equal magnitudes on the MRB: the visit order is the insertion order
# ---------------------------------------------------------------------------------------------------------------------
EQUAL = ((100, 200, 2, 1, 2), (100, 200, 2, 2, 2), (150, 321, 2, 1, 1), (150, 321, 2, 2, 1), (70, 200, 3, 1, 1))   # (k, n, order, levels, frames)


def equal_magnitudes(k, n, order, levels, F, seed=11):
    """osdx_pb_model.equal_magnitudes_in in the osdl layouts."""
    return M.equal_magnitudes_in(OF.OSDL, k, n, order, levels, F, seed)
