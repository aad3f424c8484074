"""Test helper: the inputs of the FS-OSD and one-TEP tests of the long / low-rate family (ldpc_osdl_fs_search / _fs_decode /
_tep_eval).  The CPU oracle is tests/osdx_fs_model.py, which serves any (k, n) as it is; here are the codes, frames and
parameter sets and the awkward frames; ``planted`` and ``split_masks`` bind the shared constructions to the osdl layouts
(perm [F, 64 S] u16, parity [F, 64 W, Wp] u64, W-word masks).  tests/test_osdl_fs_host.py asserts the coverage of these inputs without a GPU."""
import functools

import numpy as np

from tests import osd_family as OF
from tests import osdl_model
from tests import osdx_fs_model as M

F32 = np.float32
SEED = 7

# code -> (snr, F, order, [(beta, tau_e, tau_psc), ...]) on osdl_model.frames(code, snr, F, 7)
PARITY = {
    "wl384": (2.0, 24, 2, [(0.1, 20.5, 192), (0.02, 42.5, 60), (0.02, 42.5, 192), (0.02, 46.5, 192)]),
    "s200_100": (1.0, 48, 2, [(0.1, 9.5, 60), (0.02, 20.5, 28), (0.02, 20.5, 100), (0.02, 23.5, 100)]),
    "s321_130": (1.0, 32, 2, [(0.1, 20.5, 191), (0.02, 44.5, 60), (0.02, 44.5, 191), (0.02, 50.5, 191)]),
    "s256_192": (3.0, 24, 2, [(0.1, 4.5, 64), (0.02, 9.5, 14), (0.02, 9.5, 64), (0.02, 11.5, 64)]),
    "s128_32": (0.0, 64, 3, [(0.1, 14.5, 96), (0.02, 24.5, 32), (0.02, 24.5, 96), (0.02, 27.5, 96)]),
}
EVERY_TAG = ("zero", "bound1", "bound2", "full", "hit1", "hit2", "hit_late", "psc_blocked", "hit_after_improvement")
# the tags each code's sets reach between them: all nine, but on s128_32 (order 3) bound3 and hit3 in place of bound2
TAGS = {name: EVERY_TAG for name in PARITY}
TAGS["s128_32"] = tuple(t for t in EVERY_TAG if t != "bound2") + ("bound3", "hit3")

TEP_EVAL_ONLY = {"s193_1": (0.0, 24)}                                           # k = 1: frames for the one-TEP test alone

# the awkward frames (osdl_model.awkward_frames) run at these orders and sets: a strict and a loose tau_e
AWKWARD = {"wl384": (1, [(0.1, 20.5, 192), (0.0, 60.5, 192)]), "s128_32": (2, [(0.1, 14.5, 96), (0.0, 40.5, 96)]),
           "s100_20": (3, [(0.1, 12.5, 80), (0.0, 30.5, 80)]), "s193_1": (1, [(0.1, 40.5, 192), (0.0, 90.5, 192)])}


@functools.lru_cache(maxsize=None)
def batch(name):
    """-> (y, labels, front oracle in the osdl layouts, Batch) of the parity frames of ``name`` (s193_1: of its one-TEP frames),
    computed once and shared."""
    snr, F = (PARITY.get(name) or TEP_EVAL_ONLY[name])[:2]
    G = osdl_model.graph(name)[1]
    y, cw = osdl_model.frames(name, snr, F, SEED)
    front = osdl_model.front_oracle(G, y)
    return y, cw, front, M.Batch(y, front[0], front[3])


@functools.lru_cache(maxsize=None)
def parity_case(name):
    """-> (y, labels, front, Batch, order, sets, [Batch.fs per set]) of test 1."""
    _, _, order, sets = PARITY[name]
    y, cw, front, b = batch(name)
    return y, cw, front, b, order, sets, [b.fs(order, *s) for s in sets]


@functools.lru_cache(maxsize=None)
def awkward_case(name):
    """-> (y, front, order, sets, [Batch.fs per set]) of the six awkward frames of ``name``.  (A saturated frame overflows its
    float32 sums to +inf on purpose: NumPy's warning about it is switched off.)"""
    order, sets = AWKWARD[name]
    y = osdl_model.awkward_frames(name)
    front = osdl_model.front_oracle(osdl_model.graph(name)[1], y)
    with np.errstate(over="ignore", invalid="ignore"):
        b = M.Batch(y, front[0], front[3])
        return y, front, order, sets, [b.fs(order, *s) for s in sets]


def span(support):
    """The MRB words (positions 64 w .. 64 w + 63) a non-empty support touches, ascending: (1,) lies wholly in word 1, (0, 1)
    across positions 63 / 64, (1, 2) across 127 / 128."""
    return tuple(sorted({int(p) >> 6 for p in support}))


def spans(name):
    """osdx_fs_model.spans over the parity case of ``name`` with this module's span()."""
    return M.spans(parity_case(name), span)


def split_masks(masks, W):
    """Python-int masks (bit p = flip MRB position p < 64 W) -> [F, W] u64 in the layout of ldpc_osdl_tep_eval."""
    return OF.OSDL.split_masks(masks, 64 * W)


# ---------------------------------------------------------------------------------------------------------------------
# a planted stop
# ---------------------------------------------------------------------------------------------------------------------
PLANTED_SHAPES = {3: ((40, 140), (70, 200)), 2: ((130, 321), (192, 384))}       # weight class -> (k, n)
PLANTED_TAU_E = M.PLANTED_TAU_E
PLANTED = [(k, n, w, which) for w in (3, 2) for (k, n) in PLANTED_SHAPES[w] for which in ("first", "middle", "last")]
# Beside those twelve, at (192,384): the support {63, 64}, once as the tau_e stop and once -- under a tau_e nothing meets -- as
# the winner of the full scan.  The natural frames of wl384 have no winner and no stopping candidate across positions 63 / 64
# and no stopping candidate wholly in word 0 (tests/test_osdl_fs_host.py); these two cases and (192,384) "last" supply them.
ACROSS = [(192, 384, 2, "across", 2.5), (192, 384, 2, "across", 0.5)]
PLANTED_CODE = {(130, 321): "s321_130", (192, 384): "wl384"}                    # the contexts of the planted cases


classes_before = M.classes_before


def planted(k, n, weight, which, tau_e=None, seed=5):
    """osdx_fs_model.planted_stop in the osdl layouts (perm [1, 64 S] u16, parity [1, 64 W, Wp] u64), tau_psc = n."""
    return M.planted_stop(OF.OSDL, k, n, weight, which, tau_e, seed=seed)


planted_graph = OF.shape_graph       # (k, n) -> (H, G) of the context of a planted case
