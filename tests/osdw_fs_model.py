"""Test helper: the inputs of the FS-OSD and one-TEP tests of the high-rate family (ldpc_osdw_fs_search / _fs_decode /
_tep_eval).  The CPU oracle is tests/osdx_fs_model.py, which serves any k as it is; here are the codes, frames and parameter
sets; ``planted`` and ``split_masks`` bind the shared constructions to the osdw layouts (parity [F,128], two-word masks).
tests/test_osdw_fs_host.py asserts the coverage of these inputs without a GPU."""
import functools

import numpy as np

from tests import osd_family as OF
from tests import osdw_model
from tests import osdx_fs_model as M

F32 = np.float32
FRAMES, SEED, ORDER = 96, 7, 2

# code -> (snr, [(beta, tau_e, tau_psc), ...]) on osdw_model.frames(code, snr, 96, 7) at order 2
PARITY = {
    "array_121_80": (2.0, [(0.1, 4.5, 30), (0.02, 8.5, 14), (0.02, 8.5, 30)]),
    "s128_96": (3.0, [(0.1, 3.5, 30), (0.02, 6.5, 12)]),
    "s128_65": (1.5, [(0.1, 6.5, 30), (0.02, 11, 18), (0.02, 11, 30)]),
    "deg65": (4.0, [(0.1, 1.5, 30), (0.0, 2.5, 4)]),         # n - k = 6: zero / bound1 / hit1 only
}
EVERY_TAG = ("zero", "bound1", "bound2", "full", "hit1", "hit2", "hit_late", "psc_blocked", "hit_after_improvement")
FULL_COVERAGE = ("array_121_80", "s128_96", "s128_65")       # the codes that reach every tag of EVERY_TAG
DEG65_TAGS = ("zero", "bound1", "hit1")


@functools.lru_cache(maxsize=None)
def batch(name, snr, F=FRAMES, seed=SEED):
    """-> (y, labels, front oracle in the osdw layouts, Batch), computed once and shared."""
    G = osdw_model.graph(name)[1]
    y, cw = osdw_model.frames(name, snr, F, seed)
    front = osdw_model.front_oracle(G, y)
    return y, cw, front, M.Batch(y, front[0], front[3])


@functools.lru_cache(maxsize=None)
def parity_case(name):
    """-> (y, labels, front, Batch, order, sets, [Batch.fs per set]) of test 1."""
    snr, sets = PARITY[name]
    y, cw, front, b = batch(name, snr)
    return y, cw, front, b, ORDER, sets, [b.fs(ORDER, *s) for s in sets]


def span(support):
    """Where a non-empty support lies against MRB position 64: "below", "above" or "across"."""
    lo, hi = min(support) < 64, max(support) >= 64
    return "across" if lo and hi else ("below" if lo else "above")


def spans(name):
    """osdx_fs_model.spans over the parity case of ``name`` with this module's span()."""
    return M.spans(parity_case(name), span)


def split_masks(masks):
    """Python-int masks (bit p = flip MRB position p < 128) -> [F, 2] u64 in the layout of ldpc_osdw_tep_eval."""
    return OF.OSDW.split_masks(masks, 128)


def planted(k, n, which, seed=5):
    """osdx_fs_model.planted_stop in class 3 (tau_e = 3.5, tau_psc = 30) in the osdw layouts: parity [1, 128] u64."""
    return M.planted_stop(OF.OSDW, k, n, 3, which, tau_psc=30.0, seed=seed)


PLANTED = [(k, n, which) for (k, n) in ((67, 100), (80, 121)) for which in ("first", "middle", "last")]


planted_graph = OF.shape_graph       # (k, n) -> (H, G) of the context of a planted case
