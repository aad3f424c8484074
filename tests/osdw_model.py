"""Test helper: the codes, frames and exchange classes of the high-rate OSD entry points (ldpc_osdw_*).

  codes          array_121_80 (tests/golden/), the zoo's deg65 (80,74), the k <= 64 cross-checks ccsds and array_121_60, and
                 four synthetic codes of osd_family.h_systematic (H = [A | I_m]): s128_65, s128_96, s128_124, s70_66
  front_oracle   osd_family.front_oracle bound to the osdw layouts (parity [F,128])
  scan oracle    osdx_model.scan_oracle takes a ``front`` tuple and uses only its perm and Gps: it serves any k as it is
"""
import functools
import os

import numpy as np

from oracle import np_oracle
from tests import nms_graphs, osdx_model
from tests import osd_family as OF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAY_121_80 = os.path.join(ROOT, "tests", "golden", "ArrayCode_N121_K80_r0.66.alist")
SYNTH = {"s128_65": (128, 65, 3), "s128_96": (128, 96, 3), "s128_124": (128, 124, 1), "s70_66": (70, 66, 2)}   # n, k, colw
SYNTH_MAX_CHECK_DEGREE = {"s128_65": 7, "s128_96": 17, "s128_124": 34, "s70_66": 39}
WIDE = ("array_121_80", "deg65") + tuple(SYNTH)          # the codes ldpc_osdx_* refuses (k > 64)
NARROW = ("ccsds", "array_121_60")                       # k <= 64: held to ldpc_osdx_* on the GPU
CODES = WIDE + NARROW


@functools.lru_cache(maxsize=None)
def _synthetic(name):
    """A synthetic code: osd_family.h_systematic with its column weight; the largest check degree is pinned."""
    n, k, colw = SYNTH[name]
    H, G = OF.h_systematic(n, k, colw)
    assert int(H.sum(axis=1).max()) == SYNTH_MAX_CHECK_DEGREE[name]
    return H, G


@functools.lru_cache(maxsize=None)
def graph(name):
    """-> (H, G) int64 of ``name``."""
    if name == "array_121_80":
        c = np_oracle.Code(ARRAY_121_80)
        return c.H, c.G
    if name in SYNTH:
        return _synthetic(name)
    return osdx_model.graph(name)


def make_code(name):
    from short_ldpc_decoding_osd_amd import Code
    if name == "array_121_80":
        return Code(ARRAY_121_80)
    if name in SYNTH:
        return Code(H=graph(name)[0])
    return Code() if name == "ccsds" else nms_graphs.make_code(name)


def frames(name, snr, B, seed):
    return np_oracle.make_frames(graph(name)[1], snr, B, np.random.default_rng(seed))


front_oracle = functools.partial(OF.front_oracle, fam=OF.OSDW)       # (G, y, swaps=False) -> perm [F,128] u8, parity [F,128] u64, ...


def exchange_classes(k, ns, sws):
    """The eight classes of the front-end premises: frames by their number of exchanges, recorded exchanges (a, b) by the
    word of the pivot step a and by where the partner b lies."""
    a = np.array([p[0] for s in sws for p in s], np.int64)
    b = np.array([p[1] for s in sws for p in s], np.int64)
    return {"frames_0": int((ns == 0).sum()), "frames_ge3": int((ns >= 3).sum()), "most": int(ns.max()),
            "a_lt64": int((a < 64).sum()), "a_ge64": int((a >= 64).sum()),
            "b_lt64": int((b < 64).sum()), "b_mid": int(((b >= 64) & (b < k)).sum()), "b_gek": int((b >= k).sum())}
