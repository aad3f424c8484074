"""Test helper: the codes and the CPU oracles of the high-rate OSD entry points (ldpc_osdw_*), in the device layouts.

  codes          array_121_80 (tests/golden/), the zoo's deg65 (80,74), the k <= 64 cross-checks ccsds and array_121_60, and
                 four synthetic codes from H = [A | I_m] with seeded random columns of A: s128_65, s128_96, s128_124, s70_66
  front_oracle   osdx_model.front_oracle with parity [F,128]: the C oracle's general orc_osd_front, frame by frame
  scan oracle    osdx_model.scan_oracle takes a ``front`` tuple and uses only its perm and Gps: it serves any k as it is
"""
import functools
import os

import numpy as np

from oracle import c_oracle, np_oracle
from tests import nms_graphs, osdx_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARRAY_121_80 = os.path.join(ROOT, "tests", "golden", "ArrayCode_N121_K80_r0.66.alist")
SYNTH = {"s128_65": (128, 65, 3), "s128_96": (128, 96, 3), "s128_124": (128, 124, 1), "s70_66": (70, 66, 2)}   # n, k, colw
SYNTH_MAX_CHECK_DEGREE = {"s128_65": 7, "s128_96": 17, "s128_124": 34, "s70_66": 39}
WIDE = ("array_121_80", "deg65") + tuple(SYNTH)          # the codes ldpc_osdx_* refuses (k > 64)
NARROW = ("ccsds", "array_121_60")                       # k <= 64: held to ldpc_osdx_* on the GPU
CODES = WIDE + NARROW


@functools.lru_cache(maxsize=None)
def _synthetic():
    """The four synthetic codes, each from default_rng(5): H = [A | I_m], column c of A gets min(m, colw) ones."""
    out = {}
    for name, (n, k, colw) in SYNTH.items():
        rng = np.random.default_rng(5)
        m = n - k
        A = np.zeros((m, k), np.int64)
        for c in range(k):
            A[rng.choice(m, size=min(m, colw), replace=False), c] = 1
        H = np.concatenate([A, np.eye(m, dtype=np.int64)], axis=1)
        G = np_oracle.generator_from_H(H)
        assert G.shape == (k, n) and int(H.sum(axis=1).max()) == SYNTH_MAX_CHECK_DEGREE[name]
        out[name] = (H, G)
    return out


@functools.lru_cache(maxsize=None)
def graph(name):
    """-> (H, G) int64 of ``name``."""
    if name == "array_121_80":
        c = np_oracle.Code(ARRAY_121_80)
        return c.H, c.G
    if name in SYNTH:
        return _synthetic()[name]
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


def front_oracle(G, y, swaps=False):
    """-> (perm [F,128] u8, parity [F,128] u64, nswaps [F] i32, Gp list) in the layouts of ldpc_osdw_front: entries beyond n,
    rows beyond k and bits beyond n-k are zero.  ``swaps``: a fifth member, the recorded exchanges [(a, b), ...] per frame."""
    G = np.asarray(G)
    k, n = G.shape
    y = np.asarray(y, dtype=np.float32)
    perm = np.zeros((len(y), 128), np.uint8)
    parity = np.zeros((len(y), 128), np.uint64)
    ns = np.zeros(len(y), np.int32)
    Gps, sws = [], []
    for f, row in enumerate(y):
        p, Gp, sw = c_oracle.osd_front(G, row)
        assert np.array_equal(Gp[:, :k], np.eye(k, dtype=np.int32))
        perm[f, :n] = p
        parity[f, :k] = osdx_model._pack_rows(Gp[:, k:])
        ns[f] = len(sw)
        Gps.append(Gp.astype(np.int64))
        sws.append(list(sw))
    return (perm, parity, ns, Gps, sws) if swaps else (perm, parity, ns, Gps)


def exchange_classes(k, ns, sws):
    """The eight classes of the front-end premises: frames by their number of exchanges, recorded exchanges (a, b) by the
    word of the pivot step a and by where the partner b lies."""
    a = np.array([p[0] for s in sws for p in s], np.int64)
    b = np.array([p[1] for s in sws for p in s], np.int64)
    return {"frames_0": int((ns == 0).sum()), "frames_ge3": int((ns >= 3).sum()), "most": int(ns.max()),
            "a_lt64": int((a < 64).sum()), "a_ge64": int((a >= 64).sum()),
            "b_lt64": int((b < 64).sum()), "b_mid": int(((b >= 64) & (b < k)).sum()), "b_gek": int((b >= k).sum())}


def self_check(name, frames_=3, seed=5):
    """osdx_model.self_check on a wide code: the two front-end oracles agree and the vectorised scan costs equal
    np_oracle.convention_osd's, bit for bit."""
    G = graph(name)[1]
    y, cw = frames(name, 1.5, frames_, seed)
    for row, lab in zip(y, cw):
        yp, labp, Gp, perm, _ = np_oracle.swapped_info(row, lab, G)
        ref = np_oracle.convention_osd(yp, labp, Gp, 1)
        cost, cand = osdx_model.scan_frame(yp, Gp, 1)
        assert np.array_equal(cost.view(np.uint32), ref["costs"].view(np.uint32))
        assert int(np.argmin(cost)) == ref["best_index"] and np.array_equal(cand[ref["best_index"]], ref["codeword"])
        p_c, Gp_c, _ = c_oracle.osd_front(G, row)
        assert np.array_equal(p_c, perm) and np.array_equal(Gp_c, Gp)
    return True
