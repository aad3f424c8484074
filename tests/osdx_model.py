"""Test helper: the codes and frames of the any-shape OSD entry points (ldpc_osdx_*), and the scan oracle of every G-form
family.

  codes          ccsds and four members of tests/nms_graphs.py; frames; saturated_frames
  front_oracle   osd_family.front_oracle bound to the osdx layouts
  scan_oracle    a front_oracle result of any family + np_oracle.tep_matrix(k, order) + a cost that runs
                 np_oracle._weighted_distance_k's exact sequence of float32 additions, vectorised over the TEPs (loop over
                 positions, arrays over candidates); osd_family.self_check shows it equal to np_oracle.convention_osd's costs
                 bit for bit
"""
import functools
import os

import numpy as np

from oracle import c_oracle, np_oracle
from tests import nms_graphs
from tests import osd_family as OF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CCSDS = os.path.join(ROOT, "short_ldpc_decoding_osd_amd", "data", "CCSDS_ldpc_n128_k64.alist")
SMALL = ("ldpc_96_48", "array_121_60", "short", "thin")      # the four codes beside (128,64)
CODES = SMALL + ("ccsds",)


@functools.lru_cache(maxsize=None)
def graph(name):
    """-> (H, G) int64 of ``name``: a member of tests/nms_graphs.py, or "ccsds"."""
    if name == "ccsds":
        c = np_oracle.Code(CCSDS)
        return c.H, c.G
    return nms_graphs.graph(name)


def make_code(name):
    from short_ldpc_decoding_osd_amd import Code
    return Code() if name == "ccsds" else nms_graphs.make_code(name)


def frames(name, snr, B, seed):
    return np_oracle.make_frames(graph(name)[1], snr, B, np.random.default_rng(seed))


def saturated_frames(G):
    """Two frames with every |y| = 3.0e38 and signs no codeword has: any two disagreements overflow the metric to +inf."""
    s = np.random.default_rng(38).integers(0, 2, (2, np.asarray(G).shape[1]))
    return np.where(s, -3.0e38, 3.0e38).astype(np.float32)


front_oracle = functools.partial(OF.front_oracle, fam=OF.OSDX)       # (G, y) -> perm [F,128] u8, parity [F,64] u64, nswaps, Gp list


@functools.lru_cache(maxsize=None)
def tep_matrix(k, order):
    return np_oracle.tep_matrix(k, order)


def costs_vectorised(disc, w, k):
    """np_oracle._weighted_distance_k for every row of ``disc`` [T, n] at once: the same float32 additions in the same order
    (a row that does not flip position p keeps its sum untouched, exactly as the scalar loop skips the addition)."""
    disc = np.asarray(disc).astype(bool)
    w = np.asarray(w, dtype=np.float32)
    n = w.shape[0]
    acc = np.zeros(disc.shape[0], np.float32)
    for p in range(k):
        acc = np.where(disc[:, p], acc + w[p], acc)
    p = k
    while p < n:
        part = np.zeros(disc.shape[0], np.float32)
        for q in range(p, min(p + 8, n)):
            part = np.where(disc[:, q], part + w[q], part)
        acc = acc + part
        p += 8
    assert acc.dtype == np.float32
    return acc


def scan_frame(yp, Gp, order):
    """One frame in the primed domain -> (costs [T] f32, candidates [T, n])."""
    yp = np.asarray(yp, dtype=np.float32)
    k, n = Gp.shape
    hard = np.where(yp > 0, 0, 1).astype(np.int64)
    cand = ((tep_matrix(k, order) + hard[None, :k]) % 2).dot(Gp) % 2
    disc = (cand + hard[None, :]) % 2
    return costs_vectorised(disc, np.abs(yp), k), cand


def scan_oracle(G, y, order, front=None):
    """-> dict(cw [F, words] u64 original bit order, metric [F] f32, best [F] i32, ntep [F] i32, ties [F]: TEPs that share
    the minimum, weight [F]: flips of the winner) -- the outputs of ldpc_osdx_search / ldpc_osdx_decode."""
    G = np.asarray(G)
    k, n = G.shape
    y = np.asarray(y, dtype=np.float32)
    perm, _, _, Gps = front if front is not None else front_oracle(G, y)
    E = tep_matrix(k, order)
    F = len(y)
    bits = np.zeros((F, n), np.uint8)
    out = dict(metric=np.zeros(F, np.float32), best=np.zeros(F, np.int32), ntep=np.full(F, len(E), np.int32),
               ties=np.zeros(F, np.int64), weight=np.zeros(F, np.int64))
    for f in range(F):
        p = perm[f, :n].astype(np.int64)
        cost, cand = scan_frame(y[f][p], Gps[f], order)
        b = int(np.argmin(cost))                               # the first minimum
        out["metric"][f], out["best"][f] = cost[b], b
        out["ties"][f] = int(np.count_nonzero(cost == cost[b]))
        out["weight"][f] = int(E[b].sum())
        bits[f, p] = cand[b]
    pad = np.zeros((F, (-n) % 64), np.uint8)
    out["cw"] = np.packbits(np.concatenate([bits, pad], axis=1), axis=1, bitorder="little").view(np.uint64)
    return out
