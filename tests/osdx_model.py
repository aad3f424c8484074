"""Test helper: CPU oracles of the any-shape OSD entry points (ldpc_osdx_*), in the device layouts.

  front_oracle   the C oracle's general orc_osd_front (oracle/ldpc_oracle.c), frame by frame
  scan_oracle    front_oracle + np_oracle.tep_matrix(k, order) + a cost that runs np_oracle._weighted_distance_k's exact
                 sequence of float32 additions, vectorised over the TEPs (loop over positions, arrays over candidates);
                 ``self_check`` shows it equal to np_oracle.convention_osd's costs bit for bit
"""
import functools
import os

import numpy as np

from oracle import c_oracle, np_oracle
from tests import nms_graphs

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


def _pack_rows(bits):
    """[r, c <= 64] 0/1 -> [r] uint64, bit c of row r."""
    bits = np.asarray(bits, dtype=np.uint8)
    pad = np.zeros((bits.shape[0], 64 - bits.shape[1]), np.uint8)
    return np.packbits(np.concatenate([bits, pad], axis=1), axis=1, bitorder="little").view(np.uint64)[:, 0]


def front_oracle(G, y):
    """-> (perm [F,128] u8, parity [F,64] u64, nswaps [F] i32, Gp list) in the layouts of ldpc_osdx_front: entries beyond n,
    rows beyond k and bits beyond n-k are zero."""
    G = np.asarray(G)
    k, n = G.shape
    y = np.asarray(y, dtype=np.float32)
    perm = np.zeros((len(y), 128), np.uint8)
    parity = np.zeros((len(y), 64), np.uint64)
    ns = np.zeros(len(y), np.int32)
    Gps = []
    for f, row in enumerate(y):
        p, Gp, sw = c_oracle.osd_front(G, row)
        assert np.array_equal(Gp[:, :k], np.eye(k, dtype=np.int32))
        perm[f, :n] = p
        parity[f, :k] = _pack_rows(Gp[:, k:])
        ns[f] = len(sw)
        Gps.append(Gp.astype(np.int64))
    return perm, parity, ns, Gps


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


def self_check(name, frames_=3, seed=5):
    """The vectorised cost against np_oracle.convention_osd on a few order-1 frames, bit for bit."""
    G = graph(name)[1]
    k, n = G.shape
    y, cw = frames(name, 1.5, frames_, seed)
    for row, lab in zip(y, cw):
        yp, labp, Gp, perm, _ = np_oracle.swapped_info(row, lab, G)
        ref = np_oracle.convention_osd(yp, labp, Gp, 1)
        cost, cand = scan_frame(yp, Gp, 1)
        assert np.array_equal(cost.view(np.uint32), ref["costs"].view(np.uint32))
        assert int(np.argmin(cost)) == ref["best_index"] and np.array_equal(cand[ref["best_index"]], ref["codeword"])
        p_c, Gp_c, _ = c_oracle.osd_front(G, row)               # the two front-end oracles agree on the shape
        assert np.array_equal(p_c, perm) and np.array_equal(Gp_c, Gp)
    return True
