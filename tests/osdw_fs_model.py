"""Test helper: the inputs of the FS-OSD and one-TEP tests of the high-rate family (ldpc_osdw_fs_search / _fs_decode /
_tep_eval).  The CPU oracle is tests/osdx_fs_model.py, which serves any k as it is; here are the codes, frames and parameter
sets, the front-end results in the osdw layouts (parity [F,128]), the wide variant of ``planted`` and two-word masks.
tests/test_osdw_fs_host.py asserts the coverage of these inputs without a GPU."""
import functools

import numpy as np

from tests import osdw_model, osdx_model
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
    """-> (winner spans, stopping-candidate spans): the set of span() values over the reference-quirk winners (rank > 0) and over
    the tau_e stopping candidates of every frame and parameter set of ``name``."""
    _, _, _, b, order, sets, _ = parity_case(name)
    win, stop = set(), set()
    for s in sets:
        for scan in b.scans:
            r = scan.fs(order, *s)
            if r["ref"][0]:
                win.add(span(r["ref"][0]))
            if r["hit"] is not None and r["hit"][0]:
                stop.add(span(r["hit"][0]))
    return win, stop


def split_masks(masks):
    """Python-int masks (bit p = flip MRB position p < 128) -> [F, 2] u64 in the layout of ldpc_osdw_tep_eval."""
    lo = [int(m) & ((1 << 64) - 1) for m in masks]
    hi = [(int(m) >> 64) & ((1 << 64) - 1) for m in masks]
    return np.array([lo, hi], dtype=np.uint64).T.copy()


@functools.lru_cache(maxsize=None)
def planted(k, n, which, seed=5):
    """osdx_fs_model.planted with the front-end results in the osdw layout (parity [1, 128] u64): a tau_e = 3.5 stop planted
    at a chosen rank of weight class 3 -- "first" (a rank of the first round of the class), "middle", or "last" (the last,
    partial round).  -> dict(y [1, n], perm [1, 128] u8, parity [1, 128] u64, batch, support, rank, params)."""
    m = n - k
    sup3 = M.class_supports(k, 3)
    cnt = len(sup3)
    assert cnt % 64, "the last round must be partial"
    rank = {"first": 37, "middle": (cnt // 128) * 64 + 21, "last": (cnt // 64) * 64 + (cnt % 64) // 2}[which]
    a, b, c = (int(x) for x in sup3[rank])
    rng = np.random.default_rng(seed)
    P = rng.integers(0, 2, (k, m), dtype=np.int64)
    Gp = np.concatenate([np.eye(k, dtype=np.int64), P], axis=1)
    u0 = rng.integers(0, 2, k, dtype=np.int64)
    hp = (u0.dot(P) + P[a] + P[b] + P[c]) % 2                 # d0 = (u0 . P') ^ hp = P'[a] ^ P'[b] ^ P'[c]
    mag = np.concatenate([np.linspace(0.5, 0.05, k), rng.uniform(0.6, 1.5, m)]).astype(F32)
    y = (np.where(np.concatenate([u0, hp]) == 1, -1.0, 1.0) * mag).astype(F32)[None, :]
    perm = np.zeros((1, 128), np.uint8)
    perm[0, :n] = np.arange(n)
    parity = np.zeros((1, 128), np.uint64)
    parity[0, :k] = osdx_model._pack_rows(P)
    return dict(y=y, perm=perm, parity=parity, batch=M.Batch(y, perm, [Gp]), support=(a, b, c), rank=rank,
                params=(3, 0.0, 3.5, 30.0))


PLANTED = [(k, n, which) for (k, n) in ((67, 100), (80, 121)) for which in ("first", "middle", "last")]


@functools.lru_cache(maxsize=None)
def planted_graph(k, n):
    """(H, G) of a code of shape (k, n) to hold the context of a planted case: H = [A | I], three ones per column of A (the
    search never reads G; the caller brings the front-end results)."""
    if (k, n) == (80, 121):
        return osdw_model.graph("array_121_80")
    from oracle import np_oracle
    rng = np.random.default_rng(5)
    m = n - k
    A = np.zeros((m, k), np.int64)
    for c in range(k):
        A[rng.choice(m, size=3, replace=False), c] = 1
    H = np.concatenate([A, np.eye(m, dtype=np.int64)], axis=1)
    G = np_oracle.generator_from_H(H)
    assert G.shape == (k, n)
    return H, G
