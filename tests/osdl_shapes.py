"""Test helper: caller-made front-end results and structured codes for the long / low-rate OSD entry points (ldpc_osdl_*), at
the shape edges no tested code has.  tests/osd_shapes.py generalised to the osdl layouts (S = ceil(n/64), W = ceil(k/64),
Wp = ceil((n-k)/64): perm [F, 64 S] u16, parity [F, 64 W, Wp] u64): the same structures of P', the same magnitude modes, the
same pair forms, the same frames (osd_shapes.draw).

Shapes (k, n).  LONG: served by this family alone, each there for an edge of the templates (EDGES).  SHORT: osd_shapes.SHAPES
unchanged (k <= 127, n <= 128), which the older families serve as well: n-k = 1, 8, 16, 17 and k = 1, 2 through the FS and PB
kernels of this one.

Structured codes (``code``): H = [P'^T | I] with its columns permuted by a seeded pi, as osd_shapes.code, on six shapes up to
(192,384).  P' is thinned so that no check has more than 65 ones (MAX_CHECK_DEGREE, asserted).
"""
import functools

import numpy as np

from oracle import np_oracle
from tests import osd_shapes as S
from tests import osdl_fs_model, osdl_model

F32 = np.float32
EDGES = {
    (2, 194): "n-k = 192 with k = 2",
    (64, 129): "n-k = 65: one bit in parity word 1, n = 129",
    (65, 129): "one row in row word 1, n-k = 64 exactly",
    (63, 191): "n-k = 128 exactly",
    (128, 256): "k, n-k and n all on a word boundary",
    (129, 258): "one row in row word 2, one bit in parity word 2",
    (100, 257): "one position in slot 4, five slots routed to six",
    (192, 320): "one idle slot, n-k = 128",
    (192, 193): "W = 3, WP = 1, n-k = 1",
    (191, 383): "one below every limit of the family",
    (192, 384): "every limit of the family",
}
LONG = tuple(EDGES)
SHORT = S.SHAPES
STRUCTURES, MODES, FORMS, PB_SNRS = S.STRUCTURES, S.MODES, S.FORMS, S.PB_SNRS
LONG_FRAMES = 6
MAX_CHECK_DEGREE = S.MAX_CHECK_DEGREE

# osd_shapes.draw's ``seed`` of a LONG pair where it is not 0: chosen on the CPU so that the premises of
# tests/test_osdl_shapes_host.py hold (a winner whose discrepancy is zero in a whole word; two TEPs of equal minimal cost)
SEEDS = {(2, 194, "rank_one"): 34, (63, 191, "zero_rows"): 1974, (128, 256, "zero_rows"): 1592, (100, 257, "zero_rows"): 5697,
         (192, 320, "zero_rows"): 1333, (191, 383, "zero_rows"): 80949, (192, 384, "zero_rows"): 2658}

CODE_SHAPES = ((65, 129), (40, 200), (128, 256), (130, 321), (192, 193), (192, 384))
CODE_STRUCTURES = S.CODE_STRUCTURES
CODE_FRAMES, CODE_SNR = 24, 1.0

parity, extremes, to_grid, tep_masks, fs_sets, fs_order = S.parity, S.extremes, S.to_grid, S.tep_masks, S.fs_sets, S.fs_order


def layout(k, n):
    """-> (S, W, Wp)."""
    return (n + 63) // 64, (k + 63) // 64, (n - k + 63) // 64


def frames_of(k, n):
    return LONG_FRAMES if (k, n) in LONG else S.FRAMES


def conv_frames(k, order, F):
    """The frames of a pair the conventional scan runs on (the CPU scan dominates the time): order 3 only where k <= 64, on 2
    frames; order 2 on 2 frames where k >= 100 and on 1 where k >= 150; else all F."""
    if order == 3:
        return min(F, 2) if k <= 64 else 0
    return min(F, 1 if k >= 150 else 2) if (order == 2 and k >= 100) else F


def fs_pb_frames(k, F):
    """The frames of a sorted pair FS-OSD and PB-OSD run on: the first 2 where k >= 150 (their CPU models take up to 0.5 s per
    frame and call there), else all F."""
    return min(F, 2) if k >= 150 else F


def winner_discrepancy_words(c, r, f):
    """The words (64 parity positions each) of the discrepancy of frame f's winner in scan result r: its parity part against
    the hard decisions of y', in primed order."""
    k, n = c["k"], c["n"]
    bits = np.unpackbits(np.ascontiguousarray(r["cw"][f]).view(np.uint8), bitorder="little")[:n]
    p = c["perm"][f, :n].astype(np.int64)
    D = bits[p][k:] ^ (~(c["yp"][f, k:] > 0)).astype(np.uint8)
    return [D[q:q + 64] for q in range(0, n - k, 64)]


# --------------------------------------------------------------------------------------------------------------- the pairs
@functools.lru_cache(maxsize=None)
def pair(k, n, name, mode, form="sorted", frames=None):
    """osd_shapes.pair in the osdl layouts -> dict(k, n, name, mode, form, G = [I | P'], y [F, n] in ORIGINAL bit order, cw,
    perm [F, 64 S] u16 (0 beyond n), parity [F, 64 W, Wp] u64 (rows >= k and bits >= n-k zero), Gps, yp, cwp).  The frames are
    osd_shapes.draw's: on a SHORT shape the very frames of osd_shapes.pair; 6 frames on a LONG shape.  Cached: shared, read-only."""
    assert osdl_model.served(n, k)
    G, y, cw, p, yp, cwp = S.draw(k, n, name, mode, form, frames_of(k, n) if frames is None else frames, SEEDS.get((k, n, name), 0))
    F = len(y)
    one = osdl_model.pack_front(np.arange(n), G)[1]
    perm = np.zeros((F, 64 * layout(k, n)[0]), np.uint16)
    perm[:, :n] = p
    return S._freeze(dict(k=k, n=n, name=name, mode=mode, form=form, G=G, y=y, cw=cw, perm=perm,
                          parity=np.ascontiguousarray(np.tile(one, (F, 1, 1))), Gps=[G] * F, yp=yp, cwp=cwp))


def front_of(c):
    """The ``front`` tuple osdx_model.scan_oracle takes (it reads perm and Gps only)."""
    return (c["perm"], c["parity"], None, c["Gps"])


def has_padding(k, n):
    return bool(n % 64 or k % 64 or (n - k) % 64)


def dirty(c):
    """The pair with non-zero padding: perm entries at or beyond n set to 0xEEEE, parity rows from k to 64 W - 1 all ones, the
    bits at or beyond n-k set in every word of the live rows.  -> (perm, parity); the search entry points ignore all of it.
    (128,256), (192,320) and (192,384) have no padding of any kind: there, and only there, nothing changes.)"""
    k, n = c["k"], c["n"]
    m = n - k
    perm = np.array(c["perm"])
    perm[:, n:] = 0xEEEE
    par = np.array(c["parity"])
    for q in range(par.shape[2]):
        live = min(64, max(0, m - 64 * q))
        par[:, :k, q] |= np.uint64(((1 << 64) - 1) ^ ((1 << live) - 1))
    par[:, k:, :] = ~np.uint64(0)
    assert ((perm != c["perm"]).any() or (par != c["parity"]).any()) == has_padding(k, n)
    return perm, par


def equal_row_groups(k, n, name):
    """Whether P' has two equal non-zero rows: what tep_masks' last list flips.  (rank_one at (2,194) has one non-zero row.)"""
    rows = [r.tobytes() for r in parity(k, n, name) if r.any()]
    return len(set(rows)) < len(rows)


def split_masks(masks, k):
    return osdl_fs_model.split_masks(masks, (k + 63) // 64)


# ------------------------------------------------------------------------------------------------------ contexts and codes
def context_graph(k, n):
    """(H, G) of a plain H = [A | I] code of the shape for the pair cases, thinned as osd_shapes.context_graph thins it."""
    return S.context_graph(k, n)


@functools.lru_cache(maxsize=None)
def code_parity(k, n, name):
    """osd_shapes.code_parity with the density of the random columns lowered for long columns: 1/2 for k <= 64, else
    min(1/4, 24/k), so that a column of P' -- a check without its own bit -- stays far below 64 ones."""
    m = n - k
    rng = np.random.default_rng(S._seed(k, n, name, CODE_STRUCTURES) + 50000)
    dens = 0.5 if k <= 64 else min(0.25, 24.0 / k)
    dense = (rng.random((k, m)) < dens).astype(np.int64)
    if name == "zero_cols":
        P = dense
        P[:, ::3] = 0
    elif name == "equal_cols":
        P = np.repeat(dense[:, :(m + 1) // 2], 2, axis=1)[:, :m]
    elif name == "rank_one":
        u = (rng.random(k) < dens).astype(np.int64)
        v = rng.integers(0, 2, size=m)
        u[0] = v[0] = 1
        P = np.outer(u, v)
    elif name == "identity":
        P = np.zeros((k, m), np.int64)
        P[np.arange(k), np.arange(k) % m] = 1
        if k > 64 * m:                                       # (192,193): one check over every bit would have 193 ones
            P[64:] = 0
    else:
        raise KeyError(name)
    return np.array(P, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def code(k, n, name):
    """(H, G, pi) of a structured code: column j of [P'^T | I] lands at column pi[j] of H."""
    m = n - k
    P = code_parity(k, n, name)
    Hs = np.concatenate([P.T, np.eye(m, dtype=np.int64)], axis=1)
    pi = np.random.default_rng(S._seed(k, n, name, CODE_STRUCTURES) + 60000).permutation(n)
    H = np.empty_like(Hs)
    H[:, pi] = Hs
    G = np_oracle.generator_from_H(H)
    assert G.shape == (k, n) and int(H.sum(axis=1).max()) <= MAX_CHECK_DEGREE
    for a in (H, G, pi):
        a.setflags(write=False)
    return H, G, pi


@functools.lru_cache(maxsize=None)
def code_case(k, n, name, mode="float"):
    """CODE_FRAMES frames of the structured code at CODE_SNR dB and the front-end oracle with the recorded exchanges ->
    dict(H, G, y, cw, front = (perm [F, 64 S], parity [F, 64 W, Wp], nswaps, Gps, swaps), classes = osdl_model.exchange_classes)."""
    H, G, _ = code(k, n, name)
    rng = np.random.default_rng(S._seed(k, n, name, CODE_STRUCTURES) + 70000 + (1 if mode == "grid" else 0))
    y, cw = np_oracle.make_frames(G, CODE_SNR, CODE_FRAMES, rng)
    if mode == "grid":
        y = to_grid(y)
    y = np.ascontiguousarray(y, dtype=F32)
    front = osdl_model.front_oracle(G, y, swaps=True)
    return dict(H=H, G=G, y=y, cw=cw, front=front, classes=osdl_model.exchange_classes(k, layout(k, n)[0], front[2], front[4]))
