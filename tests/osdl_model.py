"""Test helper: the codes, frames and constructed inputs of the long / low-rate OSD entry points (ldpc_osdl_*: n <= 384,
1 <= k <= 192, 1 <= n-k <= 192).

  codes          wl384: the reference's wimax-like (384,192) code (tests/golden/); six synthetic codes of
                 osd_family.h_systematic (H = [A | I_m]); the cross-checks ccsds, ldpc_96_48, array_121_80 and s128_96, which
                 ldpc_osdx_* or ldpc_osdw_* serve as well; four refused shapes.  make_code / graph resolve every name of the
                 three families' model modules
  layouts        S = ceil(n/64), W = ceil(k/64), Wp = ceil((n-k)/64): perm [F, 64 S] u16, parity [F, 64 W, Wp] u64
                 (osd_family.OSDL; pack_front / unpack_front / front_oracle are its bindings)
  scan oracle    osdx_model.scan_oracle takes a ``front`` tuple and uses only its perm and Gps: it serves any shape as it is
  constructed    reliability orders that make the front end take the paths natural frames leave out (premises: test_osdl_host)
"""
import functools
import os

import numpy as np

from oracle import c_oracle, np_oracle
from tests import nms_graphs, osd_adversary, osdw_model, osdx_model
from tests import osd_family as OF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WL384 = os.path.join(ROOT, "tests", "golden", "wimaxlike_N384_K192_P16_set0.alist")
SYNTH = {"s128_32": (128, 32), "s100_20": (100, 20), "s200_100": (200, 100), "s321_130": (321, 130), "s193_1": (193, 1),
         "s256_192": (256, 192)}                                            # n, k; column weight 3
CROSS = ("ccsds", "ldpc_96_48", "array_121_80", "s128_96")                  # served by ldpc_osdx_* or ldpc_osdw_* as well
REFUSED = {"s385_193": (385, 193), "s384_193": (384, 193), "s384_191": (384, 191)}   # beside wimax_1056: one limit each
NEW = ("wl384",) + tuple(SYNTH)                                             # the codes every other OSD family refuses
SERVED = NEW + CROSS
LIMITS = (384, 192, 192)                                                    # n, k, n - k


@functools.lru_cache(maxsize=None)
def graph(name):
    """-> (H, G) int64 of ``name``."""
    if name == "wl384":
        c = np_oracle.Code(WL384)
        return c.H, c.G
    if name in SYNTH or name in REFUSED:
        n, k = (SYNTH.get(name) or REFUSED[name])
        return OF.h_systematic(n, k)
    if name == "wimax_1056":
        return nms_graphs.graph(name)
    return osdw_model.graph(name) if name in osdw_model.CODES else osdx_model.graph(name)


def make_code(name):
    from short_ldpc_decoding_osd_amd import Code
    if name == "wl384":
        return Code(WL384)
    if name in SYNTH or name in REFUSED:
        return Code(H=graph(name)[0])
    if name == "wimax_1056":
        return nms_graphs.make_code(name)
    return osdw_model.make_code(name) if name in osdw_model.CODES else osdx_model.make_code(name)


def shape(name):
    """-> (n, k, S, W, Wp)."""
    k, n = graph(name)[1].shape
    return n, k, (n + 63) // 64, (k + 63) // 64, (n - k + 63) // 64


def served(n, k):
    return n <= LIMITS[0] and 1 <= k <= LIMITS[1] and 1 <= n - k <= LIMITS[2]


def frames(name, snr, B, seed):
    return np_oracle.make_frames(graph(name)[1], snr, B, np.random.default_rng(seed))


# ------------------------------------------------------------------------------------------------ layouts
pack_rows, unpack_rows = OF.pack_rows, OF.unpack_rows
pack_front, unpack_front = OF.OSDL.pack_front, OF.OSDL.unpack_front
front_oracle = functools.partial(OF.front_oracle, fam=OF.OSDL)       # (G, y, swaps=False) -> perm [F, 64 S] u16, parity [F, 64 W, Wp] u64, ...


def scan_oracle(G, y, order, front):
    """osdx_model.scan_oracle on a front_oracle result (it reads perm[f, :n] and the Gp list).  (A saturated frame overflows
    its float32 sums to +inf on purpose: NumPy's warning about it is switched off.)"""
    with np.errstate(over="ignore"):
        return osdx_model.scan_oracle(G, y, order, front[:4])


# ------------------------------------------------------------------------------------------------ inputs
def awkward_frames(name):
    """Six frames no channel draws: all |y| equal (twice: signs of a natural frame, and all +1), zeros in half of the
    positions and in all of them (a zero is a hard 1 and ties with every other zero), every |y| = 3.0e38 (any two
    discrepancies overflow the metric to +inf) and 3.0e38 at a few positions of a natural frame."""
    G = graph(name)[1]
    n = G.shape[1]
    y, _ = np_oracle.make_frames(G, 2.5, 6, np.random.default_rng(12))
    y[0] = np.where(y[0] < 0, -1.0, 1.0)
    y[1] = 1.0
    y[2, ::2] = 0.0
    y[3] = 0.0
    y[4] = np.where(y[4] < 0, -3.0e38, 3.0e38)
    y[5, [0, n // 2, n - 1]] = (3.0e38, -3.0e38, 3.0e38)
    return y.astype(np.float32)


def _col_ints(G):
    return osd_adversary._col_masks(G)


def dependent_at(name, y, step, seed):
    """Frame y re-laid so that the support of a row of H -- a dependent set of columns of G -- ends at sorted position
    ``step``: the column there lies in the span of the ones before it, so the elimination finds no pivot at that step (or at
    an earlier one of the set) and exchanges.  Every other position keeps its place in y's own reliability order."""
    H, G = graph(name)
    rng = np.random.default_rng(seed)
    sup = np.flatnonzero(H[int(rng.integers(H.shape[0]))])
    natural = [int(c) for c in np.argsort(-np.abs(y), kind="stable") if c not in set(sup.tolist())]
    head = step + 1 - len(sup)
    assert head >= 0
    order = natural[:head] + [int(c) for c in rng.permutation(sup)] + natural[head:]
    return osd_adversary.frame_along(order, y, True)


def last_step_partner(name, y, b):
    """Frame y re-laid so that step k-1 exchanges with the column at sorted position b > k-1.  v: a row of G of the least
    weight; positions 0..k-2 hold k-1 independent columns outside the support of v, so logical row k-1 is then v itself (the
    only codeword that vanishes there); positions k-1..b-1 hold columns outside the support -- no pivot, no partner --
    and the support of v starts at b.  None when the code has no such arrangement for b."""
    G = graph(name)[1]
    k, n = G.shape
    cols = _col_ints(G)
    v = G[int(np.argmin(G.sum(axis=1)))]
    sup = set(np.flatnonzero(v).tolist())
    span, basis, rest = osd_adversary._Span(), [], []
    for c in np.argsort(-np.abs(y), kind="stable"):
        c = int(c)
        if c in sup:
            continue
        (basis if len(basis) < k - 1 and span.add(cols[c]) else rest).append(c)
    if len(basis) != k - 1 or b < k or b - (k - 1) > len(rest) or b + len(sup) > n:
        return None
    gap = b - (k - 1)
    order = basis + rest[:gap] + sorted(sup) + rest[gap:]
    return osd_adversary.frame_along(order, y, True)


def no_exchange(name, y):
    """Frame y re-laid along its own primed order (the MRB first): the elimination then finds every pivot in place."""
    perm, _, _ = c_oracle.osd_front(graph(name)[1], y)
    return osd_adversary.frame_along([int(c) for c in perm], y, True)


@functools.lru_cache(maxsize=None)
def constructed_frames(name):
    """The constructed reliability orders of ``name`` (wl384, s321_130): a dependent set ending in each row word, the last
    pivot step exchanging with a partner in each later slot, and a frame without an exchange."""
    n, k, S, W, _ = shape(name)
    y, _ = frames(name, 2.0, 16, 3)
    out = [no_exchange(name, y[0])]
    for w in range(W):                                              # a pivot step without a pivot in every row word
        for t, step in enumerate((64 * w + 9, min(64 * w + 40, k - 1), min(64 * w + 63, k - 1))):
            if step < k:
                out.append(dependent_at(name, y[1 + t], step, 100 * w + t))
    for s in range((k - 1) // 64, S):                               # the last step's partner in every slot from its own on
        for b in (max(64 * s, k), 64 * s + 31, min(64 * s + 63, n - 1)):
            fr = last_step_partner(name, y[8 + s], b) if b >= k else None
            if fr is not None:
                out.append(fr)
    return np.stack(out).astype(np.float32)


def exchange_classes(k, S, ns, sws):
    """What the recorded exchanges (a, b) of a set of frames cover: the row words of the pivot steps a, the slots of the
    partners b, the (word, slot) pairs, and the frames by their number of exchanges."""
    a = np.array([p[0] for s in sws for p in s], np.int64)
    b = np.array([p[1] for s in sws for p in s], np.int64)
    return {"words": sorted(set((a >> 6).tolist())), "slots": sorted(set((b >> 6).tolist())),
            "pairs": sorted(set(zip((a >> 6).tolist(), (b >> 6).tolist()))),
            "frames_0": int((ns == 0).sum()), "frames_ge3": int((ns >= 3).sum()), "most": int(ns.max())}


@functools.lru_cache(maxsize=None)
def front_case(name):
    """The front-end frames of ``name`` and their oracle with the recorded exchanges (computed once): wl384 -- 48 natural
    frames at 2.0 dB, seed 1, and the constructed ones; s321_130 -- 32 frames at 1.5 dB and the constructed ones; every other
    code -- 32 frames at 1.5 dB; then the awkward frames."""
    G = graph(name)[1]
    y = frames(name, 2.0, 48, 1)[0] if name == "wl384" else frames(name, 1.5, 32, 1)[0]
    parts = [y] + ([constructed_frames(name)] if name in ("wl384", "s321_130") else []) + [awkward_frames(name)]
    y = np.concatenate(parts).astype(np.float32)
    return y, front_oracle(G, y, swaps=True)
