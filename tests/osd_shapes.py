"""Test helper: caller-made front-end results and structured codes for the any-shape (ldpc_osdx_*) and the high-rate
(ldpc_osdw_*) OSD entry points, at the shape edges no tested code has.  tests/osd_generators.py generalised from (128,64) to
(k, n): the same structures of P', the same magnitude modes, the same direct forms.

Shapes (k, n): BOTH are served by the two families, WIDE by ldpc_osdw_* only.  They hold n-k = 1, 8, 16, 17 (the edges of the
byte LUTs and of the two-byte metric prefix, the smallest argument of the colmask shift), k = 1 and 2, k = 64 away from
n = 128, k = 65 with a one-bit parity part, k = 127, and n = 64 and 65 (a codeword of one word exactly, or of two with one bit
in the second).

Structures of P' [k, n-k], seeded per (shape, structure):
  random_dense   the control
  zero_rows      first, middle and last row zero, where k >= 3
  equal_rows     rows 2i and 2i+1 equal
  ones_row       row 0 all ones, the second half of the rows the complements of the first (rows 1..)
  identity       P'[r][r mod (n-k)] = 1
  rank_one       every row zero or one fixed vector

Magnitude modes: ``float`` as drawn; ``grid`` |y| rounded to steps of 0.5 with a floor of 0.5 (osd_generators.to_grid);
``extreme`` the six finite extremes of test_gpu_osd_adversary._extremes at width n.

Pair forms (``pair``): ``sorted`` perm = identity and the frame's magnitudes laid descending along the n positions with the signs
kept (osd_generators.direct(sorted_y=True): the front end on [I | P'] is then the identity without an exchange); ``unsorted`` a
seeded random permutation per frame and y' as drawn -- defined for the conventional search and the one-TEP evaluation only (the FS
and PB loops of the reference assume the order).

Structured codes (``code``): H = [P'^T | I] with its columns permuted by a seeded pi, G = np_oracle.generator_from_H(H), with the
column structures zero_cols / equal_cols / rank_one / identity of P'.  G then has zero columns, repeated columns or a rank-one
parity part, which drives the front end through long chains of column exchanges.  P' is thinned for k > 64 so that no check has
more than 65 ones.
"""
import functools

import numpy as np

from oracle import np_oracle
from tests import osd_family as OF
from tests import osd_generators, osdw_model, osdx_model

F32 = np.float32
BOTH = ((1, 65), (2, 10), (5, 12), (33, 64), (48, 65), (64, 65), (64, 80))
WIDE = ((65, 66), (70, 87), (100, 108), (112, 128), (127, 128))
SHAPES = BOTH + WIDE
STRUCTURES = ("random_dense", "zero_rows", "equal_rows", "ones_row", "identity", "rank_one")
MODES = ("float", "grid")
FORMS = ("sorted", "unsorted")
SNRS = (1.0, 2.5, 4.0)
FRAMES = 12
MAX_CHECK_DEGREE = 65

CODE_SHAPES = ((33, 64), (64, 65), (70, 87), (96, 128), (100, 108), (127, 128))
CODE_STRUCTURES = ("zero_cols", "equal_cols", "rank_one", "identity")
CODE_FRAMES, CODE_SNR = 64, 1.0


def _seed(k, n, name, names):
    return 7000 + 1000 * names.index(name) + 131 * k + n


def _freeze(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


# --------------------------------------------------------------------------------------------------------- P' and the pairs
def zero_rows_of(k):
    """The rows zero_rows clears: first, middle and last, where k >= 3."""
    return (0, k // 2, k - 1) if k >= 3 else ()


@functools.lru_cache(maxsize=None)
def parity(k, n, name):
    """P' [k, n-k] int64 of the structure, as written."""
    m = n - k
    rng = np.random.default_rng(_seed(k, n, name, STRUCTURES))
    dense = rng.integers(0, 2, size=(k, m))
    if name == "random_dense":
        P = dense
    elif name == "zero_rows":
        P = dense
        P[list(zero_rows_of(k))] = 0
    elif name == "equal_rows":
        P = np.repeat(dense[:(k + 1) // 2], 2, axis=0)[:k]
    elif name == "ones_row":
        P = dense
        P[0] = 1
        h = k // 2
        j = max(0, min(h - 1, k - h))
        P[h:h + j] = 1 - P[1:1 + j]
    elif name == "identity":
        P = np.zeros((k, m), np.int64)
        P[np.arange(k), np.arange(k) % m] = 1
    elif name == "rank_one":
        v = rng.integers(0, 2, size=m)
        u = rng.integers(0, 2, size=k)
        v[0] = u[0] = 1
        P = np.outer(u, v)
    else:
        raise KeyError(name)
    P = np.array(P, dtype=np.int64)
    P.setflags(write=False)
    return P


def systematic(k, n, name):
    return np.concatenate([np.eye(k, dtype=np.int64), parity(k, n, name)], axis=1)


def to_grid(y):
    return osd_generators.to_grid(y)


def extremes(y, rng):
    """The six magnitude extremes of test_gpu_osd_adversary._extremes on frames y [F, n] -> [6 F, n]: the 1e-41 scale, equal
    magnitudes, +0.0 / -0.0 entries, clipped values with zeros, one 1e30 outlier per frame, the 2^60 scale.  Every |y| sum of a
    row is finite, in float32 too."""
    frames, n = y.shape
    out = [y * F32(1e-41), np.where(np.signbit(y), F32(-0.75), F32(0.75))]
    z = y.copy()
    m = rng.random(y.shape) < 0.15
    z[m] = np.where(rng.random(m.sum()) < 0.5, F32(0.0), F32(-0.0))
    out.append(z)
    c = np.clip(y, -1.0, 1.0)
    c[:, rng.choice(n, min(6, n // 2), replace=False)] = 0.0
    out.append(c)
    o = y.copy()
    o[np.arange(frames), rng.integers(0, n, frames)] = F32(1e30)
    out.append(o)
    out.append(y * F32(2.0 ** 60))
    y_all = np.concatenate(out).astype(F32)
    assert np.isfinite(np.abs(y_all.astype(np.float64)).sum(axis=1)).all()
    assert np.isfinite(np.abs(y_all).sum(axis=1, dtype=F32)).all()
    return y_all


def pack(P, rows):
    """[F, k, m] 0/1 -> parity [F, rows] u64 in the layout of ldpc_osdx_* (rows = 64) or ldpc_osdw_* (rows = 128): rows >= k and
    bits >= m zero."""
    F, k, _ = P.shape
    out = np.zeros((F, rows), np.uint64)
    for f in range(F):
        out[f, :k] = OF.pack_rows(P[f], 1)[:, 0]
    return out


def draw(k, n, name, mode, form="sorted", frames=FRAMES, seed=0):
    """The frames of a pair before any device layout (shared with tests/osdl_shapes.py) -> (G = [I | P'], y [F, n] in ORIGINAL
    bit order, cw = the labels in original order, p [F, n] int64 = original bit at primed position q, yp = y in primed order,
    cwp).  ``extreme`` draws frames // 6 frames at 2.0 dB and returns their six extremes."""
    assert form in FORMS and mode in MODES + ("extreme",)
    G = systematic(k, n, name)
    rng = np.random.default_rng(_seed(k, n, name, STRUCTURES) * 11 + seed + 3 * (MODES + ("extreme",)).index(mode)
                                + (100 if form == "sorted" else 0))
    if mode == "extreme":
        base, lab = np_oracle.make_frames(G, 2.0, max(1, frames // 6), rng)
        yp, cwp = extremes(base, rng), np.concatenate([lab] * 6)
    else:
        yp = np.empty((frames, n), F32)
        cwp = np.empty((frames, n), np.int64)
        for i, snr in enumerate(SNRS):
            cnt = len(range(i, frames, len(SNRS)))
            yp[i::len(SNRS)], cwp[i::len(SNRS)] = np_oracle.make_frames(G, snr, cnt, rng)
        if mode == "grid":
            yp = to_grid(yp)
    F = len(yp)
    p = np.empty((F, n), np.int64)
    if form == "sorted":
        mag = -np.sort(-np.abs(yp), axis=1)
        yp = np.where(np.signbit(yp), -mag, mag).astype(F32)
        p[:] = np.arange(n)
    else:
        for f in range(F):
            p[f] = rng.permutation(n)
    y = np.empty_like(yp)
    cw = np.empty_like(cwp)
    np.put_along_axis(y, p, yp, axis=1)                      # y[f, perm[f, q]] = y'[f, q]
    np.put_along_axis(cw, p, cwp, axis=1)
    return G, np.ascontiguousarray(y, dtype=F32), cw, p, np.ascontiguousarray(yp, dtype=F32), cwp


@functools.lru_cache(maxsize=None)
def pair(k, n, name, mode, form="sorted", frames=FRAMES, seed=0):
    """The (perm, P') pair as written, the same P' for every frame -> dict(k, n, name, mode, form, G = [I | P'], y [F, n] in
    ORIGINAL bit order, cw = the labels in original order, perm [F, 128] u8 (0 beyond n), parity64 [F, 64] u64 (None for k > 64),
    parity128 [F, 128] u64, Gps = [I | P'] per frame, yp = y in primed order).  Cached: shared, read-only.
    ``extreme`` draws frames // 6 frames at 2.0 dB and returns their six extremes."""
    G, y, cw, p, yp, cwp = draw(k, n, name, mode, form, frames, seed)
    F = len(y)
    perm = np.zeros((F, 128), np.uint8)
    perm[:, :n] = p
    P = np.tile(parity(k, n, name), (F, 1, 1))
    return _freeze(dict(k=k, n=n, name=name, mode=mode, form=form, G=G, y=y, cw=cw, perm=perm,
                        parity64=pack(P, 64) if k <= 64 else None, parity128=pack(P, 128), Gps=[G] * F, yp=yp, cwp=cwp))


def front_of(c):
    """The ``front`` tuple osdx_model.scan_oracle takes (it reads perm and Gps only)."""
    return (c["perm"], c["parity128"], None, c["Gps"])


def dirty(c):
    """The pair with non-zero padding: perm entries at or beyond n set to 0xEE, parity rows at or beyond k all ones, bits at or
    beyond n-k set.  -> (perm, parity64 or None, parity128); the search entry points ignore all of it."""
    k, n = c["k"], c["n"]
    perm = np.array(c["perm"])
    perm[:, n:] = 0xEE
    high = np.uint64(0) if n - k == 64 else ~np.uint64((1 << (n - k)) - 1)
    out = []
    for key in ("parity64", "parity128"):
        if c[key] is None:
            out.append(None)
            continue
        par = np.array(c[key]) | high
        par[:, k:] = ~np.uint64(0)
        out.append(par)
    assert (perm != c["perm"]).any() or n == 128
    assert (out[1] != c["parity128"]).any()
    return perm, out[0], out[1]


def tep_masks(c, rng):
    """Per frame one mask (a Python int, bit p = flip MRB position p) of each weight 0..4 (capped at k), one over the zero rows
    of P' only and one over a group of equal non-zero rows (0 where the pair has none), as _masks of
    tests/test_gpu_osd_generators.py: a list of 7 lists of F ints."""
    k, F = c["k"], len(c["y"])
    rows = [int.from_bytes(np.packbits(r.astype(np.uint8), bitorder="little").tobytes(), "little") for r in c["G"][:, k:]]
    zero = sum(1 << p for p in range(k) if rows[p] == 0)
    groups = {}
    for p, r in enumerate(rows):
        if r:
            groups.setdefault(r, []).append(p)
    groups = [g for g in groups.values() if len(g) > 1]
    out = [[] for _ in range(7)]
    for f in range(F):
        for wt in range(5):
            out[wt].append(sum(1 << int(p) for p in rng.choice(k, size=min(wt, k), replace=False)))
        out[5].append(zero)
        out[6].append(sum(1 << p for p in groups[rng.integers(len(groups))]) if groups else 0)
    return out


# ------------------------------------------------------------------------------------------------ FS and PB parameter sets
def fs_sets(k, n):
    """(beta, tau_e, tau_psc) per shape.  Every beta is a dyadic fraction, exact in float32, so osdx_fs_model.beta_term equals
    the reference's rounding of beta * (n-k) at every n-k (the host test asserts it).  tau_e scales with n-k as 4.5 does with 17
    at (70,87); the second set has a tau_psc just above tau_e so that cheaper candidates are refused, the third never stops
    on tau_e beyond the all-zero TEP."""
    m = n - k
    te = float(max(1, round(0.26 * m))) + 0.5
    return ((1.0 / 64, te, 30.0), (0.0, te, te + 2.0), (0.125, 0.5, 30.0))


def fs_order(k):
    return min(2, k)


PB_SNRS = (1.0, 2.5)


# ------------------------------------------------------------------------------------------------------ contexts and codes
def _thin_columns(rng, m, k, colw):
    """A [m, k]: column c gets up to ``colw`` ones, in rows that have fewer than MAX_CHECK_DEGREE - 1 ones so far."""
    A = np.zeros((m, k), np.int64)
    for c in range(k):
        free = np.flatnonzero(A.sum(axis=1) < MAX_CHECK_DEGREE - 1)
        A[rng.choice(free, size=min(len(free), colw), replace=False), c] = 1
    return A


@functools.lru_cache(maxsize=None)
def context_graph(k, n):
    """(H, G) of a plain code of shape (k, n) to hold the context of the pair cases: H = [A | I], three ones per column of A as
    osdw_fs_model.planted_graph, fewer where a check would pass 65 ones (the searches never read G)."""
    m = n - k
    A = _thin_columns(np.random.default_rng(5), m, k, 3)
    H = np.concatenate([A, np.eye(m, dtype=np.int64)], axis=1)
    G = np_oracle.generator_from_H(H)
    assert G.shape == (k, n) and int(H.sum(axis=1).max()) <= MAX_CHECK_DEGREE
    return H, G


@functools.lru_cache(maxsize=None)
def code_parity(k, n, name):
    """P' [k, n-k] of a structured code: random columns (density 1/2, or 1/4 for k > 64: no column passes 64 ones) with every
    third column zero (zero_cols), adjacent columns equal (equal_cols), u v^T (rank_one) or P'[r][r mod (n-k)] = 1 (identity)."""
    m = n - k
    rng = np.random.default_rng(_seed(k, n, name, CODE_STRUCTURES) + 50000)
    dens = 0.5 if k <= 64 else 0.25
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
        if k > 64 * m:                                       # (127,128): one check over every bit would have 128 ones
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
    pi = np.random.default_rng(_seed(k, n, name, CODE_STRUCTURES) + 60000).permutation(n)
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
    dict(H, G, y, cw, front = (perm [F,128], parity [F,128], nswaps, Gps, swaps), classes = osdw_model.exchange_classes)."""
    H, G, _ = code(k, n, name)
    rng = np.random.default_rng(_seed(k, n, name, CODE_STRUCTURES) + 70000 + (1 if mode == "grid" else 0))
    y, cw = np_oracle.make_frames(G, CODE_SNR, CODE_FRAMES, rng)
    if mode == "grid":
        y = to_grid(y)
    y = np.ascontiguousarray(y, dtype=F32)
    front = osdw_model.front_oracle(G, y, swaps=True)
    return dict(H=H, G=G, y=y, cw=cw, front=front, classes=osdw_model.exchange_classes(k, front[2], front[4]))
