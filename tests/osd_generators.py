"""Test helper: a seeded zoo of 64 x 128 generators for the (128,64) OSD search kernels, whose reduced forms [I | P'] have
the structure no CCSDS frame produces -- equal rows, zero rows, an all-ones row, sparse rows, all weight inside or outside
the two parity bytes the metric prefix reads.  The search entry points (ldpc_osd_search, ldpc_osd_tep_eval) take any
(perm, P') pair and never look at the context's own generator, so the pairs made here go to a CCSDS Decoder.

Each case is G = [I | P'][:, pi^-1] (column j of [I | P'] lands at column pi[j] of G), P' by the case, pi seeded:

  random_dense   the control: dense random rows, as CCSDS
  zero_rows      8 rows of P' zero (weight-1 codewords: their columns always pivot, the rows stay zero in every P'')
  equal_rows     28 pairs of equal rows and one group of 8 equal rows (two TEPs, one discrepancy)
  ones_row       row 0 all ones, rows 32..62 the complements of rows 1..31
  identity       P' = I: a TEP of weight w flips exactly w parity bits
  sparse         row weights 1..3
  low_bytes      all weight in parity columns 0..15 (the bytes tep_cost_bounded and stage 1 of the rotation scan read)
  high_bytes     all weight in parity columns 16..63 (the six bytes they skip)
  rank_one       every row zero or one fixed vector

The C oracle's front end on (G, y) returns (perm, [I | P'']); P'' is the P' above only when no column exchange happened, so
every premise the tests state is computed here from the returned P'' and the primed values, never from a device result.

low_bytes / high_bytes have 48 / 16 all-zero columns in G.  A zero column never pivots, so it always ends in the parity
half, at the rank its reliability gives it there.  For the prefix premises the frames of these two cases are re-laid: the
sorted magnitudes of the frame are dealt so that the zero columns are the least (low_bytes) or the most (high_bytes) reliable
positions, positive (their code bit is always 0); pi puts them at the highest / lowest column numbers, so a magnitude tie
at the border sorts the same way.  All other positions keep their sign and their relative order.

Magnitude modes: ``float`` = as drawn, ``grid`` = |y| rounded to multiples of 1/GRID_Q with a floor of one step (equal
discrepancies then also mean equal metrics).  Frames: equal shares at SNRS dB.

``direct(name, ...)``: the (perm, P') pair as written, perm = identity and y already primed.  sorted: the frame's
magnitudes laid in descending order along the 128 positions (each position keeps its sign), so the front end on [I | P']
is the identity with no exchange; unsorted: as drawn -- defined for the conventional search and ldpc_osd_tep_eval only.
"""
import functools

import numpy as np

from oracle import c_oracle, np_oracle

F32 = np.float32
NAMES = ("random_dense", "zero_rows", "equal_rows", "ones_row", "identity", "sparse", "low_bytes", "high_bytes", "rank_one")
MODES = ("float", "grid")
SNRS = (1.0, 2.5, 4.0)
GRID_Q = 2.0                        # grid mode: |y| in steps of 0.5, floor 0.5
# zero_rows, grid: a TEP on a zero row costs the order-0 metric plus its own |y'| > 0, so it never ties for the minimum; the
# ties come from unrelated rows, and are frequent only where the metric is a multiple of the Hamming distance (one step of 4
# = the floor, so nearly every |y| is 4) and the order-0 candidate is poor (low SNR).  The price: in this mode of this case
# FS-OSD never meets a tau_e hit and PB-OSD never stops (every frame visits all its TEPs, every reliability sum ties) --
# the deepest run of the PB tie rules, and no stop coverage; zero_rows gets its FS hits and PB stops from the float mode.
GRID_Q_OF = {"zero_rows": 0.25}
SNRS_OF = {("zero_rows", "grid"): (-6.0, -3.0, 0.0)}
SEED_OF = {("zero_rows", "grid"): 6}     # 26 of 96 frames tie at the order-1 minimum (seeds 0..7: 18..26)
ZERO_ROWS = (0, 1, 2, 31, 32, 61, 62, 63)
EQUAL_GROUP = tuple(range(56, 64))  # equal_rows: rows 2i, 2i+1 equal for i < 28, rows 56..63 all equal
RANK_ONE_SEED, CASE_SEED = 9100, 9200
DIRECT = (("equal_rows", "grid"), ("zero_rows", "grid"), ("identity", "float"), ("rank_one", "grid"))   # cases with a direct form


def _seed(name):
    return CASE_SEED + NAMES.index(name)


@functools.lru_cache(maxsize=None)
def parity(name):
    """P' [64, 64] int64 of the case, as written."""
    rng = np.random.default_rng(_seed(name))
    dense = rng.integers(0, 2, size=(64, 64))
    if name == "random_dense":
        P = dense
    elif name == "zero_rows":
        P = dense
        P[list(ZERO_ROWS)] = 0
    elif name == "equal_rows":
        P = np.repeat(dense[:32], 2, axis=0)
        P[list(EQUAL_GROUP)] = dense[40]
    elif name == "ones_row":
        P = dense
        P[0] = 1
        P[32:63] = 1 - P[1:32]
    elif name == "identity":
        P = np.eye(64, dtype=np.int64)
    elif name == "sparse":
        P = np.zeros((64, 64), np.int64)
        for r in range(64):
            P[r, rng.choice(64, size=1 + r % 3, replace=False)] = 1
    elif name == "low_bytes":
        P = dense
        P[:, 16:] = 0
    elif name == "high_bytes":
        P = dense
        P[:, :16] = 0
    elif name == "rank_one":
        v = np.random.default_rng(RANK_ONE_SEED).integers(0, 2, size=64)
        P = np.outer(rng.integers(0, 2, size=64), v)
    else:
        raise KeyError(name)
    P = np.asarray(P, dtype=np.int64)
    P.setflags(write=False)
    return P


def systematic(name):
    return np.concatenate([np.eye(64, dtype=np.int64), parity(name)], axis=1)


def zero_columns(name):
    """Columns of [I | P'] that are all zero (only low_bytes / high_bytes have any, by construction)."""
    return np.flatnonzero(~systematic(name).any(axis=0))


@functools.lru_cache(maxsize=None)
def pi(name):
    """Column j of [I | P'] lands at column pi[j] of G.  identity: the identity (G is [I | I] as written); low_bytes /
    high_bytes: the zero columns at the highest / lowest column numbers; seeded random elsewhere."""
    rng = np.random.default_rng(_seed(name) + 500)
    if name == "identity":
        return np.arange(128)
    z = zero_columns(name) if name in ("low_bytes", "high_bytes") else np.zeros(0, np.int64)
    rest = np.setdiff1d(np.arange(128), z)
    out = np.empty(128, np.int64)
    if name == "high_bytes":
        out[z] = rng.permutation(len(z))
        out[rest] = len(z) + rng.permutation(len(rest))
    else:
        out[rest] = rng.permutation(len(rest))
        out[z] = len(rest) + rng.permutation(len(z))
    return out


@functools.lru_cache(maxsize=None)
def generator(name):
    G = np.empty((64, 128), np.int64)
    G[:, pi(name)] = systematic(name)
    G.setflags(write=False)
    return G


def grid_q(name):
    return GRID_Q_OF.get(name, GRID_Q)


def to_grid(y, q=GRID_Q):
    mag = np.maximum(np.round(np.abs(y) * F32(q)) / F32(q), F32(1.0 / q))
    return np.where(np.signbit(y), -mag, mag).astype(F32)


def _relay(y, zero_at, zeros_last):
    """Deal the frame's sorted magnitudes so that the positions ``zero_at`` are its least (zeros_last) or most reliable
    ones and positive; inside each of the two groups the positions keep their relative order and, outside zero_at, their
    sign."""
    out = np.empty_like(y)
    rest = np.setdiff1d(np.arange(y.shape[1]), zero_at)
    for f, row in enumerate(y):
        m = np.sort(np.abs(row))[::-1]
        mz, mr = (m[len(rest):], m[:len(rest)]) if zeros_last else (m[:len(zero_at)], m[len(zero_at):])
        rz = np.argsort(-np.abs(row[zero_at]), kind="stable")
        rr = np.argsort(-np.abs(row[rest]), kind="stable")
        out[f, zero_at[rz]] = mz
        out[f, rest[rr]] = np.where(np.signbit(row[rest[rr]]), -mr, mr)
    return out.astype(F32)


def make_frames(name, mode, frames, seed=0):
    """(y [F,128] f32, codewords [F,128]) of the case's G: equal shares at SNRS dB, interleaved."""
    G = generator(name)
    rng = np.random.default_rng(_seed(name) * 7 + seed + SEED_OF.get((name, mode), 0) + (1000 if mode == "grid" else 0))
    y = np.empty((frames, 128), F32)
    cw = np.empty((frames, 128), np.int64)
    snrs = SNRS_OF.get((name, mode), SNRS)
    for i, snr in enumerate(snrs):
        n = len(range(i, frames, len(snrs)))
        y[i::len(snrs)], cw[i::len(snrs)] = np_oracle.make_frames(G, snr, n, rng)
    if mode == "grid":
        y = to_grid(y, grid_q(name))
    if name in ("low_bytes", "high_bytes"):
        y = _relay(y, pi(name)[zero_columns(name)], name == "low_bytes")
    return y, cw


def pack_rows(P):
    """[..., 64, 64] 0/1 -> [..., 64] uint64, bit c of word r = P[r, c]."""
    return np.packbits(np.asarray(P, np.uint8), axis=-1, bitorder="little").view(np.uint64)[..., 0]


def front(G, y):
    """The C oracle's front end per frame: perm [F,128] int32, Gp [F,64,128] int32, exchanges [F]."""
    perm, Gp, ns = [], [], []
    for row in y:
        p, g, sw = c_oracle.osd_front(G, row)
        perm.append(p)
        Gp.append(g)
        ns.append(len(sw))
    return np.stack(perm), np.stack(Gp), np.array(ns)


@functools.lru_cache(maxsize=None)
def case(name, mode, frames=96, seed=0):
    """dict(name, mode, G, y, cw, perm, Gp, parity = packed rows of P'', nswaps, yp = y in primed order).  Cached: shared,
    read-only."""
    G = generator(name)
    y, cw = make_frames(name, mode, frames, seed)
    perm, Gp, ns = front(G, y)
    c = dict(name=name, mode=mode, G=G, y=y, cw=cw, perm=perm, Gp=Gp, parity=pack_rows(Gp[:, :, 64:]), nswaps=ns,
             yp=np.take_along_axis(y, perm.astype(np.int64), axis=1))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def direct(name, mode, sorted_y=True, frames=12, seed=0):
    """The pair as written: dict(G = [I | P'], y = y' (primed), cw = label', perm = identity, Gp, parity, yp)."""
    G = systematic(name)
    rng = np.random.default_rng(_seed(name) * 11 + seed + (1 if sorted_y else 0))
    y = np.empty((frames, 128), F32)
    cw = np.empty((frames, 128), np.int64)
    for i, snr in enumerate(SNRS):
        n = len(range(i, frames, len(SNRS)))
        y[i::len(SNRS)], cw[i::len(SNRS)] = np_oracle.make_frames(G, snr, n, rng)
    if mode == "grid":
        y = to_grid(y)
    if sorted_y:
        mag = -np.sort(-np.abs(y), axis=1)
        y = np.where(np.signbit(y), -mag, mag).astype(F32)
    perm = np.tile(np.arange(128, dtype=np.int32), (frames, 1))
    Gp = np.tile(G.astype(np.int32), (frames, 1, 1))
    c = dict(name=name, mode=mode, G=G, y=y, cw=cw, perm=perm, Gp=Gp, parity=pack_rows(Gp[:, :, 64:]),
             nswaps=np.zeros(frames, np.int64), yp=y)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


# ------------------------------------------------------------------------------------------------------ premises
_E1 = np_oracle.tep_matrix(64, 1)


def order1_costs(yp, Gp):
    """The 65 order-1 metrics of one frame (table order) in the canonical float order."""
    hard = np.where(yp > 0, 0, 1).astype(np.int64)
    cand = ((_E1 + hard[None, :64]) % 2).dot(Gp.astype(np.int64)) % 2
    return np_oracle.weighted_distance_rows((cand + hard[None]) % 2, np.abs(yp), 64)


def tie_frames(c):
    """Frames whose minimum order-1 metric is attained by two or more of the 65 TEPs (the first-minimum rule decides)."""
    out = []
    for f in range(len(c["y"])):
        cost = order1_costs(c["yp"][f], c["Gp"][f])
        out.append(int((cost.view(np.uint32) == cost.min().view(np.uint32)).sum()) >= 2)
    return np.array(out)


def structure(c):
    """What survives in P'' (per frame): zero rows, rows equal to an earlier row, all-ones rows, distinct non-zero rows."""
    rows = c["parity"]
    zero = (rows == 0).sum(axis=1)
    dup = np.array([64 - len(np.unique(r)) for r in rows])
    ones = (rows == np.uint64(0xFFFFFFFFFFFFFFFF)).sum(axis=1)
    kinds = np.array([len(np.unique(r[r != 0])) for r in rows])
    return dict(zero=zero, dup=dup, ones=ones, kinds=kinds)


def prefix_premise(c):
    """low_bytes: every TEP's prefix (MRB sum + parity bytes 0-1) is its full metric <=> no discrepancy bit at parity
    positions 16..63 for any TEP <=> P'' has no weight there and y' is positive there.  high_bytes: every TEP's prefix is
    its MRB sum, the same with positions 0..15.  -> per-frame bool."""
    lo = c["name"] == "low_bytes"
    cols = slice(80, 128) if lo else slice(64, 80)
    return ~c["Gp"][:, :, cols].any(axis=(1, 2)) & (c["yp"][:, cols] > 0).all(axis=1)
