"""Test helper: the NumPy model of the wide H-form OSD entry points (ldpc_hosdw_*): ``hosdx_model.hosdx_frame`` with m taken
as the RANK of H, so that H may have redundant rows and k = n - m may pass 64.

The elimination is np_oracle.gf2_eliminate, which deletes an all-zero row when it meets one (full_gf2elim :247-250).
``eliminate_traced`` is a copy that also returns, per deletion, the pivot step at which it happened and the rows left before
it; every call asserts that the copy's matrix and exchange list equal the oracle's.

Layouts: those of tests/hosdx_model.py except M [F,128] u64: entry r < m bits j = 0..63 of row r, entry 64 + r bits j = 64..k-1,
zeros elsewhere (``pack_M``).

Redundant-row codes (``redundant``): the structured full-rank H of ``hosdx_model.code(k, n, name)`` with R - m extra rows
inserted at the first, a middle and the last position in turn; an extra row is a sum of existing rows, a copy of one, or
all-zero as given, in turn.
"""
import functools
import itertools

import numpy as np

from oracle import np_oracle
from tests import hosdx_model as HM
from tests import osd_shapes

F32 = np.float32
FRAMES = HM.FRAMES


def eliminate_traced(M):
    """np_oracle.gf2_eliminate -> (reduced matrix, swaps, deletions): ``deletions`` lists (pivot step i, rows left before the
    deletion) in the order the rows were deleted, those after the last pivot step included."""
    M = np.array(M, dtype=np.int64, copy=True)
    swaps, deletions = [], []
    i = j = 0
    m, n = M.shape
    while i < m and j < n:
        below = np.flatnonzero(M[i:, j])
        if below.size:
            r = i + int(below[0])
            if r != i:
                M[[i, r]] = M[[r, i]]
        else:
            right = np.flatnonzero(M[i, j:])
            if right.size == 0:
                deletions.append((i, m))
                M = np.delete(M, i, axis=0)
                m -= 1
                continue
            c = j + int(right[0])
            M[:, [j, c]] = M[:, [c, j]]
            swaps.append((j, c))
        hit = M[:, j].astype(bool)
        hit[i] = False
        M[hit, j:] ^= M[i, j:]
        i += 1
        j += 1
    return M, swaps, deletions


def rank(H):
    return np_oracle.gf2_eliminate(np.asarray(H))[0].shape[0]


def identify_mrb(H_ordered, m):
    """np_oracle.hosd_identify_mrb (:43-80) for an H of rank m with any number of rows -> (uidx, M [m, k], swaps, deletions)."""
    n = H_ordered.shape[1]
    k = n - m
    R, swaps, deletions = eliminate_traced(H_ordered)
    Ro, so = np_oracle.gf2_eliminate(H_ordered)
    assert R.shape == Ro.shape == (m, n) and np.array_equal(R, Ro) and swaps == so
    idx = np.arange(n)
    for a, b in swaps:                                         # :58-62
        idx[a], idx[b] = idx[b], idx[a]
    mrb = idx[-k:]                                             # :64
    sw = np.argsort(mrb, kind="stable")                        # :66
    return np.concatenate([idx[:m], mrb[sw]]), R[:, -k:][:, sw], swaps, deletions


def hosdw_frame(order_llr, metric_llr, label, H, blocks, m=None):
    """``hosdx_model.hosdx_frame`` with m = rank(H): the same dict plus ``deletions`` (see ``eliminate_traced``)."""
    order_llr = np.asarray(order_llr, dtype=F32)
    metric_llr = np.asarray(metric_llr, dtype=F32)
    H = np.asarray(H)
    n = H.shape[1]
    m = rank(H) if m is None else m
    k = n - m
    lri = np_oracle.hosd_reorder(order_llr)
    uidx, M, swaps, deletions = identify_mrb(H[:, lri], m)
    perm = lri[uidx]
    o_in, o_orig = order_llr[perm], metric_llr[perm]
    hard_orig = np.where(o_orig > 0, 0, 1).astype(np.int64)
    mag = np.abs(o_orig)
    initial_mrb = np.where(o_in > 0, 0, 1).astype(np.int64)[-k:]
    mins, args, off = [], [], 0
    best = (None, -1, None)
    for E in blocks:
        mrb = (np.asarray(E, dtype=np.int64).reshape(-1, k) + initial_mrb[None, :]) % 2
        cand = np.concatenate([mrb.dot(M.T) % 2, mrb], axis=1)
        cost = HM.hosdx_cost((cand + hard_orig[None, :]) % 2, mag) if len(cand) else np.zeros(0, F32)
        a = int(np.argmin(cost)) if len(cost) else -1
        mins.append(cost[a] if a >= 0 else F32(np.inf))
        args.append(off + a if a >= 0 else -1)
        if a >= 0 and (best[0] is None or cost[a] < best[0]):
            best = (cost[a], off + a, cand[a])
        off += len(cost)
    truth = None
    if label is not None:
        truth = HM.hosdx_cost((np.asarray(label, dtype=np.int64)[perm] + hard_orig) % 2, mag)[0]
    cw = np.zeros(n, dtype=np.int64)
    if best[2] is not None:
        cw[perm] = best[2]
    return dict(lri=lri, uidx=uidx, perm=perm, M=M, swaps=swaps, deletions=deletions, block_min=np.array(mins, dtype=F32),
                block_arg=np.array(args, dtype=np.int64), truth=truth, best_index=best[1], metric=best[0], codeword=cw)


def pack_M(M):
    """[m, k] 0/1 -> [128] u64: entry r < m bits j = 0..63 of row r, entry 64 + r bits j = 64..k-1."""
    m, k = M.shape
    bits = np.zeros((64, 128), np.uint8)
    bits[:m, :k] = M
    w = np.packbits(bits, axis=1, bitorder="little").view(np.uint64).reshape(64, 2)
    return np.concatenate([w[:, 0], w[:, 1]])


def packed(results, nblk):
    """``hosdx_model.packed`` with the two-plane M."""
    out = HM.packed([dict(r, M=np.zeros((1, 1), np.int64)) for r in results], nblk)
    out["M"] = np.stack([pack_M(r["M"]) for r in results])
    return out


def model(x, y, cw, H, blocks):
    m = rank(H)
    return packed([hosdw_frame(x[f], y[f], cw[f], H, blocks, m) for f in range(len(x))], len(blocks))


# ------------------------------------------------------------------------------------------------------- TEP blocks
@functools.lru_cache(maxsize=None)
def wide_blocks(k):
    """``hosdx_model.edge_blocks(k)`` (order 0, singles, an empty block, all pairs) while the pair block stays a few thousand
    TEPs (k < 100); from there the pairs are a seeded sample of 1500, ascending in the enumeration order."""
    if k < 100:
        return HM.edge_blocks(k)
    pairs = list(itertools.combinations(range(k), 2))
    pick = np.sort(np.random.default_rng(4000 + k).choice(len(pairs), size=1500, replace=False))
    E = np.zeros((len(pick), k), np.int64)
    for r, t in enumerate(pick):
        E[r, list(pairs[t])] = 1
    return (np.zeros((1, k), np.int64), np.eye(k, dtype=np.int64), np.zeros((0, k), np.int64), E)


# ------------------------------------------------------------------------------------------------ redundant-row codes
KINDS = ("sum", "copy", "zero")


@functools.lru_cache(maxsize=None)
def redundant(k, n, name, R, style=None):
    """(H [R, n], G [k, n]) of rank n - k: ``hosdx_model.code(k, n, name)`` with R - (n - k) extra rows.  Extra row e goes to
    the first, a middle or the last position (e mod 3) and is a sum of two or three rows present, a copy of one, or all-zero
    ((e // 3 + e) mod 3).  ``style`` = "first" / "last" makes the last extra row an all-zero one at that end; "copies" makes
    every extra row a copy."""
    H0, G = HM.code(k, n, name)
    m = n - k
    assert R > m
    rng = np.random.default_rng(93000 + 1000 * HM.STRUCTURES.index(name) + 131 * k + n + 7 * R)
    rows = [np.array(r) for r in H0]
    for e in range(R - m):
        kind = "copy" if style == "copies" else KINDS[(e // 3 + e) % 3]
        if kind == "sum":
            pick = rng.choice(len(rows), size=min(len(rows), 2 + e % 2), replace=False)
            new = np.bitwise_xor.reduce(np.stack([rows[p] for p in pick]), axis=0)
        elif kind == "copy":
            new = rows[int(rng.integers(len(rows)))].copy()
        else:
            new = np.zeros(n, np.int64)
        pos = (0, len(rows) // 2, len(rows))[e % 3]
        if style in ("first", "last") and e == R - m - 1:
            new, pos = np.zeros(n, np.int64), (0 if style == "first" else len(rows))
        rows.insert(pos, new)
    H = np.stack(rows)
    assert H.shape == (R, n) and not (H.dot(np.asarray(G).T) % 2).any()
    H.setflags(write=False)
    return H, G


@functools.lru_cache(maxsize=None)
def case(k, n, name, mode, R=None, style=None):
    """``hosdx_model.edge_case`` for the wide family: FRAMES frames of the structured code (redundant rows with R), TEP blocks
    ``wide_blocks(k)``, the model's results -> dict(H, x, y, cw, blocks, want, results)."""
    H, G = HM.code(k, n, name) if R is None else redundant(k, n, name, R, style)
    rng = np.random.default_rng(94000 + 7919 * HM.STRUCTURES.index(name) + 131 * k + n + 17 * HM.MODES.index(mode) + (R or 0))
    count = FRAMES // 6 if mode == "extreme" else FRAMES
    y, cw = np_oracle.make_frames(G, 2.0, count, rng)[:2]
    y = np.asarray(y, F32)
    x = (y + F32(0.6) * rng.standard_normal(y.shape).astype(F32)).astype(F32)
    if mode == "grid":
        x, y = osd_shapes.to_grid(x), osd_shapes.to_grid(y)
    elif mode == "extreme":
        x, y, cw = osd_shapes.extremes(x, rng), osd_shapes.extremes(y, rng), np.concatenate([cw] * 6)
    x, y = np.ascontiguousarray(x, F32), np.ascontiguousarray(y, F32)
    blocks = wide_blocks(k)
    m = n - k
    results = [hosdw_frame(x[f], y[f], cw[f], H, blocks, m) for f in range(len(x))]
    for a in (x, y, cw):
        a.setflags(write=False)
    return dict(H=H, x=x, y=y, cw=cw, blocks=blocks, want=packed(results, len(blocks)), results=results)


# ------------------------------------------------------------------------------------------------------ array codes
ARRAY = {"121_60": "ArrayCode_N121_K60_r0.50.alist", "121_80": "ArrayCode_N121_K80_r0.66.alist"}
ARRAY_FRAMES = 48
ARRAY_SNRS = (1.0, 3.0)
# (k, n, R, style of ``redundant``) of the redundant-row cases at the shape edges
REDUNDANT = ((5, 12, 9, None), (33, 64, 64, "first"), (33, 64, 65, None), (64, 128, 127, None), (70, 87, 20, "last"),
             (100, 108, 108, None), (127, 128, 6, "copies"))


@functools.lru_cache(maxsize=None)
def array_case(golden_dir, which, snr, reverse=False):
    """ARRAY_FRAMES frames of an array code: ordering values from ``hosdx_model.refined_frames`` (on H as given), the order-2
    convention path, the model on H (rows reversed with ``reverse``) -> dict(H, G, x, y, cw, blocks, results)."""
    import os
    c = np_oracle.Code(os.path.join(golden_dir, ARRAY[which]))
    x, y, cw = HM.refined_frames(c.H, c.G, snr, ARRAY_FRAMES, 300 + int(10 * snr))
    H = np.ascontiguousarray(c.H[::-1]) if reverse else c.H
    blocks = HM.path_blocks(c.k, 2)
    m = c.H.shape[1] - c.k
    results = [hosdw_frame(x[f], y[f], cw[f], H, blocks, m) for f in range(len(x))]
    return dict(H=H, G=c.G, x=x, y=y, cw=cw, blocks=blocks, results=results)
