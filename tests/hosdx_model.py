"""Test helper: the NumPy model of the any-shape H-form OSD entry points (ldpc_hosdx_*), the packing of its results into their
device layouts, and full-rank check matrices at the shape edges.

``hosdx_cost`` is np_oracle.hosd_cost with a partial last byte: the n updated positions (LRB first) in bytes of eight, each
byte summed ascending from 0.0f, the ceil(n/8) byte sums added ascending from byte 0.  ``hosdx_frame`` is np_oracle.hosd_frame
with that cost; wherever n % 8 == 0 the two agree field by field (tests/test_hosdx_host.py).

Layouts: lri / uidx [F,128] u8 with zeros at and beyond n; M [F,64] u64, row r < m, bit j < k, zeros elsewhere; cw
[F, ceil(n/64)] u64 in original bit order.

Structured codes: H = [P'^T | I_m] with its columns permuted by a seeded pi, P' = osd_shapes.parity(k, n, .) -- random_dense,
equal_cols (P'^T has equal adjacent columns: osd_shapes' equal_rows), rank_one, identity.  H has m rows and rank m by
construction; repeated and rank-one columns drive the elimination through long chains of column exchanges.
"""
import functools
import itertools

import numpy as np

from oracle import np_oracle
from tests import osd_shapes

F32 = np.float32
STRUCTURES = ("random_dense", "equal_cols", "rank_one", "identity")
_PARITY_OF = {"random_dense": "random_dense", "equal_cols": "equal_rows", "rank_one": "rank_one", "identity": "identity"}
MODES = ("float", "grid", "extreme")
FRAMES = 12


def hosdx_cost(disc, w):
    """sum_p disc[p] * w[p] in the canonical float32 order; ``disc`` [N, n] or [n], -> [N] f32."""
    disc = np.atleast_2d(np.asarray(disc)).astype(F32)
    w = np.asarray(w, dtype=F32)
    n = disc.shape[1]
    acc = None
    for b in range((n + 7) // 8):
        part = np.zeros(disc.shape[0], dtype=F32)
        for p in range(8 * b, min(8 * b + 8, n)):
            part = (part + disc[:, p] * w[p]).astype(F32)
        acc = part if acc is None else (acc + part).astype(F32)
    return acc


def hosdx_frame(order_llr, metric_llr, label, H, blocks):
    """np_oracle.hosd_frame (one frame of sliding_osd's block evaluation, :164-186) with ``hosdx_cost``; the same dict."""
    order_llr = np.asarray(order_llr, dtype=F32)
    metric_llr = np.asarray(metric_llr, dtype=F32)
    m, n = H.shape
    k = n - m
    lri = np_oracle.hosd_reorder(order_llr)
    uidx, M, swaps = np_oracle.hosd_identify_mrb(np.asarray(H)[:, lri], k)
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
        cost = hosdx_cost((cand + hard_orig[None, :]) % 2, mag) if len(cand) else np.zeros(0, F32)
        a = int(np.argmin(cost)) if len(cost) else -1
        mins.append(cost[a] if a >= 0 else F32(np.inf))
        args.append(off + a if a >= 0 else -1)
        if a >= 0 and (best[0] is None or cost[a] < best[0]):
            best = (cost[a], off + a, cand[a])
        off += len(cost)
    truth = None
    if label is not None:
        truth = hosdx_cost((np.asarray(label, dtype=np.int64)[perm] + hard_orig) % 2, mag)[0]
    cw = np.zeros(n, dtype=np.int64)
    if best[2] is not None:
        cw[perm] = best[2]
    return dict(lri=lri, uidx=uidx, perm=perm, M=M, swaps=swaps, block_min=np.array(mins, dtype=F32),
                block_arg=np.array(args, dtype=np.int64), truth=truth, best_index=best[1], metric=best[0], codeword=cw)


# ------------------------------------------------------------------------------------------------------------ layouts
def pack_index(a):
    """[n] -> [128] u8, zeros at and beyond n (lri, uidx)."""
    out = np.zeros(128, np.uint8)
    out[:len(a)] = a
    return out


def pack_M(M):
    """[m, k] 0/1 -> [64] u64: row r < m, bit j < k."""
    m, k = M.shape
    bits = np.zeros((64, 64), np.uint8)
    bits[:m, :k] = M
    return np.packbits(bits, axis=1, bitorder="little").view(np.uint64).reshape(64)


def pack_cw(bits):
    """[n] or [F, n] 0/1 -> [ceil(n/64)] / [F, ceil(n/64)] u64, original bit order."""
    b = np.atleast_2d(np.asarray(bits, dtype=np.uint8))
    pad = (-b.shape[1]) % 64
    b = np.concatenate([b, np.zeros((b.shape[0], pad), np.uint8)], axis=1)
    w = np.packbits(b, axis=1, bitorder="little").view(np.uint64)
    return w if np.ndim(bits) == 2 else w[0]


def packed(results, nblk):
    """A list of ``hosdx_frame`` dicts -> dict of arrays in the device layouts: lri, uidx [F,128] u8, M [F,64] u64, nswaps [F]
    i32, block_min [F,nblk] f32, block_arg [F,nblk] i32, truth, metric [F] f32, best [F] i32, cw [F,words] u64."""
    F = len(results)
    inf = F32(np.inf)
    return dict(
        lri=np.stack([pack_index(r["lri"]) for r in results]), uidx=np.stack([pack_index(r["uidx"]) for r in results]),
        M=np.stack([pack_M(r["M"]) for r in results]), nswaps=np.array([len(r["swaps"]) for r in results], np.int32),
        block_min=np.stack([r["block_min"] for r in results]).reshape(F, nblk).astype(F32),
        block_arg=np.stack([r["block_arg"] for r in results]).reshape(F, nblk).astype(np.int32),
        truth=np.array([r["truth"] for r in results], F32),
        metric=np.array([inf if r["metric"] is None else r["metric"] for r in results], F32),
        best=np.array([r["best_index"] for r in results], np.int32), cw=pack_cw(np.stack([r["codeword"] for r in results])))


def teps_of(E):
    """[N, k] 0/1 pattern matrix (weight <= 3) -> [N, 4] u8 {p0, p1, p2, weight}, positions ascending."""
    E = np.asarray(E)
    out = np.zeros((E.shape[0], 4), np.uint8)
    for r in range(E.shape[0]):
        pos = np.flatnonzero(E[r])
        assert len(pos) <= 3
        out[r, :len(pos)] = pos
        out[r, 3] = len(pos)
    return out


def table(blocks):
    """TEP blocks -> (teps [N,4] u8, block_off [nblk+1] i32)."""
    tabs = [teps_of(E) for E in blocks]
    off = np.insert(np.cumsum([len(t) for t in tabs]), 0, 0).astype(np.int32)
    return (np.concatenate(tabs) if tabs else np.zeros((0, 4), np.uint8)), off


# ------------------------------------------------------------------------------------------------------- TEP blocks
def path_blocks(k, order_sum, num_seg=3):
    """The reference's convention path of total weight <= order_sum over ``segment_boundaries(k, num_seg)``: one block per
    order pattern (the three-segment patterns, zero beyond the third segment)."""
    _, b = np_oracle.segment_boundaries(k, num_seg)
    ranges = [range(int(b[i]), int(b[i + 1])) for i in range(num_seg)]
    return [np_oracle.error_pattern_gen(p + [0] * (num_seg - 3), ranges, k) for p in np_oracle.convention_path(order_sum)]


@functools.lru_cache(maxsize=None)
def edge_blocks(k):
    """Order 0, all singles, all pairs (k >= 2) and one empty block, in that order with the empty one before the pairs."""
    def rows(sets):
        E = np.zeros((len(sets), k), np.int64)
        for r, s in enumerate(sets):
            E[r, list(s)] = 1
        return E
    out = [rows([()]), rows([(p,) for p in range(k)]), np.zeros((0, k), np.int64)]
    if k >= 2:
        out.append(rows(list(itertools.combinations(range(k), 2))))
    return tuple(out)


# ---------------------------------------------------------------------------------------------------- structured codes
@functools.lru_cache(maxsize=None)
def code(k, n, name):
    """(H [m, n], G [k, n]) of the structured full-rank code: column j of [P'^T | I_m] lands at column pi[j] of H."""
    m = n - k
    P = osd_shapes.parity(k, n, _PARITY_OF[name])
    Hs = np.concatenate([P.T, np.eye(m, dtype=np.int64)], axis=1)
    pi = np.random.default_rng(90000 + 1000 * STRUCTURES.index(name) + 131 * k + n).permutation(n)
    H = np.empty_like(Hs)
    H[:, pi] = Hs
    G = np_oracle.generator_from_H(H)
    assert H.shape == (m, n) and G.shape == (k, n) and not (H.dot(G.T) % 2).any()
    H.setflags(write=False)
    G.setflags(write=False)
    return H, G


@functools.lru_cache(maxsize=None)
def edge_case(k, n, name, mode):
    """FRAMES frames of the structured code: ordering values x (a second noisy look at the codeword, so that its order and
    its MRB hard decisions differ from the metric input's), metric values y, labels cw; ``grid`` rounds both to steps of 0.5
    (ties on every magnitude), ``extreme`` gives the six extremes of osd_shapes.extremes of FRAMES // 6 frames.  With the
    model's results: dict(H, x, y, cw, blocks, want = packed(...))."""
    H, G = code(k, n, name)
    rng = np.random.default_rng(91000 + 7919 * STRUCTURES.index(name) + 131 * k + n + 17 * MODES.index(mode))
    count = FRAMES // 6 if mode == "extreme" else FRAMES
    y, cw = np_oracle.make_frames(G, 2.0, count, rng)[:2]
    y = np.asarray(y, F32)
    x = (y + F32(0.6) * rng.standard_normal(y.shape).astype(F32)).astype(F32)
    if mode == "grid":
        x, y = osd_shapes.to_grid(x), osd_shapes.to_grid(y)
    elif mode == "extreme":
        x, y, cw = osd_shapes.extremes(x, rng), osd_shapes.extremes(y, rng), np.concatenate([cw] * 6)
    x, y = np.ascontiguousarray(x, F32), np.ascontiguousarray(y, F32)
    blocks = edge_blocks(k)
    want = packed([hosdx_frame(x[f], y[f], cw[f], H, blocks) for f in range(len(x))], len(blocks))
    for a in (x, y, cw):
        a.setflags(write=False)
    return dict(H=H, x=x, y=y, cw=cw, blocks=blocks, want=want)


def refined_frames(H, G, snr, count, seed, iters=4):
    """Channel values y (the metric input), ordering values x = the NMS posterior after ``iters`` iterations (the stand-in
    for the CNN-refined values of tests/test_gpu_hosd.py), labels."""
    rng = np.random.default_rng(seed)
    y, cw = np_oracle.make_frames(G, snr, count, rng)[:2]
    y = np.asarray(y, F32)
    x = np.asarray(np_oracle.nms_sparse(y, H, iters, F32(0.669435))[-1], F32)
    return np.ascontiguousarray(x), np.ascontiguousarray(y), cw
