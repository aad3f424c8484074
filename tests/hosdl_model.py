"""Test helper: the NumPy model of the long H-form OSD entry points (ldpc_hosdl_*: n <= 384, an H of at most 192 rows of rank
m = n - k <= 192, k <= 192).  The frame model is ``hosdw_model.hosdw_frame``, which is shape-generic; only the device layouts
and the case tables are new here.

Layouts (S = ceil(n/64), Wm = ceil(m/64), Wk = ceil(k/64)): lri, uidx [64 S] u16 with zeros at and beyond n
(``pack_index``); M [64 Wm, Wk] u64, entry [r][w] bits j = 64w..64w+63 of row r (``pack_M``); codewords [S] u64.
``from_wide`` converts the results of the ldpc_hosdw_* calls (tests/hosdw_model.py's layouts) to these.
"""
import functools
import os

import numpy as np

from oracle import np_oracle
from tests import hosdw_model as WM
from tests import hosdx_model as HM
from tests import osd_shapes

F32 = np.float32
FRAMES = HM.FRAMES
GOLDEN_ALIST = "wimaxlike_N384_K192_P16_set0.alist"
# full-rank shape edges (k, n): the first m above 64, k above 64, three row words on a short code, high rate, five to six
# slots, the longest elimination on a one-bit code, 192 rows below the longest n, the largest shape, the smallest route
SHAPES_ALL = ((64, 129), (128, 257), (192, 384))          # every structure and mode
SHAPES_DENSE = ((65, 129), (1, 130), (192, 256), (1, 193), (108, 300), (5, 12))
# (k, n, R, style of ``hosdw_model.redundant``)
REDUNDANT = ((65, 129, 65, None), (64, 129, 66, None), (100, 228, 129, None), (150, 300, 192, "first"), (150, 300, 192, "last"),
             (127, 128, 6, "copies"))


def pack_index(a, n):
    out = np.zeros(64 * ((n + 63) // 64), np.uint16)
    out[:len(a)] = a
    return out


def pack_M(M):
    """[m, k] 0/1 -> [64 Wm, Wk] u64."""
    m, k = M.shape
    Wm, Wk = (m + 63) // 64, (k + 63) // 64
    bits = np.zeros((64 * Wm, 64 * Wk), np.uint8)
    bits[:m, :k] = M
    return np.packbits(bits, axis=1, bitorder="little").view(np.uint64).reshape(64 * Wm, Wk)


def packed(results, nblk):
    """A list of ``hosdw_frame`` dicts -> dict of arrays in the device layouts of ldpc_hosdl_*."""
    F = len(results)
    inf = F32(np.inf)
    n = len(results[0]["lri"])
    return dict(
        lri=np.stack([pack_index(r["lri"], n) for r in results]), uidx=np.stack([pack_index(r["uidx"], n) for r in results]),
        M=np.stack([pack_M(r["M"]) for r in results]), nswaps=np.array([len(r["swaps"]) for r in results], np.int32),
        block_min=np.stack([r["block_min"] for r in results]).reshape(F, nblk).astype(F32),
        block_arg=np.stack([r["block_arg"] for r in results]).reshape(F, nblk).astype(np.int32),
        truth=np.array([r["truth"] for r in results], F32),
        metric=np.array([inf if r["metric"] is None else r["metric"] for r in results], F32),
        best=np.array([r["best_index"] for r in results], np.int32), cw=HM.pack_cw(np.stack([r["codeword"] for r in results])))


def model(x, y, cw, H, blocks, m=None):
    m = WM.rank(H) if m is None else m
    return packed([WM.hosdw_frame(x[f], y[f], cw[f], H, blocks, m) for f in range(len(x))], len(blocks))


def from_wide(lri, uidx, M, n, m, k):
    """Front-end results of ldpc_hosdw_front ([F,128] u8, [F,128] u8, [F,128] u64) in this family's layouts."""
    S, Wm, Wk = (n + 63) // 64, (m + 63) // 64, (k + 63) // 64
    F = len(lri)
    assert Wm == 1 and S <= 2
    M = np.asarray(M).view(np.uint64).reshape(F, 2, 64)
    return (np.asarray(lri)[:, :64 * S].astype(np.uint16), np.asarray(uidx)[:, :64 * S].astype(np.uint16),
            np.ascontiguousarray(M[:, :Wk, :].transpose(0, 2, 1)))


@functools.lru_cache(maxsize=None)
def case(k, n, name, mode, R=None, style=None, frames=FRAMES):
    """``hosdw_model.case`` in this family's layouts: ``frames`` frames of the structured code (redundant rows with R), TEP
    blocks ``wide_blocks(k)``, the model's results -> dict(H, x, y, cw, blocks, want, results)."""
    H, G = HM.code(k, n, name) if R is None else WM.redundant(k, n, name, R, style)
    rng = np.random.default_rng(95000 + 7919 * HM.STRUCTURES.index(name) + 131 * k + n + 17 * HM.MODES.index(mode) + (R or 0))
    count = frames // 6 if mode == "extreme" else frames
    y, cw = np_oracle.make_frames(G, 2.0, count, rng)[:2]
    y = np.asarray(y, F32)
    x = (y + F32(0.6) * rng.standard_normal(y.shape).astype(F32)).astype(F32)
    if mode == "grid":
        x, y = osd_shapes.to_grid(x), osd_shapes.to_grid(y)
    elif mode == "extreme":
        x, y, cw = osd_shapes.extremes(x, rng), osd_shapes.extremes(y, rng), np.concatenate([cw] * 6)
    x, y = np.ascontiguousarray(x, F32), np.ascontiguousarray(y, F32)
    blocks = WM.wide_blocks(k) if k >= 2 else (np.zeros((1, k), np.int64), np.eye(k, dtype=np.int64), np.zeros((0, k), np.int64))
    m = n - k
    results = [WM.hosdw_frame(x[f], y[f], cw[f], H, blocks, m) for f in range(len(x))]
    for a in (x, y, cw):
        a.setflags(write=False)
    return dict(H=H, x=x, y=y, cw=cw, blocks=blocks, want=packed(results, len(blocks)), results=results)


@functools.lru_cache(maxsize=None)
def golden_case(golden_dir, snr, frames=24):
    """``frames`` frames of the (384,192) code of tests/golden: ordering values from ``hosdx_model.refined_frames``, the blocks
    of ``wide_blocks(192)``, the model's results."""
    c = np_oracle.Code(os.path.join(golden_dir, GOLDEN_ALIST))
    x, y, cw = HM.refined_frames(c.H, c.G, snr, frames, 700 + int(10 * snr))
    blocks = WM.wide_blocks(c.k)
    m = c.H.shape[1] - c.k
    results = [WM.hosdw_frame(x[f], y[f], cw[f], c.H, blocks, m) for f in range(len(x))]
    return dict(H=c.H, G=c.G, x=x, y=y, cw=cw, blocks=blocks, results=results)
