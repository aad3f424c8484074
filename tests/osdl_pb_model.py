"""Test helper: the CPU model of PB-OSD for any (k, n) with n - k <= 192, in the device layouts of ldpc_osdl_pb_search /
_pb_decode, and the inputs of tests/test_gpu_osdl_pb.py (tests/test_osdl_pb_host.py asserts their premises without a GPU).

The model is tests/osdx_pb_model._pb_frame with 8 ceil(m / 64) byte tables in place of 8 (m = n - k): the parity discrepancy is
an integer of m bits, the metric adds the byte sums of word 0, then of word 1, then of word 2 to the reliability sum, each
byte's set positions ascending from 0.0f.  det_expf, binom_cdf and the tags are that module's.  Where m <= 64 the two models
are the same arithmetic, and ``pb`` here equals ``osdx_pb_model.pb`` exactly (asserted on the host).
"""
import functools
import heapq
import math

import numpy as np

from tests import osdl_model
from tests import osdx_pb_model as M

F32 = np.float32
det_expf, binom_cdf, quantise, tag_counts, frontier_bound = M.det_expf, M.binom_cdf, M.quantise, M.tag_counts, M.frontier_bound


def _bits_int(bits):
    return int.from_bytes(np.packbits(np.asarray(bits, dtype=np.uint8), bitorder="little").tobytes(), "little")


def pb_frame(yp, Gp, order, snr_db):
    """One frame in the primed domain -> dict(support, cand [n], metric, best, ntep, aux (cmp, suc1, suc2, stop), tags, peak)."""
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        return _pb_frame(np.asarray(yp, dtype=F32), np.asarray(Gp, dtype=np.int64), order, snr_db)


def _pb_frame(yp, Gp, order, snr_db):
    k, n = Gp.shape
    m = n - k
    nb = 8 * ((m + 63) // 64)
    w = np.abs(yp)
    hard = np.where(yp > 0, 0, 1).astype(np.int64)
    P = [_bits_int(Gp[r, k:]) for r in range(k)]
    d0 = _bits_int(hard[k:])
    for r in range(k):
        if hard[r]:
            d0 ^= P[r]
    # byte tables of the parity part: each byte's set positions ascending from 0.0f (a position beyond n adds nothing)
    wp = np.zeros(8 * nb, F32)
    wp[:m] = w[k:]
    lut = np.zeros((nb, 256), F32)
    for b in range(nb):
        for t in range(8):
            lut[b, 1 << t:2 << t] = lut[b, 0:1 << t] + wp[8 * b + t]

    def cost(mrb, D):
        acc = F32(mrb)
        for b in range(nb):
            acc = F32(acc + lut[b, (D >> (8 * b)) & 0xFF])
        return acc

    c4 = F32(-4.0 * (1.0 / math.pow(10.0, float(F32(snr_db)) / 10.0)))
    q = [F32(F32(1.0) / F32(F32(1.0) + det_expf(-F32(c4 * w[p])))) for p in range(n)]
    acc, accw = F32(0), F32(0)
    for p in range(k, n):
        acc = F32(acc + q[p])
        accw = F32(accw + w[p])
    p1, lrb_mean = F32(acc / F32(m)), F32(accw / F32(m))
    acc, spl = F32(0), F32(1)
    for p in range(k):
        acc = F32(acc + q[p])
        spl = F32(spl * F32(F32(1.0) - q[p]))
    pt = F32(acc / F32(k))
    cdfA, cdfH = binom_cdf(m, float(p1)), binom_cdf(m, 0.5)
    niu = binom_cdf(k, float(pt))[order]
    nmax = sum(math.comb(k, i) for i in range(order + 1))
    p_t_suc, p_t_pro = 0.99 * niu, 0.002 * math.sqrt((1.0 - niu) / float(nmax))

    best, best_sup, best_D, best_idx = cost(F32(0), d0), (), d0, 0
    ntep, stop, cmp_, suc1, suc2, peak = nmax, 0, 0, 0, 0, 0
    tags = set()
    heap = [(float(w[k - 1]), 0, (k - 1,))] if order > 0 else []
    seq = 1
    for j in range(nmax - 1):
        peak = max(peak, len(heap))
        cmp_ += 1 if len(heap) == 1 else 2
        s, _, sup = heapq.heappop(heap)
        if heap and heap[0][0] == s:
            tags.add("tie")
        rs = F32(s)
        last, wt = sup[-1], len(sup)
        if last < k - 1 and wt < order:
            heapq.heappush(heap, (float(F32(rs + w[k - 1])), seq, sup + (k - 1,)))
            seq += 1
        if (last - sup[-2] > 1) if wt > 1 else (last - 1 >= 0):
            child = sup[:-1] + (last - 1,)
            a = w[child[0]]
            for p in child[1:]:
                a = F32(a + w[p])
            heapq.heappush(heap, (float(a), seq, child))
            seq += 1
        w1 = F32(det_expf(F32(c4 * rs)) * spl)
        w2 = F32(F32(1.0) - w1)
        bt = np.floor(F32(F32(best - rs) / lrb_mean))
        beta = (int(bt) if bt < F32(m) else m) if bt > 0 else 0
        bs = F32(F32(0.0) + F32(w1 * F32(cdfA[beta])))
        bs = F32(bs + F32(w2 * F32(cdfH[beta])))
        if float(bs) < p_t_pro:
            stop, ntep = 1, j + 1
            break
        D = d0
        for p in sup:
            D ^= P[p]
        c = cost(rs, D)
        suc1 += 1
        if c < best:
            best, best_sup, best_D, best_idx = c, sup, D, j + 1
            suc2 += 1
            if j + 1 >= 64:
                tags.add("late_improvement")
            prod = F32(1.0)
            for p in range(m):
                prod = F32(prod * (F32(F32(2.0) * q[k + p]) if (D >> p) & 1 else F32(F32(2.0) * F32(F32(1.0) - q[k + p]))))
            p_suc = F32(F32(1.0) / F32(F32(1.0) + F32(F32(F32(F32(1.0) - w1) / w1) / prod)))
            if p_suc > F32(p_t_suc):
                stop, ntep = 2, j + 1
                break
    tags.add(f"stop{stop}")
    if best_idx:
        tags.add("improved")
    assert peak <= frontier_bound(k), (peak, k)
    cand = hard.copy()
    for p in best_sup:
        cand[p] ^= 1
    for c in range(m):
        cand[k + c] = hard[k + c] ^ ((best_D >> c) & 1)
    return dict(support=best_sup, cand=cand, metric=best, best=best_idx, ntep=ntep, aux=(cmp_, suc1, suc2, stop), tags=tags,
                peak=peak)


def pb(y, perm, Gps, order, snr_db):
    """Frames y [F, n] in original order with front-end results (perm [F, >= n], Gps: [I | P'] per frame) -> dict of arrays in
    the layouts of ldpc_osdl_pb_search: cw [F, words] u64, metric [F] f32, best / ntep [F] i32, aux [F, 4] i32, and tags (a
    list of sets), peak [F], supports (a list of tuples)."""
    y = np.asarray(y, dtype=F32)
    k, n = np.asarray(Gps[0]).shape
    F = len(y)
    bits = np.zeros((F, n), np.uint8)
    out = dict(metric=np.zeros(F, F32), best=np.zeros(F, np.int32), ntep=np.zeros(F, np.int32), aux=np.zeros((F, 4), np.int32),
               tags=[], peak=np.zeros(F, np.int64), supports=[])
    for f in range(F):
        p = np.asarray(perm[f][:n]).astype(np.int64)
        r = pb_frame(y[f][p], Gps[f], order, snr_db)
        bits[f, p] = r["cand"]
        out["metric"][f], out["best"][f], out["ntep"][f], out["aux"][f], out["peak"][f] = r["metric"], r["best"], r["ntep"], r["aux"], r["peak"]
        out["tags"].append(r["tags"])
        out["supports"].append(r["support"])
    out["cw"] = M._pack(bits)
    return out


def span(sup):
    """The MRB words a support lies in, ascending, one entry per position: (1, 2), (1, 1), ..."""
    return tuple(p >> 6 for p in sup)


# ---------------------------------------------------------------------------------------------------------------------
# the slot tiers of osdl_pb_kernel at order 3 (ldpc_osdl_pb.h): 2048 slots serve k <= 64, 4096 k <= 91, 8064 k <= 127 and
# 18 368 k <= 192; orders <= 2 take 192 slots
# ---------------------------------------------------------------------------------------------------------------------
TIER_SLOTS = (2048, 4096, 8064, 18368)


def slots3(k):
    return k + (k - 1) * (k - 2) // 2


def tier(k):
    return min(t for t in TIER_SLOTS if slots3(k) <= t)


# ---------------------------------------------------------------------------------------------------------------------
# codes: the named ones of osdl_model, or a shape (k, n): H = [A | I] of osdl_model._h_systematic
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def graph(code):
    """-> (H, G) of a name of osdl_model or of a shape (k, n)."""
    if isinstance(code, tuple):
        from oracle import np_oracle
        k, n = code
        H = osdl_model._h_systematic(n, k)
        G = np_oracle.generator_from_H(H)
        assert G.shape == (k, n)
        return H, G
    return osdl_model.graph(code)


# ---------------------------------------------------------------------------------------------------------------------
# 1: natural frames, all from osdl_model.frames(code, dB, frames, 7), decoded with snr_db = the channel's
# ---------------------------------------------------------------------------------------------------------------------
# (code, dB, order, frames)
NATURAL = (("wl384", 2.0, 2, 12), ("wl384", 2.0, 3, 6), ("wl384", 1.0, 2, 8), ("s200_100", 1.0, 3, 8), ("s128_32", 0.0, 3, 12),
           ("s100_20", 0.0, 3, 8), ("s321_130", 1.0, 2, 8), ("s193_1", 0.0, 1, 8), ("s256_192", 3.0, 2, 8), ("s256_192", 1.0, 2, 8))
SEED = 7


@functools.lru_cache(maxsize=None)
def natural(i, quant=False):
    """-> (y, labels, front oracle in the osdl layouts, order, snr_db, model result) of NATURAL[i], computed once and shared;
    ``quant``: the same frames quantised (osdx_pb_model.quantise)."""
    name, snr, order, F = NATURAL[i]
    G = osdl_model.graph(name)[1]
    y, cw = osdl_model.frames(name, snr, F, SEED)
    if quant:
        y = quantise(y)
    y = np.ascontiguousarray(y, dtype=F32)
    front = osdl_model.front_oracle(G, y)
    return y, cw, front, order, snr, pb(y, front[0], front[3], order, snr)


# quantised inputs: reliability sums tie massively.  s200_100: k = 100, WP = 2; wl384: k = 192, WP = 3.  (index into NATURAL, frames)
QUANTISED = ((3, 4), (0, 4))


# ---------------------------------------------------------------------------------------------------------------------
# 2: loud and quiet noiseless frames
# ---------------------------------------------------------------------------------------------------------------------
LOUD_AMP, QUIET_AMP, LOUD_SNR_DB = 6.0 / 3.1773, 0.02, 1.0
IN_TURN = ("wl384", (100, 200), (80, 150), (32, 128))       # the top tier and one code per lower tier (8064, 4096, 2048 slots)
TIER_FRAMES = ((65, 130), (92, 150), (128, 320))           # one order-3 frame just above each tier boundary: WP = 2, 1, 3


@functools.lru_cache(maxsize=None)
def in_turn(code, order, loud=2, quiet=2):
    """Noiseless codewords of ``code`` decoded with snr_db = 1: ``loud`` frames with |y| = 6.0 / 3.1773 (1 +- 1 %) and ``quiet``
    ones with |y| = 0.02.  The all-zero TEP costs 0.0, nothing improves on it and beta = 0.  Loud: at order 2 no rule stops the
    search, every TEP is visited; at order 3 the first weight-3 TEP stops it by rule 1, after all of the lighter ones, with
    (k-1)(k-2)/2 weight-3 runs live: every weight-3 slot k needs has been written.  Quiet: q ~ 1/2, the search stops at its
    first TEP.  -> (y, labels, front oracle, model)."""
    G = graph(code)[1]
    n = G.shape[1]
    rng = np.random.default_rng(3)
    msg = rng.integers(0, 2, (loud + quiet, G.shape[0]))
    cw = (msg @ G % 2).astype(np.uint8)
    amp = np.concatenate([LOUD_AMP * (1.0 + rng.uniform(-0.01, 0.01, (loud, n))), np.full((quiet, n), QUIET_AMP)]).astype(F32)
    y = np.ascontiguousarray(amp * (F32(1.0) - F32(2.0) * cw.astype(F32)), dtype=F32)
    front = osdl_model.front_oracle(G, y)
    return y, cw, front, pb(y, front[0], front[3], order, LOUD_SNR_DB)


# ---------------------------------------------------------------------------------------------------------------------
# 4: equal magnitudes on the MRB: the visit order is the insertion order
# ---------------------------------------------------------------------------------------------------------------------
EQUAL = ((100, 200, 2, 1, 2), (100, 200, 2, 2, 2), (150, 321, 2, 1, 1), (150, 321, 2, 2, 1), (70, 200, 3, 1, 1))   # (k, n, order, levels, frames)


@functools.lru_cache(maxsize=None)
def equal_magnitudes(k, n, order, levels, F, seed=11):
    """osdx_pb_model.equal_magnitudes in the osdl layouts: identity permutation, random P', |y'| equal over the MRB (levels = 1)
    or of two distinct values (levels = 2), so that the sums of one weight tie and the visit order is the insertion order.
    -> dict(y [F, n], perm, parity, order, snr_db, model)."""
    m = n - k
    rng = np.random.default_rng(seed)
    ys, Gps, perms, pars = [], [], [], []
    for f in range(F):
        Pm = rng.integers(0, 2, (k, m), dtype=np.int64)
        Gp = np.concatenate([np.eye(k, dtype=np.int64), Pm], axis=1)
        p, q = osdl_model.pack_front(np.arange(n), Gp)
        Gps.append(Gp), perms.append(p), pars.append(q)
        mrb = np.full(k, 0.75, F32)
        if levels == 2:
            mrb[rng.random(k) < 0.5] = F32(0.5)
        mag = np.concatenate([mrb, rng.uniform(0.3, 1.2, m).astype(F32)]).astype(F32)
        sign = np.where(rng.integers(0, 2, n) == 1, F32(-1), F32(1))
        ys.append(mag * sign)
    y = np.ascontiguousarray(np.stack(ys), dtype=F32)
    perm, parity = np.stack(perms), np.stack(pars)
    return dict(y=y, perm=perm, parity=parity, order=order, snr_db=1.0, model=pb(y, perm, Gps, order, 1.0))
