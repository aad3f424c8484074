"""Test helper: the one CPU model of PB-OSD (pb_osd, PB_OSD/pb_testing.py:100-149) for any (k, n) -- every G-form family's
reference -- and the inputs of the any-shape family's PB tests (ldpc_osdx_pb_search / _decode).

The model is oracle/ldpc_oracle.c orc_pb_osd's deterministic float conventions with 64 + 64 replaced by k + (n - k):
    q_p = 1 / (1 + det_expf(-(c4 |y'_p|))) in float32, c4 = (float)(-4 / 10^(snr_db / 10));
    p1, lrb_mean over the parity part / (float)(n - k), pt over the MRB / (float)k, spl = prod (1 - q_p) over the MRB, every
    chain ascending in float32;
    binomial CDFs of (n - k, p1), (n - k, 1/2) and (k, pt) by the float64 pmf recurrence, q^N by left-to-right
    square-and-multiply (six squarings at N = 64);
    the frontier is a heap keyed by (sum, insertion sequence number): "first minimum in list order";
    the metric is osdx_model.costs_vectorised's order of additions, taken from byte tables as the C oracle takes it:
    8 ceil(m / 64) tables (m = n - k), the byte sums of word 0, then of word 1, then of word 2 added to the reliability sum.
Every float32 operation is rounded on its own (NumPy float32 scalars).

Tags of a frame: stop0 / stop1 / stop2, improved (the winner is not the all-zero TEP), tie (a pop whose sum equalled another
live entry's sum), late_improvement (an improvement at rank >= 64).  ``peak`` is the largest live frontier of the run.
"""
import functools
import heapq
import math

import numpy as np

from tests import osd_family as OF
from tests import osdx_model

F32 = np.float32


def det_expf(x):
    """oracle/ldpc_oracle.c det_expf: IEEE + - * / only, one rounding per operation."""
    x = F32(x)
    if x > F32(88.0):
        x = F32(88.0)
    if x < F32(-87.0):
        return F32(0.0)
    kf = F32(np.floor(F32(F32(x * F32(1.44269504)) + F32(0.5))))
    r = F32(F32(x - F32(kf * F32(0.693359375))) - F32(kf * F32(-2.12194440e-4)))
    p = F32(1.9875691500e-4)
    for c in (1.3981999507e-3, 8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1, 5.0000001201e-1):
        p = F32(F32(p * r) + F32(c))
    e = F32(F32(F32(p * F32(r * r)) + r) + F32(1.0))
    scale = np.array([(int(kf) + 127) << 23], dtype=np.int32).view(F32)[0]
    return F32(e * scale)


def binom_cdf(N, p):
    """[N + 1] float64: P[Binomial(N, p) <= b] by the pmf recurrence; q^N by square-and-multiply from the top bit of N down."""
    q = 1.0 - p
    t = q
    for bit in bin(N)[3:]:
        t = t * t
        if bit == "1":
            t = t * q
    ratio = p / q
    acc = t
    cdf = [acc]
    for i in range(N):
        t = t * (float(N - i) / float(i + 1)) * ratio
        acc = acc + t
        cdf.append(acc)
    return cdf


def frontier_bound(k):
    """One weight-1 entry, one weight-2 entry per smaller index, one weight-3 entry per pair (a, b) with b < k - 1."""
    return 1 + (k - 1) + (k - 1) * (k - 2) // 2


def pb_frame(yp, Gp, order, snr_db):
    """One frame in the primed domain -> dict(support, cand [n], metric, best, ntep, aux (cmp, suc1, suc2, stop), tags, peak)."""
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):   # (a vanishing success product: p_suc = 0, as on the device)
        return _pb_frame(np.asarray(yp, dtype=F32), np.asarray(Gp, dtype=np.int64), order, snr_db)


def _bits_int(bits):
    return int.from_bytes(np.packbits(np.asarray(bits, dtype=np.uint8), bitorder="little").tobytes(), "little")


def _pb_frame(yp, Gp, order, snr_db):
    k, n = Gp.shape
    m = n - k
    nb = 8 * ((m + 63) // 64)                                 # byte tables: 8 per word of the parity discrepancy
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


def _pack(bits):
    pad = np.zeros((bits.shape[0], (-bits.shape[1]) % 64), np.uint8)
    return np.packbits(np.concatenate([bits.astype(np.uint8), pad], axis=1), axis=1, bitorder="little").view(np.uint64)


def pb(y, perm, Gps, order, snr_db):
    """Frames y [F, n] in original order with front-end results (perm [F, >= n] of any family, Gps: [I | P'] per frame) -> dict
    of arrays in the layouts of ldpc_osd?_pb_search: cw [F, words] u64, metric [F] f32, best / ntep [F] i32, aux [F, 4] i32,
    and tags (a list of sets), peak [F], supports (a list of tuples)."""
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
    out["cw"] = _pack(bits)
    return out


def tag_counts(results):
    out = {}
    for r in results:
        for tags in r["tags"]:
            for t in tags:
                out[t] = out.get(t, 0) + 1
    return out


def quantise(y):
    """Inputs rounded to multiples of 1/4, zeros replaced by 1/4: reliability sums then tie massively."""
    yq = (np.round(np.asarray(y, dtype=F32) * F32(4)) / F32(4)).astype(F32)
    yq[yq == 0] = F32(0.25)
    return yq


# ---------------------------------------------------------------------------------------------------------------------
# the inputs of tests/test_gpu_osdx_pb.py (tests/test_osdx_pb_host.py asserts their coverage without a GPU)
# ---------------------------------------------------------------------------------------------------------------------
# code -> [(frames at dB, snr_db, order, frames, quantised)], all from osdx_model.frames(code, dB, frames, 7).
# Additions to the sets the feature was specified with:
#   thin        its specified set is full scans only (24 frames of 232 TEPs): with n - k = 13 the promising sum never falls below
#               cdfH[0] = 2^-13 while the threshold 0.002 sqrt((1 - niu) / 232) stays under it for every plausible snr_db, so
#               neither `stop1` nor `tie` occurred on this code.  The second set (the same frames quantised, a decoder told
#               snr_db = 30, so q_p ~ 1/2 and niu ~ 0.11) has both: every frame stops on rule 1, 14 of them after a tie.
#   ldpc_96_48  a quantised set, as the other long codes have.
SETS = {
    "short": [(1.0, 1.0, 3, 48, False), (1.0, 1.0, 3, 48, True)],
    "thin": [(0.0, 0.0, 3, 24, False), (0.0, 30.0, 3, 24, True)],
    "ldpc_96_48": [(0.0, -4.0, 2, 16, False), (1.5, 1.5, 2, 96, False), (1.5, 1.5, 3, 16, False), (1.5, 1.5, 2, 16, True)],
    "array_121_60": [(0.0, -4.0, 2, 24, False), (1.5, 1.5, 2, 16, True)],
    "ccsds": [(0.0, -4.0, 2, 16, False), (1.5, 1.5, 2, 32, True), (1.5, 1.5, 3, 24, False)],
}
CASES = [(name, i) for name in osdx_model.CODES for i in range(len(SETS[name]))]
EVERY_CODE = ("stop0", "stop1", "improved", "tie")
NO_STOP2 = ("thin",)


@functools.lru_cache(maxsize=None)
def case(name, i):
    """-> (y, labels, front oracle, order, snr_db, model result) of set i of ``name``, computed once and shared."""
    snr, snr_db, order, F, quant = SETS[name][i]
    G = osdx_model.graph(name)[1]
    y, cw = osdx_model.frames(name, snr, F, 7)
    if quant:
        y = quantise(y)
    y = np.ascontiguousarray(y, dtype=F32)
    front = osdx_model.front_oracle(G, y)
    return y, cw, front, order, snr_db, pb(y, front[0], front[3], order, snr_db)


@functools.lru_cache(maxsize=None)
def equal_magnitudes_in(fam, k, n, order, levels, F, seed=11):
    """Caller-made front-end results in the layouts of the family ``fam`` (osd_family): identity permutation, random P', |y'|
    equal over the MRB (levels = 1) or of two distinct values (levels = 2), so that the sums of one weight tie and the visit
    order is the insertion order.  -> dict(y [F, n], perm, parity, order, snr_db, model) for F frames with random hard
    decisions."""
    m = n - k
    rng = np.random.default_rng(seed)
    ys, Gps, perms, pars = [], [], [], []
    for f in range(F):
        Pm = rng.integers(0, 2, (k, m), dtype=np.int64)
        Gp = np.concatenate([np.eye(k, dtype=np.int64), Pm], axis=1)
        p, q = fam.pack_front(np.arange(n), Gp)
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


def equal_magnitudes(name, order, levels, seed=11):
    """equal_magnitudes_in on the shape of ``name`` in the osdx layouts, three frames."""
    k, n = osdx_model.graph(name)[1].shape
    return equal_magnitudes_in(OF.OSDX, k, n, order, levels, 3, seed)


def slots3(k):
    """The frontier slots an order-3 search of k positions needs."""
    return k + (k - 1) * (k - 2) // 2


def tier(k, slots):
    """The smallest slot tier of ``slots`` that holds slots3(k)."""
    return min(t for t in slots if slots3(k) <= t)


@functools.lru_cache(maxsize=None)
def in_turn(name="short", order=3, snr_db=1.0):
    """Four distinct frames for the frames-in-turn test: two full scans (the first two stop-0 frames of set 0 of ``name``) and
    two searches that stop at the first TEP (noiseless codewords at amplitude 0.3: the all-zero TEP costs 0.0, so beta = 0, and
    at this amplitude the threshold of the promising rule lies above cdfH[0]: the rule fires at once).  -> (y [4, n], labels [4, n], model of the four)."""
    y0, cw0, _, o, s, r = case(name, 0)
    assert (o, s) == (order, snr_db)
    full = np.flatnonzero(r["aux"][:, 3] == 0)[:2]
    clean = (F32(0.3) * (F32(1.0) - F32(2.0) * cw0[:2].astype(F32))).astype(F32)
    y = np.ascontiguousarray(np.concatenate([y0[full], clean]), dtype=F32)
    labels = np.concatenate([cw0[full], cw0[:2]])
    front = osdx_model.front_oracle(osdx_model.graph(name)[1], y)
    return y, labels, pb(y, front[0], front[3], order, snr_db)
