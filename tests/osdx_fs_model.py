"""Test helper: the one vectorised CPU oracle of FS-OSD (fs_osd, FS_OSD/fs_testing.py:129-161) for any (k, n) -- every G-form
family's reference, in the style of osdx_model.scan_oracle -- with the planted stop (``planted_stop``) and the span survey
(``spans``) in any family's layouts, and the inputs of the any-shape family's FS tests (ldpc_osdx_fs_search / _decode).

Per weight class the candidates, their Hamming distances and their costs (osdx_model.costs_vectorised: the float32 additions of
np_oracle._weighted_distance_k in the same order) are arrays over the class's TEPs in visit order.  They depend on the frame
only, so a ``FrameScan`` computes each class once and every parameter set (beta, tau_e, tau_psc) reads it.  The sequential rules
of :139-158 are recovered per class as
    first index with HD < tau_e                                                        (the stop, :143-146)
    first minimum among the earlier indices with HD < tau_psc, taken only if strictly below the running best   (:147-152)
which is what a sequential pass keeps: a later candidate replaces the best only with a strictly smaller cost, so the class
leaves the first of its smallest eligible costs behind if that beats the best the class started with.

Branch tags of a frame:
    zero                   the all-zero TEP already has HD < tau_e: nothing is scanned
    bound1 .. bound3       the lower bound of that weight ended the search (:155-158)
    full                   every class up to the order was scanned to its end
    hit1 .. hit3           a tau_e stop inside that class;  hit_late: at rank >= 64 inside its class (not in the first round)
    psc_blocked            a candidate cheaper than the running best was refused because its HD >= tau_psc
    hit_after_improvement  a tau_e stop after the best had moved off the all-zero TEP (the two quirk answers then differ
                           from each other and from order 0)
"""
import functools

import numpy as np

from oracle import np_oracle
from tests import osd_family as OF
from tests import osdx_model

F32 = np.float32


def beta_term(beta, n, k):
    """The library's (float)((double)fs_beta * (double)(n - k)) with fs_beta a float field of ldpc_osd_params.
    np_oracle.fs_osd_frame rounds the Python double beta * (n - k) instead; the two agree for n - k = 64 and can differ by one
    ulp elsewhere (beta = 0.1 with n - k = 13 does), which moves a result only where a bound ties with the best to the bit."""
    return F32(np.float64(F32(beta)) * np.float64(n - k))


@functools.lru_cache(maxsize=None)
def class_supports(k, w):
    """[C(k, w), w] int64: the supports of weight class w in FS visit order (generate_sequential_teps :32-49)."""
    if w == 0:
        return np.zeros((1, 0), np.int64)                     # the all-zero TEP
    return np.asarray(np_oracle.fs_tep_lists(k, w)[w - 1], dtype=np.int64).reshape(-1, w)


def fs_rank(k, support):
    """Rank of ``support`` inside its weight class."""
    sup = class_supports(k, len(support))
    return int(np.flatnonzero((sup == np.asarray(sorted(support))).all(axis=1))[0])


class FrameScan:
    """One frame in the primed domain: hard decisions, and per weight class (computed on first use) HD and cost arrays."""

    def __init__(self, yp, Gp):
        self.yp = np.asarray(yp, dtype=F32)
        self.Gp = np.asarray(Gp, dtype=np.int64)
        self.k, self.n = self.Gp.shape
        self.w = np.abs(self.yp)
        self.hard = np.where(self.yp > 0, 0, 1).astype(np.int64)
        self._G32 = self.Gp.astype(F32)                       # 0/1 sums up to 64: exact in float32, and a BLAS product
        self._cls = {}

    def candidates(self, supports):
        """[T, w] supports -> codewords [T, n] in primed order."""
        supports = np.asarray(supports, dtype=np.int64).reshape(len(supports), -1)
        mrb = np.repeat(self.hard[None, :self.k], len(supports), axis=0)
        for q in range(supports.shape[1]):
            mrb[np.arange(len(supports)), supports[:, q]] ^= 1
        return (mrb.astype(F32).dot(self._G32) % 2).astype(np.int64)

    def evaluate(self, supports):
        """-> (hd [T] int64, cost [T] f32) of the TEPs with these supports: one_tep_compare :58-62."""
        disc = self.candidates(supports) ^ self.hard[None, :]
        return disc.sum(axis=1), osdx_model.costs_vectorised(disc, self.w, self.k)

    def cls(self, w):
        if w not in self._cls:
            self._cls[w] = (class_supports(self.k, w),) + self.evaluate(class_supports(self.k, w))
        return self._cls[w]

    def bound(self, w):
        """acquire_pnc_boundary :22-30: the w least reliable MRB values, ascending position from 0.0f."""
        acc = F32(0)
        for t in range(self.k - w, self.k):
            acc = F32(acc + self.w[t])
        return acc

    def one_tep(self, support):
        """-> (codeword [n] primed order, metric f32, hd) of one TEP of any weight."""
        sup = np.asarray(sorted(support), dtype=np.int64).reshape(1, -1)
        hd, cost = self.evaluate(sup)
        return self.candidates(sup)[0], cost[0], int(hd[0])

    def fs(self, order, beta, tau_e, tau_psc):
        """fs_osd on this frame -> dict(ref = (support, metric, rank), hit = (support, metric, rank) or None, ntep, tags,
        depth = the heaviest weight class entered)."""
        tau_e, tau_psc = F32(tau_e), F32(tau_psc)
        _, hd0, c0 = self.cls(0)
        best, best_sup, best_rank = c0[0], (), 0
        ntep, visited, tags, hit, depth = 1, 1, set(), None, 0
        if F32(hd0[0]) < tau_e:
            tags.add("zero")
        else:
            bt = beta_term(beta, self.n, self.k)
            for w in range(1, order + 1):
                if not F32(self.bound(w) + bt) < best:
                    tags.add(f"bound{w}")
                    break
                depth = w
                sup, hd, cost = self.cls(w)
                stops = np.flatnonzero(hd.astype(F32) < tau_e)
                lim = int(stops[0]) if len(stops) else len(sup)
                ntep += lim + 1 if len(stops) else lim
                elig = hd[:lim].astype(F32) < tau_psc
                c = np.where(elig, cost[:lim], F32(np.inf))
                # the running best every candidate of the class met: the class's starting best and the eligible costs before it
                before = np.minimum(best, np.concatenate([[F32(np.inf)], np.minimum.accumulate(c)[:-1]])) if lim else c
                if np.any(~elig & (cost[:lim] < before)):
                    tags.add("psc_blocked")
                if lim and c.min() < best:
                    j = int(np.argmin(c))                     # the first minimum
                    best, best_sup, best_rank = c[j], tuple(int(x) for x in sup[j]), visited + j
                if len(stops):
                    hit = (tuple(int(x) for x in sup[lim]), cost[lim], visited + lim)
                    tags.add(f"hit{w}")
                    if lim >= 64:
                        tags.add("hit_late")
                    if best_rank != 0:
                        tags.add("hit_after_improvement")
                    break
                visited += len(sup)
            else:
                tags.add("full")
        return dict(ref=(best_sup, best, best_rank), hit=hit, ntep=ntep, tags=tags, depth=depth)


def _pack(bits):
    pad = np.zeros((bits.shape[0], (-bits.shape[1]) % 64), np.uint8)
    return np.packbits(np.concatenate([bits.astype(np.uint8), pad], axis=1), axis=1, bitorder="little").view(np.uint64)


class Batch:
    """Frames y [F, n] in original order with front-end results (perm [F, 128] u8, Gps: list of [I | P'] per frame)."""

    def __init__(self, y, perm, Gps):
        self.y = np.asarray(y, dtype=F32)
        self.k, self.n = np.asarray(Gps[0]).shape
        self.perm = np.asarray(perm)[:, :self.n].astype(np.int64)
        self.scans = [FrameScan(self.y[f][self.perm[f]], Gps[f]) for f in range(len(self.y))]

    def _cw(self, f, support):
        out = np.zeros(self.n, np.uint8)
        out[self.perm[f]] = self.scans[f].one_tep(support)[0]
        return out

    def fs(self, order, beta, tau_e, tau_psc):
        """-> dict of arrays in the layouts of ldpc_osdx_fs_search: cw_ref / metric_ref / best_ref (fs_reference_quirk = 1),
        cw_hit / metric_hit / best_hit (quirk = 0: the stopping candidate where there was a stop, else the same), ntep, hit,
        depth (the heaviest weight class entered) and tags (a list of sets)."""
        F = len(self.scans)
        res = [s.fs(order, beta, tau_e, tau_psc) for s in self.scans]
        out = dict(ntep=np.array([r["ntep"] for r in res], np.int32), hit=np.array([r["hit"] is not None for r in res]),
                   tags=[r["tags"] for r in res], depth=np.array([r["depth"] for r in res]))
        for key in ("ref", "hit"):
            pick = [r["hit"] if key == "hit" and r["hit"] is not None else r["ref"] for r in res]
            out["cw_" + key] = _pack(np.stack([self._cw(f, pick[f][0]) for f in range(F)]))
            out["metric_" + key] = np.array([p[1] for p in pick], F32)
            out["best_" + key] = np.array([p[2] for p in pick], np.int32)
        return out

    def one_tep(self, masks):
        """masks [F] (bit p = flip MRB position p) -> dict(cw [F, words] u64 original order, metric [F] f32, hd [F] i32)."""
        sups = [[p for p in range(self.k) if (int(m) >> p) & 1] for m in masks]
        got = [self.scans[f].one_tep(sups[f]) for f in range(len(masks))]
        return dict(cw=_pack(np.stack([self._cw(f, sups[f]) for f in range(len(masks))])),
                    metric=np.array([g[1] for g in got], F32), hd=np.array([g[2] for g in got], np.int32))


def tag_counts(results):
    """Frames per tag over the union of several ``Batch.fs`` results."""
    out = {}
    for r in results:
        for tags in r["tags"]:
            for t in tags:
                out[t] = out.get(t, 0) + 1
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the inputs of tests/test_gpu_osdx_fs.py (tests/test_osdx_fs_host.py asserts their coverage without a GPU)
# ---------------------------------------------------------------------------------------------------------------------
# code -> (snr, order, [(beta, tau_e, tau_psc), ...]) on osdx_model.frames(code, snr, 192, 7)
# The last set of array_121_60 and of ccsds is an addition to the sets the feature was specified with: under those, none of the
# 15 and 8 frames with a tau_e stop had left the all-zero TEP before it (np_oracle.fs_osd_frame, run frame by frame, says the
# same), so `hit_after_improvement` never occurred on these two codes; with tau_psc = 30 it does, on 12 and 6 frames.
PARITY = {
    "short": (1.0, 3, [(0.1, 3.5, 30), (0.1, 5.5, 9), (0.0, 4.5, 7)]),
    "thin": (0.0, 3, [(0.1, 2.5, 30), (0.0, 3.5, 5)]),
    "ldpc_96_48": (1.5, 2, [(0.1, 4.5, 30), (0.1, 8.5, 14), (0.02, 9.5, 12)]),
    "array_121_60": (1.5, 2, [(0.1, 4.5, 30), (0.02, 10.5, 16), (0.02, 10.5, 30)]),
    "ccsds": (1.5, 2, [(0.1, 6.5, 30), (0.02, 11, 18), (0.02, 11, 30)]),
}
ORDER3_96 = (1.5, 3, [(0.02, 4.5, 30), (0.0, 9.5, 12)])     # 32 frames of ldpc_96_48, seed 13
EVERY_CODE = ("zero", "bound1", "bound2", "full", "hit1", "psc_blocked", "hit_after_improvement")
LONG_CODES = ("ldpc_96_48", "array_121_60", "ccsds")         # these also need hit2 and hit_late; `short` bound3 and hit3


@functools.lru_cache(maxsize=None)
def batch(name, snr, F, seed):
    """-> (y, labels, front oracle, Batch), computed once and shared."""
    G = osdx_model.graph(name)[1]
    y, cw = osdx_model.frames(name, snr, F, seed)
    front = osdx_model.front_oracle(G, y)
    return y, cw, front, Batch(y, front[0], front[3])


@functools.lru_cache(maxsize=None)
def parity_case(name, order3=False):
    """-> (y, labels, front, Batch, order, sets, [Batch.fs per set]) of test 1."""
    snr, order, sets = ORDER3_96 if order3 else PARITY[name]
    y, cw, front, b = batch(name, snr, 32 if order3 else 192, 13 if order3 else 7)
    return y, cw, front, b, order, sets, [b.fs(order, *s) for s in sets]


PLANTED_TAU_E = {3: 3.5, 2: 2.5}


def classes_before(k, weight):
    """The TEPs visited before weight class ``weight``: the all-zero TEP and the lighter classes."""
    return 1 + (k if weight > 1 else 0) + (k * (k - 1) // 2 if weight > 2 else 0)


@functools.lru_cache(maxsize=None)
def planted_stop(fam, k, n, weight, which, tau_e=None, tau_psc=None, seed=5):
    """Caller-made front-end results in the layouts of the family ``fam`` (osd_family) with a tau_e stop (3.5 in class 3, 2.5 in
    class 2) planted at a chosen rank of weight class ``weight`` -- "first" (a rank of its first round), "middle", "last" (the
    last, partial round), or "across" (the support {63, 64} of class 2; ``tau_e`` then as given).  Identity permutation, random
    rows of P' (large mutual distance), y' whose hard decisions make d0 the sum of the support's rows of P': that TEP then has
    HD = weight and, as the model confirms, nothing before it has HD <= weight.  ``tau_psc``: n when None (every candidate is
    eligible, so the reference-quirk answer is a search result).
    -> dict(y [1, n], perm, parity, batch, support, rank, at = the rank in the whole visit order,
            params (order, beta, tau_e, tau_psc))."""
    m = n - k
    sup = class_supports(k, weight)
    cnt = len(sup)
    assert cnt % 64, "the last round must be partial"
    rank = fs_rank(k, (63, 64)) if which == "across" else {"first": 37, "middle": (cnt // 128) * 64 + 21,
                                                           "last": (cnt // 64) * 64 + (cnt % 64) // 2}[which]
    support = tuple(int(x) for x in sup[rank])
    rng = np.random.default_rng(seed)
    P = rng.integers(0, 2, (k, m), dtype=np.int64)
    Gp = np.concatenate([np.eye(k, dtype=np.int64), P], axis=1)
    u0 = rng.integers(0, 2, k, dtype=np.int64)
    hp = (u0.dot(P) + P[list(support)].sum(axis=0)) % 2        # d0 = (u0 . P') ^ hp = the sum of the support's rows
    mag = np.concatenate([np.linspace(0.5, 0.05, k), rng.uniform(0.6, 1.5, m)]).astype(F32)
    y = (np.where(np.concatenate([u0, hp]) == 1, -1.0, 1.0) * mag).astype(F32)[None, :]
    perm, parity = fam.pack_front(np.arange(n), Gp)
    return dict(y=y, perm=perm[None], parity=parity[None], batch=Batch(y, perm[None], [Gp]), support=support, rank=rank,
                at=classes_before(k, weight) + rank,
                params=(weight, 0.0, PLANTED_TAU_E[weight] if tau_e is None else tau_e, float(n) if tau_psc is None else tau_psc))


def planted(k, n, which, seed=5):
    """Test 2: planted_stop in class 3 (tau_e = 3.5, tau_psc = 30) in the osdx layouts: perm [1, 128] u8, parity [1, 64] u64."""
    return planted_stop(OF.OSDX, k, n, 3, which, tau_psc=30.0, seed=seed)


def spans(case, span):
    """-> (winner spans, stopping-candidate spans): the set of span() values over the reference-quirk winners (rank > 0) and over
    the tau_e stopping candidates of every frame and parameter set of a parity_case result."""
    _, _, _, b, order, sets, _ = case
    win, stop = set(), set()
    for s in sets:
        for scan in b.scans:
            r = scan.fs(order, *s)
            if r["ref"][0]:
                win.add(span(r["ref"][0]))
            if r["hit"] is not None and r["hit"][0]:
                stop.add(span(r["hit"][0]))
    return win, stop


PLANTED = [(k, n, which) for (k, n) in ((17, 40), (60, 121)) for which in ("first", "middle", "last")]
PLANTED_CODE = {17: "short", 60: "array_121_60"}
