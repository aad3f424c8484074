"""Test helper: the OSD operations held to their mathematical definitions -- NumPy only, float64 and integers.

Nothing here runs an elimination, reads a TEP table or imports a model: a result is checked against the code (H, G) and the
channel values alone, so a misreading that a kernel shares with its CPU model does not pass.

  order          rank_desc / rank_asc: the total order of the positions (f32 magnitudes compared as integers, ties to the
                 lower index)
  G-form front   front_g: criteria (a)-(d) on (perm, P') -- they determine both completely
  H-form front   front_h: the dual statements on (lri, uidx, M)
  searches       GFrame / HFrame: the candidate set by plain enumeration, the float64 metric; search / pruned: the assertions
                 on a reported (codeword, metric, ntep)
  ML             codebook / ml: all 2^k codewords for k <= 16
  symmetry       flip: y * (-1)^c, exactly

Every failure is a ``Violation`` that names its criterion, so the mutation tests can tell that a mutant was rejected for the
reason it was built for.
"""
import functools
import itertools

import numpy as np

U = 2.0 ** -24                                               # unit roundoff of float32


class Violation(AssertionError):
    def __init__(self, criterion, detail=""):
        super().__init__(f"criterion {criterion}: {detail}")
        self.criterion = criterion


def _need(ok, criterion, detail=""):
    if not ok:
        raise Violation(criterion, detail() if callable(detail) else detail)


def gamma(n):
    """gamma_{n-1} = (n-1)u / (1 - (n-1)u): the relative error bound of a float32 sum of n non-negative terms in any order
    (Higham, Accuracy and Stability of Numerical Algorithms, 4.2: |fl(sum) - sum| <= gamma_{n-1} sum |x_i|)."""
    t = (n - 1) * U
    return t / (1.0 - t)


def gap_bound(n):
    """Two sums that differ by more than this, relative to the smaller, keep their order in float32 whatever the order of
    the additions: fl(a) <= a(1+g) < b(1-g) <= fl(b) iff b/a > (1+g)/(1-g), i.e. (b-a)/a > 2g/(1-g)."""
    g = gamma(n)
    return 2.0 * g / (1.0 - g)


# ---------------------------------------------------------------------------------------------------------------------
# the order of the positions
# ---------------------------------------------------------------------------------------------------------------------
def _keys(y):
    return np.abs(np.asarray(y, dtype=np.float32)).view(np.uint32).astype(np.int64)


def rank_desc(y):
    """-> (rho [n], order [n]): rho[i] = rank of position i in DESCENDING |y|, order = its inverse.  Magnitudes of finite
    float32 values compare like their bit patterns as integers; equal magnitudes: the lower index first."""
    key = _keys(y)
    order = np.lexsort((np.arange(len(key)), -key))
    rho = np.empty(len(key), np.int64)
    rho[order] = np.arange(len(key))
    return rho, order


def rank_asc(y):
    """rank_desc for ASCENDING |y| (the H form), ties to the lower index as well."""
    key = _keys(y)
    order = np.lexsort((np.arange(len(key)), key))
    rho = np.empty(len(key), np.int64)
    rho[order] = np.arange(len(key))
    return rho, order


def hard_bits(y):
    """The hard decision: 0 iff y > 0 -- so +0.0 and -0.0 are both a 1."""
    return np.where(np.asarray(y) > 0, 0, 1).astype(np.int64)


def flip(y, c):
    """y * (-1)^c exactly: the sign bit of every position where c = 1 is inverted, nothing is rounded."""
    y = np.asarray(y, dtype=np.float32)
    return np.where(np.asarray(c).astype(bool), -y, y).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# G-form front end
# ---------------------------------------------------------------------------------------------------------------------
def front_g(H, y, perm, P, nswaps=None):
    """One frame's (perm [n], P' [k, n-k]) against the definition of the most reliable basis.

      (a) perm is a permutation of 0..n-1
      (b) rho increases along perm[:k] and along perm[k:]
      (c) every row [e_r | P'_r], put back into original bit order, satisfies H c = 0
      (d) P'[r][c] = 1 implies rho(perm[r]) < rho(perm[k+c])

    Proof.  (c) gives k codewords that are independent on perm[:k], so perm[:k] is an information set and [I | P'] its unique
    systematic generator.  By (d) column perm[k+c] is a combination of strictly more reliable basis columns, so the greedy
    scan in rho order rejects it; a basis that greedy never leaves is the greedy one, and under a total order the greedy
    basis of a matroid is unique.  (a), (b) then fix the order inside both parts: perm and P' are determined.

    ``nswaps`` is not definitional: only nswaps == 0 <=> perm[:k] is the first k positions of the sort."""
    H = np.asarray(H, dtype=np.int64)
    n = H.shape[1]
    perm = np.asarray(perm, dtype=np.int64)
    P = np.asarray(P, dtype=np.int64)
    k = P.shape[0]
    _need(perm.shape == (n,) and P.shape == (k, n - k), "a", lambda: f"shapes {perm.shape} {P.shape}")
    _need(np.array_equal(np.sort(perm), np.arange(n)), "a", "perm is no permutation")
    _need(np.isin(P, (0, 1)).all(), "a", "P' holds other values than 0 and 1")
    rho, order = rank_desc(y)
    rm, rp = rho[perm[:k]], rho[perm[k:]]
    _need(np.all(np.diff(rm) > 0), "b", "the MRB part is out of order")
    _need(np.all(np.diff(rp) > 0), "b", "the parity part is out of order")
    rows = np.zeros((k, n), np.int64)
    rows[:, perm] = np.concatenate([np.eye(k, dtype=np.int64), P], axis=1)
    bad = (H.dot(rows.T) % 2).any(axis=0)
    _need(not bad.any(), "c", lambda: f"rows {np.flatnonzero(bad)[:8].tolist()} are no codewords")
    late = (P == 1) & (rm[:, None] >= rp[None, :])
    _need(not late.any(), "d", lambda: f"not greedy at (row, column) {np.argwhere(late)[:4].tolist()}")
    if nswaps is not None:
        _need((int(nswaps) == 0) == np.array_equal(perm[:k], order[:k]), "nswaps", f"nswaps = {int(nswaps)}")


# ---------------------------------------------------------------------------------------------------------------------
# H-form front end
# ---------------------------------------------------------------------------------------------------------------------
def front_h(G, order_llr, lri, uidx, M):
    """One frame's (lri [n], uidx [n], M [m, k]) of the H form, m = n - k = rank(H): the least reliable basis of the columns
    of H, in ASCENDING |order_llr|.

      (sort) lri is the ascending order, ties to the lower index
      (a)    lri[uidx] is a permutation
      (b)    the MRB part uidx[m:] ascends (the LRB part is in whatever order it comes)
      (c)    every row [e_r | M_r], put back into original bit order, is orthogonal to every row of G
      (d)    M[r][j] = 1 implies uidx[r] < uidx[m + j]

    Proof.  (c) gives m independent vectors of the dual code, which has dimension m: [I | M] is a parity-check matrix with
    unit columns on the LRB.  Column m+j of it is then the combination of the LRB columns r with M[r][j] = 1, by (d) all less
    reliable: the greedy scan in ascending order rejects every MRB column, so the LRB is the (unique) greedy basis."""
    G = np.asarray(G, dtype=np.int64)
    k, n = G.shape
    m = n - k
    lri, uidx, M = np.asarray(lri, dtype=np.int64), np.asarray(uidx, dtype=np.int64), np.asarray(M, dtype=np.int64)
    _need(lri.shape == (n,) and uidx.shape == (n,) and M.shape == (m, k), "a", lambda: f"shapes {lri.shape} {uidx.shape} {M.shape}")
    _need(np.array_equal(lri, rank_asc(order_llr)[1]), "sort", "lri is not the ascending sort")
    _need(np.array_equal(np.sort(uidx), np.arange(n)), "a", "uidx is no permutation")
    _need(np.isin(M, (0, 1)).all(), "a", "M holds other values than 0 and 1")
    perm = lri[uidx]
    _need(np.all(np.diff(uidx[m:]) > 0), "b", "the MRB part is out of order")
    rows = np.zeros((m, n), np.int64)
    rows[:, perm] = np.concatenate([np.eye(m, dtype=np.int64), M], axis=1)
    bad = (G.dot(rows.T) % 2).any(axis=0)
    _need(not bad.any(), "c", lambda: f"rows {np.flatnonzero(bad)[:8].tolist()} are no parity checks")
    late = (M == 1) & (uidx[:m, None] >= uidx[None, m:])
    _need(not late.any(), "d", lambda: f"not greedy at (row, column) {np.argwhere(late)[:4].tolist()}")


# ---------------------------------------------------------------------------------------------------------------------
# candidate sets by plain enumeration
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def patterns(k, order):
    """Every subset of at most ``order`` of the k MRB positions as a row of a [T, k] float32 0/1 matrix."""
    order = min(order, k)
    sets = [s for w in range(order + 1) for s in itertools.combinations(range(k), w)]
    E = np.zeros((len(sets), k), np.float32)
    for w in range(1, order + 1):
        rows = [t for t, s in enumerate(sets) if len(s) == w]
        E[np.repeat(rows, w), np.concatenate([sets[t] for t in rows])] = 1
    E.setflags(write=False)
    return E


def _mod2(a):
    return (np.rint(a).astype(np.int64)) & 1


class GFrame:
    """One frame of a G-form search on a front end that front_g accepted: positions in the order of perm, MRB first."""

    def __init__(self, H, y, perm, P):
        self.H = np.asarray(H, dtype=np.int64)
        self.perm = np.asarray(perm, dtype=np.int64)
        self.P = np.asarray(P, dtype=np.int64)
        self.k, self.n = self.P.shape[0], len(self.perm)
        yp = np.asarray(y, dtype=np.float32)[self.perm]
        self.hard = hard_bits(yp)
        self.mag = np.abs(yp).astype(np.float64)
        self._of_order = {}

    def order_metrics(self, order):
        """metrics(patterns(k, order)), kept: several results of one frame are held to the same set."""
        if order not in self._of_order:
            self._of_order[order] = self.metrics(patterns(self.k, order))
        return self._of_order[order]

    def metrics(self, E):
        """The float64 metric of every candidate hard_MRB + e, e a row of E [T, k]: sum of |y_i| where it differs from the
        hard decisions.  (float32 products of 0/1 matrices: exact below 2^24 terms.)"""
        E = np.asarray(E, dtype=np.float32)
        mrb = _mod2(E + self.hard[None, :self.k])
        par = _mod2(mrb.astype(np.float32).dot(self.P.astype(np.float32)))
        disc = np.concatenate([_mod2(E), par ^ self.hard[None, self.k:]], axis=1)
        return disc.astype(np.float64).dot(self.mag)

    def codeword(self, e):
        """The candidate hard_MRB + e in ORIGINAL bit order."""
        mrb = self.hard[:self.k] ^ np.asarray(e, dtype=np.int64)
        cw = np.zeros(self.n, np.int64)
        cw[self.perm] = np.concatenate([mrb, mrb.dot(self.P) % 2])
        return cw

    def locate(self, cw, order):
        """A reported codeword (bits in ORIGINAL order) -> (its MRB flips e [k], its float64 metric).  It must be a codeword
        and differ from the hard decisions in at most ``order`` MRB places."""
        cw = np.asarray(cw, dtype=np.int64)
        _need(cw.shape == (self.n,) and np.isin(cw, (0, 1)).all(), "codeword", "shape or values")
        _need(not (self.H.dot(cw) % 2).any(), "codeword", "H c != 0")
        cp = cw[self.perm]
        e = cp[:self.k] ^ self.hard[:self.k]
        _need(int(e.sum()) <= order, "member", lambda: f"{int(e.sum())} MRB flips at order {order}")
        _need(np.array_equal(cp[self.k:], cp[:self.k].dot(self.P) % 2), "member", "parity part is not the encoding of the MRB part")
        return e, float((cp ^ self.hard).astype(np.float64).dot(self.mag))


class HFrame:
    """One frame of an H-form block scan on a front end that front_h accepted: positions in the order of lri[uidx], LRB
    first.  order_llr gives the starting MRB hard decisions, metric_llr the hard decisions and weights of the metric."""

    def __init__(self, G, order_llr, metric_llr, lri, uidx, M):
        self.G = np.asarray(G, dtype=np.int64)
        self.k, self.n = self.G.shape
        self.m = self.n - self.k
        self.perm = np.asarray(lri, dtype=np.int64)[np.asarray(uidx, dtype=np.int64)]
        self.M = np.asarray(M, dtype=np.int64)
        self.start = hard_bits(np.asarray(order_llr, dtype=np.float32)[self.perm])[self.m:]
        yo = np.asarray(metric_llr, dtype=np.float32)[self.perm]
        self.hard = hard_bits(yo)
        self.mag = np.abs(yo).astype(np.float64)

    def candidates(self, E):
        E = np.asarray(E, dtype=np.float32)
        mrb = _mod2(E + self.start[None, :])
        lrb = _mod2(mrb.astype(np.float32).dot(self.M.T.astype(np.float32)))
        return np.concatenate([lrb, mrb], axis=1)

    def metrics(self, E):
        return (self.candidates(E) ^ self.hard[None, :]).astype(np.float64).dot(self.mag)


# ---------------------------------------------------------------------------------------------------------------------
# assertions on a search result
# ---------------------------------------------------------------------------------------------------------------------
def _rel_gap(m64, skip):
    """The relative gap between the minimum of m64 and the smallest value that belongs to another candidate than ``skip``."""
    lo = float(m64.min())
    rest = np.delete(m64, skip)
    up = float(rest.min()) if len(rest) else np.inf
    if up == lo:
        return 0.0
    return (up - lo) / lo if lo > 0 else np.inf


def metric_close(metric, m64, n, criterion="metric"):
    """|metric_f32 - m64| <= gamma m64 -> the relative difference."""
    g = gamma(n)
    diff = abs(float(metric) - m64)
    _need(diff <= g * m64, criterion, lambda: f"reported {float(metric)!r}, float64 {m64!r}, bound {g * m64!r}")
    return diff / m64 if m64 > 0 else 0.0


def search(fr, order, cw, metric, ntep=None, exact=False):
    """A conventional order-p result (cw in original bit order, metric f32, ntep) on the GFrame ``fr``.

      codeword / member   the result is a codeword of the order-p candidate set
      ntep                the size of that set
      metric              |metric_f32 - m64(result)| <= gamma m64(result)
      optimum             m64(result) <= m64_min (1 + gamma) / (1 - gamma)
      argmin              the result is the float64 argmin whenever the runner-up is further than gap_bound(n) away

    ``exact`` (inputs on a grid where every sum is exact): the metric equals the minimum and the result is a minimiser.
    -> dict(skipped: inside the gap, gap, err: relative metric difference, bound: gamma)."""
    E = patterns(fr.k, order)
    m64 = fr.order_metrics(order)
    e, mine = fr.locate(cw, order)
    if ntep is not None:
        _need(int(ntep) == len(E), "ntep", f"{int(ntep)} reported, the set holds {len(E)}")
    g = gamma(fr.n)
    lo = float(m64.min())
    err = metric_close(metric, mine, fr.n)
    _need(mine <= lo * (1 + g) / (1 - g), "optimum", lambda: f"result {mine!r}, minimum {lo!r}")
    arg = int(np.argmin(m64))
    gap = _rel_gap(m64, arg)
    if exact:
        _need(mine == lo and float(metric) == lo, "exact", lambda: f"result {mine!r}, reported {float(metric)!r}, minimum {lo!r}")
    skipped = not exact and not gap > gap_bound(fr.n)          # exact: ties are the point, "a minimiser" is asserted above
    if not exact and not skipped:
        _need(np.array_equal(e, _mod2(E[arg])), "argmin", lambda: f"result {mine!r}, minimum {lo!r}, gap {gap!r}")
    return dict(skipped=skipped, gap=np.inf if exact else gap, err=err, bound=g, optimum=lo, mine=mine)


def pruned(fr, order, cw, metric, full=False):
    """An FS / PB result: a codeword of the order-p set, its reported metric within gamma of the recomputation and not below
    the order-p optimum; ``full`` (a scan that no rule stopped): it reaches the optimum within the bound."""
    m64 = fr.order_metrics(order)
    _, mine = fr.locate(cw, order)
    g = gamma(fr.n)
    lo = float(m64.min())
    err = metric_close(metric, mine, fr.n)
    _need(float(metric) >= lo * (1 - g), "bound", lambda: f"reported {float(metric)!r} below the optimum {lo!r}")
    if full:
        _need(mine <= lo * (1 + g) / (1 - g), "optimum", lambda: f"full scan {mine!r}, minimum {lo!r}")
    return dict(err=err, bound=g, optimum=lo, mine=mine)


def block_scan(fr, blocks, block_min, metric=None, cw=None, exact=False):
    """An H-form block scan on the HFrame ``fr``: ``blocks`` the pattern matrices [N_b, k] of the path, block_min [B] f32 the
    reported minima.  Each float32 sum is within gamma of its float64 value, so the smallest float32 sum lies within gamma of
    the smallest float64 one: that holds every block minimum and the overall metric.  The codeword (original bit order) is
    a candidate of some block and reaches the overall minimum within the bound."""
    g = gamma(fr.n)
    lows, worst = [], 0.0
    for b, E in enumerate(blocks):
        if not len(E):
            continue
        lo = float(fr.metrics(E).min())
        lows.append(lo)
        got = float(block_min[b])
        _need(abs(got - lo) <= g * lo, "block_min",
              lambda: f"block {b}: reported {got!r}, float64 {lo!r}")
        if exact:
            _need(got == lo, "exact", lambda: f"block {b}: reported {got!r}, float64 {lo!r}")
        worst = max(worst, abs(got - lo) / lo if lo > 0 else 0.0)
    best = min(lows)
    if metric is not None:
        _need(abs(float(metric) - best) <= g * best, "metric", lambda: f"reported {float(metric)!r}, float64 {best!r}")
    if cw is not None:
        cp = np.asarray(cw, dtype=np.int64)[fr.perm]
        found = any(len(E) and (fr.candidates(E) == cp[None, :]).all(axis=1).any() for E in blocks)
        _need(found, "member", "the codeword is in no block of the path")
        mine = float((cp ^ fr.hard).astype(np.float64).dot(fr.mag))
        _need(mine <= best * (1 + g) / (1 - g), "optimum", lambda: f"result {mine!r}, minimum {best!r}")
    return dict(err=worst, bound=g, optimum=best)


# ---------------------------------------------------------------------------------------------------------------------
# maximum likelihood by enumeration
# ---------------------------------------------------------------------------------------------------------------------
def codebook(G):
    """All 2^k codewords of G [k, n], k <= 16, as a [2^k, n] int8 matrix."""
    G = np.asarray(G, dtype=np.int64)
    k = G.shape[0]
    assert k <= 16
    msgs = (np.arange(1 << k)[:, None] >> np.arange(k)[None, :]) & 1
    return (msgs.dot(G) % 2).astype(np.int8)


def ml(book, y):
    """-> (the ML metric of frame y in float64: min over the codebook of sum |y_i| [c_i != hard_i], the index of a
    minimiser, the relative gap to the runner-up)."""
    y = np.asarray(y, dtype=np.float32)
    m64 = (book ^ hard_bits(y)[None, :].astype(np.int8)).astype(np.float64).dot(np.abs(y).astype(np.float64))
    arg = int(np.argmin(m64))
    return float(m64[arg]), arg, _rel_gap(m64, arg)


def ml_bound(fr, book, y, cw, metric, order):
    """Every OSD result has a metric >= the ML one, within the bound; at order >= k the result is the ML codeword (outside
    the gap)."""
    lo, arg, gap = ml(book, y)
    g = gamma(fr.n)
    _need(float(metric) >= lo * (1 - g), "ml", lambda: f"reported {float(metric)!r} below ML {lo!r}")
    if order >= fr.k:
        mine = float((np.asarray(cw, dtype=np.int64) ^ hard_bits(y)).astype(np.float64).dot(np.abs(np.asarray(y, dtype=np.float64))))
        _need(mine <= lo * (1 + g) / (1 - g), "ml", lambda: f"order >= k: result {mine!r}, ML {lo!r}")
        if gap > gap_bound(fr.n):
            _need(np.array_equal(np.asarray(cw, dtype=np.int64), book[arg].astype(np.int64)), "ml", "order >= k: not the ML codeword")
    return lo


# ---------------------------------------------------------------------------------------------------------------------
# a whole batch, with the figures a test prints
# ---------------------------------------------------------------------------------------------------------------------
class Tally:
    """Frames checked, frames skipped as near-ties (at most 2 %: asserted by done()), the smallest runner-up gap, the worst
    relative metric difference next to its bound."""

    def __init__(self, name):
        self.name, self.frames, self.skipped, self.gap, self.err, self.bound = name, 0, 0, np.inf, 0.0, 0.0

    def add(self, res):
        self.frames += 1
        self.skipped += int(res.get("skipped", False))
        self.gap = min(self.gap, res.get("gap", np.inf))
        self.err = max(self.err, res["err"])
        self.bound = res["bound"]

    def done(self):
        print(f"[definition] {self.name}: frames {self.frames}, near-tie skips {self.skipped}, smallest gap {self.gap:.3g} "
              f"(needs > {2 * self.bound / (1 - self.bound):.3g}), worst metric difference {self.err:.3g} (bound {self.bound:.3g})")
        _need(self.frames > 0 and self.skipped <= 0.02 * self.frames, "skips", f"{self.skipped} of {self.frames} frames inside the gap")
        return self
