"""Test helper: min-sum decoding held to its definition on cycle-free Tanner graphs -- NumPy only.

On a forest, min-sum with alpha = 1 and unit weights is dynamic programming: after as many iterations as the longest path
between two bits counts checks, the output at bit i is, in real arithmetic,

    soft[i] = min over codewords with c_i = 1 of sum_{c_j = 1} y_j  -  the same with c_i = 0,

and the hard decision is the ML codeword.  (A check-to-bit message of a subtree is the difference of the two constrained minima
over that subtree; by induction over the depth every message is final once the information of the farthest leaf has arrived.)
One iteration fewer leaves some bit without the farthest leaf's value, so an iteration miscount shows.

  graphs      tree13: 13 bits, 5 checks (degrees 3-4), bit degrees 1-3; forest70: 70 bits, 56 checks, k = 14, one check of
              degree 10, leaves of degree 1 -- a frame of more than one 64-bit word
  diameter    the longest bit-to-bit path in check hops, by breadth-first search
  exact_soft  the definition by enumeration of all 2^k codewords, float64
  bound       n u sum_j |y_j| per frame: every soft value is a signed sum of at most n distinct channel values formed by at
              most n - 1 float32 additions; min, abs and sign are exact
"""
import numpy as np

U = 2.0 ** -24


def tree13():
    """-> H [5, 13]."""
    checks = [(0, 1, 2, 3), (3, 4, 5), (5, 6, 7, 8), (3, 9, 10), (10, 11, 12)]
    H = np.zeros((len(checks), 13), np.int64)
    for r, bits in enumerate(checks):
        H[r, list(bits)] = 1
    return H


def forest70(seed=4):
    """-> H [56, 70]: one check on bits 0..9, then 5 checks of degree 3 and 50 of degree 2, each hung on one bit that exists
    already and bringing its other bits new -- so the graph stays a tree and k = 70 - 56 = 14."""
    rng = np.random.default_rng(seed)
    rows, n = [list(range(10))], 10
    for deg in rng.permutation([3] * 5 + [2] * 50):
        rows.append([int(rng.integers(n))] + list(range(n, n + deg - 1)))
        n += deg - 1
    H = np.zeros((len(rows), n), np.int64)
    for r, bits in enumerate(rows):
        H[r, bits] = 1
    assert H.shape == (56, 70)
    return H


def is_forest(H):
    """No cycle: the edges number bits + checks - components (union-find over the bipartite graph)."""
    m, n = H.shape
    parent = list(range(n + m))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for r, c in np.argwhere(H):
        a, b = find(int(c)), find(n + int(r))
        if a == b:
            return False
        parent[a] = b
    return True


def diameter(H):
    """The longest path between two bits of one component, counted in checks."""
    m, n = H.shape
    nbr = [[n + int(r) for r in np.flatnonzero(H[:, c])] for c in range(n)] + [[int(c) for c in np.flatnonzero(H[r])] for r in range(m)]
    best = 0
    for s in range(n):
        dist = {s: 0}
        todo = [s]
        while todo:
            nxt = []
            for a in todo:
                for b in nbr[a]:
                    if b not in dist:
                        dist[b] = dist[a] + 1
                        nxt.append(b)
            todo = nxt
        best = max(best, max(d for v, d in dist.items() if v < n) // 2)
    return best


def codebook(H):
    """All codewords of a forest's H = every solution of H c = 0, found without an elimination: the 2^n vectors are too many,
    so bits are fixed check by check -- each check of a forest met in breadth-first order determines one new bit from the
    others.  -> [2^k, n] int8."""
    m, n = H.shape
    assert is_forest(H)
    done_checks, order, known = set(), [], set()
    free, solved = [], []                                     # free bits; (bit, check) pairs: bit = sum of the check's other bits
    while len(known) < n:
        root = min(set(range(n)) - known)
        free.append(root)
        known.add(root)
        todo = [root]
        while todo:
            b = todo.pop()
            for r in np.flatnonzero(H[:, b]):
                if int(r) in done_checks:
                    continue
                done_checks.add(int(r))
                new = [int(c) for c in np.flatnonzero(H[r]) if int(c) not in known]
                for c in new[:-1]:
                    free.append(c)
                if new:
                    solved.append((new[-1], int(r)))
                known.update(new)
                todo.extend(new)
    k = len(free)
    assert k == n - m and k <= 16
    book = np.zeros((1 << k, n), np.int8)
    book[:, free] = (np.arange(1 << k)[:, None] >> np.arange(k)[None, :]) & 1
    for bit, r in solved:                                     # in discovery order: the check's other bits are set already
        others = [int(c) for c in np.flatnonzero(H[r]) if int(c) != bit]
        book[:, bit] = book[:, others].sum(axis=1) & 1
    assert not (book.astype(np.int64).dot(H.T) % 2).any()
    return book


def exact_soft(book, y):
    """-> (soft64 [F, n], ml [F, n] the ML codewords) of frames y [F, n]."""
    y64 = np.asarray(y, dtype=np.float64)
    cost = book.astype(np.float64).dot(y64.T)                 # [2^k, F]: sum of y over the ones of each codeword
    soft = np.empty_like(y64)
    for i in range(book.shape[1]):
        one = book[:, i] == 1
        soft[:, i] = cost[one].min(axis=0) - cost[~one].min(axis=0)
    return soft, book[np.argmin(cost, axis=0)].astype(np.int64)


def bound(y):
    """n u sum_j |y_j| per frame -> [F, 1]."""
    y64 = np.abs(np.asarray(y, dtype=np.float64))
    return (y.shape[1] * U * y64.sum(axis=1))[:, None]


def frames(H, F, sigma=1.2, seed=21):
    """Random codewords of H over BPSK + noise of deviation sigma -> y [F, n] float32."""
    book = codebook(H)
    rng = np.random.default_rng(seed)
    cw = book[rng.integers(len(book), size=F)].astype(np.float64)
    return (1.0 - 2.0 * cw + sigma * rng.standard_normal(cw.shape)).astype(np.float32)


def check(H, y, soft, hard, fail, book=None):
    """A decoder's outputs on the forest H after at least diameter(H) iterations.  -> (frames decided, the largest
    |soft - soft64|, the largest bound)."""
    book = codebook(H) if book is None else book
    soft64, ml = exact_soft(book, y)
    b = bound(y)
    diff = np.abs(np.asarray(soft, dtype=np.float64) - soft64)
    assert (diff <= b).all(), f"soft values differ from the definition by {diff.max()!r}, bound {b.max()!r}"
    clear = np.abs(soft64) > b
    assert np.array_equal(np.asarray(hard)[clear], ml[clear]), "a hard decision is not the ML codeword's"
    decided = clear.all(axis=1)
    assert not np.asarray(fail)[decided].any(), "fail set on a frame whose decisions are the ML codeword"
    return int(decided.sum()), float(diff.max()), float(b.max())
