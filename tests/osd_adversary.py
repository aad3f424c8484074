"""Host-side crafter of hard inputs for the OSD front end (GF(2) elimination with column exchanges), for the tests.
NumPy only, deterministic for a given seed.

G form (descending reliability, columns of G): a column order that puts dependent columns early -- the supports of rows
of H (every such support is a dependent set of columns of G) in a shuffled order, the row with the fewest unplaced
columns first, and before each new support every unplaced column that is already in the span of the placed ones.  H form
(ascending reliability, columns of H): the same with the supports of rows of G.  The span is kept as a GF(2) basis of
Python-int bitmasks.

An order becomes a frame by re-assigning the magnitudes of a natural AWGN frame: its |y| sorted (descending for G form,
ascending for H form) are laid along the crafted order, each position keeping its own sign -- the search then still sees
realistic error patterns and metrics.  The tie variant gives pairs of adjacent crafted positions one magnitude, so the
"lower index first" rule decides which of the two comes first.

``ge_matrices`` gives arbitrary 64 x 128 matrices for ldpc_osd_ge, rank-deficient ones included.

Nothing here is trusted: the tests read every class claim back from the C oracle's exchange records."""
import numpy as np

F32 = np.float32


def _col_masks(M):
    """Columns of a [m, n] 0/1 matrix as Python ints (bit r = row r)."""
    M = np.asarray(M, dtype=np.int64)
    return [sum(1 << int(r) for r in np.flatnonzero(M[:, c])) for c in range(M.shape[1])]


class _Span:
    """GF(2) span of bitmasks, reduced basis keyed by leading bit."""

    def __init__(self):
        self.basis = {}

    def reduce(self, v):
        while v:
            p = v.bit_length() - 1
            if p not in self.basis:
                return v
            v ^= self.basis[p]
        return 0

    def add(self, v):
        v = self.reduce(v)
        if v:
            self.basis[v.bit_length() - 1] = v
        return v != 0


def crafted_order(cols, supports, rng):
    """A column order (list of n indices) that places dependent columns early.  cols: column bitmasks; supports: lists of
    column indices that are dependent sets (rows of the dual matrix)."""
    n = len(cols)
    sup = [list(s) for s in supports]
    rank_of = {i: r for r, i in enumerate(rng.permutation(len(sup)))}   # the shuffled row order breaks ties
    placed, order, span = set(), [], _Span()

    def place(c):
        placed.add(c)
        order.append(c)
        span.add(cols[c])

    while len(order) < n:
        dep = [c for c in range(n) if c not in placed and span.reduce(cols[c]) == 0]
        if dep:
            place(dep[int(rng.integers(len(dep)))])
            continue
        live = [i for i in range(len(sup)) if any(c not in placed for c in sup[i])]
        if not live:
            rest = [c for c in range(n) if c not in placed]
            for c in rng.permutation(rest):
                place(int(c))
            break
        i = min(live, key=lambda t: (sum(c not in placed for c in sup[t]), rank_of[t]))
        for c in rng.permutation([c for c in sup[i] if c not in placed]):
            place(int(c))
    return order


def frame_along(order, y, descending=True, ties=False):
    """Lay the sorted magnitudes of frame y along ``order`` (position order[r] gets the r-th largest |y| for descending,
    the r-th smallest for ascending); each position keeps its own sign.  ties: positions order[2t] and order[2t+1] share
    one magnitude."""
    y = np.asarray(y, dtype=F32)
    mag = np.sort(np.abs(y))
    if descending:
        mag = mag[::-1]
    if ties:
        mag = np.repeat(mag[0::2], 2)[: len(mag)]
    out = np.empty_like(y)
    sign = np.where(np.signbit(y), F32(-1.0), F32(1.0))
    out[np.asarray(order)] = mag
    return (out * sign).astype(F32)


def g_form_frames(G, H, y, seed, ties=False):
    """Descending-reliability frames for the G-form front end: frame f of y re-ordered along a crafted order of the
    columns of G (dependent sets: supports of rows of H)."""
    rng = np.random.default_rng(seed)
    cols = _col_masks(G)
    sup = [np.flatnonzero(r) for r in np.asarray(H)]
    return np.stack([frame_along(crafted_order(cols, sup, rng), row, True, ties) for row in y])


def h_form_frames(G, H, y, seed, ties=False):
    """Ascending-reliability frames for the H-form front end (hosd_front): columns of H, dependent sets: supports of
    rows of G."""
    rng = np.random.default_rng(seed)
    cols = _col_masks(H)
    sup = [np.flatnonzero(r) for r in np.asarray(G)]
    return np.stack([frame_along(crafted_order(cols, sup, rng), row, False, ties) for row in y])


# ------------------------------------------------------------------------------------------------ arbitrary matrices


def _rank(M):
    s = _Span()
    return sum(s.add(v) for v in _col_masks(np.asarray(M).T))


def _invertible(rng, m):
    while True:
        T = rng.integers(0, 2, size=(m, m))
        if _rank(T) == m:
            return T


def _full_rank(rng, p):
    while True:
        M = (rng.random((64, 128)) < p).astype(np.int64)
        if _rank(M) == 64:
            return M


def _mix_rows(rng, B):
    return _invertible(rng, B.shape[0]).dot(B) % 2


def _only_127(rng):
    """Rows 0..62 = [I_63 | R], row 63 = e_127, rows mixed by a random invertible T: the row space vanishing on columns
    0..62 is {0, e_127}, so columns 63..126 (in the span of columns 0..62) never pivot and step 63 can take its pivot
    only from column 127."""
    B = np.zeros((64, 128), dtype=np.int64)
    B[:63, :63] = np.eye(63, dtype=np.int64)
    B[:63, 63:127] = rng.integers(0, 2, size=(63, 64))
    B[63, 127] = 1
    return _mix_rows(rng, B)


def _only_127_early(rng, j):
    """The 127-only pivot at step j < 63, followed by 63 - j exchanges from the second half: rows 0..j-1 = [I_j | R],
    row j = e_127, rows j+1..63 = unit vectors at columns 64..126 -- columns j..63 lie in the span of columns 0..j-1.
    Rows are not mixed: steps 0..j-1 then change nothing, so row j is still e_127 at step j."""
    B = np.zeros((64, 128), dtype=np.int64)
    B[:j, :j] = np.eye(j, dtype=np.int64)
    B[:j, j:127] = rng.integers(0, 2, size=(j, 127 - j))
    B[j, 127] = 1
    for t, r in enumerate(range(j + 1, 64)):
        B[r, 64 + t] = 1
    return B


def ge_matrices(seed=0):
    """dict class -> list of [64, 128] int64 0/1 matrices for ldpc_osd_ge / the host GE.  Classes whose name starts
    with ``deficient`` have rank < 64."""
    rng = np.random.default_rng(seed)
    out = {}
    out["dense"] = [_full_rank(rng, 0.5) for _ in range(6)]
    out["sparse"] = [_full_rank(rng, 0.06) for _ in range(6)]
    left_zero = np.zeros((64, 128), dtype=np.int64)
    left_zero[:, 64:] = np.eye(64, dtype=np.int64)
    out["left_zero"] = [left_zero, _mix_rows(rng, left_zero)]
    dup = []
    for _ in range(3):
        A = _invertible(rng, 64)
        M = np.zeros((64, 128), dtype=np.int64)
        M[:, 0::2] = A
        M[:, 1::2] = A
        dup.append(M)
        dup.append(_mix_rows(rng, M[:, rng.permutation(128)]))
    out["duplicate_pairs"] = dup
    out["only_127"] = [_only_127(rng) for _ in range(3)] + [_only_127_early(rng, j) for j in (1, 20, 40)]
    deficient63 = []
    for _ in range(3):
        B = _full_rank(rng, 0.5)
        B[63] = rng.integers(0, 2, size=63).dot(B[:63]) % 2
        deficient63.append(_mix_rows(rng, B))
    out["deficient_rank63"] = deficient63
    deficient32 = []
    for _ in range(2):
        B = _full_rank(rng, 0.5)[:32]
        deficient32.append(rng.integers(0, 2, size=(64, 32)).dot(B) % 2)
    out["deficient_rank32"] = deficient32
    zero_row = _full_rank(rng, 0.3)
    zero_row[int(rng.integers(64))] = 0
    out["deficient_zero_row"] = [zero_row]
    return out


def ge_rank(M):
    return _rank(M)


def crafted_sets(G, H, frames=24, seed=2026):
    """The crafted frames the tests share: dict name -> (y [F,128] f32, codewords [F,128]).  ``g`` / ``g_ties``: G form,
    half of the frames from 1.0 dB and half from 2.5 dB; ``h``: H form from the same natural frames."""
    from oracle import np_oracle
    rng = np.random.default_rng(seed)
    ya, ca = np_oracle.make_frames(G, 1.0, frames // 2, rng)
    yb, cb = np_oracle.make_frames(G, 2.5, frames - frames // 2, rng)
    y, cw = np.concatenate([ya, yb]), np.concatenate([ca, cb])
    return dict(g=(g_form_frames(G, H, y, seed + 1), cw), g_ties=(g_form_frames(G, H, y, seed + 2, ties=True), cw),
                h=(h_form_frames(G, H, y, seed + 3), cw))
