"""Step pattern of the OSD front end's GF(2) elimination (ge_columns, csrc/ldpc_wave.h), counted on the host, and the crafted
inputs of tests/test_gpu_ge_known_steps.py.  NumPy only.

``pattern(M)`` replays full_gf2elim on a 64 x 128 matrix whose columns are already in elimination order, with the
bookkeeping of the two short cuts of profiles/ge_known/README.md, and says per step which kind it was:

  trivial     the pivot column arrived as a unit vector e_k, no column exchange has happened yet and row k has not been a
              pivot row: one candidate row, nothing to eliminate
  stale       the column arrived as e_k, no column exchange yet, but row k was taken by an earlier step
  barred      the column arrived as a unit vector but a column exchange came before it
  row_exchange  the pivot row was not at logical position i; ``known`` counts those in which position i had never received a
              displaced row, so its row-map entry is still the initial one
  col_exchanges (step, column) pairs, as the reference records them

Its reduced matrix and exchange list are what c_oracle.gf2elim gives -- the tests assert that, so the counts are statements
about the oracle's own elimination, not about a second implementation."""
import numpy as np

F32 = np.float32


def pattern(M):
    M = (np.asarray(M, dtype=np.int64) & 1).copy()
    k, n = M.shape
    unit_row = [int(np.flatnonzero(M[:, c])[0]) if M[:, c].sum() == 1 else -1 for c in range(k)]
    rows = list(range(k))          # logical position -> physical row
    used = set()
    moved = set()
    exchanged = False
    out = dict(trivial=[], stale=[], barred=[], row_exchange=[], known=[], col_exchanges=[], deficient=False)
    for i in range(k):
        flagged = unit_row[i] >= 0
        if flagged and not exchanged and unit_row[i] not in used:
            assert M[:, i].sum() == 1 and M[unit_row[i], i] == 1          # such a column is still e_k when its step comes
            out["trivial"].append(i)
        elif flagged and not exchanged:
            out["stale"].append(i)
        elif flagged:
            out["barred"].append(i)
        cand = [l for l in range(i, k) if M[rows[l], i]]
        if not cand:
            pri = rows[i]
            cols = [c for c in range(i, n) if M[pri, c]]
            if not cols:
                out["deficient"] = True
                return out
            c = cols[0]
            M[:, [i, c]] = M[:, [c, i]]
            out["col_exchanges"].append((i, c))
            exchanged = True
            cand = [i]
        r = cand[0]
        if r != i:
            out["row_exchange"].append(i)
            if i not in moved:
                out["known"].append(i)
            rows[i], rows[r] = rows[r], rows[i]
            moved.add(r)
        pr = rows[i]
        used.add(pr)
        col = M[:, i].copy()
        col[pr] = 0
        if col.any():
            hit = np.flatnonzero(M[pr])
            M[:, hit] ^= col[:, None]
    out["reduced"] = M[rows]
    return out


def summary(p):
    first = p["col_exchanges"][0][0] if p["col_exchanges"] else None
    return dict(trivial=len(p["trivial"]), stale=len(p["stale"]), barred=len(p["barred"]), row_exchanges=len(p["row_exchange"]),
                known=len(p["known"]), col_exchanges=len(p["col_exchanges"]), first_exchange=first)


def sorted_matrix(G, y):
    """G with its columns in the front end's order: descending |y|, ties -> lower index."""
    order = np.argsort(-np.abs(np.asarray(y, dtype=F32)).astype(np.float64), kind="stable")
    return np.asarray(G)[:, order], order


def unit_columns(G):
    """(ucol[k] = the column of G that is e_k, the other columns) -- G = [P | I] has one unit column per row."""
    G = np.asarray(G)
    ucol = np.full(G.shape[0], -1)
    for c in np.flatnonzero(G.sum(axis=0) == 1):
        ucol[int(np.flatnonzero(G[:, c])[0])] = c
    assert (ucol >= 0).all()
    return ucol, np.setdiff1d(np.arange(G.shape[1]), ucol)


def frame_along(order, y):
    """Frame y with its magnitudes laid along ``order`` in descending order (position order[r] gets the r-th largest |y|);
    every position keeps its own sign.  The magnitudes must be distinct."""
    y = np.asarray(y, dtype=F32)
    mag = np.sort(np.abs(y))[::-1]
    assert len(np.unique(mag)) == len(mag)
    out = np.empty_like(y)
    out[np.asarray(order)] = mag
    return (out * np.where(np.signbit(y), F32(-1.0), F32(1.0))).astype(F32)


def _dependent_order(G, H, t, rng):
    """A column order in which the support of a row of H ends at sorted position t: column t then lies in the span of the
    columns before it."""
    sup = rng.permutation(np.flatnonzero(np.asarray(H)[int(rng.integers(len(H)))]))
    rest = rng.permutation(np.setdiff1d(np.arange(128), sup))
    return np.concatenate([rest[:t + 1 - len(sup)], sup, rest[t + 1 - len(sup):]])


def first_exchange_order(G, H, t, seed):
    """A column order of G whose FIRST column exchange falls at step t (t + 1 >= the weight of a row of H), found by drawing
    dependent orders until the replay says so.  Deterministic for a seed."""
    rng = np.random.default_rng(seed)
    for _ in range(2000):
        order = _dependent_order(G, H, t, rng)
        p = pattern(np.asarray(G)[:, order])
        if p["col_exchanges"] and p["col_exchanges"][0][0] == t:
            return order
    raise AssertionError("no order with its first exchange at step %d" % t)


def orders(G, H, seed=7411):
    """dict name -> column order (128) of the crafted front-end cases."""
    rng = np.random.default_rng(seed)
    ucol, dense = unit_columns(G)
    out = {}
    out["units_first"] = np.concatenate([rng.permutation(ucol), rng.permutation(dense)])
    out["units_last"] = np.concatenate([rng.permutation(dense), rng.permutation(ucol)])
    u, d = rng.permutation(ucol), rng.permutation(dense)
    out["alternating"] = np.stack([u, d], axis=1).reshape(-1)
    out["units_descending"] = np.concatenate([ucol[::-1], rng.permutation(dense)])
    out["units_rotated"] = np.concatenate([np.roll(ucol, -1), rng.permutation(dense)])     # e_1, ..., e_63, e_0
    out["units_ascending"] = np.concatenate([ucol, rng.permutation(dense)])
    # a dense column first; its pivot row is its lowest row k; then e_k, whose note is stale by then
    d0 = int(dense[0])
    k0 = int(np.flatnonzero(np.asarray(G)[:, d0])[0])
    others = rng.permutation(np.setdiff1d(np.arange(128), [d0, ucol[k0]]))
    out["stale_unit"] = np.concatenate([[d0, ucol[k0]], others])
    for t in (31, 32, 47, 63):
        out["first_exchange_%d" % t] = first_exchange_order(G, H, t, seed + t)
    return out


def exchange_matrix(t, rng):
    """64 x 128 matrix for ldpc_osd_ge whose first column exchange falls at step t (any t in 0..63), with unit columns -- trivial
    candidates -- behind it, and for t < 63 a second exchange at step 63 that takes its column from the parity half.
    Columns 0..63 are e_c, except column t (a copy of e_0, or the zero column for t = 0: dependent on what came before) and
    column 63 = e_t, which step t exchanges in; step 63 then finds e_0 / the zero column and must go to columns 64..127."""
    M = np.zeros((64, 128), dtype=np.int64)
    M[:, :64] = np.eye(64, dtype=np.int64)
    if t < 63:
        M[:, 63] = M[:, t]
    M[:, t] = 0
    if t:
        M[0, t] = 1
    M[:, 64:] = rng.integers(0, 2, size=(64, 64))
    M[63, 64 + int(rng.integers(1, 64))] = 1          # row 63 has a 1 in the parity half, not in its first column
    M[63, 64] = 0
    return M


# what each crafted order must show in the replay: key -> exact value, or (lo, hi) bounds
EXPECT = {
    "units_first": dict(trivial=64, col_exchanges=0),
    "units_last": dict(trivial=0, stale=0, barred=0),
    "alternating": dict(flagged=32, trivial=(1, 32)),
    "units_descending": dict(trivial=64, row_exchanges=32, known=32, col_exchanges=0),
    "units_rotated": dict(trivial=64, row_exchanges=63, known=1, col_exchanges=0),
    "units_ascending": dict(trivial=64, row_exchanges=0, col_exchanges=0),
    "stale_unit": dict(stale=(1, 64)),
    "first_exchange_31": dict(first_exchange=31, barred=(1, 32)),
    "first_exchange_32": dict(first_exchange=32, barred=(1, 31)),
    "first_exchange_47": dict(first_exchange=47, barred=(1, 16)),
    "first_exchange_63": dict(first_exchange=63, barred=0),
}
GE_STEPS = (0, 1, 31, 32, 47, 63)


def check_expectation(name, p):
    s = summary(p)
    s["flagged"] = s["trivial"] + s["stale"] + s["barred"]
    for key, want in EXPECT[name].items():
        if isinstance(want, tuple):
            assert want[0] <= s[key] <= want[1], (name, key, s)
        else:
            assert s[key] == want, (name, key, s)
    if name == "stale_unit":
        assert 1 in p["stale"], (name, p["stale"])


def crafted_frames(G, H, y, per_case=3):
    """dict name -> frames [per_case, 128]: the crafted orders laid on the magnitudes of the natural frames y."""
    return {name: np.stack([frame_along(o, y[f]) for f in range(per_case)]) for name, o in orders(G, H).items()}


def ge_matrices(seed=7412):
    rng = np.random.default_rng(seed)
    return {t: exchange_matrix(t, rng) for t in GE_STEPS}


def check_ge_matrix(t, p):
    s = summary(p)
    assert s["first_exchange"] == t, (t, s)
    assert s["trivial"] == t and s["barred"] == (63 - t if t else 63), (t, s)
    if t < 63:
        assert [a for a, _ in p["col_exchanges"]] == [t, 63] and p["col_exchanges"][0][1] == 63 and p["col_exchanges"][1][1] >= 64, (t, p["col_exchanges"])
    else:
        assert len(p["col_exchanges"]) == 1 and p["col_exchanges"][0][0] == 63 and p["col_exchanges"][0][1] >= 64
