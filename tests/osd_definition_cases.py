"""Test helper: the codes and the input kinds that tests/test_osd_definition_host.py (CPU models) and
tests/test_gpu_osd_definition.py (kernels) put before the definitions of tests/osd_definition.py.

  codes    G_CASES: (family, code, orders, frames of the highest order) -- a name of osdl_model.graph, a shape (k, n) of
           osd_family.h_systematic, or "tiny" (the (6,2) code of osd_family.tiny_case)
  inputs   kinds(): natural frames (the front end exchanges columns), the dependent-sets-first frames of tests/osd_adversary.py
           with and without ties, values quantised to 1/4 (ties, exact sums), frames with exact +0.0 and -0.0 entries.  The
           tie frames and the zero frames lie on the 1/4 grid as well: equal magnitudes and zeros in the MRB make candidates
           tie exactly, so these frames are held to the exact statement -- the metric is the minimum, the result one of
           the minimisers -- not to the unique-argmin one
EXACT: the kinds whose sums are exact.
"""
import functools

import numpy as np

from oracle import np_oracle
from tests import osd_adversary, osdl_model
from tests import osd_definition as D
from tests import osd_family as OF

TINY_H = np.array([[1, 1, 0, 1, 0, 0], [0, 1, 1, 0, 1, 0], [1, 0, 1, 0, 0, 1], [1, 1, 1, 1, 1, 0]], dtype=np.int64)   # osd_family.tiny_case

# family, code, orders on every frame, (a higher order, on that many natural frames) or None
G_CASES = [
    ("osdx", "tiny", (0, 1, 2), None),                       # order 2 = k: ML
    ("osdx", (3, 20), (0, 1, 2, 3), None),                   # order 3 = k: ML
    ("osdx", (8, 72), (0, 1, 2), None),                      # n - k = 64
    ("osdx", "ldpc_96_48", (0, 1, 2), None),
    ("osdw", (12, 76), (0, 1, 2), None),                     # n - k = 64 and n > 64
    ("osdw", "array_121_80", (0, 1, 2), None),               # k > 64
    ("osdw", "tiny", (0, 1, 2), None),                       # a code ldpc_osdx_* serves, forced through ldpc_osdw_*
    ("osdl", (12, 204), (0, 1, 2), None),                    # n - k = 192, Wp = 3
    ("osdl", "s193_1", (0, 1), None),                        # k = 1: order 1 is ML
    ("osdl", "s200_100", (0, 1, 2), None),
    ("osdl", "wl384", (0, 1), (2, 4)),                       # (384,192): order 2 holds 18 529 candidates a frame
]
SNR = 1.0                                                    # dB: the front end exchanges columns on every code here
FRAMES = dict(natural=60, dependent=8, dependent_ties=8, quantised=24, zeros=12)


EXACT = ("dependent_ties", "quantised", "zeros")


def case_id(c):
    code = c[1] if isinstance(c[1], str) else "%dx%d" % (c[1][1], c[1][0])
    return f"{c[0]}-{code}"


@functools.lru_cache(maxsize=None)
def graph(code):
    """-> (H, G) int64."""
    if code == "tiny":
        return TINY_H, np_oracle.generator_from_H(TINY_H)
    if isinstance(code, tuple):
        return OF.shape_graph(*code)
    return osdl_model.graph(code)


def decoder(code):
    if code == "tiny":
        dec = OF.tiny_case()[0]
        assert np.array_equal(np.asarray(dec.code.H), TINY_H)
        return dec
    return OF.decoder(code)


def quantise(y):
    """Multiples of 1/4, zeros kept: every partial sum of magnitudes is exact in float32 and in float64."""
    return (np.round(np.asarray(y, dtype=np.float32) * np.float32(4)) / np.float32(4)).astype(np.float32)


def with_zeros(y, k, seed):
    """Exact +0.0 and -0.0 entries: a few in every frame, and more than n - k of them in every third frame, so that zeros
    reach the MRB and the hard-decision rule at 0 decides a candidate set."""
    y = np.array(y, dtype=np.float32)
    rng = np.random.default_rng(seed)
    n = y.shape[1]
    for f, row in enumerate(y):
        count = min(n - 1, n - k + 1 + k // 2) if f % 3 == 0 else 3
        at = rng.choice(n, size=count, replace=False)
        row[at] = np.where(rng.integers(0, 2, count) == 1, np.float32(-0.0), np.float32(0.0))
    return y


@functools.lru_cache(maxsize=None)
def kinds(code, scale=1.0):
    """-> dict kind -> y [F, n] float32 of ``code``; ``scale`` < 1 shrinks the frame counts (long codes)."""
    H, G = graph(code)
    k = G.shape[0]
    cnt = {key: max(4, int(v * scale)) for key, v in FRAMES.items()}
    nat = np_oracle.make_frames(G, SNR, cnt["natural"], np.random.default_rng(3))[0]
    base = np_oracle.make_frames(G, SNR, cnt["dependent"] + cnt["dependent_ties"], np.random.default_rng(4))[0]
    out = dict(natural=nat,
               dependent=osd_adversary.g_form_frames(G, H, base[:cnt["dependent"]], 11),
               dependent_ties=osd_adversary.g_form_frames(G, H, quantise(base[cnt["dependent"]:]), 12, ties=True),
               quantised=quantise(np_oracle.make_frames(G, SNR, cnt["quantised"], np.random.default_rng(5))[0]),
               zeros=with_zeros(quantise(np_oracle.make_frames(G, SNR, cnt["zeros"], np.random.default_rng(6))[0]), k, 7))
    return {key: np.ascontiguousarray(v, dtype=np.float32) for key, v in out.items()}


def scale_of(code):
    return 0.5 if code == "wl384" else 1.0


def unpack_cw(words, n):
    """[F, words] u64 -> [F, n] 0/1 in original bit order."""
    return OF.unpack_rows(np.ascontiguousarray(words).view(np.uint64), n).astype(np.int64)


def min_swaps(k):
    """The premise on natural frames: some frame takes at least this many column exchanges."""
    return min(3, k)


def check_fronts(fam, H, k, y, perm, parity, nswaps):
    """Criteria (a)-(d) and the nswaps statement on every frame, and the padding: entries of perm beyond n, rows of parity
    beyond k and bits beyond n - k are zero, as the header states.  -> the GFrames."""
    n = H.shape[1]
    frames = []
    for f in range(len(y)):
        p, P = fam.unpack_front(perm[f], parity[f], n, k)
        try:
            D.front_g(H, y[f], p, P, None if nswaps is None else nswaps[f])
        except D.Violation as v:
            raise D.Violation(v.criterion, f"frame {f}: {v}") from v
        pp, qq = fam.pack_front(p, np.concatenate([np.eye(k, dtype=np.int64), P], axis=1))
        if not (np.array_equal(pp, perm[f]) and np.array_equal(np.ravel(qq), np.ravel(parity[f]))):
            raise D.Violation("a", f"frame {f}: the padding of perm or parity is not zero")
        frames.append(D.GFrame(H, y[f], p, P))
    return frames


def check_g_case(case, front_fn, scan_fn, label):
    """One entry of G_CASES on every input kind.  ``front_fn(y)`` -> (perm [F, .] and parity in the family's model layout,
    nswaps [F], ...); ``scan_fn(y, order, front)`` -> a list of (name, dict(cw [F, words] u64, metric, ntep)) -- every way the
    side under test has to run that order.  Prints and returns the tallies per order."""
    famname, code, orders, extra = case
    fam = OF.FAMILIES[famname]
    H, G = graph(code)
    k, n = G.shape
    book = D.codebook(G) if k <= 16 else None
    tallies = {}
    for kind, y in kinds(code, scale_of(code)).items():
        front = front_fn(y)
        try:
            frames = check_fronts(fam, H, k, y, np.asarray(front[0]), np.asarray(front[1]), np.asarray(front[2]))
        except D.Violation as v:
            raise AssertionError(f"{case_id(case)} {kind} front end: {v}") from v
        if kind == "natural":
            assert int(np.max(front[2])) >= min_swaps(k), "premise: the natural frames exchange columns"
        todo = [(o, len(y)) for o in orders] + ([extra] if extra and kind == "natural" else [])
        for order, F in todo:
            sub = tuple(a[:F] for a in front)
            for name, out in scan_fn(y[:F], order, sub):
                tally = tallies.setdefault((order, name), D.Tally(f"{label} {case_id(case)} order {order} {name}"))
                cw = unpack_cw(out["cw"], n)
                for f in range(F):
                    try:
                        res = D.search(frames[f], order, cw[f], out["metric"][f], out["ntep"][f], exact=kind in EXACT)
                        if book is not None:
                            D.ml_bound(frames[f], book, y[f], cw[f], out["metric"][f], order)
                    except D.Violation as v:
                        raise AssertionError(f"{case_id(case)} {kind} frame {f} order {order} {name}: {v}") from v
                    tally.add(res)
    return [t.done() for t in tallies.values()]


# ---------------------------------------------------------------------------------------------------------------------
# pruned searches: one code per family, order 2
# ---------------------------------------------------------------------------------------------------------------------
PRUNED = [("osdx", "ldpc_96_48"), ("osdw", "array_121_80"), ("osdl", "s200_100")]
FS_SETS = [(0.1, 6.5, 30.0), (0.02, 9.5, 12.0)]               # beta, tau_e, tau_psc
PB_SNR_DB = -4.0                                             # told to the decoder
PB_FULL = ("ccsds", 0)                                       # the set of osdx_pb_model.SETS that every family runs for the full-scan
                                                             # equality: 16 frames of (128,64) at 0 dB, half of them stop on no rule


@functools.lru_cache(maxsize=None)
def pruned_frames(code, F=24):
    """Frames of the family's own code at 0 dB for the FS / PB inequalities."""
    return np.ascontiguousarray(np_oracle.make_frames(graph(code)[1], 0.0, F, np.random.default_rng(7))[0], dtype=np.float32)


def check_pruned(frames, n, order, out, full=None):
    """D.pruned on every frame of a result dict(cw, metric); ``full`` [F] bool: the frames no rule stopped.  -> their number."""
    cw = unpack_cw(out["cw"], n)
    for f, fr in enumerate(frames):
        try:
            D.pruned(fr, order, cw[f], out["metric"][f], full=bool(full[f]) if full is not None else False)
        except D.Violation as v:
            raise AssertionError(f"frame {f}: {v}") from v
    return 0 if full is None else int(np.sum(full))
