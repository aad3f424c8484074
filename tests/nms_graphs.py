"""Test helper: a seeded zoo of Tanner graphs for the generic NMS decode kernel and the NMS training kernel, generated at
test time.  These are not good codes and need not converge: they exist to put every shape-dependent path of
ldpc_nms_generic.h / ldpc_nms_train.hip under an exact comparison.

  array_121_60, ldpc_96_48, wimax_1056   the alist codes of tests/golden/: n not a multiple of 64, m = 176 > 128 (three
                                checks per lane), irregular degrees, the generic kernel's LDS opt-in (WiMAX)
  wide   40 x 130   check degrees 31, 32, 33, 34, 47, 63, 64 next to 2, 3 and random ones up to 30 in ONE code (the second
                    tape word of the training kernel, with and without a second word per check); three label words, two
                    live bits in the last; variable WIDE_ONLY sits in every check above 32 edges and in no other; the
                    degree-64 check ends on variables 128 and 129 (row positions 62, 63)
  thin   14 x 24    checks of degree 1, 2 and 3, an all-zero row, a variable in no check.  A degree-1 check sends
                    alpha * 1e30 (THIN_SINGLE: row -> variable); one of those variables sits in a degree-2 check, the
                    other in a degree-3 check: with alpha > 1 the clip stops the gradient of that check's m2 edge
  short  24 x 40    n < 64: lanes beyond n and beyond m idle, one label word
  deg65  6 x 80     one check of degree 65: above the training kernel's two tape words
"""
import os

import numpy as np

from oracle import np_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALISTS = {"array_121_60": "tests/golden/ArrayCode_N121_K60_r0.50.alist",
          "ldpc_96_48": "tests/golden/LDPC_N96_K48_P8_set0_dmin10.alist",
          "wimax_1056": "tests/golden/wimax_1056_0.83.alist"}
SYNTHETIC = ("wide", "thin", "short", "deg65")
NAMES = tuple(ALISTS) + SYNTHETIC

WIDE_ONLY = 5                       # wide: the variable that sits in the checks above 32 edges only
WIDE_DEGREES = (2, 3, 31, 32, 33, 34, 47, 63, 64)
THIN_SINGLE = {0: 3, 1: 7}          # thin: the degree-1 checks and their variables
THIN_ZERO_ROW, THIN_FREE_VAR = 5, 11


def _balanced_rows(degrees, n, rng, banned=(), forced=None, hubs=()):
    """One support per degree: the variables covered least so far (random jitter; ``hubs`` count for less, so they end up
    in more checks), never ``banned`` ones; forced[r] are put into row r first."""
    cover = np.zeros(n)
    H = np.zeros((len(degrees), n), np.int64)
    for r, d in enumerate(degrees):
        pick = list((forced or {}).get(r, ()))
        score = cover + rng.random(n)
        score[list(hubs)] *= 0.4
        score[list(banned) + pick] = np.inf
        pick += np.argsort(score)[:d - len(pick)].tolist()
        H[r, pick] = 1
        cover[pick] += 1
    return H


def wide_H():
    rng = np.random.default_rng(130)
    degrees = list(WIDE_DEGREES) + rng.integers(2, 31, size=40 - len(WIDE_DEGREES)).tolist()
    order = rng.permutation(len(degrees))
    degrees = [degrees[i] for i in order]                   # wide and narrow checks interleaved over the lanes
    forced = {r: [WIDE_ONLY] for r, d in enumerate(degrees) if d > 32}
    forced[degrees.index(64)] = [WIDE_ONLY, 128, 129]
    H = _balanced_rows(degrees, 130, rng, forced=forced, hubs=(0, 1, 2, 3))
    H[[r for r, d in enumerate(degrees) if d <= 32], WIDE_ONLY] = 0
    for r in np.flatnonzero(H.sum(axis=1) != np.array(degrees)):       # a narrow row that had picked WIDE_ONLY
        free = np.flatnonzero(H[r] == 0)
        H[r, free[free != WIDE_ONLY][0]] = 1
    assert H.sum(axis=1).tolist() == degrees and H.sum(axis=0).min() >= 1
    return H


def thin_H():
    rng = np.random.default_rng(24)
    m, n = 14, 24
    H = np.zeros((m, n), np.int64)
    (ra, a), (rb, b) = THIN_SINGLE.items()
    H[ra, a] = H[rb, b] = 1
    H[2, [b, 13]] = 1                                       # degree 2, one edge from a degree-1 check's variable
    H[3, [0, 4]] = 1                                        # degree 2
    H[4, [1, a, 9]] = 1                                     # degree 3, one edge from a degree-1 check's variable
    rest = [r for r in range(6, m)]
    H[rest] = _balanced_rows([3, 4, 5, 6, 4, 5, 3, 6], n, rng, banned=[THIN_FREE_VAR, a, b])
    assert not H[THIN_ZERO_ROW].any() and not H[:, THIN_FREE_VAR].any()
    return H


def short_H():
    rng = np.random.default_rng(40)
    return _balanced_rows(rng.integers(3, 9, size=24).tolist(), 40, rng)


def deg65_H():
    rng = np.random.default_rng(65)
    return _balanced_rows([65, 4, 7, 12, 33, 5], 80, rng)


_BUILDERS = dict(wide=wide_H, thin=thin_H, short=short_H, deg65=deg65_H)
_cache = {}


def graph(name):
    """-> (H [m, n] int64, G [k, n] int64) of zoo member ``name`` (cached)."""
    if name not in _cache:
        if name in ALISTS:
            c = np_oracle.Code(os.path.join(ROOT, ALISTS[name]))
            _cache[name] = (c.H, c.G)
        else:
            H = _BUILDERS[name]()
            _cache[name] = (H, np_oracle.generator_from_H(H))
    return _cache[name]


def make_code(name):
    """The library's Code of zoo member ``name``: from the alist path, or from the dense H."""
    from short_ldpc_decoding_osd_amd import Code
    return Code(os.path.join(ROOT, ALISTS[name])) if name in ALISTS else Code(H=graph(name)[0])


def frames(name, snr, B, seed, quantise=False):
    """(y [B, n] f32, codewords [B, n]) of ``name``; ``quantise``: half-integer channel values with every 17th zero
    (exact ties in |vc|, S = 0 rows, zeros in mid-decode)."""
    y, cw = np_oracle.make_frames(graph(name)[1], snr, B, np.random.default_rng(seed))
    if quantise:
        y = (np.round(y * 2) / 2).astype(np.float32)
        y[:, ::17] = 0.0
    return y, cw


EXTREME = (1e30, 3e30, 3e38)        # at and above the clip, near FLT_MAX.  (+-inf is left out: the reference formulation
#                                     multiplies the totals by H, and inf * 0 is NaN -- np_oracle.nms_dense shows it)


def extreme_frames(y):
    """A copy of y (at least 2 len(EXTREME) frames): frame i takes magnitude EXTREME[i] with the signs of y on every
    position, frame len(EXTREME) + i takes +EXTREME[i] on position 3 and -EXTREME[i] on the last position."""
    y = np.array(y, np.float32)
    k, n = len(EXTREME), y.shape[1]
    for i, v in enumerate(EXTREME):
        y[i] = np.where(y[i] < 0, -np.float32(v), np.float32(v))
        y[k + i, [3, n - 1]] = [np.float32(v), -np.float32(v)]
    return y


def degrees(H):
    """(largest check degree, largest variable degree), at least 1 each."""
    H = np.asarray(H)
    return max(1, int(H.sum(axis=1).max())), max(1, int(H.sum(axis=0).max()))


def tape_words(H):
    dc = degrees(H)[0]
    return 2 if dc > 32 else 1


def train_lds_bytes(H, T):
    """LDS of one frame of nms_train_kernel (ldpc_nms_train.hip, train_frame_words): messages, totals and channel values,
    then T tape slices of n + m (3 + 2 sw) words."""
    H = np.asarray(H)
    m, n = H.shape
    E, sw = int(H.sum()), tape_words(H)
    return 4 * (E + 2 * n + T * (n + m * (3 + 2 * sw)))


TRAIN_LDS_BUDGET = 160 * 1024


def train_waves(H, T):
    """Frames per workgroup of the training launch: as many as fit 64 KiB, 1..4 (launch_nms_train)."""
    return min(4, max(1, (64 * 1024) // train_lds_bytes(H, T)))


def assert_train_launch(H, T, waves=None, opt_in=None):
    """The premise of a training test: (H, T) fits the budget and launches with ``waves`` frames per workgroup; ``opt_in``:
    whether one frame exceeds 64 KiB (the 160 KiB form)."""
    b = train_lds_bytes(H, T)
    assert b <= TRAIN_LDS_BUDGET, f"T={T}: {b} B of LDS per frame, budget {TRAIN_LDS_BUDGET}"
    if waves is not None:
        assert train_waves(H, T) == waves, f"T={T}: {b} B per frame are {train_waves(H, T)} frames per workgroup, {waves} wanted"
    if opt_in is not None:
        assert (b > 64 * 1024) == opt_in, f"T={T}: {b} B per frame, opt-in {'wanted' if opt_in else 'not wanted'}"
    return b
