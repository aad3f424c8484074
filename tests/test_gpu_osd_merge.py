"""-m gpu: ldpc_osd_merge against NumPy on hand-made inputs, one code per word count W = ceil(n/64):

    W = 1   the (6,2) code of osd_family.tiny_case          W = 6   s321_130: ONE valid bit in the last word
    W = 2   array_121_80: a partial last word               W = 17  wimax_1056, which no OSD family serves
    W = 4   s200_100

1000 frames; frame lists of 0, 1, 63, 65 and 300 entries, ascending and not contiguous; the device-side count below, at and
above F; every subset of the nullable {d_hard, counters}; the counters accumulated over two calls (the second call finds the
merged rows in d_hard, so its `before` is the first call's `after`).  d_hard holds sentinel words in every row no list names:
the whole array is compared, so a write outside the listed rows, or at or beyond min(count, F), shows.  Integers equal.
"""
import numpy as np
import pytest
import torch

from tests import abi_calls as A
from tests import osd_family as OF
from tests.gpu_util import to_dev, words_np

pytestmark = pytest.mark.gpu
FRAMES = 1000
LISTS = (0, 1, 63, 65, 300)
SENT64 = np.uint64(A.SENT[torch.int64])
CODES = {"tiny": 1, "array_121_80": 2, "s200_100": 4, "s321_130": 6, "wimax_1056": 17}


def _dec(name):
    return OF.tiny_case()[0] if name == "tiny" else OF.decoder(name)


def _ptr(t):
    return None if t is None else t.data_ptr()


def merge(dec, cw, index, count, F, hard, label, counts):
    """ldpc_osd_merge by the header's argument order: the status code."""
    return dec.L.ldpc_osd_merge(dec._ctx, _ptr(cw), _ptr(index), _ptr(count), F, _ptr(hard), _ptr(label), _ptr(counts), dec._stream())


def popcount(a):
    """[r, W] uint64 -> [r] set bits."""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return np.unpackbits(a.view(np.uint8).reshape(a.shape[0], 8 * a.shape[1]), axis=1).sum(axis=1).astype(np.int64)


def model(cw, index, count, F, hard, label, counts):
    """The header's contract in NumPy, in place on ``hard`` and ``counts`` (each may be None; the counters need ``label``)."""
    m = max(0, min(int(count), int(F)))
    rows = index[:m]
    if label is not None and counts is not None:
        after = popcount(cw[:m] ^ label[rows])
        before = popcount(hard[rows] ^ label[rows]) if hard is not None else np.zeros(m, np.int64)
        counts += np.array([m, int((after != 0).sum()), int(after.sum()), int(before.sum())], dtype=np.int64)
    if hard is not None:
        hard[rows] = cw[:m]


def make_case(n, L, seed):
    """-> (label, hard, cw, index) uint64 / int32: random n-bit labels; the listed rows of hard and cw are the label with a few
    bits flipped (a third of the rows of cw equal their label), bit n-1 among them in the first listed row of both; the rows
    of hard no list names hold the sentinel."""
    rng = np.random.default_rng(seed)
    W = (n + 63) // 64
    bits = rng.integers(0, 2, size=(FRAMES, 64 * W), dtype=np.uint8)
    bits[:, n:] = 0

    def pack(b):
        return np.packbits(b, axis=1, bitorder="little").view(np.uint64).reshape(len(b), W)

    def noisy(b, p):
        e = (rng.random(b.shape) < p).astype(np.uint8)
        e[:, n:] = 0
        return b ^ e

    index = np.sort(rng.choice(FRAMES, size=L, replace=False)).astype(np.int32)
    assert L < 3 or (np.diff(index) > 1).any()                      # ascending, not contiguous
    label = pack(bits)
    hb, cb = noisy(bits[index], 3.0 / n + 0.02), noisy(bits[index], 2.0 / n + 0.01)
    cb[1::3] = bits[index][1::3]
    if L:
        hb[0, n - 1] = bits[index[0], n - 1] ^ 1
        cb[0, n - 1] = bits[index[0], n - 1] ^ 1
    hard = np.full((FRAMES, W), SENT64, np.uint64)
    hard[index] = pack(hb)
    return label, hard, pack(cb), index


def counts_and_F(L):
    """(count, F) with the count below, at and above F."""
    return [(L // 2, L), (L, L), (L, max(L - 9, 0)), (L + 5, L)]


@pytest.mark.parametrize("name", list(CODES))
def test_merge_equals_numpy(name):
    dec = _dec(name)
    assert dec.words == CODES[name]
    n, W = dec.n, dec.words
    for L in LISTS:
        label, hard0, cw, index = make_case(n, L, 100 + L)
        if L:                                                        # premise: errors in the LAST label word, before and after
            assert (hard0[index[0], W - 1] ^ label[index[0], W - 1]) and (cw[0, W - 1] ^ label[index[0], W - 1])
        d_label, d_cw = to_dev(label.view(np.int64), dec), to_dev(cw.view(np.int64), dec)
        d_index = to_dev(np.concatenate([index, np.full(7, -1, np.int32)]), dec)   # (entries beyond the list are never read)
        for count, F in counts_and_F(L):
            d_count = to_dev(np.array([count], np.int32), dec)
            for with_hard in (True, False):
                for with_counts in (True, False):
                    where = (name, L, count, F, with_hard, with_counts)
                    hard = hard0.copy()
                    counts = np.array([11, 12, 13, 14], np.int64)
                    d_hard = to_dev(hard.view(np.int64), dec)
                    d_counts = to_dev(counts, dec)
                    calls = 2 if with_hard and with_counts else 1
                    for _ in range(calls):
                        assert merge(dec, d_cw, d_index, d_count, F, d_hard if with_hard else None,
                                     d_label if with_counts else None, d_counts if with_counts else None) == 0, where
                        model(cw, index, count, F, hard if with_hard else None, label, counts if with_counts else None)
                    torch.cuda.synchronize()
                    assert np.array_equal(words_np(d_hard), hard), where
                    assert d_counts.cpu().tolist() == counts.tolist(), where
                    if with_counts and not with_hard:
                        assert counts[3] == 14, where                # the fourth counter does not move without d_hard
                    m = max(0, min(count, F))
                    rest = np.setdiff1d(np.arange(FRAMES), index[:m])
                    assert (hard[rest] == hard0[rest]).all(), where  # (the model itself leaves the other rows alone)


def test_labels_and_counters_are_a_pair():
    """Labels without counters, or counters without labels: no counting; with d_hard the merge still happens, without it
    nothing is launched."""
    dec = _dec("s200_100")
    label, hard0, cw, index = make_case(dec.n, 65, 7)
    d_label, d_cw, d_index = to_dev(label.view(np.int64), dec), to_dev(cw.view(np.int64), dec), to_dev(index, dec)
    d_count = to_dev(np.array([65], np.int32), dec)
    want = hard0.copy()
    model(cw, index, 65, 65, want, None, None)
    for lab, with_counts in ((d_label, False), (None, True)):
        d_hard, d_counts = to_dev(hard0.view(np.int64), dec), to_dev(np.array([1, 2, 3, 4], np.int64), dec)
        assert merge(dec, d_cw, d_index, d_count, 65, d_hard, lab, d_counts if with_counts else None) == 0
        assert merge(dec, d_cw, d_index, d_count, 65, None, lab, d_counts if with_counts else None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(words_np(d_hard), want) and d_counts.cpu().tolist() == [1, 2, 3, 4]


def test_decoder_method():
    """Decoder.osd_merge: counters allocated when labels come without them, F from cw."""
    dec = _dec("array_121_80")
    label, hard0, cw, index = make_case(dec.n, 63, 3)
    d_hard = to_dev(hard0.view(np.int64), dec)
    got = dec.osd_merge(to_dev(cw.view(np.int64), dec), to_dev(index, dec), to_dev(np.array([40], np.int32), dec), hard=d_hard,
                        label_bits=to_dev(label.view(np.int64), dec))
    want_hard, want = hard0.copy(), np.zeros(4, np.int64)
    model(cw, index, 40, 63, want_hard, label, want)
    torch.cuda.synchronize()
    assert got.cpu().tolist() == want.tolist() and np.array_equal(words_np(d_hard), want_hard)
    assert dec.osd_merge(to_dev(cw.view(np.int64), dec), to_dev(index, dec), to_dev(np.array([40], np.int32), dec), hard=d_hard) is None


def test_bad_arguments():
    """-1 naming the pointer, before any launch: the buffers keep their contents.  F == 0 is LDPC_OK whatever else is NULL."""
    dec = _dec("s321_130")
    label, hard0, cw, index = make_case(dec.n, 63, 5)
    bufs = dict(cw=to_dev(cw.view(np.int64), dec), index=to_dev(index, dec), count=to_dev(np.array([63], np.int32), dec),
                hard=to_dev(hard0.view(np.int64), dec), label=to_dev(label.view(np.int64), dec),
                counts=to_dev(np.array([1, 2, 3, 4], np.int64), dec))
    clean = {k: v.clone() for k, v in bufs.items()}

    def call(F=63, **gone):
        a = dict(bufs, **gone)
        return merge(dec, a["cw"], a["index"], a["count"], F, a["hard"], a["label"], a["counts"])

    for missing in ("cw", "index", "count"):
        assert call(**{missing: None}) == A.E_ARG
        assert f"ldpc_osd_merge: d_{missing} is NULL" in A.last_error(dec)
    assert call(F=-1) == A.E_ARG and "ldpc_osd_merge: bad arguments" in A.last_error(dec)
    assert dec.L.ldpc_osd_merge(None, _ptr(bufs["cw"]), _ptr(bufs["index"]), _ptr(bufs["count"]), 63, None, None, None, None) == A.E_ARG
    assert merge(dec, None, None, None, 0, None, None, None) == 0
    torch.cuda.synchronize()
    OF.assert_untouched(bufs, clean)
