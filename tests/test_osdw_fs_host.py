"""CPU: the premises of tests/test_gpu_osdw_fs.py -- the branches and the supports the very inputs of the GPU tests reach under
the FS-OSD model of tests/osdx_fs_model.py (a drift of the frame generator shows up here, not as a silently weaker GPU test),
the planted stops, the exports of the three entry points, and ldpc_tep_table_fs beyond k = 64."""
import ctypes as C
from math import comb

import numpy as np
import pytest

from oracle import np_oracle
from tests import osdw_fs_model as W
from tests import osdx_fs_model as M


def test_the_three_entry_points_are_bound_and_exported():
    from short_ldpc_decoding_osd_amd import _lib
    L = _lib.load()
    for name in ("ldpc_osdw_fs_search", "ldpc_osdw_fs_decode", "ldpc_osdw_tep_eval"):
        assert name in _lib.SYMBOLS
        assert getattr(L, name).argtypes is not None
    assert L.ldpc_abi_version() == 5


@pytest.mark.parametrize("name", list(W.PARITY))
def test_coverage_of_the_gpu_inputs(name):
    _, _, front, b, order, sets, res = W.parity_case(name)
    assert b.k > 64 and front[1].shape[1] == 128
    counts = M.tag_counts(res)
    print(name, sorted(counts.items()))
    for tag in (W.EVERY_TAG if name in W.FULL_COVERAGE else W.DEG65_TAGS):
        assert counts.get(tag, 0) >= 1, tag
    assert any((r["best_ref"] != r["best_hit"]).any() for r in res) or name == "deg65"


@pytest.mark.parametrize("name,winner,stop", [("array_121_80", True, True), ("s128_65", True, False), ("s128_96", False, True)])
def test_supports_lie_on_both_sides_of_position_64(name, winner, stop):
    win, st = W.spans(name)
    print(name, sorted(win), sorted(st))
    every = {"below", "above", "across"}
    if winner:
        assert win == every
    if stop:
        assert st == every


@pytest.mark.parametrize("k,w", [(65, 1), (65, 2), (80, 1), (80, 2), (127, 1), (127, 2), (67, 3)])
def test_fs_table_beyond_k_64(k, w):
    from short_ldpc_decoding_osd_amd import _lib
    L = _lib.load()
    cnt = L.ldpc_tep_table_fs(k, w, None)
    assert cnt == comb(k, w)
    buf = np.full((cnt, 3), 0xEE, np.uint8)
    assert L.ldpc_tep_table_fs(k, w, buf.ctypes.data_as(C.POINTER(C.c_uint8))) == cnt
    want = np.asarray(np_oracle.fs_tep_lists(k, w)[w - 1], dtype=np.int64).reshape(cnt, w)
    assert np.array_equal(buf[:, :w].astype(np.int64), want)
    assert (buf[:, w:] == 0xFF).all()


def test_planted_round_sizes():
    assert comb(67, 3) % 64 == 33 and comb(80, 3) % 64 == 48 and comb(66, 3) % 64 == 0


@pytest.mark.parametrize("k,n,which", W.PLANTED)
def test_planted_stop_premises(k, n, which):
    p = W.planted(k, n, which)
    assert W.planted_graph(k, n)[1].shape == (k, n)
    assert p["parity"].shape == (1, 128) and not p["parity"][0, k:].any()
    cnt = len(M.class_supports(k, 3))
    lo, hi = {"first": (0, 64), "middle": (64, (cnt // 64) * 64), "last": ((cnt // 64) * 64, cnt)}[which]
    assert lo <= p["rank"] < hi and M.fs_rank(k, p["support"]) == p["rank"]
    r = p["batch"].fs(*p["params"])
    at = 1 + k + k * (k - 1) // 2 + p["rank"]                # all-zero TEP, classes 1 and 2, then the rank inside class 3
    assert r["hit"][0] and r["best_hit"][0] == at and r["ntep"][0] == at + 1 and "hit3" in r["tags"][0]
    assert r["best_ref"][0] not in (0, at)                   # the two quirk answers differ


def test_planted_supports_named_by_the_specification():
    sups = {W.planted(k, n, which)["support"] for k, n, which in W.PLANTED}
    print(sorted(sups))
    assert {(27, 65, 66), (40, 78, 79), (25, 53, 63)} <= sups
    assert {W.span(s) for s in sups} >= {"below", "across"}


def test_split_masks():
    m = W.split_masks([0, 1, 1 << 63, 1 << 64, (1 << 127) | (1 << 5)])
    assert m.shape == (5, 2) and m.dtype == np.uint64
    assert m.tolist() == [[0, 0], [1, 0], [1 << 63, 0], [0, 1], [1 << 5, 1 << 63]]
