"""CPU: the exports of the high-rate PB entry points and the coverage of the very inputs tests/test_gpu_osdw_pb.py decodes
(tests/osdw_pb_model.py): a drift of the frame generator shows up here, not as a silently weaker GPU test.  The model itself
(tests/osdx_pb_model.py) is held to the C oracle by tests/test_osdx_pb_host.py."""
import collections
import math

import numpy as np
import pytest

from tests import osd_shapes as S
from tests import osdw_model
from tests import osdw_pb_model as W

# the stop reasons per set of W.SETS
STOPS = {
    ("array_121_80", 0): {1: 33, 2: 15}, ("array_121_80", 1): {1: 8}, ("array_121_80", 2): {1: 11, 2: 5},
    ("s128_96", 0): {1: 20, 2: 4}, ("s128_65", 0): {1: 8}, ("s128_124", 0): {0: 8}, ("deg65", 0): {0: 2}, ("s70_66", 0): {0: 2},
}


def nmax(k, order):
    return sum(math.comb(k, w) for w in range(order + 1))


def test_the_two_entry_points_are_bound_and_exported():
    from short_ldpc_decoding_osd_amd import _lib
    from short_ldpc_decoding_osd_amd.runtime import Decoder
    L = _lib.load()
    for name in ("ldpc_osdw_pb_search", "ldpc_osdw_pb_decode"):
        assert name in _lib.SYMBOLS
        assert getattr(L, name).argtypes is not None
        assert getattr(L, name).argtypes == getattr(L, name.replace("osdw", "osdx")).argtypes
    assert callable(Decoder.osdw_pb_search) and callable(Decoder.osdw_pb_decode)


def test_the_header_serves_pb_osd_in_the_high_rate_family():
    import os
    text = open(os.path.join(osdw_model.ROOT, "include", "ldpc_osd.h")).read()
    assert "PB-OSD stays with k <= 64" not in " ".join(text.split())
    assert "int ldpc_osdw_pb_search(" in text and "int ldpc_osdw_pb_decode(" in text


def test_stop_reasons_and_tags_of_the_gpu_inputs():
    res = {c: W.case(*c)[5] for c in W.CASES}
    for c, r in res.items():
        assert dict(collections.Counter(r["aux"][:, 3].tolist())) == STOPS[c], c
    counts = W.tag_counts(res.values())
    print(sorted(counts.items()))
    for tag in W.EVERY_TAG:
        assert counts.get(tag, 0) >= 1, tag
    # per set, what it is there for
    a0, a1 = W.tag_counts([res["array_121_80", 0]]), W.tag_counts([res["array_121_80", 1]])
    assert (a0["improved"], a0["late_improvement"], a0["tie"]) == (40, 19, 2)
    assert (a1["tie"], a1["late_improvement"]) == (7, 5) and res["array_121_80", 1]["ntep"].mean() == 822.5
    assert res["array_121_80", 2]["peak"].max() == 262 and (res["array_121_80", 2]["ntep"] < nmax(80, 3)).all()
    assert res["s128_65", 0]["ntep"].max() == 1254
    # full scans visit every TEP
    for (name, i), r in res.items():
        k = osdw_model.graph(name)[1].shape[0]
        N = nmax(k, W.SETS[name][i][2])
        assert np.all(r["ntep"][r["aux"][:, 3] == 0] == N) and np.all(r["ntep"] <= N)
        assert 0 < r["peak"].max() <= W.frontier_bound(k)


def test_winner_spans():
    """Winner supports below, above and across MRB position 64 on (121,80); all above on (128,96); all below on (128,65)."""
    assert W.winner_spans("array_121_80", 0) == {"below": 17, "above": 16, "across": 7}
    assert set(W.winner_spans("s128_96", 0)) == {"above"}
    assert set(W.winner_spans("s128_65", 0)) == {"below"}


def test_more_than_64_live_runs_at_order_2():
    r = W.case("s128_124", 0)[5]
    assert W.SETS["s128_124"][0][2] == 2 and r["peak"].max() == 91 and (r["ntep"] == 7751).all()


def test_full_order_3_scans_beyond_k_66():
    """Every slot of k = 74 is popped, pairs with b >= 64 among them; (70,66) likewise."""
    for name, k, N in (("deg65", 74, 67600), ("s70_66", 66, 47972)):     # (k = 74 > 66: the issue's "some k > 66")
        r = W.case(name, 0)[5]
        assert osdw_model.graph(name)[1].shape[0] == k and nmax(k, 3) == N
        assert W.SETS[name][0][2] == 3 and (r["ntep"] == N).all() and (r["aux"][:, 3] == 0).all()
        assert all("tie" in t for t in r["tags"]) and r["peak"].max() > 1000


def test_the_slot_tiers_and_their_frames():
    assert [W.tier(k) for k in (1, 64, 65, 91, 92, 127)] == [2048, 2048, 4096, 4096, 8064, 8064]
    assert W.slots3(127) == 8002 == W.frontier_bound(127) and W.slots3(64) == 2017
    assert [W.tier(k) for k, _, _ in W.TIER_FRAMES] == [4096, 8064] and [W.tier(k - 1) for k, _, _ in W.TIER_FRAMES] == [2048, 4096]
    for k, n, snr_db in W.TIER_FRAMES:
        _, r = W.order3_frame(k, n, snr_db)
        assert r["ntep"][0] > 64 * 64 and r["peak"][0] > 64                # (both happen to scan in full)


def test_the_largest_frontier():
    """(127,128) at order 3: a full scan of 341 504 TEPs, thousands of live runs, chunks beyond lane 63 of the 126."""
    k, n, snr_db = W.LARGEST
    _, r = W.order3_frame(k, n, snr_db)
    assert r["ntep"].tolist() == [341504] and r["aux"][0].tolist() == [682999, 341503, 0, 0]
    assert r["peak"][0] > 2048 and W.tier(k) == 8064 and (W.slots3(k) + 63) // 64 == 126


@pytest.mark.parametrize("k,n", S.WIDE)
def test_shape_edges_random_dense_float(k, n):
    """What the wide shape edges reach on random_dense / float: (127,128) and (65,66) scan in full, (112,128) stops on rule 1."""
    stops, nteps = set(), set()
    for snr_db in S.PB_SNRS:
        _, F, r = W.edge(k, n, "random_dense", "float", snr_db)
        assert F == W.edge_frames(k) and len(r["best"]) == F
        stops |= set(r["aux"][:, 3].tolist())
        nteps |= set(r["ntep"].tolist())
    print(k, n, sorted(stops), max(nteps))
    if (k, n) == (127, 128):
        assert 8129 in nteps and 0 in stops
    if (k, n) == (65, 66):
        assert 2146 in nteps and 0 in stops
    if (k, n) == (112, 128):
        assert 1 in stops


@pytest.mark.parametrize("k,n,order,levels,F", W.EQUAL)
def test_equal_magnitude_premises(k, n, order, levels, F):
    r = W.equal_magnitudes(k, n, order, levels, F)["model"]
    assert k > 64 and all("tie" in t for t in r["tags"])
    assert (r["ntep"] > 64).any()                            # the visit order matters beyond the first entries


@pytest.mark.parametrize("order", [2, 3])
def test_in_turn_premises(order):
    y, labels, front, r = W.in_turn(order)
    assert r["ntep"].tolist() == [4657, 4657, 1, 1] and nmax(96, 2) == 4657
    assert r["aux"][:, 3].tolist() == [order - 2, order - 2, 1, 1]
    assert len({row.tobytes() for row in y}) == 4
    if order == 3:
        assert W.tier(96) == 8064 and r["peak"][0] > 4096    # live runs in the chunks of the second minimum per lane
