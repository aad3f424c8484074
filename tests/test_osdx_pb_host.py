"""CPU: the PB-OSD model of tests/osdx_pb_model.py against the C oracle (bit for bit, on CCSDS) and the NumPy oracle (the other
codes), the exports of the any-shape PB entry points, and the coverage of the very inputs tests/test_gpu_osdx_pb.py decodes (a
drift of the frame generator shows up here, not as a silently weaker GPU test)."""
import collections

import numpy as np
import pytest

from oracle import c_oracle, np_oracle
from tests import osdx_model
from tests import osdx_pb_model as M
from tests.gpu_util import pack_np

bits32 = lambda a: np.asarray(a, dtype=np.float32).view(np.uint32)      # noqa: E731

# the stop reasons the feature was specified with, per set of M.SETS (the two added sets are counted here for the first time)
STOPS = {
    ("short", 0): {1: 38, 0: 8, 2: 2}, ("short", 1): {1: 38, 0: 9, 2: 1},
    ("thin", 0): {0: 24}, ("thin", 1): {1: 24},
    ("ldpc_96_48", 0): {1: 14, 0: 2}, ("ldpc_96_48", 1): {2: 37, 1: 59}, ("ldpc_96_48", 2): {2: 6, 1: 10},
    ("ldpc_96_48", 3): {2: 9, 1: 7},
    ("array_121_60", 0): {0: 7, 1: 17}, ("array_121_60", 1): {2: 9, 1: 7},
    ("ccsds", 0): {0: 8, 1: 8}, ("ccsds", 1): {2: 16, 1: 16}, ("ccsds", 2): {2: 14, 1: 10},
}


@pytest.mark.parametrize("i", range(len(M.SETS["ccsds"])))
def test_model_equals_the_c_oracle_on_ccsds(i):
    y, cw, _, order, snr_db, r = M.case("ccsds", i)
    ref = c_oracle.pb_osd(osdx_model.graph("ccsds")[1], y, cw, order, snr_db)
    assert np.array_equal(ref["num_teps"], r["ntep"]) and np.array_equal(ref["best_index"], r["best"])
    for col, key in enumerate(("comparisons", "suc1", "suc2", "stop")):
        assert np.array_equal(ref[key], r["aux"][:, col]), key
    assert np.array_equal(bits32(ref["metric"]), bits32(r["metric"]))
    assert np.array_equal(pack_np(ref["codeword"]), r["cw"])


def test_det_expf_and_the_cdf_recurrence_equal_the_c_oracle():
    x = np.concatenate([np.linspace(-90, 3, 400), [-87.0, -87.5, 0.0, 88.5]]).astype(np.float32)
    assert np.array_equal(bits32(c_oracle.det_expf(x)), bits32([M.det_expf(v) for v in x]))
    for p in (0.5, 0.03125, 0.2071, 1e-3):
        assert np.array_equal(c_oracle.binom_cdf64(p), np.array(M.binom_cdf(64, p)))


@pytest.mark.parametrize("name,i", [c for c in M.CASES if c[0] != "ccsds"])
def test_model_agrees_with_the_numpy_oracle(name, i):
    """(num_teps, best_index, comparisons, stop) of np_oracle.pb_osd_frame, which uses libm's exp and SciPy's binom.cdf: a frame
    may differ only where a decision sits within float rounding of a threshold, at most 2 % of a set."""
    y, cw, front, order, snr_db, r = M.case(name, i)
    G = osdx_model.graph(name)[1]
    n = G.shape[1]
    differ = 0
    for f in range(len(y)):
        p = front[0][f, :n].astype(np.int64)
        with np.errstate(over="ignore", divide="ignore"):     # (a vanishing success product: p_suc = 0)
            ref = np_oracle.pb_osd_frame(y[f][p], None, front[3][f], order, snr_db)
        got = (int(r["ntep"][f]), int(r["best"][f]), int(r["aux"][f, 0]), int(r["aux"][f, 3]))
        differ += got != (ref["num_teps"], ref["best_index"], ref["comparisons"], ref["stop"])
    print(name, i, "frames that differ:", differ, "of", len(y))
    assert differ <= 0.02 * len(y)


def test_the_two_entry_points_are_bound_and_exported():
    from short_ldpc_decoding_osd_amd import _lib
    L = _lib.load()
    for name in ("ldpc_osdx_pb_search", "ldpc_osdx_pb_decode"):
        assert name in _lib.SYMBOLS
        assert getattr(L, name).argtypes is not None


@pytest.mark.parametrize("name", osdx_model.CODES)
def test_coverage_of_the_gpu_inputs(name):
    res = [M.case(name, i)[5] for i in range(len(M.SETS[name]))]
    counts = M.tag_counts(res)
    print(name, sorted(counts.items()))
    for tag in M.EVERY_CODE + (() if name in M.NO_STOP2 else ("stop2",)):
        assert counts.get(tag, 0) >= 1, tag
    for i, r in enumerate(res):
        assert dict(collections.Counter(r["aux"][:, 3].tolist())) == STOPS[name, i], (name, i)
    # a full scan visits every TEP; the long codes improve beyond the first 64 ranks somewhere
    k = osdx_model.graph(name)[1].shape[0]
    for (_, _, order, _, _), r in zip(M.SETS[name], res):
        nmax = len(osdx_model.tep_matrix(k, order))
        assert np.all(r["ntep"][r["aux"][:, 3] == 0] == nmax) and np.all(r["ntep"] <= nmax)
    if name in ("ldpc_96_48", "array_121_60", "ccsds"):
        assert counts.get("late_improvement", 0) >= 1


@pytest.mark.parametrize("name", osdx_model.CODES)
def test_the_live_frontier_stays_within_its_bound(name):
    """1 + (k - 1) + C(k - 1, 2): one slot of the kernel's LDS per run (pb_frame asserts it per frame as well)."""
    k = osdx_model.graph(name)[1].shape[0]
    peak = max(int(M.case(name, i)[5]["peak"].max()) for i in range(len(M.SETS[name])))
    print(name, "peak", peak, "bound", M.frontier_bound(k))
    assert 0 < peak <= M.frontier_bound(k)
    assert M.frontier_bound(64) == 2017


@pytest.mark.parametrize("name,order,levels", [("short", 3, 1), ("short", 3, 2), ("array_121_60", 2, 1), ("array_121_60", 2, 2)])
def test_equal_magnitude_premises(name, order, levels):
    c = M.equal_magnitudes(name, order, levels)
    r = c["model"]
    assert all("tie" in t for t in r["tags"])
    assert (r["ntep"] > 64).any()                            # the visit order matters beyond the first entries
