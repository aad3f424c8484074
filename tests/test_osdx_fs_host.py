"""CPU: the FS-OSD model of tests/osdx_fs_model.py against the scalar oracles, the exports of the any-shape FS entry points,
and the coverage of the very inputs tests/test_gpu_osdx_fs.py decodes (a drift of the frame generator shows up here, not as a
silently weaker GPU test)."""
import numpy as np
import pytest

from oracle import c_oracle, np_oracle
from tests import osdx_fs_model as M
from tests import osdx_model
from tests.gpu_util import pack_np

bits32 = lambda a: np.asarray(a, dtype=np.float32).view(np.uint32)      # noqa: E731


def _pick(tags, wanted):
    """Three frames of different branches: the first frame whose tags meet each group of ``wanted`` (else frames 0, 1, 2)."""
    out = []
    for group in wanted:
        hits = [f for f, t in enumerate(tags) if t & group and f not in out]
        out.append(hits[0] if hits else min(set(range(len(tags))) - set(out)))
    return out


@pytest.mark.parametrize("name,order", [(n, 2) for n in osdx_model.CODES] + [("short", 3), ("thin", 3)])
def test_model_equals_the_scalar_oracle(name, order):
    y, cw, _, b, _, sets, res = M.parity_case(name)
    G = osdx_model.graph(name)[1]
    params, at_case_order = sets[1], res[1]
    frames = _pick(at_case_order["tags"], [{"hit1", "hit2", "hit3"}, {"full"}, {"bound1", "bound2", "bound3"}])
    hit_seen = False
    for f in frames:
        yp, labp, Gp, perm, _ = np_oracle.swapped_info(y[f], cw[f], G)
        assert np.array_equal(perm, b.perm[f])
        ref = np_oracle.fs_osd_frame(yp, labp, Gp, order, *params)
        got = b.scans[f].fs(order, *params)
        assert got["ntep"] == ref["num_teps"]
        assert bits32(got["ref"][1]) == bits32(ref["metric_ref"])
        assert np.array_equal(b.scans[f].one_tep(got["ref"][0])[0], ref["codeword_ref"])
        assert (got["hit"] is None) == (ref["codeword_hit"] is None)
        if got["hit"] is not None:
            hit_seen = True
            assert bits32(got["hit"][1]) == bits32(ref["metric_hit"])
            assert np.array_equal(b.scans[f].one_tep(got["hit"][0])[0], ref["codeword_hit"])
    assert hit_seen                                          # premise: one of the three frames stops on tau_e


def test_model_equals_the_c_oracle_on_ccsds():
    y, cw, _, b, order, sets, res = M.parity_case("ccsds")
    G = osdx_model.graph("ccsds")[1]
    F = 64
    for params, r in zip(sets[:2], res[:2]):
        ref = c_oracle.fs_osd(G, y[:F], cw[:F], order, *params)
        assert np.array_equal(ref["num_teps"], r["ntep"][:F]) and np.array_equal(ref["hit"], r["hit"][:F])
        assert np.array_equal(ref["best_index"], r["best_ref"][:F])
        assert np.array_equal(bits32(ref["metric_ref"]), bits32(r["metric_ref"][:F]))
        assert np.array_equal(bits32(ref["metric_hit"]), bits32(r["metric_hit"][:F]))
        assert np.array_equal(pack_np(ref["codeword_ref"]), r["cw_ref"][:F])
        assert np.array_equal(pack_np(ref["codeword_hit"]), r["cw_hit"][:F])
    assert res[1]["hit"][:F].any() and not res[1]["hit"][:F].all()


def test_the_three_entry_points_are_bound_and_exported():
    from short_ldpc_decoding_osd_amd import _lib
    L = _lib.load()
    for name in ("ldpc_osdx_fs_search", "ldpc_osdx_fs_decode", "ldpc_osdx_tep_eval"):
        assert name in _lib.SYMBOLS
        assert getattr(L, name).argtypes is not None


@pytest.mark.parametrize("name", osdx_model.CODES)
def test_coverage_of_the_gpu_inputs(name):
    counts = M.tag_counts(M.parity_case(name)[6])
    print(name, sorted(counts.items()))
    wanted = M.EVERY_CODE + (("hit2", "hit_late") if name in M.LONG_CODES else ()) + (("bound3", "hit3") if name == "short" else ())
    for tag in wanted:
        assert counts.get(tag, 0) >= 1, tag


def test_coverage_of_the_order_3_frames_of_96_48():
    res = M.parity_case("ldpc_96_48", order3=True)[6]
    for r in res:
        print(int((r["depth"] == 3).sum()))
        assert (r["depth"] == 3).sum() >= 8                  # frames that reach weight class 3


@pytest.mark.parametrize("k,n,which", M.PLANTED)
def test_planted_stop_premises(k, n, which):
    p = M.planted(k, n, which)
    assert osdx_model.graph(M.PLANTED_CODE[k])[1].shape == (k, n)
    cnt = len(M.class_supports(k, 3))
    lo, hi = {"first": (0, 64), "middle": (64, (cnt // 64) * 64), "last": ((cnt // 64) * 64, cnt)}[which]
    assert lo <= p["rank"] < hi and M.fs_rank(k, p["support"]) == p["rank"]
    r = p["batch"].fs(*p["params"])
    at = 1 + k + k * (k - 1) // 2 + p["rank"]                # all-zero TEP, classes 1 and 2, then the rank inside class 3
    assert r["hit"][0] and r["best_hit"][0] == at and r["ntep"][0] == at + 1 and "hit3" in r["tags"][0]
    assert r["best_ref"][0] not in (0, at)                   # the two quirk answers differ
