"""CPU: the premises of tests/test_gpu_osdl_pb.py -- what the very inputs of the GPU tests reach under the PB-OSD model of
tests/osdl_pb_model.py (a drift of the frame generator shows up here, not as a silently weaker GPU test) --, the model's
equality with tests/osdx_pb_model.py where n - k <= 64, the declarations of the two entry points, the PB table of (384,192) and
the resource use of the kernels."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from short_ldpc_decoding_osd_amd import _lib, build
from tests import osdl_model, osdw_pb_model, osdx_model
from tests import osdl_pb_model as LP
from tests import osdx_pb_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ldpc_osdl_pb_search", "ldpc_osdl_pb_decode")


def test_header_binding_and_library_declare_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "ldpc_osd.h")).read()
    declared = set(re.findall(r"\b(ldpc_[A-Za-z0-9_]+)\s*\(", hdr))
    L = _lib.load()
    for name in NAMES:
        assert name in declared, name
        assert name in _lib.SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    assert L.ldpc_osdl_pb_search.argtypes == L.ldpc_osdw_pb_search.argtypes
    assert L.ldpc_osdl_pb_decode.argtypes == L.ldpc_osdw_pb_decode.argtypes
    assert "int ldpc_osdl_pb_search(" in hdr and "int ldpc_osdl_pb_decode(" in hdr
    assert "PB-OSD, the H-form" not in hdr                       # the family's comment no longer lists PB-OSD as missing
    assert L.ldpc_abi_version() == 5 and "#define LDPC_OSD_ABI_VERSION 5" in hdr
    stubs = open(os.path.join(build.CSRC, "ldpc_sanitizer_stubs.cpp")).read()
    for name in NAMES:
        assert f"LDPC_STUB({name})" in stubs, name
    assert "ldpc_osdl_pb.hip" in build.SOURCES
    for doc in ("README.md", "INTEGRATION.md"):
        assert "PB-OSD is not served for these shapes" not in open(os.path.join(ROOT, doc)).read(), doc


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,i", [("short", 0), ("ldpc_96_48", 3), ("ccsds", 1)])
def test_model_equals_the_any_shape_model_on_narrow_codes(name, i):
    y, _, front, order, snr_db, ref = M.case(name, i)
    got = LP.pb(y, front[0], front[3], order, snr_db)
    for key in ("cw", "best", "ntep", "aux", "peak"):
        assert np.array_equal(got[key], ref[key]), key
    assert np.array_equal(got["metric"].view(np.uint32), ref["metric"].view(np.uint32))
    assert got["tags"] == ref["tags"]


def test_model_equals_the_any_shape_model_on_a_high_rate_code():
    y, _, front, order, snr_db, ref = osdw_pb_model.case("array_121_80", 0)
    got = LP.pb(y[:12], front[0][:12], front[3][:12], order, snr_db)
    for key in ("cw", "best", "ntep", "aux"):
        assert np.array_equal(got[key], ref[key][:12]), key
    assert np.array_equal(got["metric"].view(np.uint32), ref["metric"][:12].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# the PB table
# ---------------------------------------------------------------------------------------------------------------------
def _table(n, k):
    L = _lib.load()
    assert L.ldpc_osdl_pb_table(n, k, None) == 449
    t = np.full(449, np.nan)
    assert L.ldpc_osdl_pb_table(n, k, t.ctypes.data_as(C.POINTER(C.c_double))) == 449
    return t


@pytest.mark.parametrize("n,k", [(384, 192), (321, 130), (193, 1), (128, 96)])
def test_pb_table(n, k):
    m = n - k
    t = _table(n, k)
    cdf = np.array(LP.binom_cdf(m, 0.5))
    assert np.array_equal(t[:m + 1].view(np.uint64), cdf.view(np.uint64)) and not t[m + 1:193].any()
    assert abs(t[m] - 1.0) < 1e-12 and t[0] == 0.5 ** m
    assert t[193:193 + m].tolist() == [float(m - i) / float(i + 1) for i in range(m)] and not t[193 + m:385].any()
    kk = min(k, 64)
    assert t[385:385 + kk].tolist() == [float(k - i) / float(i + 1) for i in range(kk)] and not t[385 + kk:].any()


def test_pb_table_refuses_other_shapes():
    L = _lib.load()
    for n, k in ((385, 193), (384, 191), (10, 0), (10, 10)):
        assert L.ldpc_osdl_pb_table(n, k, None) == -1, (n, k)


# ---------------------------------------------------------------------------------------------------------------------
# the premises of the GPU inputs
# ---------------------------------------------------------------------------------------------------------------------
def test_the_inputs_are_the_specified_ones():
    assert LP.NATURAL[:9] == (("wl384", 2.0, 2, 12), ("wl384", 2.0, 3, 6), ("wl384", 1.0, 2, 8), ("s200_100", 1.0, 3, 8),
                              ("s128_32", 0.0, 3, 12), ("s100_20", 0.0, 3, 8), ("s321_130", 1.0, 2, 8), ("s193_1", 0.0, 1, 8),
                              ("s256_192", 3.0, 2, 8))
    assert LP.SEED == 7 and all(name in osdl_model.NEW for name, *_ in LP.NATURAL)
    assert LP.LOUD_AMP == 6.0 / 3.1773 and LP.QUIET_AMP == 0.02 and LP.LOUD_SNR_DB == 1.0


def _nat(i):
    r = LP.natural(i)[5]
    print(LP.NATURAL[i], "ntep", r["ntep"].tolist(), "stop", r["aux"][:, 3].tolist(), "peak", r["peak"].tolist(),
          "spans", [LP.span(s) for s in r["supports"]])
    return r, r["aux"][:, 3].tolist(), [LP.span(s) for s in r["supports"]]


def test_natural_wl384_2dB_order_2():
    r, stop, spans = _nat(0)
    assert set(stop) == {1, 2} and (r["ntep"] == 1).sum() == 3 and int(r["ntep"].max()) == 2487
    assert (0,) in spans and any(s and set(s) == {2} for s in spans)
    y, _, front, _, _, _ = LP.natural(0)
    assert front[0].shape == (12, 384) and front[0].dtype == np.uint16 and front[1].shape == (12, 192, 3)


def test_natural_wl384_2dB_order_3():
    r, stop, spans = _nat(1)
    assert {1862, 5434, 5632} <= set(r["peak"].tolist()) and int(r["ntep"].max()) == 5866 and spans.count((1, 1)) == 1
    assert LP.tier(192) == 18368 and int(r["peak"].max()) > 4096


def test_natural_wl384_1dB_order_2():
    r, stop, spans = _nat(2)
    assert (int(r["ntep"].min()), int(r["ntep"].max())) == (825, 6408) and {(1, 2), (1, 1), (2, 2)} <= set(spans)


def test_natural_s200_100():
    r, stop, spans = _nat(3)
    assert set(stop) == {1, 2} and int(r["peak"].max()) == 2192 and (0, 1, 1) in spans


def test_natural_s128_32_and_s100_20():
    r, stop, spans = _nat(4)
    assert set(stop) == {1} and (int(r["ntep"].min()), int(r["ntep"].max())) == (220, 5427) and (r["best"] == 0).sum() == 2
    r, stop, spans = _nat(5)
    assert sum(len(s) == 3 for s in spans) >= 2


def test_natural_s321_130_and_s193_1():
    r, stop, spans = _nat(6)
    assert set(stop) == {2} and int(r["ntep"].max()) == 43
    r, stop, spans = _nat(7)
    assert r["ntep"].tolist() == [2] * 8 and set(stop) == {0} and (r["best"] == 1).sum() == 1


def test_natural_s256_192():
    """At 3.0 dB every frame stops at its first TEP; 1.0 dB, chosen on the CPU, is the set at which some do not."""
    r, stop, spans = _nat(8)
    assert r["ntep"].tolist() == [1] * 8
    r, stop, spans = _nat(9)
    assert LP.NATURAL[9] == ("s256_192", 1.0, 2, 8) and (r["ntep"] > 1).sum() >= 4 and set(stop) == {1, 2}


def test_loud_and_quiet_frames_on_wl384():
    r = LP.in_turn("wl384", 2)[3]
    assert r["ntep"].tolist() == [18529, 18529, 1, 1] and r["aux"][0].tolist() == [37052, 18528, 0, 0] and r["aux"][2].tolist() == [1, 0, 0, 1]
    r = LP.in_turn("wl384", 3)[3]
    assert r["ntep"].tolist() == [18529, 18529, 1, 1] and r["aux"][:, 3].tolist() == [1, 1, 1, 1]
    assert r["peak"][:2].tolist() == [191 * 190 // 2] * 2 == [18145] * 2 and LP.slots3(192) == 18337


@pytest.mark.parametrize("code", LP.IN_TURN[1:])
def test_loud_and_quiet_frames_on_the_lower_tiers(code):
    k, n = code
    nmax2 = 1 + k + k * (k - 1) // 2
    assert osdl_model.served(n, k) and [LP.tier(c[0]) for c in LP.IN_TURN[1:]] == [8064, 4096, 2048]
    for order in (2, 3):
        r = LP.in_turn(code, order)[3]
        assert r["ntep"].tolist() == [nmax2, nmax2, 1, 1] and r["aux"][:, 3].tolist() == [order - 2, order - 2, 1, 1]
        assert order == 2 or r["peak"][0] == (k - 1) * (k - 2) // 2


@pytest.mark.parametrize("code", LP.TIER_FRAMES)
def test_tier_boundary_frames(code):
    """k = 65, 92 and 128 are the first k of the 4096-, 8064- and 18 368-slot tiers; the loud frame has every weight-3 run live."""
    k, n = code
    assert LP.tier(k) > LP.tier(k - 1) and osdl_model.served(n, k)
    r = LP.in_turn(code, 3, 1, 0)[3]
    assert r["peak"][0] == (k - 1) * (k - 2) // 2 and r["aux"][0, 3] == 1 and LP.slots3(k) > LP.tier(k - 1)
    assert sorted((c[1] - c[0] + 63) // 64 for c in LP.TIER_FRAMES) == [1, 2, 3]


def test_tie_inputs():
    assert {((k > 128) + 1, (n - k + 63) // 64) for k, n, *_ in LP.EQUAL if k > 64} >= {(1, 2), (2, 3)}
    for c in LP.EQUAL:
        r = LP.equal_magnitudes(*c)["model"]
        assert all("tie" in t for t in r["tags"]) and int(r["best"].max()) > 0, c
    for i, F in LP.QUANTISED:
        r = LP.natural(i, True)[5]
        assert sum("tie" in t for t in r["tags"][:F]) >= 2, i
    assert [osdl_model.shape(LP.NATURAL[i][0])[1::3] for i, _ in LP.QUANTISED] == [(100, 2), (192, 3)]


def test_cross_codes():
    assert osdl_model.CROSS == ("ccsds", "ldpc_96_48", "array_121_80", "s128_96")
    assert osdx_model.graph("ccsds")[1].shape == (64, 128)


# ---------------------------------------------------------------------------------------------------------------------
# the resources of the kernels
# ---------------------------------------------------------------------------------------------------------------------
def test_kernels_use_no_scratch(tmp_path):
    """Device-only compile of ldpc_osdl_pb.hip with the library's flags and the resource remarks: every instantiation has 0
    bytes of scratch and fits the 160 KiB of LDS a workgroup may take on gfx950.  The table of profiles/osdl_pb/README.md holds
    the same numbers."""
    src = os.path.join(build.CSRC, "ldpc_osdl_pb.hip")
    cmd = [build._hipcc(), "-x", "hip", "--cuda-device-only", "-c", src, "-o", str(tmp_path / "osdl_pb.o")] + build.FLAGS + [
        "-Rpass-analysis=kernel-resource-usage"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    res = {}
    for blk in p.stderr.split("Function Name: ")[1:]:
        sym = blk.split()[0]
        num = lambda key: int(re.search(key + r"[^:]*: (\d+)", blk).group(1))      # noqa: E731
        res[sym] = (num("VGPRs"), num("LDS Size"), num("ScratchSize"))
    readme = open(os.path.join(ROOT, "profiles", "osdl_pb", "README.md")).read()
    for wp in (1, 2, 3):
        for o3, slots in ((0, 192), (1, 2048), (1, 4096), (1, 8064), (1, 18368)):
            (sym,) = [k for k in res if f"osdl_pb_kernelILi{wp}ELb{o3}ELi{slots}E" in k]
            vgprs, lds, scratch = res[sym]
            print(f"osdl_pb_kernel<{wp},{'true' if o3 else 'false'},{slots}>: {vgprs} VGPRs, {lds} B LDS, {scratch} B scratch")
            assert scratch == 0 and lds <= 163840, (wp, slots, res[sym])
            assert f"| `osdl_pb_kernel<{wp},{'true' if o3 else 'false'},{slots}>` | {vgprs} | {lds} | {scratch} |" in readme
    assert len(res) == 15                                     # nothing else is instantiated here: the front end stays in ldpc_osdl.hip
