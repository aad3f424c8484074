"""CPU: the premises of tests/test_gpu_osdl_fs.py -- the branches and the supports the very inputs of the GPU tests reach under
the FS-OSD model of tests/osdx_fs_model.py (a drift of the frame generator shows up here, not as a silently weaker GPU test),
the planted stops, the declarations of the three entry points, the FS table of k = 192 and the resource use of the kernels."""
import ctypes as C
import os
import re
import subprocess
from math import comb

import numpy as np
import pytest

from oracle import np_oracle
from short_ldpc_decoding_osd_amd import _lib, build
from tests import osdl_fs_model as LF
from tests import osdl_model
from tests import osdx_fs_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ldpc_osdl_fs_search", "ldpc_osdl_fs_decode", "ldpc_osdl_tep_eval")


def test_header_binding_and_library_declare_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "ldpc_osd.h")).read()
    declared = set(re.findall(r"\b(ldpc_[A-Za-z0-9_]+)\s*\(", hdr))
    L = _lib.load()
    for name in NAMES:
        assert name in declared, name
        assert name in _lib.SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    assert getattr(L, "ldpc_osdl_fs_search").argtypes == getattr(L, "ldpc_osdw_fs_search").argtypes
    assert getattr(L, "ldpc_osdl_fs_decode").argtypes == getattr(L, "ldpc_osdw_fs_decode").argtypes
    assert getattr(L, "ldpc_osdl_tep_eval").argtypes == getattr(L, "ldpc_osdw_tep_eval").argtypes
    assert "are not served for these shapes" in hdr and "FS-OSD, PB-OSD, one-TEP evaluation" not in hdr
    assert L.ldpc_abi_version() == 5 and "#define LDPC_OSD_ABI_VERSION 5" in hdr
    stubs = open(os.path.join(build.CSRC, "ldpc_sanitizer_stubs.cpp")).read()
    for name in NAMES:
        assert f"LDPC_STUB({name})" in stubs, name
    assert "ldpc_osdl_fs.hip" in build.SOURCES


# ---------------------------------------------------------------------------------------------------------------------
# the inputs of the parity test
# ---------------------------------------------------------------------------------------------------------------------
def test_the_inputs_are_the_specified_ones():
    assert {k: v[:3] for k, v in LF.PARITY.items()} == {"wl384": (2.0, 24, 2), "s200_100": (1.0, 48, 2), "s321_130": (1.0, 32, 2),
                                                        "s256_192": (3.0, 24, 2), "s128_32": (0.0, 64, 3)}
    assert LF.SEED == 7 and all(len(v[3]) == 4 for v in LF.PARITY.values())
    assert LF.EVERY_TAG == ("zero", "bound1", "bound2", "full", "hit1", "hit2", "hit_late", "psc_blocked", "hit_after_improvement")
    assert set(LF.TAGS["s128_32"]) == (set(LF.EVERY_TAG) - {"bound2"}) | {"bound3", "hit3"}


@pytest.mark.parametrize("name", list(LF.PARITY))
def test_coverage_of_the_gpu_inputs(name):
    y, _, front, b, order, sets, res = LF.parity_case(name)
    n, k, S, W, Wp = osdl_model.shape(name)
    assert name in osdl_model.NEW and (b.k, b.n) == (k, n)
    assert front[0].shape == (len(y), 64 * S) and front[0].dtype == np.uint16 and front[1].shape == (len(y), 64 * W, Wp)
    counts = M.tag_counts(res)
    print(name, sorted(counts.items()))
    for tag in LF.TAGS[name]:
        assert counts.get(tag, 0) >= 1, tag
    differ = [int((r["best_ref"] != r["best_hit"]).sum()) for r in res]
    print(name, "frames where the quirk answers differ, per set:", differ)
    assert max(differ) >= 1
    if name == "wl384":
        assert differ[0] == 0 and all(6 <= d <= 8 for d in differ[1:])


def test_supports_lie_in_every_mrb_word_and_across_their_borders_on_wl384():
    """Winners and stopping candidates wholly in word 0, 1 and 2 and across positions 63 / 64 and 127 / 128.  The natural
    frames of wl384 leave three of the ten out -- FS-OSD visits the least reliable positions first, so a stop rarely lies in
    word 0 --: the caller-made (192,384) cases of the planted test supply them."""
    win, stop = LF.spans("wl384")
    print("natural:", sorted(win), sorted(stop))
    every = {(0,), (1,), (2,), (0, 1), (1, 2)}
    assert win >= every - {(0, 1)} and stop >= every - {(0,), (0, 1)}
    cases = [(192, 384, 2, which, None) for which in ("first", "middle", "last")] + LF.ACROSS
    for c in cases:
        p = LF.planted(*c)
        r = p["batch"].scans[0].fs(*p["params"])
        if r["ref"][0]:
            win.add(LF.span(r["ref"][0]))
        if r["hit"] is not None:
            stop.add(LF.span(r["hit"][0]))
    print("with the caller-made cases:", sorted(win), sorted(stop))
    assert win >= every and stop >= every


# ---------------------------------------------------------------------------------------------------------------------
# the planted stops
# ---------------------------------------------------------------------------------------------------------------------
def test_planted_round_sizes():
    assert [comb(40, 3) % 64, comb(70, 3) % 64, comb(130, 2) % 64, comb(192, 2) % 64] == [24, 20, 1, 32]
    assert len(LF.PLANTED) == 12 and {(k, n, w) for k, n, w, _ in LF.PLANTED} == {(40, 140, 3), (70, 200, 3), (130, 321, 2), (192, 384, 2)}
    assert LF.PLANTED_TAU_E == {3: 3.5, 2: 2.5}


@pytest.mark.parametrize("k,n,weight,which", LF.PLANTED)
def test_planted_stop_premises(k, n, weight, which):
    p = LF.planted(k, n, weight, which)
    assert LF.planted_graph(k, n)[1].shape == (k, n) and osdl_model.served(n, k)
    assert not ((k <= 64 and n - k <= 64) or (n <= 128 and n - k <= 64))           # no older family serves the shape
    S, W, Wp = (n + 63) // 64, (k + 63) // 64, (n - k + 63) // 64
    assert p["perm"].shape == (1, 64 * S) and p["parity"].shape == (1, 64 * W, Wp) and not p["parity"][0, k:].any()
    cnt = comb(k, weight)
    lo, hi = {"first": (0, 64), "middle": (64, (cnt // 64) * 64), "last": ((cnt // 64) * 64, cnt)}[which]
    assert lo <= p["rank"] < hi and M.fs_rank(k, p["support"]) == p["rank"] and len(p["support"]) == weight
    r = p["batch"].fs(*p["params"])
    at = p["at"]
    assert at == 1 + k + (k * (k - 1) // 2 if weight == 3 else 0) + p["rank"]
    assert r["hit"][0] and r["best_hit"][0] == at and r["ntep"][0] == at + 1 and f"hit{weight}" in r["tags"][0]
    assert r["best_ref"][0] not in (0, at)                   # the two quirk answers differ


def test_across_cases():
    stop, winner = (LF.planted(*c) for c in LF.ACROSS)
    assert stop["support"] == winner["support"] == (63, 64) and stop["rank"] >= 64
    r = stop["batch"].fs(*stop["params"])
    assert r["hit"][0] and r["best_hit"][0] == stop["at"] and r["ntep"][0] == stop["at"] + 1 and r["best_ref"][0] not in (0, stop["at"])
    r = winner["batch"].fs(*winner["params"])
    assert not r["hit"][0] and r["best_ref"][0] == winner["at"] and r["ntep"][0] == 1 + 192 + comb(192, 2) and r["tags"][0] == {"full"}


def test_awkward_frames_run_through_the_model():
    """Ties, zeros and saturation: the model settles them without an error; the saturated frame's metric is +inf."""
    for name in LF.AWKWARD:
        y, front, order, sets, res = LF.awkward_case(name)
        assert len(y) == 6 and order <= min(3, osdl_model.shape(name)[1])
        for r in res:
            assert np.isinf(r["metric_ref"][4]) and r["metric_ref"][4] > 0 and not np.isnan(r["metric_ref"]).any()
            assert (r["ntep"] >= 1).all()
        assert len({tuple(r["ntep"].tolist()) for r in res}) == 2          # the strict and the loose set scan differently


def test_split_masks():
    m = LF.split_masks([0, 1, 1 << 63, 1 << 64, (1 << 127) | (1 << 5), (1 << 128) | (1 << 191)], 3)
    assert m.shape == (6, 3) and m.dtype == np.uint64
    assert m.tolist() == [[0, 0, 0], [1, 0, 0], [1 << 63, 0, 0], [0, 1, 0], [1 << 5, 1 << 63, 0], [0, 0, 1 | (1 << 63)]]
    assert LF.split_masks([5, 1 << 64], 1).tolist() == [[5], [0]]           # W = 1: the bits beyond are dropped


# ---------------------------------------------------------------------------------------------------------------------
# the FS table of the largest k
# ---------------------------------------------------------------------------------------------------------------------
def test_fs_table_of_k_192():
    L = _lib.load()
    cnts = [L.ldpc_tep_table_fs(192, w, None) for w in (1, 2, 3)]
    assert cnts == [192, 18336, 1161280] and sum(cnts) == 1179808
    for w in (1, 2):
        buf = np.full((cnts[w - 1], 3), 0xEE, np.uint8)
        assert L.ldpc_tep_table_fs(192, w, buf.ctypes.data_as(C.POINTER(C.c_uint8))) == cnts[w - 1]
        want = np.asarray(np_oracle.fs_tep_lists(192, w)[w - 1], dtype=np.int64).reshape(cnts[w - 1], w)
        assert np.array_equal(buf[:, :w].astype(np.int64), want)
        assert (buf[:, w:] == 0xFF).all()
    buf = np.full((cnts[2], 3), 0xEE, np.uint8)
    assert L.ldpc_tep_table_fs(192, 3, buf.ctypes.data_as(C.POINTER(C.c_uint8))) == cnts[2]
    assert buf[0].tolist() == [189, 190, 191] and buf[-1].tolist() == [0, 1, 2] and int(buf.max()) == 191
    assert np.all(buf[:, 0] < buf[:, 1]) and np.all(buf[:, 1] < buf[:, 2])


# ---------------------------------------------------------------------------------------------------------------------
# the resources of the kernels
# ---------------------------------------------------------------------------------------------------------------------
def test_kernels_use_no_scratch(tmp_path):
    """Device-only compile of ldpc_osdl_fs.hip with the library's flags and the resource remarks: every instantiation has 0
    bytes of scratch and fits the 64 KiB of LDS a workgroup may take.  The table of profiles/osdl_fs/README.md holds the same
    numbers."""
    src = os.path.join(build.CSRC, "ldpc_osdl_fs.hip")
    cmd = [build._hipcc(), "-x", "hip", "--cuda-device-only", "-c", src, "-o", str(tmp_path / "osdl_fs.o")] + build.FLAGS + [
        "-Rpass-analysis=kernel-resource-usage"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    res = {}
    for blk in p.stderr.split("Function Name: ")[1:]:
        sym = blk.split()[0]
        num = lambda key: int(re.search(key + r"[^:]*: (\d+)", blk).group(1))      # noqa: E731
        res[sym] = (num("VGPRs"), num("LDS Size"), num("ScratchSize"))
    readme = open(os.path.join(ROOT, "profiles", "osdl_fs", "README.md")).read()
    for kern in ("osdl_fs_kernel", "osdl_tep_eval_kernel"):
        for wp in (1, 2, 3):
            (sym,) = [k for k in res if f"{kern}ILi{wp}E" in k]
            vgprs, lds, scratch = res[sym]
            print(f"{kern}<{wp}>: {vgprs} VGPRs, {lds} B LDS, {scratch} B scratch")
            assert scratch == 0 and lds <= 65536, (kern, wp, res[sym])
            assert f"| `{kern}<{wp}>` | {vgprs} | {lds} | {scratch} |" in readme
    assert len(res) == 6                                      # nothing else is instantiated here: the front end stays in ldpc_osdl.hip
