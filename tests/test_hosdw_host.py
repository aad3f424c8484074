"""CPU: the model of the wide H-form OSD entry points (tests/hosdw_model.py) against tests/hosdx_model.py wherever H has
full row rank, its layouts and constructed codes, the agreement of header, binding and exports on the four ldpc_hosdw_* names,
the library's pattern enumeration beyond position 64, and the coverage conditions of the inputs of tests/test_gpu_hosdw.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import np_oracle
from tests import hosdw_model as WM
from tests import hosdx_model as HM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ldpc_hosdw_supported", "ldpc_hosdw_front", "ldpc_hosdw_search", "ldpc_hosdw_sliding")
FIELDS = ("lri", "uidx", "perm", "M", "swaps", "block_min", "block_arg", "truth", "best_index", "metric", "codeword")
ARRAY_SNRS, REDUNDANT = WM.ARRAY_SNRS, WM.REDUNDANT


def test_header_binding_and_exports_agree():
    hdr = open(os.path.join(ROOT, "include", "ldpc_osd.h")).read()
    declared = set(re.findall(r"\b(ldpc_[A-Za-z0-9_]+)\s*\(", hdr))
    from short_ldpc_decoding_osd_amd import _lib
    L = _lib.load()
    for name in NAMES:
        assert name in declared, name
        assert name in _lib.SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    for op in ("front", "search", "sliding"):
        assert getattr(L, f"ldpc_hosdw_{op}").argtypes == getattr(L, f"ldpc_hosdx_{op}").argtypes
    assert "#define LDPC_OSD_ABI_VERSION 5" in hdr and L.ldpc_abi_version() == 5
    assert L.ldpc_hosdw_supported(None) == 0
    stubs = open(os.path.join(ROOT, "short_ldpc_decoding_osd_amd", "csrc", "ldpc_sanitizer_stubs.cpp")).read()
    for name in NAMES:
        assert f"LDPC_STUB({name})" in stubs, name


@pytest.mark.parametrize("k,n", [(5, 12), (33, 64), (64, 65), (64, 128)])
def test_model_equals_the_any_shape_model_on_full_rank(k, n):
    H, G = HM.code(k, n, "random_dense")
    blocks = HM.edge_blocks(k) if k < 64 else HM.path_blocks(k, 1)
    x, y, cw = HM.refined_frames(H, G, 2.0, 5, 5)
    x[1, : n // 2] = np.float32(0.5) * np.sign(x[1, : n // 2])           # ties
    for f in range(len(x)):
        a, b = WM.hosdw_frame(x[f], y[f], cw[f], H, blocks), HM.hosdx_frame(x[f], y[f], cw[f], H, blocks)
        assert a["deletions"] == []
        for key in FIELDS:
            if key == "swaps":
                assert list(a[key]) == list(b[key])
            elif key in ("truth", "metric", "block_min"):
                assert np.array_equal(np.asarray(a[key], np.float32).view(np.uint32), np.asarray(b[key], np.float32).view(np.uint32)), key
            else:
                assert np.array_equal(a[key], b[key]), key
        assert np.array_equal(WM.pack_M(a["M"])[:64], HM.pack_M(b["M"])) and not WM.pack_M(a["M"])[64:].any()


def test_pack_M_layout():
    M = np.zeros((2, 70), np.int64)
    M[0, [0, 2, 64]] = 1
    M[1, [1, 63, 69]] = 1
    p = WM.pack_M(M)
    assert p.shape == (128,) and p.dtype == np.uint64
    assert p[0] == 5 and p[1] == (1 << 63) | 2 and p[64] == 1 and p[65] == 1 << 5
    assert not p[2:64].any() and not p[66:].any()
    small = WM.pack_M(np.array([[1, 0, 1], [0, 1, 1]]))
    assert small[:2].tolist() == [5, 6] and not small[2:].any()


def test_traced_elimination_equals_the_oracle():
    rng = np.random.default_rng(3)
    for rows, cols in ((9, 12), (66, 121), (127, 128), (6, 128)):
        A = rng.integers(0, 2, size=(rows // 2, cols))
        M = np.concatenate([A, A[rng.integers(0, len(A), size=rows - len(A))]])[rng.permutation(rows)]
        R, swaps, deletions = WM.eliminate_traced(M)
        Ro, so = np_oracle.gf2_eliminate(M)
        assert np.array_equal(R, Ro) and swaps == so and len(deletions) == rows - R.shape[0]
        assert all(0 <= i < left <= rows for i, left in deletions)


@pytest.mark.parametrize("k,n,R,style", REDUNDANT)
def test_constructed_codes_have_the_stated_rows_and_rank(k, n, R, style):
    H, G = WM.redundant(k, n, "random_dense", R, style)
    assert H.shape == (R, n) and WM.rank(H) == n - k and G.shape == (k, n)
    if style == "first":
        assert not H[0].any()
    if style == "last":
        assert not H[-1].any()
    if (k, n, R) == (127, 128, 6):
        assert H[0].any() and (H == H[0]).all()
    from short_ldpc_decoding_osd_amd import Code
    code = Code(H=np.array(H))                                        # as many rows as columns, or more, is still a code
    assert (code.check_matrix_row, code.check_matrix_column, code.k) == (R, n, k)
    assert not (np.asarray(H).dot(np.asarray(code.G).T) % 2).any()


def test_array_codes_are_what_the_family_is_for(golden_dir):
    for which, (rows, m) in {"121_60": (66, 61), "121_80": (44, 41)}.items():
        c = np_oracle.Code(os.path.join(golden_dir, WM.ARRAY[which]))
        assert c.H.shape == (rows, 121) and WM.rank(c.H) == m and c.k == 121 - m


def test_pattern_teps_on_80_positions():
    from short_ldpc_decoding_osd_amd import _lib
    L = _lib.load()
    _, b = np_oracle.segment_boundaries(80, 3)
    assert int(b[-1]) == 80
    ranges = [range(int(b[i]), int(b[i + 1])) for i in range(3)]
    bounds = (C.c_int32 * 4)(*[int(v) for v in b])
    seen = 0
    for pat in np_oracle.convention_path(2):
        p = (C.c_int32 * 3)(*pat)
        cnt = _lib.check(L.ldpc_hosd_pattern_teps(3, bounds, p, None), "ldpc_hosd_pattern_teps")
        t = np.zeros((max(cnt, 1), 4), np.uint8)
        _lib.check(L.ldpc_hosd_pattern_teps(3, bounds, p, t.ctypes.data_as(C.POINTER(C.c_uint8))), "ldpc_hosd_pattern_teps")
        E = np_oracle.error_pattern_gen(pat, ranges, 80)
        assert cnt == len(E) and np.array_equal(t[:cnt], HM.teps_of(E)), pat
        seen = max(seen, int(t[:cnt, :3].max()) if cnt else 0)
    assert seen == 79
    wide = (C.c_int32 * 2)(0, 128)
    assert L.ldpc_hosd_pattern_teps(1, wide, (C.c_int32 * 1)(1), None) == 128
    assert L.ldpc_hosd_pattern_teps(1, (C.c_int32 * 2)(0, 129), (C.c_int32 * 1)(1), None) == -1


# ---------------------------------------------------------------------- coverage of the GPU inputs, from the model
@pytest.mark.parametrize("which", sorted(WM.ARRAY))
def test_array_frames_exercise_the_deletion_rule(golden_dir, which):
    """The frames of tests/test_gpu_hosdw.py cannot pass vacuously: at least a quarter of them delete a row before the last
    pivot step, at least a tenth record other column exchanges when the rows of H are reversed, and on (121,60) a row is
    deleted while more than 64 rows are left (the row map's move from its upper into its lower half)."""
    early = other = crossing = total = 0
    for snr in ARRAY_SNRS:
        c = WM.array_case(golden_dir, which, snr)
        r = WM.array_case(golden_dir, which, snr, reverse=True)
        m = c["H"].shape[1] - c["G"].shape[0]
        for a, b in zip(c["results"], r["results"]):
            total += 1
            early += any(i < m for i, _ in a["deletions"])
            crossing += any(i < m and left > 64 for i, left in a["deletions"])
            other += list(a["swaps"]) != list(b["swaps"])
    print(which, "frames", total, "early deletion", early, "other exchanges under reversed rows", other, "crossing", crossing)
    assert early >= 0.25 * total and other >= 0.10 * total
    if which == "121_60":
        assert crossing >= 1


def test_constructed_frames_delete_rows_before_the_last_step():
    early = 0
    for k, n, R, style in REDUNDANT:
        c = WM.case(k, n, "random_dense", "float", R, style)
        early += sum(any(i < n - k for i, _ in r["deletions"]) for r in c["results"])
        assert all(len(r["deletions"]) == R - (n - k) for r in c["results"])
    assert early >= 1
