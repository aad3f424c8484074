"""Host side of the long H-form family (ldpc_hosdl_*), no GPU: the header, the binding and the exports agree, the entry points
refuse a NULL context by name, ldpc_hosdl_pattern_teps enumerates like itertools on bounds up to 192, and the NumPy
elimination equals the reference-made fixture of the long elimination (tests/golden/gf2elim_hform_long.npz)."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from oracle import np_oracle
from short_ldpc_decoding_osd_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ldpc_hosdl_supported", "ldpc_hosdl_pattern_teps", "ldpc_hosdl_front", "ldpc_hosdl_search", "ldpc_hosdl_sliding")


@pytest.fixture(scope="module")
def L():
    return _lib.load()


def test_header_binding_and_exports_agree(L):
    header = open(os.path.join(ROOT, "include", "ldpc_osd.h")).read()
    assert "#define LDPC_OSD_ABI_VERSION 5" in header and L.ldpc_abi_version() == 5
    for name in NAMES:
        assert len(re.findall(rf"\b{name}\(", header)) == 1, name
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    decl = {name: re.search(rf"{name}\((.*?)\);", header, re.S).group(1) for name in NAMES}
    for op in ("front", "search", "sliding"):                   # the parameters of the hosdw call, indices as uint16_t
        wide = re.search(rf"ldpc_hosdw_{op}\((.*?)\);", header, re.S).group(1)
        norm = lambda t: re.sub(r"\s+", " ", t).strip()   # noqa: E731
        assert norm(decl[f"ldpc_hosdl_{op}"]) == norm(wide).replace("uint8_t *d_lri", "uint16_t *d_lri").replace("uint8_t *d_uidx", "uint16_t *d_uidx")
        assert getattr(L, f"ldpc_hosdl_{op}").argtypes == getattr(L, f"ldpc_hosdw_{op}").argtypes
    assert "bit for bit, once the layouts are converted" in header


def test_null_context(L):
    assert L.ldpc_hosdl_supported(None) == 0
    fw = (C.c_float * 8)()
    calls = (("ldpc_hosdl_front", lambda: L.ldpc_hosdl_front(None, None, 1, None, None, None, None, None)),
             ("ldpc_hosdl_search", lambda: L.ldpc_hosdl_search(None, None, None, 1, None, None, None, None, None, 1, None, None, None, None,
                                                               None, None, None, None)),
             ("ldpc_hosdl_sliding", lambda: L.ldpc_hosdl_sliding(None, None, None, 1, None, None, None, None, None, 2, 1, 0.9, fw, 8, 0, None,
                                                                 None, None, None, None, None, None, None, None, None)))
    for who, call in calls:
        assert call() == -1 and L.ldpc_last_error().decode().startswith(f"{who}: bad arguments (ctx "), who


def _teps(L, fn, bounds, pattern):
    nseg = len(pattern)
    b, p = (C.c_int32 * (nseg + 1))(*bounds), (C.c_int32 * nseg)(*pattern)
    n = getattr(L, fn)(nseg, b, p, None)
    if n < 0:
        return n, None
    t = np.zeros((max(n, 1), 4), np.uint8)
    assert getattr(L, fn)(nseg, b, p, t.ctypes.data_as(C.POINTER(C.c_uint8))) == n
    return n, t[:n]


@pytest.mark.parametrize("bounds,pattern", [((0, 64, 150, 192), (1, 0, 1)), ((0, 100, 192), (2, 1)), ((120, 192), (2,)),
                                            ((0, 30, 130, 160, 192), (0, 1, 1, 1)), ((0, 192), (0,)), ((190, 192), (3,))])
def test_pattern_teps_equal_itertools(L, bounds, pattern):
    n, t = _teps(L, "ldpc_hosdl_pattern_teps", bounds, pattern)
    want = [sum(parts, ()) for parts in itertools.product(*[itertools.combinations(range(bounds[s], bounds[s + 1]), pattern[s])
                                                            for s in range(len(pattern))])]
    assert n == len(want)
    for row, pos in zip(t, want):
        assert row[3] == len(pos) and tuple(row[:len(pos)]) == pos and not row[len(pos):3].any()


def test_pattern_teps_limits(L):
    n, t = _teps(L, "ldpc_hosdl_pattern_teps", (0, 192), (1,))
    assert n == 192 and np.array_equal(t[:, 0], np.arange(192)) and (t[:, 3] == 1).all()
    assert _teps(L, "ldpc_hosdl_pattern_teps", (0, 193), (1,))[0] == -1 and "segment 0 = [0, 193)" in L.ldpc_last_error().decode()
    assert _teps(L, "ldpc_hosd_pattern_teps", (0, 129), (1,))[0] == -1          # the older entry point keeps its limit
    assert _teps(L, "ldpc_hosdl_pattern_teps", (0, 192), (4,))[0] == -5
    a, b = _teps(L, "ldpc_hosd_pattern_teps", (0, 40, 128), (1, 1)), _teps(L, "ldpc_hosdl_pattern_teps", (0, 40, 128), (1, 1))
    assert a[0] == b[0] and np.array_equal(a[1], b[1])


def test_numpy_elimination_equals_the_reference_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "gf2elim_hform_long.npz"))
    assert os.path.getsize(os.path.join(golden_dir, "gf2elim_hform_long.npz")) <= 496 * 1024
    gH = np_oracle.Code(os.path.join(golden_dir, "wimaxlike_N384_K192_P16_set0.alist")).H
    for p, H, frames, m in (("g", gH, 32, 192), ("r", z["r_H"].astype(np.int64), 16, 150)):
        x, order = z[p + "_x"], z[p + "_order"].astype(np.int64)
        assert x.shape == (frames, H.shape[1]) and x.dtype == np.float32
        assert np.array_equal(order, np.argsort(np.abs(x), axis=1, kind="stable"))
        for f in range(frames):
            R, swaps = np_oracle.gf2_eliminate(H[:, order[f]])
            ns = int(z[p + "_nswaps"][f])
            assert R.shape == (m, H.shape[1]) and len(swaps) == ns
            assert [tuple(int(v) for v in s) for s in swaps] == [tuple(int(v) for v in s) for s in z[p + "_swaps"][f][:ns]]
            assert np.array_equal(np.packbits(R[:, m:].astype(np.uint8), axis=1, bitorder="little"), z[p + "_M"][f])
    assert H.shape[0] == 192 and m == 150                                      # the second set: 42 rows deleted on the way
