"""Host side of the any-shape OSD entry points (ldpc_osdx_*): declarations, the TEP tables of other k, and the self-check of
the scan oracle the GPU tests rely on (tests/osdx_model.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import np_oracle
from short_ldpc_decoding_osd_amd import _lib
from tests import osdx_model
from tests import osd_family as OF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ldpc_osdx_supported", "ldpc_osdx_front", "ldpc_osdx_search", "ldpc_osdx_decode")


def test_header_and_binding_declare_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "ldpc_osd.h")).read()
    declared = set(re.findall(r"\b(ldpc_[A-Za-z0-9_]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared, name
        assert name in _lib.SYMBOLS, name
        assert hasattr(_lib.load(), name), name
    assert "OSD for short codes of any shape" in hdr


@pytest.mark.parametrize("k", [16, 48, 60])
@pytest.mark.parametrize("order", [0, 1, 2])
def test_tep_table_of_other_k(k, order):
    L = _lib.load()
    bounds = (C.c_int64 * (order + 1))()
    total = L.ldpc_tep_table(k, order, None, bounds)
    want = np_oracle.tep_table(k, order)
    assert total == len(want) and list(bounds) == np_oracle.tep_boundaries(k, order)
    sup = np.zeros((total, 3), np.uint8)
    assert L.ldpc_tep_table(k, order, sup.ctypes.data_as(C.POINTER(C.c_uint8)), None) == total
    got = [tuple(int(v) for v in row if v != 0xFF) for row in sup]
    assert got == want


@pytest.mark.parametrize("name", ["ldpc_96_48", "array_121_60", "short", "thin"])
def test_scan_oracle_self_check(name):
    assert OF.self_check(osdx_model, name)
