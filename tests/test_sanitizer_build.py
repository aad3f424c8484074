"""CPU sanitizer run: the library's host code and the C oracle compiled with
-fsanitize=address,undefined, and the host-side test files run against those builds in a child process.  A heap
overflow, use-after-free, signed overflow or misaligned access in the alist parser / GF(2) elimination / TEP tables /
CRC / oracle aborts the child.  Device code is out of reach of this (GPU sanitizers are not available on the pool)."""
import shutil

import pytest


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with libasan")
def test_host_code_and_abi5_binding_under_asan_ubsan():
    from short_ldpc_decoding_osd_amd import build
    r = build.run_asan_tests()
    tail = (r.stdout[-2500:] + "\n" + r.stderr[-2500:])
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and "ERROR: AddressSanitizer" not in tail and "runtime error" not in tail, tail
