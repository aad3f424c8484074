"""No GPU: transpose8x8 (csrc/ldpc_bits.h), the 8x8 bit-block transposition that the OSD front end runs per lane, compiled as HOST
code into a small shared library and checked against the naive definition -- out byte i bit j = in byte j bit i -- on every
single-bit input, the identity block, the empty and the full block, and 10 000 random blocks."""
import ctypes
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = """
#include "ldpc_bits.h"
extern "C" void transpose8x8_many(const unsigned long long *in, unsigned long long *out, long n)
{
    for (long i = 0; i < n; ++i) out[i] = ldpc::transpose8x8(in[i]);
}
"""


def naive(x):
    bits = np.unpackbits(np.asarray(x, np.uint64).view(np.uint8).reshape(-1, 8, 1), axis=2, bitorder="little")   # [n, byte j, bit i]
    return np.packbits(bits.transpose(0, 2, 1), axis=2, bitorder="little").reshape(-1, 8).view(np.uint64)[:, 0]


def test_transpose8x8_against_naive(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "a host C++ compiler is needed"
    src, lib = tmp_path / "t8.cpp", tmp_path / "libt8.so"
    src.write_text(SRC)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I",
                    os.path.join(ROOT, "short_ldpc_decoding_osd_amd", "csrc"), str(src), "-o", str(lib)], check=True, capture_output=True)
    fn = ctypes.CDLL(str(lib)).transpose8x8_many
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long]
    single = np.uint64(1) << np.arange(64, dtype=np.uint64)
    ident = np.uint64(0x8040201008040201)
    rng = np.random.default_rng(8808)
    x = np.concatenate([single, [ident, np.uint64(0), ~np.uint64(0)], rng.integers(0, 1 << 64, size=10000, dtype=np.uint64)])
    x = np.ascontiguousarray(x, dtype=np.uint64)
    out = np.empty_like(x)
    fn(x.ctypes.data, out.ctypes.data, len(x))
    assert np.array_equal(naive(single), np.uint64(1) << (8 * (np.arange(64) % 8) + np.arange(64) // 8).astype(np.uint64))   # the definition itself
    assert out[64] == ident                                     # the identity block is symmetric
    assert np.array_equal(out, naive(x))
    back = np.empty_like(x)
    fn(out.ctypes.data, back.ctypes.data, len(x))
    assert np.array_equal(back, x)                              # an involution
