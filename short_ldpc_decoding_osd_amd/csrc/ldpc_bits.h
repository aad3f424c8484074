// Bit-matrix helpers that are plain integer code: usable from device code and, compiled as host code, from a CPU test
// (tests/test_transpose8x8_host.py).  No HIP header is needed here.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LDPC_HOST_DEVICE __host__ __device__
#else
#define LDPC_HOST_DEVICE
#endif

namespace ldpc {

// Transpose of an 8x8 bit block held in one 64-bit word: in, byte j bit i = entry (i, j); out, byte i bit j = entry (i, j).
// Three delta swaps (the off-diagonal 1x1, 2x2 and 4x4 sub-blocks change places), 18 operations on 64-bit words.
LDPC_HOST_DEVICE inline unsigned long long transpose8x8(unsigned long long x)
{
    unsigned long long t;
    t = (x ^ (x >> 7)) & 0x00AA00AA00AA00AAull;  x ^= t ^ (t << 7);
    t = (x ^ (x >> 14)) & 0x0000CCCC0000CCCCull; x ^= t ^ (t << 14);
    t = (x ^ (x >> 28)) & 0x00000000F0F0F0F0ull; x ^= t ^ (t << 28);
    return x;
}

}  // namespace ldpc
