"""NumPy restatement of the frame generator's stream contract (include/ldpc_osd.h, 'Frame generator').
No GPU, no library: Philox4x32-10, the three streams, encoding with a dense G and the packing of ldpc_pack_bits.

The f32 steps of the contract (ua, tb) are done in np.float32; log, sqrt, cos(2 pi .) and sin(2 pi .) in float64, and so are
the products and sums of a sample.  The device rounds those to f32 with its own logf / sqrtf / sincospif: it agrees with this
model to a few ULP (tests/test_gpu_gen.py derives the bound), never bit for bit; the message bits and labels are exact.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S_MESSAGE, S_NOISE, S_FADE = 0, 1, 2


def philox4x32_10(counter, key):
    """counter: four broadcastable integer arrays (each < 2^32), key: two integers.  Returns four uint64 arrays (< 2^32)."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) for c in counter])
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2          # 32 x 32 -> 64 bit: no overflow
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & MASK
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def _key(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, seed >> 32


def _draw(seed, idx, block, stream):
    idx = np.asarray(idx, dtype=np.uint64)
    return philox4x32_10((idx & MASK, idx >> np.uint64(32), block, stream), _key(seed))


def ua(x):
    """float(x) 2^-32 + 2^-33 in f32: (0, 1]."""
    return np.asarray(x, dtype=np.uint64).astype(np.float32) * np.float32(2.0 ** -32) + np.float32(2.0 ** -33)


def tb(x):
    """float(x >> 8) 2^-24, exact: [0, 1)."""
    return (np.asarray(x, dtype=np.uint64) >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def message_bits(seed, frames, k):
    """[F, k] uint8: stream 0, block b = bits 128 b .., word w of a block = bits 32 w .., LSB first."""
    frames = np.asarray(frames, dtype=np.uint64).reshape(-1)
    kb = (k + 127) // 128
    words = np.stack(_draw(seed, frames[:, None], np.arange(kb, dtype=np.uint64)[None, :], S_MESSAGE), axis=-1)   # [F, kb, 4]
    bits = (words.reshape(len(frames), kb * 4, 1) >> np.arange(32, dtype=np.uint64)) & np.uint64(1)
    return bits.reshape(len(frames), kb * 128)[:, :k].astype(np.uint8)


def normals_of_block(seed, frames, block):
    """The four normals (float64) of noise block ``block`` of every frame: [F, 4]."""
    x0, x1, x2, x3 = _draw(seed, np.asarray(frames, dtype=np.uint64), block, S_NOISE)
    out = []
    for xa, xb in ((x0, x1), (x2, x3)):
        r = np.sqrt(-2.0 * np.log(ua(xa).astype(np.float64)))
        t = 2.0 * tb(xb).astype(np.float64)
        out += [r * np.cos(np.pi * t), r * np.sin(np.pi * t)]
    return np.stack(out, axis=-1)


def noise(seed, frames, n):
    """[F, n] float64 standard normals: stream 1, block b = columns 4 b .. 4 b + 3."""
    frames = np.asarray(frames, dtype=np.uint64).reshape(-1)
    nb = (n + 3) // 4
    z = normals_of_block(seed, frames[:, None], np.arange(nb, dtype=np.uint64)[None, :])   # [F, nb, 4]
    return z.reshape(len(frames), nb * 4)[:, :n]


def fade_amplitude(seed, q):
    """Rayleigh amplitude (float64) of fading block(s) q: stream 2, block 0, sqrt(-log ua(x0))."""
    x0 = _draw(seed, np.asarray(q, dtype=np.uint64), 0, S_FADE)[0]
    return np.sqrt(-np.log(ua(x0).astype(np.float64)))


def pack_bits(bits):
    """[F, n] 0/1 -> [F, ceil(n/64)] uint64, bit v in word v // 64 at position v % 64, pad bits zero."""
    bits = np.asarray(bits, dtype=np.uint64)
    F, n = bits.shape
    words = (n + 63) // 64
    pad = np.zeros((F, words * 64), dtype=np.uint64)
    pad[:, :n] = bits
    return (pad.reshape(F, words, 64) << np.arange(64, dtype=np.uint64)).sum(axis=2, dtype=np.uint64)


def gen_frames(G, B, seed, sigma, mean=1.0, frame0=0, all_zeros=False, rayleigh=False, fade_len=16):
    """The model of ldpc_gen_frames.  Returns dict(y [B, n] float64, label_bits [B, words] uint64, bits [B, n] uint8,
    amp [B, n] float64 (the fading amplitude of every sample; 1 without fading), z [B, n])."""
    G = np.asarray(G, dtype=np.int64)
    k, n = G.shape
    frames = np.uint64(frame0) + np.arange(B, dtype=np.uint64)
    sigma, mean = float(np.float32(sigma)), float(np.float32(mean))
    if all_zeros:
        bits = np.zeros((B, n), dtype=np.uint8)
    else:
        bits = (message_bits(seed, frames, k).astype(np.int64) @ G % 2).astype(np.uint8)
    z = noise(seed, frames, n)
    if rayleigh:
        sample = frames[:, None] * np.uint64(n) + np.arange(n, dtype=np.uint64)[None, :]     # (modulo 2^64)
        amp = fade_amplitude(seed, sample // np.uint64(fade_len))
    else:
        amp = np.ones((B, n))
    v = mean * amp + sigma * z
    return dict(y=np.where(bits != 0, -v, v), label_bits=pack_bits(bits), bits=bits, amp=amp, z=z)
