"""CPU: the frame generator's stream contract as tests/gen_model.py restates it -- Philox known answers, the statistics of
the three streams -- and the binding of ldpc_gen_frames (symbol, struct layout against the header)."""
import ctypes as C
import os
import re

import numpy as np

from tests import gen_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 12345


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


def test_philox_known_answers():
    f = 0xFFFFFFFF
    assert _hex(gen_model.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert _hex(gen_model.philox4x32_10((f, f, f, f), (f, f))) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(gen_model.philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0))) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"
    # vectorised calls give the scalar answers
    out = gen_model.philox4x32_10((np.array([0, f]), np.array([0, f]), np.array([0, f]), np.array([0, f])), (0, 0))
    assert _hex(o[0] for o in out) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"


def test_uniform_maps_stay_in_range():
    x = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFF], dtype=np.uint64)
    u, t = gen_model.ua(x), gen_model.tb(x)
    assert u.dtype == np.float32 and t.dtype == np.float32
    assert u.min() == np.float32(2.0 ** -33) and u.max() == np.float32(1.0) and np.all(u > 0)
    assert t.min() == 0 and t.max() == np.float32(1.0 - 2.0 ** -24)
    x = np.random.default_rng(1).integers(0, 1 << 32, size=1 << 16, dtype=np.uint64)
    u = gen_model.ua(x)
    assert np.all((u > 0) & (u <= 1))
    # the largest radius: ua = 2^-33 -> |z| <= sqrt(66 ln 2) = 6.764
    assert np.sqrt(-2 * np.log(float(np.float32(2.0 ** -33)))) <= 6.77


def test_noise_moments():
    """seed 12345, frames 0 .. 2^20 - 1, noise block 0, z0 and z1: 2^21 samples; mean, variance and fourth moment within 4
    standard errors (6.9e-4, 9.8e-4, 6.8e-3) of 0, 1, 3."""
    z = gen_model.normals_of_block(SEED, np.arange(1 << 20, dtype=np.uint64), 0)[:, :2].reshape(-1)
    assert z.size == 1 << 21 and np.abs(z).max() <= 6.77
    m, v, m4 = z.mean(), z.var(), (z ** 4).mean()
    print("noise moments: mean %.3g variance %.6g fourth %.6g" % (m, v, m4))
    assert abs(m) <= 4 * 6.9e-4
    assert abs(v - 1) <= 4 * 9.8e-4
    assert abs(m4 - 3) <= 4 * 6.8e-3


def test_message_bits_are_balanced():
    bits = gen_model.message_bits(SEED, np.arange(1 << 16, dtype=np.uint64), 64)
    assert bits.shape == (1 << 16, 64) and set(np.unique(bits)) == {0, 1}
    share = bits.mean(axis=0)
    assert np.abs(share - 0.5).max() <= 4 * 0.5 / np.sqrt(1 << 16)
    # bit positions: word w of block b holds bits 128 b + 32 w .., LSB first; bits >= k are discarded, not shifted
    wide = gen_model.message_bits(SEED, np.arange(4, dtype=np.uint64), 200)
    assert np.array_equal(wide[:, :64], bits[:4])
    w = gen_model.philox4x32_10((3, 0, 1, 0), (SEED, 0))
    assert [int(b) for b in wide[3, 128:136]] == [(int(w[0]) >> i) & 1 for i in range(8)]
    assert [int(b) for b in wide[3, 192:200]] == [(int(w[2]) >> i) & 1 for i in range(8)]


def test_fading_amplitude_has_unit_power():
    a = gen_model.fade_amplitude(SEED, np.arange(1 << 20, dtype=np.uint64))
    assert a.min() >= 0 and a.max() <= 4.8
    assert abs((a ** 2).mean() - 1) <= 4 / np.sqrt(1 << 20)       # a^2 is exponential with mean 1, variance 1


def test_model_frames_are_a_function_of_the_frame_number(np_code):
    G = np_code.G
    whole = gen_model.gen_frames(G, 10, SEED, 0.7, mean=0.8, frame0=(1 << 32) - 4, rayleigh=True, fade_len=100)
    tail = gen_model.gen_frames(G, 4, SEED, 0.7, mean=0.8, frame0=(1 << 32) + 2, rayleigh=True, fade_len=100)
    assert np.array_equal(whole["y"][6:], tail["y"]) and np.array_equal(whole["label_bits"][6:], tail["label_bits"])
    assert not np.array_equal(whole["y"][3], whole["y"][4])      # (the counter's high word changes between these two)
    zero = gen_model.gen_frames(G, 10, SEED, 0.7, mean=0.8, frame0=(1 << 32) - 4, rayleigh=True, fade_len=100, all_zeros=True)
    assert not zero["label_bits"].any() and np.array_equal(np.where(whole["bits"] != 0, -zero["y"], zero["y"]), whole["y"])
    assert np.array_equal(whole["bits"] @ np_code.H.T % 2, np.zeros((10, np_code.H.shape[0])))
    assert np.array_equal(gen_model.pack_bits(whole["bits"]), whole["label_bits"])


def test_awgn_host_path_is_unchanged(np_code):
    """testing_data_generating with a seeded rng: the AWGN path draws normal(1, sigma) for the channel and then the message,
    bit for bit as before the device forms were added."""
    from short_ldpc_decoding_osd_amd import Code, data_generating
    from short_ldpc_decoding_osd_amd import globalmap as GL
    code = Code()
    for key in ("Rayleigh_fading", "ALL_ZEROS_CODEWORD_TESTING"):
        GL.del_map(key)
    y, lab = data_generating.testing_data_generating(code, 2.5, 7, rng=np.random.default_rng(5))
    rng = np.random.default_rng(5)
    sigma = np.sqrt(1. / (2 * (64. / 128.) * 10 ** (2.5 / 10)))
    ch = rng.normal(1, sigma, size=(7, 128))
    cw = rng.integers(0, 2, size=[7, 64]).dot(code.G) % 2
    assert np.array_equal(y, np.where(cw == 0, ch, -ch)) and np.array_equal(lab, cw)


def test_binding_of_gen_frames():
    """Fails without the feature: the symbol, the flags and the 32-byte struct in the header's field order."""
    from short_ldpc_decoding_osd_amd import _lib
    assert "ldpc_gen_frames" in _lib.SYMBOLS
    assert C.sizeof(_lib.GenParams) == 32
    hdr = open(os.path.join(ROOT, "include", "ldpc_osd.h")).read()
    m = re.search(r"typedef struct ldpc_gen_params \{(.*?)\} ldpc_gen_params;", hdr, re.S)
    names = re.findall(r"^\s*(?:uint64_t|int64_t|float|uint32_t|int32_t)\s+(\w+);", m.group(1), re.M)
    assert names == [n for n, _ in _lib.GenParams._fields_] == ["seed", "frame0", "sigma", "mean", "flags", "fade_len"]
    assert [getattr(_lib.GenParams, n).offset for n in names] == [0, 8, 16, 20, 24, 28]
    flags = dict(re.findall(r"#define LDPC_GEN_F_(\w+)\s+\(1u << (\d+)\)", hdr))
    assert {k: getattr(_lib, "GEN_F_" + k) for k in flags} == {k: 1 << int(v) for k, v in flags.items()} and len(flags) == 2
    assert getattr(_lib.load(), "ldpc_gen_frames") is not None
