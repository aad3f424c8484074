"""-m gpu: the device-side frame generator (ldpc_gen_frames) against the NumPy restatement of its stream contract
(tests/gen_model.py): labels word for word, channel values within a derived bound, and exact identities on the device's
own output (any split of a set, any stream, switched-off outputs, guard words, graph replay).

The bound on the channel values.  The inputs ua and tb of the transforms are exact on both sides (integer conversion, one
f32 rounding that NumPy reproduces), so the device differs from the float64 model by the errors of logf, sqrtf and
sincospif and by its own f32 roundings.  The ROCm installation carries no table of the HIP math API's ULP bounds to read
them from; the figures used here are the ones the HIP programming guide publishes for the device library (logf 1 ULP,
sqrtf 1 ULP, sinpif / cospif 1 ULP), each doubled to stay on the safe side:
  L = -2 logf(ua) <= 45.8 (ua >= 2^-33): relative error 2 ULP = 2.4e-7;
  r = sqrtf(L) <= 6.77: half of that plus 2 ULP of its own = 3.6e-7 relative, 2.4e-6 absolute;
  cospif / sinpif: 2 ULP of a value <= 1 = 2.4e-7 absolute, times r: 1.6e-6;
  the product r c: half an ULP of |z| <= 6.77 = 2.4e-7.
Together |z_dev - z| <= 4.3e-6 (the issue's estimate: below 6e-6).  A sample adds the rounding of sigma z (half an ULP of at
most 6.77 sigma: 2.4e-7 max(1, sigma)), of the sum v (|v| <= 0.8 .. 1 + 6.77 sigma: at most 4.8e-7 max(1, sigma) for sigma <= 1.2)
and nothing for the sign.  Total <= sigma 4.3e-6 + 7.2e-7 max(1, sigma) < 1e-5 max(1, sigma): the documented bounds do not give
a larger figure than the issue's, so the issue's bound is the one asserted.  Under fading the amplitude a = sqrtf(-logf(ua))
<= 4.8 carries 3 ULP relative (3.6e-7), mean a one more rounding, and v grows to mean a + 6.77 sigma: the same bound scaled
by max(1, mean a) of the sample covers it.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from oracle import c_oracle
from tests import gen_model
from tests.gpu_util import words_np

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA0 = 0.669435
SEED = 0x1234_5678_9ABC_DEF1            # (both key words non-zero)
CODES = {"ccsds": None,                                                  # (128,64)
         "ldpc_96_48": "tests/golden/LDPC_N96_K48_P8_set0_dmin10.alist",
         "array_121_80": "tests/golden/ArrayCode_N121_K80_r0.66.alist",   # n no multiple of 4, k > 64
         "code1": "tests/golden/code1.alist",                            # (64,32)
         "wimax": "tests/golden/wimax_1056_0.83.alist"}                  # n, k > 128: seven message blocks, G outside LDS
BIG0 = (1 << 32) - 100                   # the counter's high word changes inside the batch


@functools.lru_cache(maxsize=None)
def _dec(name):
    from short_ldpc_decoding_osd_amd import Code
    from short_ldpc_decoding_osd_amd.runtime import Decoder
    return Decoder(Code(os.path.join(ROOT, CODES[name])) if CODES[name] else Code())


@functools.lru_cache(maxsize=None)
def _model(name, B, frame0, rayleigh=False, fade_len=16):
    """bits, labels, z and amplitudes of the model for the set SEED: computed once, shared, never written."""
    m = gen_model.gen_frames(_dec(name).code.G, B, SEED, 1.0, mean=0.0, frame0=frame0, rayleigh=rayleigh, fade_len=fade_len)
    for a in m.values():
        a.setflags(write=False)
    return m


def _expect(m, sigma, mean):
    v = float(np.float32(mean)) * m["amp"] + float(np.float32(sigma)) * m["z"]
    return np.where(m["bits"] != 0, -v, v)


def _bits(t):
    """Bit pattern of a float tensor (so that -0.0 != 0.0 and NaNs compare)."""
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return all(torch.equal(_bits(x) if x.dtype == torch.float32 else x, _bits(y) if y.dtype == torch.float32 else y) for x, y in zip(a, b))


@pytest.mark.parametrize("frame0", [0, BIG0])
@pytest.mark.parametrize("B", [1, 63, 257])
@pytest.mark.parametrize("name", list(CODES))
def test_labels_exact_and_values_within_the_bound(name, B, frame0):
    dec, m = _dec(name), _model(name, B, frame0)
    assert (m["label_bits"] != 0).any()
    for sigma in (0.0, 0.5, 1.2):
        for mean in (1.0, 0.8):
            y, lab = dec.gen_frames(B, seed=SEED, sigma=sigma, mean=mean, frame0=frame0)
            torch.cuda.synchronize()
            assert np.array_equal(words_np(lab), m["label_bits"]), (sigma, mean)      # word for word, pad bits included
            got, want = y.cpu().numpy(), _expect(m, sigma, mean)
            err = float(np.abs(got.astype(np.float64) - want).max())
            print(f"{name} B={B} frame0={frame0} sigma={sigma} mean={mean}: max |y_dev - y_model| = {err:.3g}")
            assert err <= 1e-5 * max(1.0, sigma)
            if sigma == 0.0:
                assert np.array_equal(got, np.where(m["bits"] != 0, -np.float32(mean), np.float32(mean)))


@pytest.mark.parametrize("rayleigh", [False, True])
@pytest.mark.parametrize("name", ["ccsds", "array_121_80"])
def test_coded_set_is_the_signed_all_zeros_set_and_splits_concatenate(name, rayleigh):
    dec = _dec(name)
    kw = dict(seed=SEED, sigma=0.7, mean=0.8, rayleigh=rayleigh, fade_len=100)
    y, lab = dec.gen_frames(1000, frame0=BIG0 - 300, **kw)
    v, zero = dec.gen_frames(1000, frame0=BIG0 - 300, all_zeros=True, **kw)
    bits = dec.unpack_bits(lab, torch.uint8)
    assert not zero.any() and lab.any()
    assert torch.equal(_bits(y), _bits(torch.where(bits != 0, -v, v)))
    a = dec.gen_frames(600, frame0=BIG0 - 300, **kw)
    b = dec.gen_frames(400, frame0=BIG0 + 300, **kw)
    assert torch.equal(_bits(torch.cat([a[0], b[0]])), _bits(y)) and torch.equal(torch.cat([a[1], b[1]]), lab)
    other = dec.gen_frames(1000, frame0=BIG0 - 300, **{**kw, "seed": SEED + 1})
    assert not torch.equal(_bits(other[0]), _bits(y)) and not torch.equal(other[1], lab)
    assert (other[0] != y).float().mean() > 0.99
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        r1 = dec.gen_frames(1000, frame0=BIG0 - 300, **kw)
    with torch.cuda.stream(s2):
        r2 = dec.gen_frames(1000, frame0=BIG0 - 300, **kw)
    torch.cuda.synchronize()
    assert _same(r1, (y, lab)) and _same(r2, (y, lab))


@pytest.mark.parametrize("name,B,step", [("ccsds", 70001, 2000), ("array_121_80", 70003, 2000), ("wimax", 9001, 500)])
def test_large_batch_equals_small_batches(name, B, step):
    """The launcher gives a workgroup more frames per pass as the batch grows (from one pass of its 256 lanes up to 2048 noise
    blocks): a batch large enough for the upper end, and with a ragged last group, equals the concatenation of batches at
    the lower end -- the size at which the tests above compare against the model -- bit for bit."""
    dec = _dec(name)
    kw = dict(seed=SEED, sigma=0.9, mean=1.0)
    y, lab = dec.gen_frames(B, frame0=BIG0 - 5000, **kw)
    for s in range(0, B, step):
        e = min(B, s + step)
        py, pl = dec.gen_frames(e - s, frame0=BIG0 - 5000 + s, **kw)
        assert torch.equal(_bits(py), _bits(y[s:e])) and torch.equal(pl, lab[s:e]), s


@pytest.mark.parametrize("name,B", [("ccsds", 257), ("array_121_80", 63), ("wimax", 5)])
def test_switched_off_outputs_and_guard_words(name, B):
    dec = _dec(name)
    n, words = dec.n, dec.words
    kw = dict(seed=SEED, sigma=0.5, frame0=7)
    y, lab = dec.gen_frames(B, **kw)
    for off in (0, 1):      # off = 1: a y that is not 16-byte aligned takes the scalar stores -- same bits
        ybuf = torch.full((off + B * n + 1024,), -7.25, dtype=torch.float32, device=dec.device)
        lbuf = torch.full((off + B * words + 1024,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dec.device)
        out = dict(y=ybuf[off:off + B * n].view(B, n), label_bits=lbuf[off:off + B * words].view(B, words))
        dec.gen_frames(B, out=out, **kw)
        assert _same((out["y"], out["label_bits"]), (y, lab))
        assert (ybuf[:off] == -7.25).all() and (ybuf[off + B * n:] == -7.25).all()          # nothing before or past the buffers
        assert (lbuf[:off] == 0x5A5A5A5A5A5A5A5A).all() and (lbuf[off + B * words:] == 0x5A5A5A5A5A5A5A5A).all()
        # each output switched off on its own: the other unchanged, the buffer of the switched-off one untouched
        ybuf.fill_(-7.25)
        ry, rl = dec.gen_frames(B, want_y=False, out=out, **kw)
        assert ry is None and torch.equal(rl, lab) and (ybuf == -7.25).all()
        lbuf.fill_(0x5A5A5A5A5A5A5A5A)
        ry, rl = dec.gen_frames(B, want_labels=False, out=out, **kw)
        assert rl is None and torch.equal(_bits(ry), _bits(y)) and (lbuf == 0x5A5A5A5A5A5A5A5A).all()
    # the all-zeros set writes zero labels over the pattern, and only there
    lbuf.fill_(0x5A5A5A5A5A5A5A5A)
    dec.gen_frames(B, all_zeros=True, want_y=False, out=out, **kw)
    assert not out["label_bits"].any() and (lbuf[off + B * words:] == 0x5A5A5A5A5A5A5A5A).all()


@pytest.mark.parametrize("fade_len", [1, 16, 100, 10 ** 6])
@pytest.mark.parametrize("name", ["ccsds", "array_121_80"])
def test_rayleigh_against_the_model(name, fade_len):
    dec, B, frame0 = _dec(name), 63, BIG0 + 69
    m = _model(name, B, frame0, True, fade_len)
    assert m["amp"].max() <= 4.8
    for sigma, mean in ((0.5, 1.0), (1.2, 0.8)):
        y, lab = dec.gen_frames(B, seed=SEED, sigma=sigma, mean=mean, frame0=frame0, rayleigh=True, fade_len=fade_len)
        assert np.array_equal(words_np(lab), m["label_bits"])
        err = np.abs(y.cpu().numpy().astype(np.float64) - _expect(m, sigma, mean))
        tol = 1e-5 * max(1.0, sigma) * np.maximum(1.0, float(np.float32(mean)) * m["amp"])
        print(f"{name} fade_len={fade_len} sigma={sigma} mean={mean}: max err {err.max():.3g}, max err / tol {(err / tol).max():.3g}")
        assert (err <= tol).all()
    # sigma = 0: the samples of one fading block are bit-identical, neighbouring blocks differ
    y, _ = dec.gen_frames(B, seed=SEED, sigma=0.0, mean=1.0, frame0=frame0, rayleigh=True, fade_len=fade_len, all_zeros=True)
    flat = y.cpu().numpy().reshape(-1)
    q = (frame0 * dec.n + np.arange(flat.size, dtype=np.int64)) // fade_len
    same_block = q[1:] == q[:-1]
    assert np.array_equal(flat[1:][same_block], flat[:-1][same_block])
    assert (flat[1:][~same_block] != flat[:-1][~same_block]).all()
    assert (flat >= 0).all()
    assert np.abs(flat - m["amp"].reshape(-1)).max() <= 1e-5 * 4.8


def test_refusals_name_the_call():
    from short_ldpc_decoding_osd_amd import _lib
    dec = _dec("ccsds")
    ybuf = torch.full((4, dec.n), -7.25, dtype=torch.float32, device=dec.device)
    lbuf = torch.full((4, dec.words), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dec.device)
    yp, lp = C.c_void_p(ybuf.data_ptr()), C.c_void_p(lbuf.data_ptr())

    def call(B=4, null_p=False, **fields):
        p = _lib.GenParams(**{**dict(seed=1, frame0=0, sigma=0.5, mean=1.0, flags=0, fade_len=16), **fields})
        rc = dec.L.ldpc_gen_frames(dec._ctx, None if null_p else C.byref(p), B, yp, lp, None)
        return rc, (dec.L.ldpc_last_error() or b"").decode()

    bad = [dict(B=-1), dict(frame0=-1), dict(sigma=-0.5), dict(sigma=float("inf")), dict(sigma=float("nan")),
           dict(flags=_lib.GEN_F_RAYLEIGH, fade_len=0), dict(flags=_lib.GEN_F_RAYLEIGH, fade_len=-3), dict(flags=4),
           dict(flags=0x80000001), dict(null_p=True)]
    for kw in bad:
        rc, msg = call(**kw)
        assert rc == -1 and "ldpc_gen_frames" in msg, (kw, rc, msg)
    assert call(B=0)[0] == 0                                  # B = 0: LDPC_OK, no launch
    torch.cuda.synchronize()
    assert (ybuf == -7.25).all() and (lbuf == 0x5A5A5A5A5A5A5A5A).all()      # neither the refused calls nor B = 0 wrote
    assert call(flags=0, fade_len=0)[0] == 0                  # fade_len is read only with the Rayleigh flag
    torch.cuda.synchronize()
    assert (ybuf != -7.25).all() and (lbuf != 0x5A5A5A5A5A5A5A5A).all()
    with pytest.raises(ValueError, match="exactly one"):
        dec.gen_frames(4, seed=1)
    with pytest.raises(ValueError, match="exactly one"):
        dec.gen_frames(4, seed=1, snr_db=2.0, sigma=0.5)
    y, _ = dec.gen_frames(4, seed=1, snr_db=2.5)
    y2, _ = dec.gen_frames(4, seed=1, sigma=float(np.sqrt(1. / (2 * 0.5 * 10 ** 0.25))))
    assert torch.equal(_bits(y), _bits(y2))


def test_generated_frames_through_the_pipeline_and_the_cpu_oracle():
    """CCSDS at 2.5 dB: 20 000 generated frames through NMS-10 + order-2 OSD on the device, and the same y and labels, copied
    to the host, through the C oracle: equal counters."""
    from short_ldpc_decoding_osd_amd.pipeline import BatchPipeline
    dec, B = _dec("ccsds"), 20000
    y, lab = dec.gen_frames(B, seed=20241020, snr_db=2.5)
    pipe = BatchPipeline(dec, B, 10, ALPHA0, osd_order=2).bind(y, lab)
    pipe.reset_counters()
    pipe.run()
    torch.cuda.synchronize()
    c = pipe.counters().cpu().numpy()
    yh, cw = y.cpu().numpy(), dec.unpack_bits(lab, torch.uint8).cpu().numpy()
    soft = c_oracle.nms(dec.code.H, yh, 10, ALPHA0)
    _, fail, cnt = c_oracle.evaluate(dec.code.H, soft, cw)
    idx = np.flatnonzero(fail)
    ref = c_oracle.conv_osd(dec.code.G, yh[idx], cw[idx], 2)
    assert 0.1 * B < idx.size < 0.5 * B
    assert [int(x) for x in c[:5]] == [cnt[k] for k in ("frames", "frame_err", "bit_err", "undetected", "synd_fail")]
    assert int(c[5]) == idx.size and int(c[6]) == int((~ref["correct"]).sum())


def test_data_generating_device_forms():
    from short_ldpc_decoding_osd_amd import data_generating
    from short_ldpc_decoding_osd_amd import globalmap as GL
    dec = _dec("ccsds")
    keys = ("ALL_ZEROS_CODEWORD_TESTING", "ALL_ZEROS_CODEWORD_TRAINING", "Rayleigh_fading", "duration")
    saved = {k: GL.get_map(k, None) for k in keys}
    try:
        for k in keys:
            GL.del_map(k)
        y, lab = data_generating.testing_data_generating_device(dec, 2.5, 300, seed=9, frame0=11)
        assert _same((y, lab), dec.gen_frames(300, seed=9, snr_db=2.5, frame0=11)) and lab.any()
        GL.set_map("ALL_ZEROS_CODEWORD_TESTING", True)
        y0, lab0 = data_generating.testing_data_generating_device(dec, 2.5, 300, seed=9, frame0=11)
        assert not lab0.any() and torch.equal(_bits(y0), _bits(dec.gen_frames(300, seed=9, snr_db=2.5, frame0=11, all_zeros=True)[0]))
        GL.set_map("Rayleigh_fading", True)
        GL.set_map("duration", 2)
        yr, _ = data_generating.testing_data_generating_device(dec, 2.5, 300, seed=9, frame0=11)
        assert torch.equal(_bits(yr), _bits(dec.gen_frames(300, seed=9, snr_db=2.5, frame0=11, all_zeros=True, rayleigh=True, fade_len=32)[0]))
        GL.del_map("Rayleigh_fading")
        # training set: the blended sigma and mean of the host function
        sigma, mean = data_generating._training_channel(dec.n, dec.k, (2.0, 4.0))
        assert mean != 1 and sigma > 0
        yt, labt = data_generating.training_data_generating_device(dec, (2.0, 4.0), 300, seed=9)
        assert _same((yt, labt), dec.gen_frames(300, seed=9, sigma=float(sigma), mean=float(mean))) and labt.any()
        GL.set_map("ALL_ZEROS_CODEWORD_TRAINING", True)
        yz, labz = data_generating.training_data_generating_device(dec, (3.0, 3.0), 300, seed=9)
        assert not labz.any() and torch.equal(_bits(yz), _bits(dec.gen_frames(300, seed=9, snr_db=3.0, all_zeros=True)[0]))
    finally:
        for k, v in saved.items():
            GL.del_map(k) if v is None else GL.set_map(k, v)


def test_generator_and_nms_in_one_captured_graph():
    """One chain, no parallel branches: gen_frames then nms, captured and replayed, give the bits of the eager calls."""
    dec, B = _dec("ccsds"), 3000
    kw = dict(seed=SEED, snr_db=2.5, frame0=BIG0)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        y, lab = dec.gen_frames(B, **kw)
        res = dec.nms(y, 10, ALPHA0, want_soft=True)
    torch.cuda.synchronize()
    want = (y.clone(), lab.clone(), res["soft"].clone(), res["hard"].clone(), res["fail"].clone())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        dec.gen_frames(B, out=dict(y=y, label_bits=lab), **kw)
        dec.nms(y, 10, ALPHA0, out=res)
    for t in (y, lab, res["soft"], res["hard"], res["fail"]):
        t.zero_()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert _same((y, lab, res["soft"], res["hard"], res["fail"]), want)
