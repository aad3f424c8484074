"""-m gpu: the order-2 rotation scan (osd_search2r_kernel, and osd_fused2r_kernel, which runs the same scan) against the
readlane scan, the table scan and the C oracle on inputs that exercise its survivor ring: frames whose bound never
tightens (many full batches, the ring restarts over and over), frames whose last batch fills exactly at round 32, and
quantised channel values (equal metrics, so the table-rank order of ties decides).

Which frames reach which case is decided on the host by a model of stage 1 (prefix metric, keep rule, batch points and
the bound after each batch) on the C oracle's front end, so the test states what it covers instead of hoping for it."""
import numpy as np
import pytest
import torch

from oracle import c_oracle, np_oracle
from tests.gpu_util import pack_np, to_dev, words_np

pytestmark = pytest.mark.gpu
F32 = np.float32


def _byte_sums(w_par):
    """lut[b][v] = sum of w_par[8b + t] over the set bits t of v, ascending t, from 0.0f (the canonical byte order)."""
    lut = np.zeros((8, 256), F32)
    for b in range(8):
        for v in range(256):
            acc = F32(0.0)
            for t in range(8):
                if (v >> t) & 1:
                    acc = F32(acc + w_par[8 * b + t])
            lut[b, v] = acc
    return lut


def stage1_model(G, y):
    """Per frame: (number of full batches, round at which the last full batch filled or 0, survivors of the last
    partial batch).  Round r pairs lane l with lane l - r (the other rotation direction pairs the same lanes)."""
    out = []
    lane = np.arange(64)
    for row in y:
        perm, Gp, _ = c_oracle.osd_front(G, row)
        yp = row[perm].astype(F32)
        w = np.abs(yp)
        hm = ~(yp[:64] > 0)
        hp = ~(yp[64:] > 0)
        P = Gp[:, 64:].astype(bool)                           # row i of P' as 64 parity bits
        d0 = (np.bitwise_xor.reduce(P[hm], axis=0) if hm.any() else np.zeros(64, bool)) ^ hp
        lut = _byte_sums(w[64:])
        byte = lambda D, b: int(np.dot(D[8 * b:8 * b + 8], 1 << np.arange(8)))

        def full(mrb, D, first=0, acc=None):
            acc = F32(mrb) if acc is None else acc
            for b in range(first, 8):
                acc = F32(acc + lut[b, byte(D, b)])
            return acc

        best = full(F32(0.0), d0)
        for l in range(64):
            best = min(best, full(w[l], d0 ^ P[l]))
        ring, nbatch, last = [], 0, 0
        for r in range(1, 33):
            m = (lane - r) & 63
            for l in range(64 if r < 32 else 32):
                D = d0 ^ P[l] ^ P[m[l]]
                acc = F32(F32(F32(w[l] + w[m[l]]) + lut[0, byte(D, 0)]) + lut[1, byte(D, 1)])
                if not acc > best:
                    ring.append((acc, D))
            if len(ring) >= 64:
                for acc, D in ring[:64]:
                    best = min(best, full(None, D, 2, acc))
                ring = ring[64:]
                nbatch, last = nbatch + 1, r
        out.append((nbatch, last, len(ring)))
    return np.array(out)


@pytest.fixture(scope="module")
def dec():
    from short_ldpc_decoding_osd_amd import Code
    from short_ldpc_decoding_osd_amd.runtime import Decoder
    return Decoder(Code())


def _all_routes_agree(dec, y, cw):
    yd = to_dev(y, dec)
    perm, parity, _ = dec.osd_front(yd)
    scan = dec.osd_search(yd, perm, parity, dec.osd_params(2))                          # osd_search2r_kernel
    fused = dec.osd_decode(yd, 2)                                                       # osd_fused2r_kernel
    table = dec.osd_decode(yd, 2, params=dec.osd_params(2, table_scan=True))
    readlane = dec.osd_decode(yd, 2, params=dec.osd_params(2, readlane_scan=True))
    torch.cuda.synchronize()
    for other in (fused, table, readlane):
        for k in ("cw", "metric", "best", "ntep"):
            assert torch.equal(scan[k], other[k]), k
    ref = c_oracle.conv_osd(dec.code.G, y, cw, 2)
    assert np.array_equal(scan["best"].cpu().numpy(), ref["best"])
    assert np.array_equal(words_np(scan["cw"]), pack_np(ref["codeword"]))
    assert np.array_equal(scan["metric"].cpu().numpy(), ref["metric"])


def _frames(dec, snr_db, frames, seed):
    return np_oracle.make_frames(dec.code.G, snr_db, frames, np.random.default_rng(seed))


def test_bound_never_tightens_many_batches(dec):
    """All |y| equal at 1.0 dB: prefixes are 2 + (set bits of parity bytes 0, 1), the bound stays high, most TEPs
    survive stage 1 and a frame runs many full batches (the ring is restarted after each)."""
    y, cw = _frames(dec, 1.0, 300, 501)
    y = np.sign(y).astype(F32)
    stats = stage1_model(dec.code.G, y[:40])
    assert stats[:, 0].max() >= 20 and stats[:, 0].min() >= 5
    _all_routes_agree(dec, y, cw)


def test_batch_fills_exactly_at_round_32(dec):
    """Frames whose ring reaches exactly 64 survivors in round 32 (a full batch after the last round, an empty final
    batch), mixed with frames of every other ending."""
    y, cw = _frames(dec, 1.0, 400, 502)
    y = (np.sign(y) * np.maximum(np.round(np.abs(y) * 2) / 2, 0.5)).astype(F32)
    stats = stage1_model(dec.code.G, y)
    at32 = (stats[:, 1] == 32) & (stats[:, 2] == 0)
    assert at32.sum() >= 1
    _all_routes_agree(dec, y, cw)


def test_quantised_ties(dec):
    """|y| on a coarse grid at 2.5 dB and 2.0 dB (many equal metrics: the table-rank order of ties decides)."""
    ya, ca = _frames(dec, 2.5, 500, 503)
    yb, cb = _frames(dec, 2.0, 500, 504)
    y, cw = np.concatenate([ya, yb]), np.concatenate([ca, cb])
    y = (np.sign(y) * np.maximum(np.round(np.abs(y) * 4) / 4, 0.25)).astype(F32)
    _all_routes_agree(dec, y, cw)
