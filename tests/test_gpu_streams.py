"""-m gpu: decode calls on DIFFERENT streams of ONE context must not disturb each other (include/ldpc_osd.h,
ldpc_ctx_create): the compaction uses no scratch, everything else a per-stream workspace.  Three pipelines with
different batches run concurrently on three streams; every output must equal the single-stream run.  The compaction
itself: ragged and unaligned inputs, and segments of more than one step per block (above 256 x 8192 flags), alone and with
the counters riding along.

Wall time on one MI355X: 5 s for the file's 10 cases; the slowest takes 1.3 s (test_three_streams_one_context[pb-3-72000]),
a compaction case 0.3 s at the most."""
import numpy as np
import pytest
import torch

from oracle import np_oracle
from tests.gpu_util import pack_np, to_dev

pytestmark = pytest.mark.gpu
ALPHA0 = 0.669435


@pytest.fixture(scope="module")
def dec():
    from short_ldpc_decoding_osd_amd import Code
    from short_ldpc_decoding_osd_amd.runtime import Decoder
    return Decoder(Code())


def _snapshot(pipe):
    n = int(pipe.count.cpu()[0])
    return dict(count=n, index=pipe.index[:n].cpu().numpy().copy(), cw=pipe.cw[:n].cpu().numpy().copy(),
                metric=pipe.metric[:n].cpu().numpy().copy(), ntep=pipe.ntep[:n].cpu().numpy().copy(),
                hard=pipe.hard.cpu().numpy().copy(), counters=pipe.counters().cpu().numpy().copy())


# ("pb", 3, 72000): ~6000 frames per stream search beyond the weight-1 head, more than the 4608 from which the chunk kernel's tail
# rule is on: every stream counts its own finished frames (control words of the stream's workspace) and hands searches on at
# moments that depend on the other streams' load
@pytest.mark.parametrize("algo,order,B", [("conv", 2, 40000), ("pb", 3, 6000), ("fs", 2, 20000), ("pb", 3, 72000)])
def test_three_streams_one_context(dec, algo, order, B):
    from short_ldpc_decoding_osd_amd import _lib
    from short_ldpc_decoding_osd_amd.pipeline import BatchPipeline
    algo_id = {"conv": _lib.OSD_CONVENTIONAL, "pb": _lib.OSD_PB, "fs": _lib.OSD_FS}[algo]
    pipes = []
    for lane in range(3):
        rng = np.random.default_rng(100 + lane)
        y, cw = np_oracle.make_frames(dec.code.G, 2.5, B - 1000 * lane, rng)    # different sizes: different block counts
        # keep_front=False: the OSD goes through ldpc_osd_decode and the stream's own workspace
        p = BatchPipeline(dec, y.shape[0], 10, ALPHA0, osd_order=order, osd_algo=algo_id, snr_db=2.5, keep_front=(lane != 1))
        pipes.append(p.bind(to_dev(y, dec), to_dev(pack_np(cw).view(np.int64), dec)))
    want = []
    for p in pipes:                      # reference: one after the other on the current stream
        p.reset_counters()
        p.run()
        torch.cuda.synchronize()
        want.append(_snapshot(p))
    streams = [torch.cuda.Stream() for _ in pipes]
    rounds = 4
    for p in pipes:
        p.reset_counters()
    torch.cuda.synchronize()
    for _ in range(rounds):              # all three in flight at once, several times
        for st, p in zip(streams, pipes):
            with torch.cuda.stream(st):
                p.run()
    torch.cuda.synchronize()
    for p, w in zip(pipes, want):
        got = _snapshot(p)
        assert got["count"] == w["count"]
        for k in ("index", "cw", "metric", "ntep", "hard"):
            assert np.array_equal(got[k], w[k]), k
        assert np.array_equal(got["counters"], rounds * w["counters"])


def test_compact_unaligned_and_ragged(dec):
    """The one-launch compaction: segment boundaries, a flag pointer that is not 16-byte aligned, empty and full inputs."""
    rng = np.random.default_rng(5)
    for B in (1, 7, 2047, 2048, 2049, 65536 + 13, 600001):
        base = torch.from_numpy((rng.random(B + 3) < 0.3).astype(np.uint8) * rng.integers(1, 255, B + 3).astype(np.uint8)).to(dec.device)
        for off in (0, 3):
            flag = base[off:off + B]
            index, count = dec.compact(flag)
            torch.cuda.synchronize()
            ref = np.flatnonzero(flag.cpu().numpy())
            n = int(count.cpu()[0])
            assert n == ref.size and np.array_equal(index[:n].cpu().numpy(), ref), (B, off)
    for val in (0, 1):
        flag = torch.full((5000,), val, dtype=torch.uint8, device=dec.device)
        index, count = dec.compact(flag)
        assert int(count.cpu()[0]) == 5000 * val
        if val:
            assert np.array_equal(index.cpu().numpy(), np.arange(5000))


COMPACT_ONE_STEP = 256 * 8192          # ldpc_util.hip: kMaxSeg segments of one step of compact_kernel<EVAL, 8> (1024 threads x 8 flags)


@pytest.mark.parametrize("B,steps", [(COMPACT_ONE_STEP, 1), (COMPACT_ONE_STEP + 1, 2), (3 * 2 ** 20 + 12345, 2),
                                     (4 * 2 ** 20 + 8192 + 5, 3)])
def test_compact_segments_of_several_steps(dec, B, steps):
    """Above 256 x 8192 flags a block of compact_kernel loops over its own segment (``c0 += kStep``, ``base += tot``): the
    last size with one step per block, the first with two, and sizes with two and three; count and list against torch.nonzero."""
    chunks = -(-B // 8192)
    assert -(-chunks // 256) == steps                   # compact_geometry(): steps per segment
    g = torch.Generator(device=dec.device).manual_seed(B)
    base = torch.where(torch.rand(B + 3, device=dec.device, generator=g) < 0.3,
                       torch.randint(1, 256, (B + 3,), device=dec.device, generator=g), 0).to(torch.uint8)
    for off in (0, 3):
        flag = base[off:off + B]
        index, count = dec.compact(flag)
        ref = torch.nonzero(flag).flatten().to(torch.int32)
        n = int(count.cpu()[0])
        assert n == ref.numel() and 0.29 * B < n < 0.31 * B and torch.equal(index[:n], ref), (B, off)


def test_counting_compaction_segments_of_two_steps(dec):
    """compact_kernel<true, 8> (ldpc_pipeline_run with labels) with two steps per segment: the NMS counters, the failure list
    and the OSD stage over it against the separate calls on the same frames, all on the device (the parts are pinned
    against the oracle at small sizes)."""
    from short_ldpc_decoding_osd_amd.pipeline import BatchPipeline
    B = COMPACT_ONE_STEP + 1 + 8192
    y, lab = dec.gen_frames(B, seed=20241020, snr_db=4.0)
    pipe = BatchPipeline(dec, B, 10, ALPHA0, osd_order=0, want_soft=False).bind(y, lab)
    pipe.index.fill_(-7)
    pipe.run()
    res = dec.nms(y, 10, ALPHA0, want_soft=False)
    five = dec.eval_counts(res["hard"], lab, res["fail"])
    ref = torch.nonzero(res["fail"]).flatten().to(torch.int32)
    nf = ref.numel()
    out = dec.osd_decode(y, 0, index=ref)
    three = dec.osd_counts(out["cw"], lab, index=ref, ntep=out["ntep"])
    torch.cuda.synchronize()
    c = pipe.counters()
    assert 0 < nf < B and int(c[0]) == B and int(c[4]) == nf
    assert torch.equal(pipe.hard, res["hard"]) and torch.equal(pipe.fail, res["fail"])
    assert torch.equal(c[:5], five) and torch.equal(c[5:], three)
    assert int(pipe.count[0]) == nf and torch.equal(pipe.index[:nf], ref) and bool((pipe.index[nf:] == -7).all())
    for k in ("cw", "metric", "best"):
        assert torch.equal(getattr(pipe, k)[:nf].view(torch.uint8), out[k].view(torch.uint8)), k
