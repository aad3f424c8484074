"""-m gpu: ldpc_osd_params.flags -- combinations the library refuses before it launches anything, and the OSD counters
of ldpc_pipeline_run, which do not depend on the route a call takes."""
import numpy as np
import pytest
import torch

from oracle import np_oracle
from tests.gpu_util import to_dev

pytestmark = pytest.mark.gpu
ALPHA0 = 0.669435
SENT_I = -7
SENT_CW = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def dec():
    from short_ldpc_decoding_osd_amd import Code
    from short_ldpc_decoding_osd_amd.runtime import Decoder
    return Decoder(Code())


def _rejected():
    """(name, order, algo, flags, entry points that refuse it)."""
    from short_ldpc_decoding_osd_amd import _lib as L
    CONV, FS, PB = L.OSD_CONVENTIONAL, L.OSD_FS, L.OSD_PB
    every = ("decode", "search", "reserve", "pipeline")
    return [
        ("unknown bit", 2, CONV, 1 << 5, every),
        ("unknown high bit", 3, PB, 1 << 31, every),
        ("table scan with FS", 2, FS, L.OSD_F_TABLE_SCAN, every),
        ("table scan with PB", 2, PB, L.OSD_F_TABLE_SCAN, every),
        ("readlane with FS", 2, FS, L.OSD_F_READLANE_SCAN, every),
        ("readlane with PB", 2, PB, L.OSD_F_READLANE_SCAN, every),
        ("readlane at order 1", 1, CONV, L.OSD_F_READLANE_SCAN, every),
        ("readlane at order 3", 3, CONV, L.OSD_F_READLANE_SCAN, every),
        ("readlane with table scan", 2, CONV, L.OSD_F_READLANE_SCAN | L.OSD_F_TABLE_SCAN, every),
        ("PB block with conventional", 2, CONV, L.OSD_F_PB_BLOCK, every),
        ("PB replay with FS", 2, FS, L.OSD_F_PB_REPLAY, every),
        ("PB front inside with conventional", 2, CONV, L.OSD_F_PB_FRONT_INSIDE, every),
        ("PB block with PB replay", 3, PB, L.OSD_F_PB_BLOCK | L.OSD_F_PB_REPLAY, every),
        ("PB front inside with PB replay", 3, PB, L.OSD_F_PB_FRONT_INSIDE | L.OSD_F_PB_REPLAY, every),
        ("PB front inside on the caller's front end", 3, PB, L.OSD_F_PB_FRONT_INSIDE, ("search", "pipeline_front")),
    ]


def _fill(out, aux):
    out["cw"].fill_(SENT_CW)
    out["metric"].fill_(float(SENT_I))
    out["best"].fill_(SENT_I)
    out["ntep"].fill_(SENT_I)
    aux.fill_(SENT_I)


def _untouched(out, aux):
    return (bool((out["cw"] == SENT_CW).all()) and bool((out["metric"] == float(SENT_I)).all()) and
            all(bool((out[k] == SENT_I).all()) for k in ("best", "ntep")) and bool((aux == SENT_I).all()))


def test_rejected_flag_combinations_launch_nothing(dec):
    from short_ldpc_decoding_osd_amd import _lib
    from short_ldpc_decoding_osd_amd.pipeline import BatchPipeline
    rng = np.random.default_rng(5)
    F = 64
    y, cw = np_oracle.make_frames(dec.code.G, 1.5, F, rng)
    yd, lab = to_dev(y, dec), dec.pack_bits(to_dev(cw, dec))
    perm, parity, _ = dec.osd_front(yd)
    torch.cuda.synchronize()
    e = dec.empty
    out = dict(cw=e((F, 2), torch.int64), metric=e((F,), torch.float32), best=e((F,), torch.int32), ntep=e((F,), torch.int32))
    aux = torch.empty((F, 4), dtype=torch.int32, device=dec.device)
    for name, order, algo, flags, where in _rejected():
        p = dec.osd_params(order, algo, snr_db=1.5, aux=aux)
        p.flags = flags
        calls = {
            "decode": lambda: dec.osd_decode(yd, order, params=p, out=out),
            "search": lambda: dec.osd_search(yd, perm, parity, p, out=out),
            "reserve": lambda: dec.osd_reserve_stream(F, p),
        }
        for entry in where:
            _fill(out, aux)
            if entry.startswith("pipeline"):
                pipe = BatchPipeline(dec, F, 10, ALPHA0, osd_order=order, osd_algo=algo, snr_db=1.5,
                                     keep_front=entry == "pipeline_front").bind(yd, lab)
                pipe._p.osd.flags = flags
                pipe._p.osd.d_aux = aux.data_ptr()
                for k in ("cw", "metric", "best", "ntep"):
                    getattr(pipe, k).copy_(out[k])
                with pytest.raises(_lib.LdpcError, match="OSD|flag|order"):
                    pipe.run()
                torch.cuda.synchronize()
                assert _untouched({k: getattr(pipe, k) for k in out}, aux), (name, entry)
                assert int(pipe.counters().abs().sum().cpu()) == 0, (name, entry)
            else:
                with pytest.raises(_lib.LdpcError, match="OSD_F_|flags"):
                    calls[entry]()
                torch.cuda.synchronize()
                assert _untouched(out, aux), (name, entry)


def test_accepted_flag_combinations_still_run(dec):
    """TABLE_SCAN names the route orders 0, 1 and 3 take anyway; PB_FRONT_INSIDE | PB_BLOCK is the chunk kernel from the
    first TEP with the front end inside: both stay accepted and equal their flag-free twins."""
    from short_ldpc_decoding_osd_amd import _lib
    rng = np.random.default_rng(6)
    y, _ = np_oracle.make_frames(dec.code.G, 1.5, 300, rng)
    yd = to_dev(y, dec)
    for order in (0, 1, 3):
        a = dec.osd_decode(yd, order, params=dec.osd_params(order))
        b = dec.osd_decode(yd, order, params=dec.osd_params(order, table_scan=True))
        torch.cuda.synchronize()
        for k in a:
            assert torch.equal(a[k], b[k]), (order, k)
    a = dec.osd_decode(yd, 2, params=dec.osd_params(2, _lib.OSD_PB, snr_db=1.5, pb_path="block"))
    b = dec.osd_decode(yd, 2, params=dec.osd_params(2, _lib.OSD_PB, snr_db=1.5, pb_path="block", pb_front_inside=True))
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_pipeline_osd_counts_do_not_depend_on_the_route(dec):
    """d_osd_counts = {frames, wrong, TEPs} is the same for the fused order-2 kernel, front end + osd_search2r (both count
    inside the scan), the readlane and the table scan (ldpc_osd_counts after the search); TEPs are counted only with
    d_ntep, as ldpc_osd_counts does."""
    from short_ldpc_decoding_osd_amd.pipeline import BatchPipeline
    rng = np.random.default_rng(72)
    B = 3000
    y, cw = np_oracle.make_frames(dec.code.G, 2.0, B, rng)
    yd, lab = to_dev(y, dec), dec.pack_bits(to_dev(cw, dec))
    routes = {"fused": dict(keep_front=False), "search2r": dict(keep_front=True),
              "readlane": dict(keep_front=True, readlane_scan=True), "table": dict(keep_front=False, table_scan=True)}
    seen = {}
    for with_ntep in (True, False):
        for name, kw in routes.items():
            pipe = BatchPipeline(dec, B, 10, ALPHA0, osd_order=2, **kw).bind(yd, lab)
            if not with_ntep:
                pipe._p.d_ntep = None
            pipe.reset_counters()
            pipe.run()
            torch.cuda.synchronize()
            seen[(with_ntep, name)] = pipe.osd_counts.cpu().numpy().copy()
            nf = int(pipe.count.cpu()[0])
    for with_ntep in (True, False):
        ref = seen[(with_ntep, "fused")]
        assert ref[0] == nf > 0 and ref[2] == (nf * 2081 if with_ntep else 0), (with_ntep, ref)
        for name in routes:
            assert np.array_equal(seen[(with_ntep, name)], ref), (with_ntep, name, seen[(with_ntep, name)], ref)
