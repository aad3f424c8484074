"""-m gpu: osd_front_kernel as a frame pipeline (a grid of front_grid() workgroups that each decode frames b, b + grid, ...,
with the frame number two frames and the y row one frame ahead, G's columns in LDS) and the frame pipelines of the order-2
scan kernels at the same edges of their grid -- bit for bit against the C oracle (c_oracle.osd_front, conv_osd, fs_osd,
pb_osd) through ldpc_osd_front, ldpc_osd_search and ldpc_osd_decode.

The oracle decodes 256 distinct frames once: syndrome failures of NMS-10 at 2.5 dB, drawn as bench.py's CPU baseline draws
its frames.  Every launch reaches them through a repeating frame list (index[f] = f mod 256), or, where frames are taken
directly, through a y buffer whose row f is frame f mod 256, so any frame count costs the same 256 oracle frames and the
comparison runs on the device.

What each group is for:
  frame counts    0, 1, 2 and G - 1, G, G + 1, 2G, 2G + 1, 3G + 1 for the front end's grid and for the scan's: a workgroup
                  with no frame, one, two, three and four frames -- the pipeline's prologue alone, one and two trips with
                  nothing left to load, and the steady state -- on ldpc_osd_front, front + ldpc_osd_search, ldpc_osd_decode.
  count < F       a device-side count below the capacity: rows at and beyond the count keep their sentinel in every output,
                  and the tail of the frame list (all 0 / all F - 1: valid frames, but not the list's) changes nothing.
  index = NULL    frames taken directly, one count above both grids.
  other routes    FS-OSD and PB-OSD through ldpc_osd_decode (front end into the workspace, then their own scans) at G + 1.
  graph           one capture of front + search at 2G + 1 frames, replayed under two different device-side counts.

The grids are computed here from the rules the library states: front_grid() in csrc/ldpc_internal.h (kFrontGridX x 32
wavefronts per CU, capped by F) and grid2r() in csrc/ldpc_osd.hip (6 x 16 per CU, capped by F)."""
import numpy as np
import pytest
import torch

from oracle import c_oracle, np_oracle
from tests import osd_generators as Z
from tests.gpu_util import pack_np, to_dev
from tests.test_gpu_osd_generators import check_fs, check_pb

pytestmark = pytest.mark.gpu
NSRC = 256                    # distinct frames
FRONT_GRID_X = 1             # kFrontGridX (ldpc_internal.h)
SENT = dict(perm=0xEE, parity=-0x1234567, ns=-7, cw=-0x7654321, metric=123.0, best=-5, ntep=-9)
_CACHE = {}


@pytest.fixture(scope="module")
def dec():
    from short_ldpc_decoding_osd_amd import Code
    from short_ldpc_decoding_osd_amd.runtime import Decoder
    return Decoder(Code())


def grid(dec, which):
    cu = torch.cuda.get_device_properties(dec.device).multi_processor_count
    return cu * 32 * FRONT_GRID_X if which == "front" else cu * 16 * 6


def base(dec):
    """The 256 frames, their oracle results (host) and the expected outputs as device tensors: computed once, never changed."""
    if "base" in _CACHE:
        return _CACHE["base"]
    from short_ldpc_decoding_osd_amd.weights import STORED_NMS1_WEIGHT, softplus32
    G, H = np.asarray(dec.code.G), np.asarray(dec.code.H)
    y, cw = np_oracle.make_frames(G, 2.5, 1400, np.random.default_rng(20241020))
    soft = c_oracle.nms(H, y, 10, float(softplus32(STORED_NMS1_WEIGHT)))
    fail = np.flatnonzero(c_oracle.evaluate(H, soft, cw)[1])[:NSRC]
    assert len(fail) == NSRC
    y, cw = np.ascontiguousarray(y[fail]), np.ascontiguousarray(cw[fail])
    perm, Gp, ns = Z.front(G, y)
    r = c_oracle.conv_osd(G, y, cw, 2)
    assert (ns > 0).any() and (ns == 0).any()                    # frames with and without a column exchange
    want = dict(perm=to_dev(perm.astype(np.uint8), dec), parity=to_dev(Z.pack_rows(Gp[:, :, 64:]).view(np.int64), dec),
                ns=to_dev(ns.astype(np.int32), dec), cw=to_dev(pack_np(r["codeword"]).view(np.int64), dec),
                metric=to_dev(np.asarray(r["metric"], np.float32), dec), best=to_dev(np.asarray(r["best"], np.int32), dec))
    _CACHE["base"] = dict(y=y, cw=cw, yd=to_dev(y, dec), want=want)
    return _CACHE["base"]


def sources(dec, n):
    """(frame list index[f] = f mod 256 as int32, the same as int64 row numbers of the expected tensors)."""
    rows = torch.arange(n, device=dec.device) % NSRC
    return rows.to(torch.int32), rows


def same(got, want):
    if got.dtype == torch.float32:
        got, want = got.view(torch.int32), want.view(torch.int32)
    return torch.equal(got, want)


def check_front(b, got, rows, n, tag):
    for k, t in zip(("perm", "parity", "ns"), got):
        assert same(t[:n], b["want"][k][rows[:n]]), tag + (k,)


def check_scan(b, out, rows, n, tag):
    for k in ("cw", "metric", "best"):
        assert same(out[k][:n], b["want"][k][rows[:n]]), tag + (k,)
    assert bool((out["ntep"][:n] == 2081).all()), tag + ("ntep",)


def run_all(dec, b, yd, n, tag, **lists):
    """ldpc_osd_front, then ldpc_osd_search on its results (osd_search2r_kernel), then ldpc_osd_decode (osd_fused2r_kernel)."""
    rows = sources(dec, n)[1]
    front = dec.osd_front(yd, **lists)
    check_front(b, front, rows, n, tag + ("front",))
    check_scan(b, dec.osd_search(yd, front[0], front[1], dec.osd_params(2), **lists), rows, n, tag + ("search",))
    check_scan(b, dec.osd_decode(yd, 2, **lists), rows, n, tag + ("decode",))


COUNTS = [("small", 0, 0), ("small", 0, 1), ("small", 0, 2)] + [
    (which, m, d) for which in ("front", "scan") for m, d in ((1, -1), (1, 0), (1, 1), (2, 0), (2, 1), (3, 1))]


@pytest.mark.parametrize("which,mult,delta", COUNTS, ids=[f"{w}-{m}G{d:+d}" for w, m, d in COUNTS])
def test_frame_counts(dec, which, mult, delta):
    b = base(dec)
    if which == "small":          # 0, 1, 2 frames by a device-side count in buffers of three: a launch there is, also for no frame
        n = delta
        lists = dict(index=sources(dec, 3)[0], count=torch.tensor([n], dtype=torch.int32, device=dec.device), F=3)
    else:
        n = mult * grid(dec, which) + delta
        lists = dict(index=sources(dec, n)[0], F=n)
    run_all(dec, b, b["yd"], n, (which, n), **lists)


def _filled(dec, F):
    front = (torch.full((F, 128), SENT["perm"], dtype=torch.uint8, device=dec.device),
             torch.full((F, 64), SENT["parity"], dtype=torch.int64, device=dec.device),
             torch.full((F,), SENT["ns"], dtype=torch.int32, device=dec.device))
    scan = lambda: dict(cw=torch.full((F, 2), SENT["cw"], dtype=torch.int64, device=dec.device),          # noqa: E731
                        metric=torch.full((F,), SENT["metric"], dtype=torch.float32, device=dec.device),
                        best=torch.full((F,), SENT["best"], dtype=torch.int32, device=dec.device),
                        ntep=torch.full((F,), SENT["ntep"], dtype=torch.int32, device=dec.device))
    return front, scan


def _tail_untouched(front, outs, n, tag):
    for k, t in zip(("perm", "parity", "ns"), front):
        assert bool((t[n:] == SENT[k]).all()), tag + (k,)
    for name, out in outs.items():
        for k in ("cw", "metric", "best", "ntep"):
            assert bool((out[k][n:] == SENT[k]).all()), tag + (name, k)


@pytest.mark.parametrize("tail", ["zeros", "last"])
def test_count_below_capacity(dec, tail):
    """n = (scan grid) + 1 frames in buffers of F = 2 (scan grid) + 1: workgroups whose second frame lies below F but at or
    beyond the count.  y holds F rows, so every entry of the list's tail names a frame that exists."""
    b = base(dec)
    GS = grid(dec, "scan")
    n, F = GS + 1, 2 * GS + 1
    assert n > grid(dec, "front") + 1
    index, rows = sources(dec, F)
    yd = b["yd"][rows]                                                       # row f = frame f mod 256
    index = index.clone()
    index[n:] = 0 if tail == "zeros" else F - 1
    assert bool((index[n:] != (rows[n:] % NSRC).to(torch.int32)).any())
    count = torch.tensor([n], dtype=torch.int32, device=dec.device)
    front, scan = _filled(dec, F)
    lists = dict(index=index, count=count, F=F)
    dec.osd_front(yd, out=front, **lists)
    check_front(b, front, rows, n, (tail, "front"))
    outs = dict(search=dec.osd_search(yd, front[0], front[1], dec.osd_params(2), out=scan(), **lists),
                decode=dec.osd_decode(yd, 2, out=scan(), **lists))
    for name, out in outs.items():
        check_scan(b, out, rows, n, (tail, name))
    _tail_untouched(front, outs, n, (tail,))


def test_frames_taken_directly(dec):
    b = base(dec)
    n = grid(dec, "scan") + 1
    assert n > grid(dec, "front") + 1
    rows = sources(dec, n)[1]
    run_all(dec, b, b["yd"][rows], n, ("direct", n))


def test_fs_and_pb_routes(dec):
    """ldpc_osd_decode with the FS and the PB algorithm: osd_front_kernel into the stream's workspace, then their scans."""
    from short_ldpc_decoding_osd_amd import _lib
    b = base(dec)
    G = dec.code.G
    n = grid(dec, "front") + 1
    index, rows = sources(dec, n)
    sel = rows.cpu().numpy()
    th = (0.1, 6.5, 30.0)
    p = dec.osd_params(2, _lib.OSD_FS, fs_beta=th[0], fs_tau_e=th[1], fs_tau_psc=th[2], fs_reference_quirk=1)
    out = dec.osd_decode(b["yd"], 2, params=p, index=index, F=n)
    torch.cuda.synchronize()
    check_fs(out, c_oracle.fs_osd(G, b["y"], b["cw"], 2, *th), 1, ("fs",), sel)
    aux = torch.zeros((n, 4), dtype=torch.int32, device=dec.device)
    out = dec.osd_decode(b["yd"], 2, params=dec.osd_params(2, _lib.OSD_PB, snr_db=2.5, aux=aux), index=index, F=n)
    torch.cuda.synchronize()
    check_pb(out, aux, c_oracle.pb_osd(G, b["y"], b["cw"], 2, 2.5), ("pb",), sel)


def test_graph_replays_follow_the_count(dec):
    """front + search captured once at a capacity of 2G + 1 frames (G: the front end's grid); the count is device data, so a
    replay decodes as many frames as it holds then."""
    b = base(dec)
    GF = grid(dec, "front")
    F = 2 * GF + 1
    index, rows = sources(dec, F)
    count = torch.tensor([F], dtype=torch.int32, device=dec.device)
    front, scan = _filled(dec, F)
    out = scan()
    lists = dict(index=index, count=count, F=F)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        dec.osd_front(b["yd"], out=front, **lists)
        dec.osd_search(b["yd"], front[0], front[1], dec.osd_params(2), out=out, **lists)
    for n in (F, GF - 1):
        for k, t in zip(("perm", "parity", "ns"), front):
            t.fill_(SENT[k])
        for k in out:
            out[k].fill_(SENT[k])
        count.fill_(n)
        graph.replay()
        torch.cuda.synchronize()
        check_front(b, front, rows, n, ("graph", n))
        check_scan(b, out, rows, n, ("graph", n))
        _tail_untouched(front, dict(search=out), n, ("graph", n))
