"""-m gpu: two promises of include/ldpc_osd.h on the OSD entry points, route by route.

1. The frame count read ON THE DEVICE: min(*d_count, F) frames are decoded -- counts of 0, 1, 2, 3, 5 (the kernels that
   keep two or three frames in flight, or four per workgroup), F - 1, F, and a count ABOVE the capacity, which must be
   truncated.  Rows below the count equal the same route run on an explicit list of exactly that length, bit for bit;
   every row at or beyond it keeps its sentinel.
2. Nullable outputs: every subset of {d_metric, d_best, d_ntep} (and params.d_aux for PB-OSD) left out; what is passed
   equals the all-present call bit for bit.

Safe by construction: every buffer a missed clamp could overrun (frame list, front-end results, all outputs, the
stream's workspaces) holds N > F frames and the count above the capacity is N, so a kernel that forgets the clamp
writes rows F .. N-1 of a sentinel-filled buffer and fails an assertion instead of leaving the buffers.  (The NMS,
pipeline and H-form halves of the contract: test_gpu_abi_contract_null.py.)"""
import ctypes as C
import itertools
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import c_oracle, np_oracle
from tests import abi_calls as A
from tests.gpu_util import pack_np, to_dev, words_np

pytestmark = pytest.mark.gpu
ALPHA0 = 0.669435
SNR = 2.5
NY, N, F = 400, 187, 150        # frames in d_y, listed frames (= size of every buffer), capacity
N3, F3 = 31, 24                 # order 3 (43 745 TEPs per frame)
CONV, FS, PB = 0, 1, 2
TABLE, PB_BLOCK, PB_REPLAY, READLANE, INSIDE = 1, 2, 4, 8, 16
DECODE, SEARCH = "ldpc_osd_decode", "ldpc_osd_search"

Route = namedtuple("Route", "name order algo flags y_frames entries F N")


def _route(name, order, algo, flags=0, y_frames=0, entries=(DECODE, SEARCH)):
    return Route(name, order, algo, flags, y_frames, entries, F3 if order == 3 else F, N3 if order == 3 else N)


ROUTES = [
    _route("conv0", 0, CONV), _route("conv1", 1, CONV), _route("conv2", 2, CONV),
    _route("conv2_table", 2, CONV, TABLE), _route("conv2_readlane", 2, CONV, READLANE), _route("conv3", 3, CONV),
    _route("fs1", 1, FS), _route("fs2", 2, FS),
    _route("pb2", 2, PB), _route("pb2_block", 2, PB, PB_BLOCK), _route("pb2_replay", 2, PB, PB_REPLAY),
    _route("pb2_front_inside", 2, PB, INSIDE, entries=(DECODE,)),
    _route("conv2_y_frames", 2, CONV, y_frames=NY), _route("pb2_y_frames", 2, PB, y_frames=NY),
]
IDS = [r.name for r in ROUTES]


def _counts(r):
    return (0, 1, 2, 3, 5, r.F - 1, r.F, r.N)


@pytest.fixture(scope="module")
def dec():
    from short_ldpc_decoding_osd_amd import Code
    from short_ldpc_decoding_osd_amd.runtime import Decoder
    return Decoder(Code())


@pytest.fixture(scope="module")
def data(dec):
    """NY NMS-10 failures at 2.5 dB as d_y; a list of N of them in a shuffled order; their front-end results."""
    rng = np.random.default_rng(2024)
    y, cw = np_oracle.make_frames(dec.code.G, SNR, 4000, rng)
    soft = c_oracle.nms(dec.code.H, y, 10, ALPHA0)
    _, fail, _ = c_oracle.evaluate(dec.code.H, soft, cw)
    idx = np.flatnonzero(fail)[:NY]
    assert idx.size == NY
    y, cw = y[idx], cw[idx]
    lst = np.random.default_rng(7).permutation(NY)[:N].astype(np.int32)
    assert (np.diff(lst) < 0).any() and (np.diff(lst) > 0).any()
    d = SimpleNamespace(y=y, cw=cw, list=lst, yd=to_dev(y, dec), index=to_dev(lst, dec))
    d.lab = dec.pack_bits(to_dev(cw, dec))
    d.perm, d.parity = A.sentinel(dec, (N, 128), torch.uint8), A.sentinel(dec, (N, 64), torch.int64)
    assert A.call(dec, "ldpc_osd_front", d_y=d.yd, d_index=d.index, F=N, d_perm=d.perm, d_parity=d.parity) == 0
    torch.cuda.synchronize()
    return d


def _count(dec, c):
    return torch.tensor([c], dtype=torch.int32, device=dec.device)


def _outputs(dec, r):
    """Sentinel-filled outputs for r.N frames."""
    o = dict(cw=A.sentinel(dec, (r.N, 2), torch.int64), metric=A.sentinel(dec, (r.N,), torch.float32),
             best=A.sentinel(dec, (r.N,), torch.int32), ntep=A.sentinel(dec, (r.N,), torch.int32))
    if r.algo == PB:
        o["aux"] = A.sentinel(dec, (r.N, 4), torch.int32)
    return o


def _run(dec, d, r, entry, nframes, count, o):
    """One call of `entry` on route r: frames d.index[0 .. nframes), or min(*count, nframes) of them.  Outputs missing
    from o are passed as NULL."""
    p = A.params(r.order, r.algo, r.flags, SNR, o.get("aux"), r.y_frames)
    kw = dict(d_y=d.yd, d_index=d.index, d_count=count, F=nframes, params=p, d_cw=o["cw"], d_metric=o.get("metric"),
              d_best=o.get("best"), d_ntep=o.get("ntep"))
    if entry == SEARCH:
        kw.update(d_perm=d.perm, d_parity=d.parity)
    rc = A.call(dec, entry, **kw)
    assert rc == 0, (r.name, entry, A.last_error(dec))


_oracle_cache = {}


def _against_oracle(dec, d, r, o):
    """Rows 0 .. r.F-1 of an explicit-list run against the C oracle of the route's algorithm."""
    sel = d.list[:r.F]
    key = (r.algo, r.order)
    if key not in _oracle_cache:
        fn = {CONV: lambda: c_oracle.conv_osd(dec.code.G, d.y[sel], d.cw[sel], r.order),
              FS: lambda: c_oracle.fs_osd(dec.code.G, d.y[sel], d.cw[sel], r.order),
              PB: lambda: c_oracle.pb_osd(dec.code.G, d.y[sel], d.cw[sel], r.order, SNR)}[r.algo]
        _oracle_cache[key] = fn()
    ref = _oracle_cache[key]
    got = {k: v[:r.F].cpu().numpy() for k, v in o.items()}
    names = {CONV: ("codeword", "metric", "best"), FS: ("codeword_ref", "metric_ref", "best_index"),
             PB: ("codeword", "metric", "best_index")}[r.algo]
    assert np.array_equal(got["cw"].view(np.uint64), pack_np(ref[names[0]])), r.name
    assert np.array_equal(got["metric"].view(np.uint32), ref[names[1]].view(np.uint32)), r.name
    assert np.array_equal(got["best"], ref[names[2]]), r.name
    assert np.array_equal(got["ntep"], np.full(r.F, ref["teps_size"]) if r.algo == CONV else ref["num_teps"]), r.name
    if r.algo == PB:
        assert np.array_equal(got["aux"], np.stack([ref[k] for k in ("comparisons", "suc1", "suc2", "stop")], axis=1)), r.name


def _reserve(dec, d, r):
    """Every workspace of the stream for r.N frames: the front-end results and the PB-OSD lists and records by
    ldpc_osd_reserve_stream, the checked copy of the list (y_frames) by one call on all r.N frames."""
    p = A.params(r.order, r.algo, r.flags, SNR, None, r.y_frames)
    assert dec.L.ldpc_osd_reserve_stream(dec._ctx, r.N, C.byref(p), dec._stream()) == 0, A.last_error(dec)
    _run(dec, d, r, DECODE, r.N, None, _outputs(dec, r))
    torch.cuda.synchronize()


def _same_rows(got, ref, n, what):
    for k in got:
        assert A.same_bits(got[k][:n], ref[k][:n]), (*what, k, "rows below the count")
        assert A.untouched(got[k], n), (*what, k, "rows at or beyond the count")


# ---------------------------------------------------------------------------------------------- 1. the device count
@pytest.mark.parametrize("r", ROUTES, ids=IDS)
def test_device_count_decode_and_search(dec, data, r):
    d = data
    _reserve(dec, d, r)
    if SEARCH not in r.entries:        # PB_FRONT_INSIDE keeps the front-end results inside the PB kernels
        o = _outputs(dec, r)
        p = A.params(r.order, r.algo, r.flags, SNR)
        rc = A.call(dec, SEARCH, d_y=d.yd, d_index=d.index, F=r.F, d_perm=d.perm, d_parity=d.parity, params=p, d_cw=o["cw"])
        assert rc == A.E_ARG and "ldpc_osd_search" in A.last_error(dec) and "PB_FRONT_INSIDE" in A.last_error(dec)
        torch.cuda.synchronize()
        assert all(A.untouched(t) for t in o.values())
    for entry in r.entries:
        full = _outputs(dec, r)
        _run(dec, d, r, entry, r.F, None, full)
        torch.cuda.synchronize()
        _against_oracle(dec, d, r, full)
        assert all(A.untouched(t, r.F) for t in full.values())
        for c in _counts(r):
            n = min(c, r.F)
            ref, got = _outputs(dec, r), _outputs(dec, r)
            if n:
                _run(dec, d, r, entry, n, None, ref)                  # an explicit list of exactly n frames
            _run(dec, d, r, entry, r.F, _count(dec, c), got)
            torch.cuda.synchronize()
            _same_rows(got, ref, n, (r.name, entry, c))
    assert dec.osd_index_errors() == 0


def test_device_count_front(dec, data):
    d = data

    def outs():
        return dict(perm=A.sentinel(dec, (N, 128), torch.uint8), parity=A.sentinel(dec, (N, 64), torch.int64),
                    nswaps=A.sentinel(dec, (N,), torch.int32))

    def run(nframes, count, o):
        assert A.call(dec, "ldpc_osd_front", d_y=d.yd, d_index=d.index, d_count=count, F=nframes, d_perm=o["perm"],
                      d_parity=o["parity"], d_nswaps=o.get("nswaps")) == 0, A.last_error(dec)

    full = outs()
    run(F, None, full)
    torch.cuda.synchronize()
    for f in range(0, F, 5):                                   # the explicit-list run against the C oracle
        perm, Gp, sw = c_oracle.osd_front(dec.code.G, d.y[d.list[f]])
        assert np.array_equal(full["perm"][f].cpu().numpy(), perm) and int(full["nswaps"][f]) == len(sw)
        par = np.packbits(Gp[:, 64:].astype(np.uint8), axis=1, bitorder="little").view(np.uint64)[:, 0]
        assert np.array_equal(words_np(full["parity"][f]), par)
    for c in (0, 1, 2, 3, 5, F - 1, F, N):
        n = min(c, F)
        ref, got = outs(), outs()
        if n:
            run(n, None, ref)
        run(F, _count(dec, c), got)
        torch.cuda.synchronize()
        _same_rows(got, ref, n, ("front", c))
    # d_nswaps NULL: the permutation and P' do not change
    got = outs()
    del got["nswaps"]
    run(F, None, got)
    torch.cuda.synchronize()
    _same_rows(got, full, F, ("front", "no nswaps"))


def _masks(rng, n):
    masks = np.zeros(n, dtype=np.uint64)
    for f in range(n):
        for p in rng.choice(64, size=int(rng.integers(0, 7)), replace=False):
            masks[f] |= np.uint64(1) << np.uint64(p)
    return masks


def test_device_count_and_nullable_tep_eval(dec, data):
    d = data
    masks = _masks(np.random.default_rng(78), N)
    md = to_dev(masks.view(np.int64), dec)

    def outs(keep=("metric", "hd")):
        o = dict(cw=A.sentinel(dec, (N, 2), torch.int64), metric=A.sentinel(dec, (N,), torch.float32),
                 hd=A.sentinel(dec, (N,), torch.int32))
        return {k: v for k, v in o.items() if k == "cw" or k in keep}

    def run(nframes, count, o):
        assert A.call(dec, "ldpc_osd_tep_eval", d_y=d.yd, d_index=d.index, d_count=count, F=nframes, d_perm=d.perm,
                      d_parity=d.parity, d_mask=md, d_cw=o["cw"], d_metric=o.get("metric"), d_hd=o.get("hd")) == 0, A.last_error(dec)

    full = outs()
    run(F, None, full)
    torch.cuda.synchronize()
    got_cw, got_m, got_hd = words_np(full["cw"]), full["metric"].cpu().numpy(), full["hd"].cpu().numpy()
    for f in range(0, F, 10):                                  # the explicit-list run against the NumPy restatement
        src = d.list[f]
        yp, _, Gp, pm, _ = np_oracle.swapped_info(d.y[src], d.cw[src], dec.code.G)
        hard = np.where(yp > 0, 0, 1).astype(np.int64)
        e = np.array([(int(masks[f]) >> p) & 1 for p in range(64)], dtype=np.int64)
        cand = ((hard[:64] + e) % 2).dot(Gp) % 2
        disc = (cand + hard) % 2
        assert got_hd[f] == disc.sum() and got_m[f] == np_oracle.weighted_distance(disc, np.abs(yp))
        orig = np.empty(128, dtype=np.int64)
        orig[pm] = cand
        assert np.array_equal(got_cw[f], pack_np(orig[None])[0])
    for c in (0, 1, 2, 3, 4, 5, F - 1, F, N):                  # (four frames per workgroup)
        n = min(c, F)
        ref, got = outs(), outs()
        if n:
            run(n, None, ref)
        run(F, _count(dec, c), got)
        torch.cuda.synchronize()
        _same_rows(got, ref, n, ("tep_eval", c))
    for keep in ((), ("metric",), ("hd",)):
        got = outs(keep)
        run(F, None, got)
        torch.cuda.synchronize()
        _same_rows(got, full, F, ("tep_eval", keep))


def test_device_count_and_nullable_osd_counts(dec, data):
    """ldpc_osd_counts adds exactly {min(count, F), wrong codewords, sum of d_ntep} -- nothing for TEPs without d_ntep --
    and addresses the labels directly without d_index."""
    d = data
    rng = np.random.default_rng(79)
    cw = pack_np(d.cw[d.list]).copy()                          # the listed frames' labels, a third of them spoiled
    wrong = rng.random(N) < 0.33
    cw[wrong, rng.integers(0, 2, size=int(wrong.sum()))] ^= np.uint64(1) << np.uint64(17)
    ntep = rng.integers(1, 50000, size=N).astype(np.int32)
    cwd, ntd = to_dev(cw.view(np.int64), dec), to_dev(ntep, dec)
    start = np.array([1000, 2000, 3000], dtype=np.int64)

    def run(count, **kw):
        counts = to_dev(start, dec)
        args = dict(d_cw=cwd, d_label_bits=d.lab, d_index=d.index, d_count=count, d_ntep=ntd, F=F, d_counts=counts)
        args.update(kw)
        assert A.call(dec, "ldpc_osd_counts", **args) == 0, A.last_error(dec)
        torch.cuda.synchronize()
        return counts.cpu().numpy() - start

    for c in (0, 1, 2, 3, 5, F - 1, F, N):
        n = min(c, F)
        assert run(_count(dec, c)).tolist() == [n, int(wrong[:n].sum()), int(ntep[:n].astype(np.int64).sum())], c
        assert run(_count(dec, c), d_ntep=None).tolist() == [n, int(wrong[:n].sum()), 0], c
    assert run(None).tolist() == [F, int(wrong[:F].sum()), int(ntep[:F].astype(np.int64).sum())]
    # direct addressing: codeword f against label f
    direct = to_dev(pack_np(d.cw[:N]).view(np.int64), dec)
    direct[::7, 1] ^= 1
    assert run(None, d_cw=direct, d_index=None).tolist() == [F, len(range(0, F, 7)), int(ntep[:F].astype(np.int64).sum())]
    assert run(None, d_cw=direct, d_index=None, d_ntep=None, F=N).tolist() == [N, len(range(0, N, 7)), 0]


@pytest.mark.parametrize("kernel", [1, 2], ids=["generic", "qc16"])
def test_device_count_traj_rows(dec, data, kernel):
    """ldpc_nms_traj_rows: rows of min(count, F) listed frames = the rows of ldpc_nms_decode's trajectory."""
    d = data
    T = 10
    a = A.alpha_array(ALPHA0, T)
    traj = torch.empty((T, NY, 128), dtype=torch.float32, device=dec.device)
    assert A.call(dec, "ldpc_nms_decode", d_llr=d.yd, B=NY, T=T, alpha=a, d_traj=traj, kernel=kernel) == 0, A.last_error(dec)
    idx = d.index.long()
    want = torch.cat([d.yd[idx].unsqueeze(1), traj[:, idx, :].permute(1, 0, 2)], dim=1)          # [N][T+1][128]
    soft_o = c_oracle.nms(dec.code.H, d.y[d.list[:8]], T, ALPHA0)
    assert np.array_equal(want[:8, T].cpu().numpy(), soft_o)
    for c in (0, 1, 2, 3, 4, 5, 15, 16, 17, F - 1, F, N):      # (four frames per wavefront, sixteen per workgroup)
        n = min(c, F)
        rows = A.sentinel(dec, (N, T + 1, 128), torch.float32)
        assert A.call(dec, "ldpc_nms_traj_rows", d_llr=d.yd, d_index=d.index, d_count=_count(dec, c), F=F, T=T, alpha=a,
                      d_rows=rows, kernel=kernel) == 0, A.last_error(dec)
        torch.cuda.synchronize()
        assert A.same_bits(rows[:n], want[:n]), (kernel, c)
        assert A.untouched(rows, n), (kernel, c)


def test_pipeline_count_written_by_the_library(dec, data):
    """ldpc_pipeline_run writes d_count itself: a batch whose frames all fail (count = B = capacity) and one whose frames
    all decode (count = 0: no OSD output is written, d_osd_counts does not move)."""
    from short_ldpc_decoding_osd_amd.pipeline import BatchPipeline
    d = data
    B = N
    rng = np.random.default_rng(80)
    yg, cwg = np_oracle.make_frames(dec.code.G, SNR, 600, rng)
    _, failg, _ = c_oracle.evaluate(dec.code.H, c_oracle.nms(dec.code.H, yg, 10, ALPHA0), cwg)
    good = np.flatnonzero(failg == 0)[:B]
    assert good.size == B
    inputs = {"all set": (d.y[:B], d.cw[:B], B), "all clear": (yg[good], cwg[good], 0)}
    for kw in (dict(keep_front=False), dict(keep_front=True), dict(osd_algo=FS, keep_front=False),
               dict(osd_algo=PB, snr_db=SNR, keep_front=True)):
        for name, (y, cw, nf) in inputs.items():
            pipe = BatchPipeline(dec, B, 10, ALPHA0, osd_order=2, **kw).bind(to_dev(y, dec), dec.pack_bits(to_dev(cw, dec)))
            outs = [pipe.cw, pipe.metric, pipe.best, pipe.ntep] + ([pipe.perm, pipe.parity] if pipe.perm is not None else [])
            for t in outs:
                t.fill_(A.SENT[t.dtype])
            pipe._counts[5:] = torch.tensor([11, 22, 33], device=dec.device)
            assert A.run_pipeline(dec, pipe._p) == 0, A.last_error(dec)
            torch.cuda.synchronize()
            assert int(pipe.count[0]) == nf, (kw, name)
            c = pipe.osd_counts.cpu().numpy() - [11, 22, 33]
            if nf == 0:
                assert all(A.untouched(t) for t in outs), (kw, name)
                assert c.tolist() == [0, 0, 0], (kw, name)
            else:
                assert np.array_equal(pipe.index.cpu().numpy(), np.arange(B)), (kw, name)
                wrong = int((words_np(pipe.cw) != pack_np(cw)).any(axis=1).sum())
                assert c.tolist() == [B, wrong, int(pipe.ntep.long().sum())], (kw, name)
                assert not any(bool((t == A.SENT[t.dtype]).any()) for t in outs), (kw, name)      # every row was written
                if "osd_algo" not in kw:
                    ref = c_oracle.conv_osd(dec.code.G, y, cw, 2)
                    assert np.array_equal(words_np(pipe.cw), pack_np(ref["codeword"])), (kw, name)


# ---------------------------------------------------------------------------------------- 2. nullable outputs (OSD)
@pytest.mark.parametrize("r", ROUTES, ids=IDS)
def test_nullable_outputs_decode_and_search(dec, data, r):
    d = data
    _reserve(dec, d, r)
    opt = ("metric", "best", "ntep")
    for entry in r.entries:
        full = _outputs(dec, r)
        _run(dec, d, r, entry, r.F, None, full)
        for k in range(len(opt) + 1):
            for keep in itertools.combinations(opt, k):
                for with_aux in ((True, False) if r.algo == PB else (False,)):
                    if len(keep) == 3 and with_aux == (r.algo == PB):
                        continue                               # that is `full`
                    got = {n: t for n, t in _outputs(dec, r).items() if n == "cw" or n in keep or (n == "aux" and with_aux)}
                    _run(dec, d, r, entry, r.F, None, got)
                    torch.cuda.synchronize()
                    _same_rows(got, full, r.F, (r.name, entry, keep, with_aux))
    assert dec.osd_index_errors() == 0
