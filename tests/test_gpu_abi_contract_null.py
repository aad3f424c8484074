"""-m gpu: the nullable outputs of the NMS, pipeline and H-form entry points of include/ldpc_osd.h, and the refusal of a
NULL in every pointer the header requires (the OSD half, and the device-side frame count: test_gpu_abi_contract.py).

An output left out must change nothing else: what is passed equals the all-present call bit for bit, the counters of a
stage that was switched off do not move.  A required pointer left out is LDPC_E_ARG with a message that names the entry
point, and nothing is launched: every output keeps its sentinel."""
import itertools
import os

import numpy as np
import pytest
import torch

from oracle import c_oracle, np_oracle
from tests import abi_calls as A
from tests import dlosd_model as DM
from tests.gpu_util import pack_np, to_dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA0 = 0.669435
SNR = 2.5
CONV, FS, PB = 0, 1, 2


@pytest.fixture(scope="module")
def dec():
    from short_ldpc_decoding_osd_amd import Code
    from short_ldpc_decoding_osd_amd.runtime import Decoder
    return Decoder(Code())


def _same(got, full, what):
    for k in got:
        assert A.same_bits(got[k], full[k]), (*what, k)


# ------------------------------------------------------------------------------------------------------------- NMS
def _nms_outputs(d, B, T):
    return dict(d_soft=A.sentinel(d, (B, d.n), torch.float32), d_traj=A.sentinel(d, (max(T, 1), B, d.n), torch.float32),
                d_hard=A.sentinel(d, (B, d.words), torch.int64), d_fail=A.sentinel(d, (B,), torch.uint8))


def _nms_subsets(d, y, T, alpha, kernel):
    """All 16 subsets of the four outputs; the all-present call against the C oracle (exact: np.array_equal, which takes
    +0 and -0 for equal, as tests/test_gpu_nms.py does)."""
    B = y.shape[0]
    yd, a = to_dev(y, d), A.alpha_array(alpha, T)
    full = _nms_outputs(d, B, T)
    assert A.call(d, "ldpc_nms_decode", d_llr=yd, B=B, T=T, alpha=a, kernel=kernel, **full) == 0, A.last_error(d)
    torch.cuda.synchronize()
    soft_o, traj_o = c_oracle.nms(d.code.H, y, T, alpha, want_traj=True)
    hard_o, fail_o, _ = c_oracle.evaluate(d.code.H, soft_o, None)
    assert np.array_equal(full["d_soft"].cpu().numpy(), soft_o)
    if T:
        assert np.array_equal(full["d_traj"].cpu().numpy(), traj_o[1:])
    else:
        assert A.untouched(full["d_traj"])
    assert np.array_equal(full["d_hard"].cpu().numpy().view(np.uint64), pack_np(hard_o))
    assert np.array_equal(full["d_fail"].cpu().numpy(), fail_o)
    names = tuple(full)
    for k in range(len(names)):
        for keep in itertools.combinations(names, k):
            got = {n: t for n, t in _nms_outputs(d, B, T).items() if n in keep}
            rc = A.call(d, "ldpc_nms_decode", d_llr=yd, B=B, T=T, alpha=a, kernel=kernel, **got)
            assert rc == 0, (keep, A.last_error(d))            # the empty set too: the call succeeds and writes nothing
            torch.cuda.synchronize()
            _same(got, full, (kernel, T, keep))


@pytest.mark.parametrize("kernel", [1, 2], ids=["generic", "qc16"])
@pytest.mark.parametrize("T", [0, 1, 10])
def test_nms_nullable_outputs_ccsds(dec, kernel, T):
    y, _ = np_oracle.make_frames(dec.code.G, SNR, 37, np.random.default_rng(300 + T))     # 37: a ragged last wavefront
    _nms_subsets(dec, y, T, ALPHA0, kernel)


@pytest.mark.parametrize("alist", ["LDPC_N96_K48_P8_set0_dmin10.alist", "ArrayCode_N121_K60_r0.50.alist"])
def test_nms_nullable_outputs_generic_codes(alist):
    from short_ldpc_decoding_osd_amd import Code
    from short_ldpc_decoding_osd_amd.runtime import Decoder
    d = Decoder(Code(os.path.join(ROOT, "tests", "golden", alist)))
    y, _ = np_oracle.make_frames(d.code.G, 3.0, 37, np.random.default_rng(5))
    _nms_subsets(d, y, 3, 0.75, 1)


# -------------------------------------------------------------------------------------------------------- pipeline
PIPE_ROUTES = {"conv2_fused": dict(keep_front=False), "conv2_front": dict(keep_front=True),
               "fs2": dict(osd_algo=FS, keep_front=False), "pb2": dict(osd_algo=PB, snr_db=SNR, keep_front=True)}
NMS0, OSD0 = [101, 102, 103, 104, 105], [11, 22, 33]


@pytest.fixture(scope="module")
def batch(dec):
    y, cw = np_oracle.make_frames(dec.code.G, SNR, 400, np.random.default_rng(81))
    return to_dev(y, dec), dec.pack_bits(to_dev(cw, dec))


def _pipe(dec, batch, osd=True, **kw):
    """A bound pipeline whose outputs hold sentinels and whose counters start from NMS0 / OSD0."""
    from short_ldpc_decoding_osd_amd.pipeline import BatchPipeline
    pipe = BatchPipeline(dec, 400, 10, ALPHA0, osd_order=2 if osd else None, **kw).bind(*batch)
    names = ["soft", "hard", "fail"] + (["index", "cw", "metric", "best", "ntep", "perm", "parity", "aux"] if osd else [])
    outs = {n: getattr(pipe, n) for n in names if getattr(pipe, n) is not None}
    for t in outs.values():
        t.fill_(A.SENT[t.dtype])
    pipe._counts.copy_(torch.tensor(NMS0 + OSD0))
    return pipe, outs


@pytest.mark.parametrize("route", list(PIPE_ROUTES), ids=list(PIPE_ROUTES))
def test_pipeline_nullable_members(dec, batch, route):
    kw = PIPE_ROUTES[route]
    ref, full = _pipe(dec, batch, **kw)
    assert A.run_pipeline(dec, ref._p) == 0, A.last_error(dec)
    torch.cuda.synchronize()
    nf = int(ref.count[0])
    cnt_full = ref.counters().cpu().numpy()
    assert 50 < nf < 200 and cnt_full[0] - NMS0[0] == 400 and cnt_full[5] - OSD0[0] == nf
    assert cnt_full[7] - OSD0[2] == int(ref.ntep[:nf].long().sum()) > 0
    members = ("d_soft", "d_label_bits", "d_nms_counts", "d_osd_counts", "d_metric", "d_best", "d_ntep")
    for null in [(m,) for m in members] + [members]:
        pipe, outs = _pipe(dec, batch, **kw)
        for m in null:
            setattr(pipe._p, m, None)
            outs.pop(m[2:], None)
        assert A.run_pipeline(dec, pipe._p) == 0, (null, A.last_error(dec))
        torch.cuda.synchronize()
        assert int(pipe.count[0]) == nf, null
        _same(outs, full, (route, null))
        for m in null:                                          # a buffer that was not passed was not written
            assert m[2:] not in full or A.untouched(getattr(pipe, m[2:])), (route, null, m)
        cnt = pipe.counters().cpu().numpy()
        nms_on = "d_label_bits" not in null and "d_nms_counts" not in null
        osd_on = "d_label_bits" not in null and "d_osd_counts" not in null
        assert np.array_equal(cnt[:5], cnt_full[:5] if nms_on else NMS0), (route, null)
        want = list(cnt_full[5:]) if osd_on else OSD0
        if osd_on and "d_ntep" in null:
            want[2] = OSD0[2]                                   # teps_total moves only with d_ntep, on every route
        assert cnt[5:].tolist() == [int(v) for v in want], (route, null)


def test_pipeline_without_the_osd_stage(dec, batch):
    """osd_enable = 0: every OSD member is NULL; NMS outputs and counters as with the stage on."""
    ref, full = _pipe(dec, batch, keep_front=False)
    assert A.run_pipeline(dec, ref._p) == 0, A.last_error(dec)
    pipe, outs = _pipe(dec, batch, osd=False)
    p = pipe._p
    assert p.osd_enable == 0 and not any((p.d_index, p.d_count, p.d_perm, p.d_parity, p.d_cw, p.d_metric, p.d_best, p.d_ntep,
                                          p.d_osd_counts))
    assert A.run_pipeline(dec, p) == 0, A.last_error(dec)
    torch.cuda.synchronize()
    _same(outs, full, ("no osd",))
    assert torch.equal(pipe.nms_counts, ref.nms_counts) and pipe.osd_counts.tolist() == OSD0


@pytest.mark.parametrize("missing", ["d_perm", "d_parity"])
def test_pipeline_refuses_one_of_perm_and_parity(dec, batch, missing):
    pipe, outs = _pipe(dec, batch, keep_front=True)
    setattr(pipe._p, missing, None)
    assert A.run_pipeline(dec, pipe._p) == A.E_ARG
    assert "ldpc_pipeline_run" in A.last_error(dec) and missing in A.last_error(dec)
    torch.cuda.synchronize()
    assert all(A.untouched(t) for t in outs.values())
    assert pipe.counters().tolist() == NMS0 + OSD0


# ----------------------------------------------------------------------------------------------------------- H-form
@pytest.fixture(scope="module")
def hform(dec):
    """200 frames on the convention path of tests/test_gpu_dlosd.py: ordering values = NMS-8 posteriors, metric = channel
    values, the TEP blocks of query_convention_path(3), the front-end results."""
    from short_ldpc_decoding_osd_amd.ordered_statistics_decoding import _teps_from_matrix, query_convention_path
    Fh = 200
    y, cw = np_oracle.make_frames(dec.code.G, 2.7, Fh, np.random.default_rng(41))
    x = c_oracle.nms(dec.code.H, y, 8, ALPHA0)
    _, b = np_oracle.segment_boundaries(64, 6)
    ranges = [range(int(b[i]), int(b[i + 1])) for i in range(6)]
    blocks = [np_oracle.error_pattern_gen(p + [0, 0, 0], ranges, 64) for p in query_convention_path(3)]
    off = np.insert(np.cumsum([len(E) for E in blocks]), 0, 0).astype(np.int32)
    h = dict(d_order_llr=to_dev(x, dec), d_metric_llr=to_dev(y, dec), F=Fh,
             d_teps=to_dev(np.concatenate([_teps_from_matrix(E) for E in blocks]), dec), d_block_off=to_dev(off, dec),
             nblk=len(blocks), d_label_bits=to_dev(pack_np(cw).view(np.int64), dec))
    front = _hfront_outputs(dec, Fh)
    assert A.call(dec, "ldpc_hosd_front", d_order_llr=h["d_order_llr"], F=Fh, **front) == 0, A.last_error(dec)
    torch.cuda.synchronize()
    assert int(front["d_nswaps"].min()) >= 0
    h.update({k: front[k] for k in ("d_lri", "d_uidx", "d_M")})
    return h, front


def _hfront_outputs(dec, Fh):
    return dict(d_lri=A.sentinel(dec, (Fh, 128), torch.uint8), d_uidx=A.sentinel(dec, (Fh, 128), torch.uint8),
                d_M=A.sentinel(dec, (Fh, 64), torch.int64), d_nswaps=A.sentinel(dec, (Fh,), torch.int32))


def _hsearch_outputs(dec, Fh, nblk):
    return dict(d_block_min=A.sentinel(dec, (Fh, nblk), torch.float32), d_block_arg=A.sentinel(dec, (Fh, nblk), torch.int32),
                d_truth=A.sentinel(dec, (Fh,), torch.float32), d_cw=A.sentinel(dec, (Fh, 2), torch.int64),
                d_metric=A.sentinel(dec, (Fh,), torch.float32), d_best=A.sentinel(dec, (Fh,), torch.int32))


def _hsliding_outputs(dec, Fh):
    return dict(d_deep_limit=A.sentinel(dec, (Fh,), torch.int32), d_global_min=A.sentinel(dec, (Fh,), torch.float32),
                d_truth=A.sentinel(dec, (Fh,), torch.float32), d_success=A.sentinel(dec, (Fh,), torch.uint8),
                d_cw=A.sentinel(dec, (Fh, 2), torch.int64), d_metric=A.sentinel(dec, (Fh,), torch.float32),
                d_best=A.sentinel(dec, (Fh,), torch.int32), d_teps_evaluated=A.sentinel(dec, (Fh,), torch.int32))


def _sliding_args(win=3):
    w = np.ascontiguousarray(np.concatenate([a.ravel() for a in DM.stopping_fcn_weights(win)]), dtype=np.float32)
    return dict(win=win, soft_margin=0.9, fcn_weights=w, n_weights=w.size, group=0)


def test_hosd_front_without_nswaps(dec, hform):
    h, front = hform
    got = _hfront_outputs(dec, h["F"])
    del got["d_nswaps"]
    assert A.call(dec, "ldpc_hosd_front", d_order_llr=h["d_order_llr"], F=h["F"], **got) == 0, A.last_error(dec)
    torch.cuda.synchronize()
    _same(got, front, ("hosd_front",))


def test_hosd_search_nullable_outputs(dec, hform):
    h, _ = hform
    full = _hsearch_outputs(dec, h["F"], h["nblk"])
    assert A.call(dec, "ldpc_hosd_search", **h, **full) == 0, A.last_error(dec)
    torch.cuda.synchronize()
    assert not any(bool((t == A.SENT[t.dtype]).any()) for t in full.values())
    for null in (("d_block_arg",), ("d_truth", "d_label_bits"), ("d_truth",), ("d_cw", "d_metric", "d_best"), ("d_cw",),
                 ("d_metric",), ("d_best",), ("d_block_arg", "d_truth", "d_label_bits", "d_cw", "d_metric", "d_best")):
        got = {k: t for k, t in _hsearch_outputs(dec, h["F"], h["nblk"]).items() if k not in null}
        args = {k: v for k, v in h.items() if k not in null}
        assert A.call(dec, "ldpc_hosd_search", **args, **got) == 0, (null, A.last_error(dec))
        torch.cuda.synchronize()
        _same(got, full, ("hosd_search", null))


def test_hosd_sliding_nullable_outputs(dec, hform):
    h, _ = hform
    sl = _sliding_args()
    full = _hsliding_outputs(dec, h["F"])
    assert A.call(dec, "ldpc_hosd_sliding", **h, **sl, **full) == 0, A.last_error(dec)
    torch.cuda.synchronize()
    assert not any(bool((t == A.SENT[t.dtype]).any()) for t in full.values())
    assert len(torch.unique(full["d_deep_limit"])) > 1                  # the early stop is at work
    for null in [(k,) for k in full] + [tuple(full)]:
        got = {k: t for k, t in _hsliding_outputs(dec, h["F"]).items() if k not in null}
        assert A.call(dec, "ldpc_hosd_sliding", **h, **sl, **got) == 0, (null, A.last_error(dec))
        torch.cuda.synchronize()
        _same(got, full, ("hosd_sliding", null))
    # without labels: no d_truth, no d_success, the rest as before
    got = {k: t for k, t in _hsliding_outputs(dec, h["F"]).items() if k not in ("d_truth", "d_success")}
    args = {k: v for k, v in h.items() if k != "d_label_bits"}
    assert A.call(dec, "ldpc_hosd_sliding", **args, **sl, **got) == 0, A.last_error(dec)
    torch.cuda.synchronize()
    _same(got, full, ("hosd_sliding", "no labels"))


def _ge_rows(dec, Fg):
    rows = np.random.default_rng(6).integers(0, 2 ** 63, size=(Fg, 64, 2), dtype=np.int64)
    return to_dev(rows, dec)


def test_osd_ge_nullable_outputs(dec):
    Fg = 9

    def outs():
        return dict(d_rows_out=A.sentinel(dec, (Fg, 64, 2), torch.int64), d_swaps=A.sentinel(dec, (Fg, 64, 2), torch.uint8),
                    d_nswaps=A.sentinel(dec, (Fg,), torch.int32))

    rows = _ge_rows(dec, Fg)
    full = outs()
    assert A.call(dec, "ldpc_osd_ge", d_rows_in=rows, F=Fg, **full) == 0, A.last_error(dec)
    for null in (("d_swaps",), ("d_nswaps",), ("d_swaps", "d_nswaps")):
        got = {k: t for k, t in outs().items() if k not in null}
        assert A.call(dec, "ldpc_osd_ge", d_rows_in=rows, F=Fg, **got) == 0, (null, A.last_error(dec))
        torch.cuda.synchronize()
        _same(got, full, ("osd_ge", null))


# ------------------------------------------------------------------------ 3. required pointers: refused, nothing launched
def _required_table(dec, hform):
    """(entry point, valid arguments, outputs among them, required pointers) for 8 frames; the required sets are the
    header's."""
    h, _ = hform
    n = 8
    y = h["d_metric_llr"][:n].contiguous()
    index = torch.arange(n, dtype=torch.int32, device=dec.device)
    count = torch.tensor([n], dtype=torch.int32, device=dec.device)
    perm, parity = A.sentinel(dec, (n, 128), torch.uint8), A.sentinel(dec, (n, 64), torch.int64)
    assert A.call(dec, "ldpc_osd_front", d_y=y, F=n, d_perm=perm, d_parity=parity) == 0
    a = A.alpha_array(ALPHA0, 4)
    S = lambda shape, dt: A.sentinel(dec, shape, dt)           # noqa: E731
    search_out = lambda: dict(d_cw=S((n, 2), torch.int64), d_metric=S((n,), torch.float32), d_best=S((n,), torch.int32),   # noqa: E731
                              d_ntep=S((n,), torch.int32))
    per_frame = ("d_order_llr", "d_metric_llr", "d_label_bits", "d_lri", "d_uidx", "d_M")
    hs = {k: (v[:n].contiguous() if k in per_frame else v) for k, v in h.items()}
    hs["F"] = n
    hrequired = ("d_order_llr", "d_metric_llr", "d_lri", "d_uidx", "d_M", "d_teps", "d_block_off")
    table = [
        ("ldpc_nms_decode", dict(d_llr=y, B=n, T=4, alpha=a, d_soft=S((n, 128), torch.float32), d_traj=S((4, n, 128), torch.float32),
                                 d_hard=S((n, 2), torch.int64), d_fail=S((n,), torch.uint8)), ("d_llr", "alpha")),
        ("ldpc_nms_traj_rows", dict(d_llr=y, d_index=index, d_count=count, F=n, T=4, alpha=a, d_rows=S((n, 5, 128), torch.float32)),
         ("d_llr", "d_index", "d_count", "alpha", "d_rows")),
        ("ldpc_osd_ge", dict(d_rows_in=_ge_rows(dec, n), F=n, d_rows_out=S((n, 64, 2), torch.int64), d_swaps=S((n, 64, 2), torch.uint8),
                             d_nswaps=S((n,), torch.int32)), ("d_rows_in", "d_rows_out")),
        ("ldpc_osd_front", dict(d_y=y, d_index=index, d_count=count, F=n, d_perm=S((n, 128), torch.uint8),
                                d_parity=S((n, 64), torch.int64), d_nswaps=S((n,), torch.int32)), ("d_y", "d_perm", "d_parity")),
        ("ldpc_osd_decode", dict(d_y=y, d_index=index, d_count=count, F=n, params=A.params(2), **search_out()),
         ("d_y", "params", "d_cw")),
        ("ldpc_osd_decode", dict(d_y=y, d_index=index, d_count=count, F=n, params=A.params(2, PB), **search_out()),
         ("d_y", "params", "d_cw")),
        ("ldpc_osd_search", dict(d_y=y, d_index=index, d_count=count, F=n, d_perm=perm, d_parity=parity, params=A.params(2, FS),
                                 **search_out()), ("d_y", "d_perm", "d_parity", "params", "d_cw")),
        ("ldpc_osd_tep_eval", dict(d_y=y, d_index=index, d_count=count, F=n, d_perm=perm, d_parity=parity,
                                   d_mask=torch.arange(n, dtype=torch.int64, device=dec.device), d_cw=S((n, 2), torch.int64),
                                   d_metric=S((n,), torch.float32), d_hd=S((n,), torch.int32)),
         ("d_y", "d_perm", "d_parity", "d_mask", "d_cw")),
        ("ldpc_osd_counts", dict(d_cw=torch.zeros((n, 2), dtype=torch.int64, device=dec.device), d_label_bits=hs["d_label_bits"],
                                 d_index=index, d_count=count, d_ntep=torch.ones(n, dtype=torch.int32, device=dec.device), F=n,
                                 d_counts=S((3,), torch.int64)), ("d_cw", "d_label_bits", "d_counts")),
        ("ldpc_hosd_front", dict(d_order_llr=hs["d_order_llr"], F=n, **_hfront_outputs(dec, n)),
         ("d_order_llr", "d_lri", "d_uidx", "d_M")),
        ("ldpc_hosd_search", dict(**hs, **_hsearch_outputs(dec, n, h["nblk"])), hrequired + ("d_block_min", "d_label_bits")),
        ("ldpc_hosd_sliding", dict(**hs, **_sliding_args(), **_hsliding_outputs(dec, n)), hrequired + ("fcn_weights", "d_label_bits")),
    ]
    inputs = {id(t) for t in (perm, parity)}
    return [(e, kw, [t for k, t in kw.items() if isinstance(t, torch.Tensor) and id(t) not in inputs and
                     bool((t == A.SENT[t.dtype]).all())], req) for e, kw, req in table]


def test_required_pointers_are_refused_before_any_launch(dec, hform, batch):
    torch.cuda.synchronize()
    for entry, kw, outs, required in _required_table(dec, hform):
        assert len(outs) >= 1, entry
        for name in required:
            args = dict(kw)
            args[name] = None
            assert A.call(dec, entry, **args) == A.E_ARG, (entry, name)
            assert entry in A.last_error(dec), (entry, name, A.last_error(dec))
            torch.cuda.synchronize()
            assert all(A.untouched(t) for t in outs), (entry, name)
        assert A.call(dec, entry, **kw) == 0, (entry, A.last_error(dec))       # the arguments were valid: now it runs
        torch.cuda.synchronize()
        assert not any(A.untouched(t) for t in outs), entry
    for name in ("d_llr", "alpha", "d_hard", "d_fail", "d_index", "d_count", "d_cw"):
        pipe, outs = _pipe(dec, batch, keep_front=True)
        setattr(pipe._p, name, None)
        assert A.run_pipeline(dec, pipe._p) == A.E_ARG, name
        assert "ldpc_pipeline_run" in A.last_error(dec), (name, A.last_error(dec))
        torch.cuda.synchronize()
        assert all(A.untouched(t) for t in outs.values()), name
        assert pipe.counters().tolist() == NMS0 + OSD0, name
