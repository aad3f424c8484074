"""-m gpu: ldpc_dlosd_pipeline_run / pipeline.DlOsdPipeline against the call sequence it stands for
(tests/dlosd_pipeline_oracle.py): the entry points that existed before it, one call at a time with the failure count read back
to the host, and NumPy for the gather, the six stage counters and the scatter of the merge.  Every buffer of both sides starts
as sentinels and is compared whole -- soft, hard, fail, index, count, the sixteen list buffers and the 15 counters: integers
equal, floats by their bits.  500 frames of NMS-6 per code at an SNR where some but not all fail (premise asserted), a path of
ten TEP blocks of order <= 2 (466 TEPs), a window of 3 and a classifier that stops some frames early and lets others run to
the last block (premise asserted).  The capacity, zero-failure and replay cases are the ones that catch a counted kernel that
ignores the device-side count."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import abi_calls as A
from tests import dlosd_pipeline_oracle as P
from tests import osd_family as OF
from tests import osdl_model
from tests.gpu_util import pack_np, to_dev

pytestmark = pytest.mark.gpu
B, T, ALPHA = P.B, P.T, P.ALPHA
# (code, family, forced)
SEQUENCE = [(name, fam, False) for name, (_, fam) in P.CODES.items()] + [("ccsds", fam, True) for fam in ("hosdx", "hosdw", "hosdl")]


@pytest.mark.parametrize("cnn", [True, False], ids=["cnn", "nocnn"])
@pytest.mark.parametrize("name,fam,forced", SEQUENCE, ids=[f"{n}-{f}{'!' if x else ''}" for n, f, x in SEQUENCE])
def test_pipeline_equals_the_call_sequence(name, fam, forced, cnn):
    ref = P.reference(name, fam, cnn)
    got = P.run(P.make_pipe(name, fam, cnn, forced))
    assert set(got) == set(ref)
    P.assert_equal(got, ref, (name, fam, cnn))
    c = got["counters"].cpu().tolist()
    nf = P.batch(name)["nf"]
    assert c[5] == c[4] == c[11] == nf and c[0] == B and c[6] + c[7] == nf     # every failure went through the stage and the merge
    deep = got["deep_limit"][:nf].cpu().numpy()
    print(name, fam, cnn, "failures", nf, "deep_limit histogram", np.bincount(deep, minlength=11).tolist(), "counters", c)
    assert (deep < 10).any() and (deep == 10).any()          # the premise: the stop fires for some frames only
    if not cnn:                                              # DIA = False: no trajectory, no ordering buffer
        assert "rows" not in got and "order_llr" not in got


@pytest.mark.parametrize("cnn", [True, False], ids=["cnn", "nocnn"])
@pytest.mark.parametrize("fam", ["hosdx", "hosdw", "hosdl"])
def test_forced_families_equal_hosd_on_ccsds(fam, cnn):
    """(128,64) is served by all four families: their results are the same once the layouts are converted."""
    want = P.run(P.make_pipe("ccsds", "hosd", cnn))
    got = P.run(P.make_pipe("ccsds", fam, cnn, forced=True))
    nf = P.batch("ccsds")["nf"]
    for k in got:
        if k not in ("lri", "uidx", "M"):
            assert A.same_bits(P.raw(got[k]), P.raw(want[k])), (fam, k)
    for k in ("lri", "uidx"):
        assert torch.equal(got[k][:nf].to(torch.int64), want[k][:nf].to(torch.int64)) and P.untouched(got[k], nf), (fam, k)
    M = got["M"][:nf].reshape(nf, -1)
    assert torch.equal(M[:, :64], want["M"][:nf]) and (fam != "hosdw" or bool((M[:, 64:] == 0).all())) and P.untouched(got["M"], nf)


def test_capacity_below_the_failure_count():
    name, fam = "s200_100", "hosdl"
    b = P.batch(name)
    cap = b["nf"] // 2
    assert cap >= 8
    ref = P.reference(name, fam, True, cap=cap)
    # the buffers hold B rows, the capacity says fewer: nothing at or beyond it is written, `rows` included
    pipe = P.make_pipe(name, fam, True)
    pipe._p.osd_capacity = cap
    got = P.run(pipe)
    P.assert_equal(got, ref, "B rows", keys=P.NMS_OUT + ("index", "count", "counters"))
    for k in P.LIST_OUT:
        assert A.same_bits(P.raw(got[k][:cap]), P.raw(ref[k])) and P.untouched(got[k], cap), k
    c = got["counters"].cpu().tolist()
    assert int(got["count"].item()) == b["nf"] == c[4] and c[5] == cap == c[11] and c[5] < c[4]
    # and the object that allocates `capacity` rows
    got = P.run(P.make_pipe(name, fam, True, cap=cap))
    P.assert_equal(got, ref, "cap rows")


def test_zero_failures():
    name, fam, snr = "ldpc_96_48", "hosdx", 9.0
    b = P.batch(name, snr=snr)
    assert b["nf"] == 0                                      # the premise: a batch that NMS decodes whole
    got = P.run(P.make_pipe(name, fam, True, snr=snr))
    for k in P.LIST_OUT:
        assert P.untouched(got[k]), k
    c = got["counters"].cpu().tolist()
    assert c[0] == B and c[5:] == [0] * 10 and got["count"].item() == 0 and P.untouched(got["index"])
    P.assert_equal(got, P.reference(name, fam, True, snr=snr), "zero failures")


NULLABLE = ["d_soft", "d_label_bits", "d_nms_counts", "d_dl_counts", "d_final_counts", "merge", "d_nswaps", "d_global_min", "d_truth",
            "d_success", "d_metric", "d_best", "d_teps_evaluated", "d_deep_limit", "d_success+d_truth"]


@pytest.mark.parametrize("member", NULLABLE)
def test_nullable_members(member):
    """One member out at a time: its own output keeps the sentinel (its counters stay 0), the others do not change.
    d_deep_limit goes together with d_dl_counts, which needs it; without labels d_list_labels, d_truth and d_success are
    not written either.  The success and failure counters do not need d_success: without it they compare d_global_min with
    d_truth, and stay only when one of those is missing too."""
    name, fam = "array_121_60", "hosdw"
    labels = member != "d_label_bits"
    ref = P.reference(name, fam, True, labels=labels)
    pipe = P.make_pipe(name, fam, True)
    both = member == "d_success+d_truth"
    member = "d_success" if both else member
    setattr(pipe._p, member, 0 if member == "merge" else None)
    if both:
        pipe._p.d_truth = None
    if member == "d_deep_limit":
        pipe._p.d_dl_counts = None
    got = P.run(pipe)
    want = dict(ref)
    cnt = ref["counters"].clone()
    own = {"d_soft": "soft", "d_teps_evaluated": "teps_evaluated"}.get(member, member[2:])
    if own in want and member != "d_label_bits":
        want[own] = P.sentinel(pipe.dec, tuple(ref[own].shape), ref[own].dtype)
    if member == "d_nms_counts":
        cnt[:5] = 0
    elif member in ("d_dl_counts", "d_deep_limit"):
        cnt[5:11] = 0
    elif member == "d_final_counts":
        cnt[11:] = 0
    elif member == "merge":
        cnt[11:] = 0
        want["hard"] = P.batch(name)["hard"]
    elif both:
        cnt[6:8] = 0
        want["truth"] = P.sentinel(pipe.dec, tuple(ref["truth"].shape), ref["truth"].dtype)
    elif member == "d_teps_evaluated":
        cnt[10] = 0
    want["counters"] = cnt
    assert set(got) == set(want)
    P.assert_equal(got, want, member)
    if not labels:
        assert cnt.cpu().tolist()[:5] == [0] * 5 and cnt[5].item() > 0 and cnt[6:8].cpu().tolist() == [0, 0] and P.untouched(got["truth"])


def test_ordering_buffer_without_a_cnn():
    """DIA = False: d_order_llr is NULL (the object's choice: front end and scan read d_metric_llr twice) or a buffer of its own
    that the gather fills with the channel values of the listed frames; the results are the same."""
    name, fam = "ldpc_96_48", "hosdx"
    ref = P.reference(name, fam, False)
    pipe = P.make_pipe(name, fam, False)
    assert pipe._p.d_order_llr is None and pipe.order_llr is None
    order = P.sentinel(pipe.dec, tuple(pipe.metric_llr.shape), torch.float32)
    pipe._p.d_order_llr = order.data_ptr()
    got = P.run(pipe)
    P.assert_equal(got, ref, "own ordering buffer")
    nf = P.batch(name)["nf"]
    assert A.same_bits(order[:nf], got["metric_llr"][:nf]) and P.untouched(order, nf)


def test_nms_only_on_a_code_no_family_serves():
    from short_ldpc_decoding_osd_amd.pipeline import BatchPipeline, DlOsdPipeline
    dec = OF.decoder("wimax_1056")
    y, cw = osdl_model.frames("wimax_1056", 3.0, 300, 4)
    yd, label = to_dev(y, dec), to_dev(pack_np(cw).view(np.int64), dec)
    old = BatchPipeline(dec, 300, T, ALPHA).bind(yd, label)
    new = DlOsdPipeline(dec, 300, T, ALPHA, None, None, 0, 0.0, None).bind(yd, label)
    assert new.family is None
    for p in (old, new):
        for k in P.NMS_OUT:
            getattr(p, k).fill_(A.SENT[getattr(p, k).dtype])
        p.reset_counters()
        p.run()
    torch.cuda.synchronize()
    for k in P.NMS_OUT:
        assert A.same_bits(getattr(new, k), getattr(old, k)), k
    assert new.counters().cpu().tolist() == old.counters().cpu().tolist()[:5] + [0] * 10
    assert new.counters()[4].item() > 0 and new.counters()[2].item() > 0          # (the counters are not trivially zero)


def _refused(pipe, code, *texts):
    clean = P.snapshot(pipe)
    rc = pipe.dec.L.ldpc_dlosd_pipeline_run(pipe.dec._ctx, C.byref(pipe._p), pipe.dec._stream())
    err = A.last_error(pipe.dec)
    assert rc == code and all(t in err for t in texts), (rc, err)
    torch.cuda.synchronize()
    P.assert_equal(P.snapshot(pipe), clean, texts)


def test_refusals_before_any_launch():
    from short_ldpc_decoding_osd_amd.pipeline import DlOsdPipeline
    who = "ldpc_dlosd_pipeline_run: "
    # AUTO with the stage on, on a code no family serves: the sentence of the last family tried
    dec = OF.decoder("wimax_1056")
    y, cw = osdl_model.frames("wimax_1056", 1.0, 64, 4)
    teps, off = P.tep_path(P.decoder("ccsds"))
    pipe = DlOsdPipeline(dec, 64, T, ALPHA, teps.to(dec.device), off.to(dec.device), P.WIN, P.MARGIN, P.fcn_weights())
    pipe.bind(to_dev(y, dec), to_dev(pack_np(cw).view(np.int64), dec))
    assert pipe.family == "hosdl"
    P.fill(pipe)
    _refused(pipe, -5, who + "long H-form OSD kernels need n <= 384, an H of 1 <= R <= 192 rows, 1 <= n-k <= 192 and 1 <= k <= 192; "
             "this H has 176 rows, n-k = 176, code (1056,880)")
    # a forced family that does not serve the code: its own sentence, word for word
    for fam, text in (("hosd", "H-form OSD kernels need n=128, m=k=64; this code is n=121 m=66 k=60"),
                      ("hosdx", who + "H-form OSD kernels need 1 <= k <= 64 and an H of exactly n-k <= 64 rows; this H has 66 rows, "
                       "n-k = 61, code (121,60)")):
        pipe = P.make_pipe("array_121_60", "hosdw", True)
        pipe._p.family = {"hosd": 1, "hosdx": 2}[fam]
        P.fill(pipe)
        _refused(pipe, -5, text)

    def bad(code, text, cnn=True, **members):
        p = P.make_pipe("array_121_60", "hosdw", cnn)
        P.fill(p)
        for k, v in members.items():
            setattr(p._p, k, v)
        _refused(p, code, who, text)

    for member in ("d_index", "d_count", "d_teps", "d_block_off", "d_metric_llr", "d_lri", "d_uidx", "d_M", "d_cw", "d_rows",
                   "d_order_llr", "fcn_weights"):
        bad(A.E_ARG, f"{member} is NULL", **{member: None})
    bad(A.E_ARG, "d_hard and d_fail are required", d_hard=None)
    bad(A.E_ARG, "d_hard and d_fail are required", d_fail=None)
    bad(A.E_ARG, "n_cnn_weights 149, T + 1 = 7 rows take 147", n_cnn_weights=149)
    bad(A.E_ARG, "cnn_weights with T 5", T=5)
    bad(A.E_ARG, "win 0 outside 1..15", win=0)
    bad(A.E_ARG, "win 16 outside 1..15", win=16)
    bad(A.E_ARG, "nblk 2 is below win 3", nblk=2)
    bad(-5, "nblk 1025 TEP blocks, at most 1024", nblk=1025)
    bad(A.E_ARG, "n_fcn_weights 23, a window of 3 takes 24", n_fcn_weights=23)
    bad(A.E_ARG, "group -1 is negative", group=-1)
    bad(A.E_ARG, "osd_capacity -1 is negative", osd_capacity=-1)
    bad(A.E_ARG, "family 5 is no LDPC_HOSD_FAMILY_* value", family=5)
    bad(A.E_ARG, "d_list_labels is NULL (required with d_label_bits)", d_list_labels=None)
    bad(A.E_ARG, "d_deep_limit is NULL (required with d_dl_counts)", d_deep_limit=None)
    bad(A.E_ARG, "timing_slot 64", timing_slot=64)
    # B = 0 with the stage on: the count word is zeroed, nothing else is written
    p = P.make_pipe("array_121_60", "hosdw", True)
    P.fill(p)
    clean = P.snapshot(p)
    p._p.B = 0
    assert p.dec.L.ldpc_dlosd_pipeline_run(p.dec._ctx, C.byref(p._p), p.dec._stream()) == 0
    torch.cuda.synchronize()
    assert p.count.item() == 0
    P.assert_equal(P.snapshot(p), clean, "B = 0", keys=[k for k in clean if k != "count"])


def test_timing_slots_serve_this_pipeline():
    pipe = P.make_pipe("ldpc_96_48", "hosdx", True)
    P.fill(pipe)
    pipe.run(timing_slot=7)
    torch.cuda.synchronize()
    ms = pipe.timing(7)
    assert len(ms) == 3 and all(v > 0.0 for v in ms)


# ------------------------------------------------------------------------------------------------------- captured graphs
def _rebind(pipe, b):
    pipe._y.copy_(b["yd"])
    pipe._labels.copy_(b["label"])


def test_captured_chain_replayed_on_rebound_data():
    """run() captured as one chain; three replays, each on other data in the same input buffers (another failure count each
    time), equal three eager runs: the outputs of every run and the counters accumulated over the three."""
    from short_ldpc_decoding_osd_amd.pipeline import DlOsdPipeline
    name, fam = "ldpc_96_48", "hosdx"
    seeds = (31, 32, 33)
    data = [P.batch(name, seed) for seed in seeds]
    assert len({b["nf"] for b in data}) > 1                  # (the count differs between the replays)
    dec = data[0]["dec"]
    teps, off = P.tep_path(dec)
    pipe = DlOsdPipeline(dec, B, T, ALPHA, teps, off, P.WIN, P.MARGIN, P.fcn_weights(), P.cnn_weights())
    pipe.bind(data[0]["yd"].clone(), data[0]["label"].clone())
    eager = []
    pipe.reset_counters()
    for b in data:
        _rebind(pipe, b)
        P.fill(pipe, counters=False)
        pipe.run()
        torch.cuda.synchronize()
        eager.append(P.snapshot(pipe))
    for seed, snap in zip(seeds, eager):                                 # (and the eager runs are the sequence's)
        P.assert_equal(snap, P.reference(name, fam, True, seed=seed), ("eager", seed), keys=P.NMS_OUT + P.LIST_OUT + ("index", "count"))
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        pipe.run()
    pipe.reset_counters()
    for b, want in zip(data, eager):
        _rebind(pipe, b)
        P.fill(pipe, counters=False)
        g.replay()
        torch.cuda.synchronize()
        P.assert_equal(P.snapshot(pipe), want, "replay")
    assert pipe.counters().cpu().tolist() == eager[-1]["counters"].cpu().tolist()
    assert pipe.counters()[0].item() == 3 * B


def test_two_pipelines_on_two_streams():
    """Two objects, each on a stream of its own: no state is shared."""
    name, fam = "array_121_60", "hosdw"
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    pipes = [P.make_pipe(name, fam, True, seed=s) for s in (31, 32)]
    for p in pipes:
        P.fill(p)
    torch.cuda.synchronize()
    for _ in range(2):
        for p, st in zip(pipes, streams):
            with torch.cuda.stream(st):
                p.run()
    torch.cuda.synchronize()
    for p, s in zip(pipes, (31, 32)):
        ref = dict(P.reference(name, fam, True, seed=s))
        ref["counters"] = 2 * ref["counters"]
        # (NMS rewrites hard before the merge, so both runs give the same outputs)
        P.assert_equal(P.snapshot(p), ref, ("stream", s))
