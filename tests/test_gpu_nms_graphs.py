"""-m gpu: nms_generic_kernel, nms_train_kernel and the streaming kernels on the Tanner graphs of tests/nms_graphs.py.
Decoder outputs against the C oracle bit for bit; the training kernel's loss and gradient against the float64 model of
tests/nms_grad_model.py within rel_bound (test_gpu_nms_train.py) fed with the graph's own degrees; every launch form of
the training kernel (4, 3, 2, 1 frames per workgroup, one frame above 64 KiB) asserted from the LDS formula restated in
nms_graphs.train_lds_bytes."""
import numpy as np
import pytest
import torch

from oracle import c_oracle, np_oracle
from tests import nms_graphs as Z
from tests.gpu_util import pack_np, to_dev, words_np
from tests.nms_grad_model import Graph, forward32, grad_model
from tests.test_gpu_nms_train import rel_bound

pytestmark = pytest.mark.gpu

PER_ITER = np.array([0.7 * (1 + 0.04 * (t % 7)) for t in range(64)], np.float32)
SIZES = [1, 3, 5, 63, 65, 1000]
_decs = {}


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def decoder(name):
    from short_ldpc_decoding_osd_amd import Code
    from short_ldpc_decoding_osd_amd.runtime import Decoder
    if name not in _decs:
        _decs[name] = Decoder(Code() if name == "ccsds" else Z.make_code(name))
    return _decs[name]


def check_decode(dec, y, T, alpha, w_in=1.0, w_out=1.0, kernel=1, skip=()):
    """ldpc_nms_decode against the C oracle: soft, trajectory (bits), hard words incl. zero padding, syndrome flags.
    ``skip``: frames whose own outputs are not compared."""
    H = dec.code.H
    a = alpha if T else 1.0
    keep = np.setdiff1d(np.arange(y.shape[0]), np.asarray(skip, dtype=np.int64))
    soft_o, traj_o = c_oracle.nms(H, y[keep], T, a, w_in, w_out, want_traj=True)
    hard_o, fail_o, _ = c_oracle.evaluate(H, soft_o, None)
    res = dec.nms(to_dev(y, dec), T, a, w_in, w_out, want_traj=True, kernel=kernel)
    torch.cuda.synchronize()
    same = (lambda g, w: np.array_equal(_u32(g), _u32(w))) if kernel == 1 else np.array_equal   # (QC16: the sign of a zero)
    assert same(res["soft"].cpu().numpy()[keep], soft_o)
    if T:
        assert same(res["traj"].cpu().numpy()[:, keep], traj_o[1:])
    hard = words_np(res["hard"])
    assert np.array_equal(hard[keep], pack_np(hard_o))
    if dec.n % 64:
        assert not (hard[:, -1] >> np.uint64(dec.n % 64)).any(), "padding bits of the last hard word"
    assert np.array_equal(res["fail"].cpu().numpy()[keep], fail_o)
    return res


# ------------------------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("T", [0, 1, 8, 64])
@pytest.mark.parametrize("name", Z.NAMES)
def test_generic_decode_exact(name, T):
    from short_ldpc_decoding_osd_amd import _lib
    dec = decoder(name)
    assert dec.nms_kernel == _lib.NMS_GENERIC
    kinds = [(1.0, False), (4.0, False), (2.0, True)]
    weights = [(0.75, 1.0, 1.0), (PER_ITER[:max(T, 1)], 0.85, 1.2)]
    i = [0, 1, 8, 64].index(T)
    for snr, quant in kinds:
        for alpha, w_in, w_out in weights:
            B = SIZES[i % len(SIZES)]
            i += 1
            y, _ = Z.frames(name, snr, B, 1000 * T + i, quant)
            check_decode(dec, y, T, alpha, w_in, w_out)


def test_all_batch_sizes_reach_every_graph():
    """The rotation of test_generic_decode_exact gives every graph every batch size (over its four T)."""
    seen = set()
    for t in range(4):
        seen |= {SIZES[(t + k) % len(SIZES)] for k in range(6)}
    assert seen == set(SIZES)


@pytest.mark.parametrize("name", Z.NAMES)
def test_refusals_and_listed_rows(name):
    from short_ldpc_decoding_osd_amd import _lib
    dec = decoder(name)
    y, _ = Z.frames(name, 2.0, 70, 5)
    yd = to_dev(y, dec)
    with pytest.raises(_lib.LdpcError, match="T=65"):
        dec.nms(yd, 65, np.ones(65, np.float32))
    with pytest.raises(_lib.LdpcError, match="QC16"):
        dec.nms(yd, 8, 0.75, kernel=_lib.NMS_QC16)
    # ldpc_nms_traj_rows: a shuffled list with a repeated frame, capacity above the count
    T = 6
    lst = np.array([69, 4, 33, 0, 4, 68, 12], np.int32)
    cap = len(lst) + 5
    index = to_dev(np.concatenate([lst, np.full(5, 7, np.int32)]), dec)
    count = to_dev(np.array([len(lst)], np.int32), dec)
    rows = dec.nms_traj_rows(yd, index, count, cap, T, PER_ITER[:T], 0.85, 1.2, out=torch.full((cap, T + 1, dec.n), -7.0, device=dec.device))
    full = dec.nms(yd, T, PER_ITER[:T], 0.85, 1.2, want_traj=True)["traj"]
    torch.cuda.synchronize()
    for k, f in enumerate(lst.tolist()):
        assert torch.equal(rows[k, 0], yd[f]) and torch.equal(rows[k, 1:].view(torch.int32), full[:, f, :].view(torch.int32)), (k, f)
    assert (rows[len(lst):] == -7.0).all()
    _, traj_o = c_oracle.nms(dec.code.H, y[lst], T, PER_ITER[:T], 0.85, 1.2, want_traj=True)
    assert np.array_equal(_u32(rows[:len(lst)].cpu().numpy()), _u32(np.transpose(traj_o, (1, 0, 2))))


@pytest.mark.parametrize("name,kernel", [("ccsds", 1), ("ccsds", 2), ("wide", 1)])
def test_extreme_channel_values(name, kernel):
    """|y| = 1e30, 3e30, 3e38 on whole frames and on single positions (+-inf: see nms_graphs.EXTREME)."""
    dec = decoder(name)
    y, _ = np_oracle.make_frames(dec.code.G, 2.0, 12, np.random.default_rng(3))
    ys = Z.extreme_frames(y)
    for T in (1, 8):
        check_decode(dec, ys, T, 0.7, kernel=kernel)
        check_decode(dec, ys, T, np.linspace(0.5, 1.3, T).astype(np.float32), 0.85, 1.2, kernel=kernel)


@pytest.mark.parametrize("name,kernel", [("ccsds", 1), ("ccsds", 2), ("wide", 1), ("wimax_1056", 1)])
def test_one_nan_frame_leaves_the_others_alone(name, kernel):
    """A frame of NaN among finite ones: every other frame equals the oracle -- in the QC16 kernel the three that share
    its wavefront (frames 4, 6, 7 of frame 5), in the generic kernel the frames its wavefront decodes before and after."""
    dec = decoder(name)
    y, _ = np_oracle.make_frames(dec.code.G, 2.0, 67, np.random.default_rng(9))
    y[5] = np.nan
    y[66, ::3] = np.nan
    for T in (0, 1, 10):
        check_decode(dec, y, T, 0.7, kernel=kernel, skip=(5, 66))


# --------------------------------------------------------------------------------------------------- streaming kernels
@pytest.mark.parametrize("name", [n for n in Z.NAMES if n != "deg65"])
def test_streaming_kernels_on_other_word_counts(name):
    from short_ldpc_decoding_osd_amd import _lib
    from short_ldpc_decoding_osd_amd.pipeline import BatchPipeline
    dec = decoder(name)
    B, T, alpha = 3000, 5, 0.75
    y, cw = Z.frames(name, 1.0, B, 21)
    yd = to_dev(y, dec)
    label = dec.pack_bits(to_dev(cw, dec))
    assert label.shape == (B, (dec.n + 63) // 64) and np.array_equal(words_np(label), pack_np(cw))
    for dt in (torch.uint8, torch.int32):
        assert torch.equal(dec.pack_bits(to_dev(cw, dec, dt)), label)
    for dt in (torch.uint8, torch.int32, torch.int64):
        assert np.array_equal(dec.unpack_bits(label, dt).cpu().numpy(), cw)
    res = dec.nms(yd, T, alpha)
    soft = res["soft"].cpu().numpy()
    hard_o, fail_o, cnt_o = c_oracle.evaluate(dec.code.H, soft, cw)
    want = [cnt_o[k] for k in ("frames", "frame_err", "bit_err", "undetected", "synd_fail")]
    last = (dec.n - 1) // 64 * 64
    assert (hard_o[:, last:] != cw[:, last:]).any(), "the premise: bit errors in the last label word"
    assert dec.eval_counts(res["hard"], label, res["fail"]).cpu().tolist() == want
    no_flags = dec.eval_counts(res["hard"], label).cpu().tolist()
    assert no_flags == want[:3] + [0, 0]
    # the one-call pipeline: without OSD its counters are eval_counts'; with OSD it refuses a code that is not (128, 64), so
    # the compaction's ride-along counters (their words != 2 branch) cannot be reached through the library
    pipe = BatchPipeline(dec, B, T, alpha).bind(yd, label)
    pipe.run()
    torch.cuda.synchronize()
    assert pipe.counters().cpu().tolist()[:5] == want
    assert np.array_equal(pipe.fail.cpu().numpy(), fail_o) and np.array_equal(words_np(pipe.hard), pack_np(hard_o))
    with pytest.raises(_lib.LdpcError, match=rf"OSD kernels need an \(n=128, k=64\) code; this one is \({dec.n},{dec.k}\)") as e:
        BatchPipeline(dec, B, T, alpha, osd_order=2).bind(yd, label).run()
    assert "(-5)" in str(e.value)


# ----------------------------------------------------------------------------------------------------- training kernel
def graph_bound(H, T):
    dc, dv = Z.degrees(H)
    return rel_bound(T, n=max(H.shape), dc=dc, dv=dv)


def check_grad(dec, y, cw, T, alpha, w_in=1.0, w_out=1.0, check_dense=True):
    """ldpc_nms_train_grad against the model: loss and gradient within the derived bound times the model's mass, exactly 0
    where the model's mass is 0; the decoder outputs against ldpc_nms_decode (generic kernel).  Returns (result, model)."""
    H = dec.code.H
    yd, lab = to_dev(y, dec), to_dev(pack_np(cw).view(np.int64), dec)
    res = dec.nms_grad(yd, lab, T, alpha, w_in, w_out, want_traj=True, want_hard=True, want_fail=True)
    ref = dec.nms(yd, T, alpha if T else 1.0, w_in, w_out, want_traj=True, kernel=1)
    torch.cuda.synchronize()
    if T:
        assert np.array_equal(_u32(res["traj"].cpu().numpy()), _u32(ref["traj"].cpu().numpy()))
    assert torch.equal(res["hard"], ref["hard"]) and torch.equal(res["fail"], ref["fail"])
    model = grad_model(H, y, cw, T, alpha, w_in, w_out, check_dense=check_dense)
    if T:
        assert np.array_equal(_u32(res["traj"].cpu().numpy()[-1]), _u32(model["outs"][-1]))
    bound = graph_bound(H, T)
    loss = res["loss"].cpu().numpy().astype(np.float64)
    grad = res["grad"].cpu().numpy().astype(np.float64)
    assert np.isfinite(loss).all() and np.isfinite(grad).all()
    worst_l = float(np.max(np.abs(loss - model["loss"]) / np.maximum(model["loss"], 1e-300)))
    err = np.abs(grad - model["grad"])
    worst_g = float(np.max(err / np.maximum(model["mass"], 1e-300) * (model["mass"] > 1e-20)))   # (printed only: masses near
    #                                                   float32's underflow are covered by the absolute 1e-30 below)
    print(f"n={dec.n} m={dec.m} T={T}: bound {bound:.3e}, loss error {worst_l:.3e}, gradient error / mass {worst_g:.3e}")
    assert np.all(np.abs(loss - model["loss"]) <= bound * model["loss"] + 1e-30)
    assert np.all(err <= bound * model["mass"] + 1e-30), worst_g
    assert np.all(grad[model["mass"] == 0] == 0), "components without any contribution are exact zeros"
    return res, model


def _mixed_frames(name, B, seed):
    """Half plain frames at two SNRs, half quantised ones (ties and zeros)."""
    parts = [Z.frames(name, 1.0, B // 4, seed), Z.frames(name, 3.0, B // 4, seed + 1), Z.frames(name, 2.0, B - 2 * (B // 4), seed + 2, True)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


# (graph, T, frames per workgroup, one frame above 64 KiB): every launch form of launch_nms_train, each on several graphs
TRAIN_CASES = [("wide", 4, 4, False), ("wide", 8, 3, False), ("wide", 12, 2, False), ("wide", 18, 1, False), ("wide", 40, 1, True),
               ("thin", 4, 4, False), ("thin", 64, 2, False),
               ("short", 8, 4, False), ("short", 30, 3, False), ("short", 40, 2, False), ("short", 64, 1, False),
               ("array_121_60", 5, 4, False), ("array_121_60", 12, 2, False), ("array_121_60", 40, 1, True),
               ("ldpc_96_48", 12, 3, False), ("ldpc_96_48", 64, 1, True),
               ("wimax_1056", 1, 2, False), ("wimax_1056", 18, 1, True), ("ccsds", 64, 1, True)]


@pytest.mark.parametrize("name,T,waves,opt_in", TRAIN_CASES)
def test_train_loss_and_gradient(name, T, waves, opt_in):
    dec = decoder(name)
    Z.assert_train_launch(dec.code.H, T, waves, opt_in)
    if name == "ccsds":
        rng = np.random.default_rng(64)
        y, cw = np_oracle.make_frames(dec.code.G, 2.7, 10, rng)
    else:
        y, cw = _mixed_frames(name, 6 if name == "wimax_1056" else 22, 10 * T)
    for alpha, w_in, w_out in ((0.669435, 1.0, 1.0), (PER_ITER[:T], 0.85, 1.2)):
        res, _ = check_grad(dec, y, cw, T, alpha, w_in, w_out)
        soft_o, traj_o = c_oracle.nms(dec.code.H, y, T, alpha, w_in, w_out, want_traj=True)
        hard_o, fail_o, _ = c_oracle.evaluate(dec.code.H, soft_o, None)
        assert np.array_equal(_u32(res["traj"].cpu().numpy()), _u32(traj_o[1:]))
        assert np.array_equal(words_np(res["hard"]), pack_np(hard_o)) and np.array_equal(res["fail"].cpu().numpy(), fail_o)


def test_wimax_beyond_the_budget_is_refused():
    from short_ldpc_decoding_osd_amd import _lib
    dec = decoder("wimax_1056")
    assert Z.train_lds_bytes(dec.code.H, 19) > Z.TRAIN_LDS_BUDGET
    y, cw = Z.frames("wimax_1056", 2.0, 2, 1)
    with pytest.raises(_lib.LdpcError, match=rf"needs {Z.train_lds_bytes(dec.code.H, 19)} B of LDS at T=19"):
        dec.nms_grad(to_dev(y, dec), to_dev(pack_np(cw).view(np.int64), dec), 19, PER_ITER[:19])


def test_degree_65_trains_nowhere_and_decodes_everywhere():
    from short_ldpc_decoding_osd_amd import _lib
    dec = decoder("deg65")
    y, cw = Z.frames("deg65", 2.0, 9, 1)
    with pytest.raises(_lib.LdpcError, match="check degree 65 above 64") as e:
        dec.nms_grad(to_dev(y, dec), to_dev(pack_np(cw).view(np.int64), dec), 3, PER_ITER[:3])
    assert "(-5)" in str(e.value)                 # LDPC_E_UNSUPPORTED
    check_decode(dec, y, 3, PER_ITER[:3])          # (every T and batch size: test_generic_decode_exact)


def test_wide_code_with_every_wide_check_silent():
    """A two-tape-word launch in which only checks of at most 32 edges carry gradient: a zero channel value on WIDE_ONLY
    makes S = 0 in every check above 32 edges, in every iteration.  Such frames alternate with ordinary ones, whose
    second tape words they must neither read nor need."""
    dec = decoder("wide")
    H = dec.code.H
    T = 6
    y, cw = _mixed_frames("wide", 48, 77)
    y[::2, Z.WIDE_ONLY] = 0.0
    _, recs = forward32(Graph(H), y[::2], T, PER_ITER[:T], 0.85, 1.2)
    wide_rows = H.sum(axis=1) > 32
    assert wide_rows.sum() >= 5 and all(r["zero"][:, wide_rows].all() for r in recs)
    assert not all(r["zero"][:, ~wide_rows].all() for r in recs)
    check_grad(dec, y, cw, T, PER_ITER[:T], 0.85, 1.2)


def test_wide_check_with_both_minima_in_the_second_word():
    """The two smallest |y| of the degree-64 check are its last two variables (row positions 62 and 63); other wide checks
    take theirs from the second word at random."""
    dec = decoder("wide")
    H = dec.code.H
    r64 = int(np.flatnonzero(H.sum(axis=1) == 64)[0])
    y, cw = Z.frames("wide", 3.0, 24, 5)
    y = np.where(np.abs(y) < 0.05, np.float32(0.05), y).astype(np.float32)
    y[:, 128] = np.where(np.arange(24) % 2, 0.01, -0.02).astype(np.float32)
    y[:, 129] = np.where(np.arange(24) % 3, -0.015, 0.015).astype(np.float32)
    for T in (1, 5):
        _, recs = forward32(Graph(H), y, T, PER_ITER[:T], 1.0, 1.0)
        assert set(np.unique(recs[0]["j1"][:, r64])) == {62, 63} and set(np.unique(recs[0]["j2"][:, r64])) == {62, 63}
        wide_rows = np.flatnonzero(H.sum(axis=1) > 32)
        assert (np.stack([r["j1"][:, wide_rows] for r in recs]) >= 32).mean() > 0.2
        check_grad(dec, y, cw, T, PER_ITER[:T])


def test_thin_clip_and_missing_second_edge():
    """`thin` with an alpha above 1: a degree-1 check (no second edge) sends alpha * 1e30 > 1e30, which the clip of the
    neighbouring checks stops; the all-zero row and S = 0 rows send nothing back.  The premises are read from the model's
    records; the gradient holds to the bound and is exactly 0 where nothing contributes."""
    dec = decoder("thin")
    H = dec.code.H
    T = 5
    alpha = np.array([1.25, 0.7, 1.5, 1.25, 0.8], np.float32)
    y, cw = _mixed_frames("thin", 40, 3)
    g = Graph(H)
    _, recs = forward32(g, y, T, alpha, 1.0, 1.0)
    single = list(Z.THIN_SINGLE)
    a = [np.where(g.valid[None], np.abs(r["vc"]), 0) for r in recs]
    assert any((x[:, 2].max(axis=1) > 1e30).any() for x in a), "an m2 edge above the clip in the degree-2 check"
    assert any(r["zero"].any() for r in recs) and not recs[0]["has2"][:, single].any()
    res, model = check_grad(dec, y, cw, T, alpha)
    # whole frames above the clip with some labels against the signs: no |vc| of iteration 1 passes the clip, so nothing
    # reaches w_in at T = 1 (the model's mass is 0 there: check_grad compares for equality)
    for name in ("thin", "wide", "ccsds"):
        d = decoder(name)
        yy, cc = np_oracle.make_frames(d.code.G, 2.0, 16, np.random.default_rng(4))
        yy = np.where(yy < 0, np.float32(-3e30), np.float32(3e30))
        cc = cc.copy()
        cc[:, ::5] ^= 1
        res, model = check_grad(d, yy, cc, 1, np.float32([0.7]), 0.85, 1.2)
        assert (model["mass"][:, 1] == 0).all() and (model["mass"][:, 0] > 0).all()
        assert (res["grad"][:, 1] == 0).all().item()
        check_grad(d, yy, cc, 3, PER_ITER[:3], 0.85, 1.2)


@pytest.mark.parametrize("name", ["wide", "thin", "short", "wimax_1056"])
def test_train_edges_of_the_call(name):
    dec = decoder(name)
    y, cw = _mixed_frames(name, 8, 2)
    yd, lab = to_dev(y, dec), to_dev(pack_np(cw).view(np.int64), dec)
    # T = 0: no iteration, no loss, grad = {dL/dw_in, dL/dw_out} = 0; the decoder outputs are the channel's
    res = dec.nms_grad(yd, lab, 0, 1.0, want_hard=True, want_fail=True)
    ref = dec.nms(yd, 0, 1.0, kernel=1)
    torch.cuda.synchronize()
    assert res["grad"].shape == (8, 2) and not res["grad"].any() and not res["loss"].any()
    assert res["loss_sum"].item() == 0 and not res["grad_sum"].any()
    assert torch.equal(res["hard"], ref["hard"]) and torch.equal(res["fail"], ref["fail"])
    # B = 0
    res = dec.nms_grad(yd[:0], lab[:0], 3, PER_ITER[:3])
    torch.cuda.synchronize()
    assert res["loss"].shape == (0,) and res["grad"].shape == (0, 5)
    # without the gradient (the kernel leaves a frame after its forward pass): the forward outputs are the full call's,
    # and the full call after it is unchanged
    T = 4
    full = dec.nms_grad(yd, lab, T, PER_ITER[:T], want_traj=True, want_hard=True, want_fail=True)
    part = dec.nms_grad(yd, lab, T, PER_ITER[:T], want_grad=False, want_sums=False, want_traj=True, want_hard=True, want_fail=True)
    again = dec.nms_grad(yd, lab, T, PER_ITER[:T], want_traj=True, want_hard=True, want_fail=True)
    torch.cuda.synchronize()
    assert part["grad"] is None
    for k in ("loss", "traj", "hard", "fail"):
        assert torch.equal(part[k], full[k]), k
    for k in ("loss", "grad", "loss_sum", "grad_sum", "traj", "hard", "fail"):
        assert torch.equal(again[k].view(torch.uint8), full[k].view(torch.uint8)), k
