"""-m gpu: ldpc_fcn_windows and ldpc_fcn_grad (csrc/ldpc_fcn.h) -- the windows bit for bit against the restatement of
tests/fcn_training_model.py; the forward pass against the host order of the sliding kernel's classifier; loss, gradient,
accuracy sums and counts against the float64 model fed the kernel's own probabilities; determinism, additivity, saturated
and zero weights, the refusals, and a replay of the sliding scan's decisions from the training kernels' outputs."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from oracle import np_oracle
from tests import dlosd_model as DM
from tests import fcn_training_model as FM
from tests.gpu_util import pack_np, to_dev

pytestmark = pytest.mark.gpu

TREE = 1e-12        # float64 tree rounding, relative to the L1 mass of the summed terms (test_gpu_dia_train's additivity bound)


@pytest.fixture(scope="module")
def dec():
    from short_ldpc_decoding_osd_amd import Code
    from short_ldpc_decoding_osd_amd.runtime import Decoder
    return Decoder(Code())


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream(dec):
    return C.c_void_p(torch.cuda.current_stream(dec.device).cuda_stream)


def _bits(t, dt):
    return t.cpu().numpy().view(dt)


def _records(rng, F, nblk, inf_every=11):
    """Block minima on a grid of halves (many duplicates, inside windows and across them) with +inf sprinkled in."""
    rec = (rng.integers(0, 9, (F, nblk)) / 2).astype(np.float32)
    rec.reshape(-1)[::inf_every] = np.inf
    return rec, rng.integers(0, 2, F).astype(bool)


# ---------------------------------------------------------------------------------------------------------- windows
WINS = tuple(range(1, 16))             # every width LDPC_FCN_DISPATCH instantiates the two kernels for


@pytest.mark.parametrize("R,nblk,win", [(1, 1, 1), (1, 5, 5), (3, 6, 5), (257, 30, 5), (100, 16, 15), (5000, 40, 3)]
                         + [(3, win + 1, win) for win in WINS if win != 5])
def test_windows_bit_for_bit(dec, R, nblk, win):
    rng = np.random.default_rng(R + nblk + win)
    F = R + 13
    rec, ok = _records(rng, F, nblk)
    rec_d, ok_d = to_dev(rec, dec), to_dev(ok, dec)
    # every frame, no list
    x, y, cc = dec.fcn_windows(rec_d, ok_d, win=win)
    wx, wy = FM.windows(rec, ok, win)
    assert x.shape == ((nblk - win + 1) * F, win + 1) and y.dtype == torch.uint8
    assert np.array_equal(_bits(x, np.uint32), wx.view(np.uint32)) and np.array_equal(y.cpu().numpy(), wy)
    assert cc.cpu().numpy().tolist() == [int((wy == 0).sum()), int((wy == 1).sum())]
    assert np.isinf(wx).any() and len(np.unique(wx[:, :win])) < wx[:, :win].size
    # a shuffled subset of the frames
    index = rng.permutation(F)[:R].astype(np.int32)
    x, y, cc = dec.fcn_windows(rec_d, ok_d, index=to_dev(index, dec), win=win)
    wx, wy = FM.windows(rec[index], ok[index], win)
    assert x.shape == ((nblk - win + 1) * R, win + 1)
    assert np.array_equal(_bits(x, np.uint32), wx.view(np.uint32)) and np.array_equal(y.cpu().numpy(), wy)
    assert cc.cpu().numpy().tolist() == [int((wy == 0).sum()), int((wy == 1).sum())]
    # the compaction's own list: index[:count]
    idx_d, count = dec.compact(ok_d.to(torch.uint8))
    n = int(count.item())
    x, y, _ = dec.fcn_windows(rec_d, ok_d, index=idx_d[:n], win=win)
    wx, wy = FM.windows(rec[ok], ok[ok], win)
    assert np.array_equal(_bits(x, np.uint32), wx.view(np.uint32)) and np.array_equal(y.cpu().numpy(), wy)


def _abi_windows(dec, rec_d, ok_d, idx_d, R, nblk, win, fill=7):
    rows = max((nblk - win + 1) * max(R, 1), 1) if 1 <= win <= nblk else 8
    x = torch.full((rows, max(win, 1) + 1), float(fill), dtype=torch.float32, device=dec.device)
    y = torch.full((rows,), fill, dtype=torch.uint8, device=dec.device)
    cc = torch.full((2,), fill, dtype=torch.int64, device=dec.device)
    rc = dec.L.ldpc_fcn_windows(dec._ctx, _p(rec_d), _p(ok_d), _p(idx_d), R, nblk, win, _p(x), _p(y), _p(cc), _stream(dec))
    torch.cuda.synchronize()
    return rc, x, y, cc


def test_windows_no_records_and_refusals(dec):
    rec, ok = _records(np.random.default_rng(0), 9, 12)
    rec_d, ok_d = to_dev(rec, dec), to_dev(ok, dec)
    rc, x, y, cc = _abi_windows(dec, rec_d, ok_d, None, 0, 12, 5)
    assert rc == 0 and torch.all(x == 7) and torch.all(y == 7) and torch.all(cc == 7)
    x0, y0, cc0 = dec.fcn_windows(rec_d[:0].contiguous(), ok_d[:0].contiguous(), win=5)
    assert x0.shape == (0, 6) and y0.shape == (0,) and cc0.tolist() == [0, 0]
    err = lambda: dec.L.ldpc_last_error().decode()     # noqa: E731

    def refused(expect, *args):
        rc, x, y, cc = _abi_windows(dec, *args)
        msg = err()
        assert rc == -1 and msg.startswith("ldpc_fcn_windows: ") and expect in msg, (rc, msg)
        assert torch.all(x == 7) and torch.all(y == 7) and torch.all(cc == 7), "refused, yet an output was written"

    refused("win = 0", rec_d, ok_d, None, 9, 12, 0)
    refused("win = 16", rec_d, ok_d, None, 9, 12, 16)
    refused("nblk = 4", rec_d, ok_d, None, 9, 4, 5)
    refused("nblk = 1025", rec_d, ok_d, None, 9, 1025, 5)
    refused("R = -1", rec_d, ok_d, None, -1, 12, 5)
    refused("d_block_min is NULL", None, ok_d, None, 9, 12, 5)
    refused("d_success is NULL", rec_d, None, None, 9, 12, 5)
    for missing, name in ((7, "d_inputs"), (8, "d_labels")):
        args = [dec._ctx, _p(rec_d), _p(ok_d), None, 9, 12, 5, _p(torch.zeros(8 * 9 * 6, device=dec.device)),
                _p(torch.zeros(72, dtype=torch.uint8, device=dec.device)), None, _stream(dec)]
        args[missing] = None
        assert dec.L.ldpc_fcn_windows(*args) == -1 and err() == f"ldpc_fcn_windows: {name} is NULL"
    # the Python layer
    with pytest.raises(ValueError, match="win = 13"):
        dec.fcn_windows(rec_d, ok_d, win=13)
    with pytest.raises(ValueError, match="success"):
        dec.fcn_windows(rec_d, ok_d[:5].contiguous(), win=5)
    with pytest.raises(ValueError, match="block_min"):
        dec.fcn_windows(rec_d.double(), ok_d, win=5)
    with pytest.raises(ValueError, match="outside the 9 rows"):
        dec.fcn_windows(rec_d, ok_d, index=to_dev(np.array([0, 9], np.int32), dec), win=5)
    with pytest.raises(ValueError, match="index"):
        dec.fcn_windows(rec_d, ok_d, index=to_dev(np.array([0, 1], np.int64), dec), win=5)


# ---------------------------------------------------------------------------------------------------------- the batch
def _batch(dec, win, N, seed, scale=0.05, weights=None):
    """N windows of finite random records with labels by the window rule, per-class weights, random classifier weights."""
    rng = np.random.default_rng(seed)
    nblk = win + 7
    R = -(-N // 8)
    rec = rng.uniform(0, 20, (R, nblk)).astype(np.float32)
    x, y = FM.windows(rec, rng.integers(0, 4, R) > 0, win)
    x, y = x[:N], y[:N].copy()
    sw = rng.uniform(0.25, 4.0, N).astype(np.float32)
    W1, W2 = weights if weights is not None else DM.random_fcn_weights(rng, win, scale)
    return dict(x=x, y=y, sw=sw, W1=W1, W2=W2, w=np.concatenate([W1.ravel(), W2.ravel()]).astype(np.float32),
                x_d=to_dev(x, dec), y_d=to_dev(y, dec), sw_d=to_dev(sw, dec), win=win)


def _abi_grad(dec, c, idx_d, B, penalty=10.0, want=(1, 1, 1, 1, 1), fill=None, w="own", nw=None, win=None, weight=True,
              x_d="own", y_d="own"):
    """The C call with any subset of (p, loss, grad, acc, counts); -> (rc, [tensors or None])."""
    win = c["win"] if win is None else win
    w = c["w"] if isinstance(w, str) else w
    nw = (w.size if w is not None else (win + 1) ** 2 + 2 * (win + 1)) if nw is None else nw
    mk = (lambda shape, dt: torch.full(shape, fill, dtype=dt, device=dec.device)) if fill is not None else dec.empty
    shapes = [((max(B, 1), 2), torch.float32), ((1,), torch.float64), ((max(nw, 1),), torch.float64), ((2,), torch.float64),
              ((3,), torch.int64)]
    outs = [mk(s, dt) if on else None for (s, dt), on in zip(shapes, want)]
    rc = dec.L.ldpc_fcn_grad(dec._ctx, _p(c["x_d"] if isinstance(x_d, str) else x_d), _p(c["y_d"] if isinstance(y_d, str) else y_d),
                             _p(c["sw_d"]) if weight else None, _p(idx_d), B, win,
                             w.ctypes.data_as(C.POINTER(C.c_float)) if w is not None else None, nw, penalty, *[_p(o) for o in outs],
                             _stream(dec))
    torch.cuda.synchronize()
    return rc, outs


DT = (np.uint32, np.uint64, np.uint64, np.uint64, np.int64)


@pytest.mark.parametrize("win", [1, 5, 15])
def test_forward_in_the_sliding_kernels_order_and_every_subset_of_outputs(dec, win):
    """d_p against DM.classifier_p1, the host order of the sliding kernel's classifier, under the rule the scan tests accept
    that comparison by (DM.Classifier.near): the device's expf may differ from NumPy's in the last place, which moves p1 by
    far less than 1e-6, and a logit difference beyond 110 saturates p1 to exactly 0 or 1 in any float32 exp."""
    for weights in (None, DM.stopping_fcn_weights(win), DM.stopping_fcn_weights(win, per_block=40.0, per_metric=3.0)):
        c = _batch(dec, win, 257, 10 + win, weights=weights)
        rc, full = _abi_grad(dec, c, None, 257)
        assert rc == 0
        p = full[0].cpu().numpy()
        want = DM.classifier_p1(c["x"], c["W1"], c["W2"])
        z = DM.classifier_logits(c["x"], c["W1"], c["W2"]).astype(np.float64)
        saturated = np.abs(z[:, 1] - z[:, 0]) > 110
        assert np.all(np.abs(p[:, 1] - want) < 1e-6) and np.array_equal(p[saturated, 1], want[saturated])
        assert np.all(np.abs(p[:, 0] - (1 - want.astype(np.float64))) < 1e-6)
        assert weights is None or saturated.any() == (weights[1][win, 1] == 40.0)
        ref = [_bits(t, dt) for t, dt in zip(full, DT)]
        for want_mask in itertools.product((0, 1), repeat=5):
            rc, outs = _abi_grad(dec, c, None, 257, want=want_mask)
            assert rc == 0
            for k, t in enumerate(outs):
                assert t is None or np.array_equal(_bits(t, DT[k]), ref[k]), (want_mask, k)
        # the Python layer: the same bits
        out = dec.fcn_grad(c["x_d"], c["y_d"], c["w"], win, 10.0, weight=c["sw_d"], want_p=True)
        got = [out["p"], out["loss_sum"], out["grad"], out["acc"], out["counts"]]
        assert all(np.array_equal(_bits(t, DT[k]), ref[k]) for k, t in enumerate(got))
        out = dec.fcn_grad(c["x_d"], c["y_d"], c["w"], win, 10.0, weight=c["sw_d"], want_grad=False)
        assert out["grad"] is None and out["p"] is None and np.array_equal(_bits(out["loss_sum"], np.uint64), ref[1])


def _check_model(dec, c, index, penalty, use_weight, what):
    """Loss, gradient, accuracy sums and counts against the float64 model fed the kernel's own d_p: what is left is the
    rounding of float64 sums taken in another order, TREE x the L1 mass of the summed terms."""
    idx_d = to_dev(index, dec) if index is not None else None
    out = dec.fcn_grad(c["x_d"], c["y_d"], c["w"], c["win"], penalty, weight=c["sw_d"] if use_weight else None, index=idx_d,
                       want_p=True)
    sel = index if index is not None else slice(None)
    model = FM.loss_grad(c["x"][sel], c["y"][sel], c["sw"][sel] if use_weight else None, c["W1"], c["W2"], penalty,
                         p=out["p"].cpu().numpy())
    grad, mass = out["grad"].cpu().numpy(), FM.pack(model["mass_dW1"], model["mass_dW2"])
    err = np.abs(grad - FM.pack(model["dW1"], model["dW2"]))
    lerr = abs(out["loss_sum"].item() - model["loss"])
    print(f"{what}: worst gradient error / bound {float(np.max(err / np.maximum(TREE * mass, 1e-300))):.3g}, "
          f"loss error / bound {lerr / max(TREE * model['abs_loss'], 1e-300):.3g}")
    assert np.all(np.isfinite(grad)) and np.all(err <= TREE * mass)
    assert lerr <= TREE * model["abs_loss"]
    assert tuple(out["counts"].cpu().numpy().tolist()) == model["counts"]
    acc = out["acc"].cpu().numpy()
    assert abs(acc[0] - model["acc"][0]) <= TREE * model["abs_acc"] and abs(acc[1] - model["acc"][1]) <= TREE * model["abs_acc"]
    return out, model


# At these widths the draw of seed 1000 win + B predicts "stop" for no window labelled "continue" (by the host classifier), so
# the penalty would apply to no sample: the first later draw in which it does (to 1, 160 and 133 of the 257)
SEED_SHIFT = {2: 5, 7: 1, 11: 3}


@pytest.mark.parametrize("B,win", [(B, win) for win in (1, 5, 15) for B in (1, 3, 100, 257, 70001)]
                         + [(257, win) for win in WINS if win not in (1, 5, 15)])
def test_loss_and_gradient_against_the_model(dec, B, win):
    assert B <= 256 * 256 or B == 70001          # 70 001: more windows than the grid has threads, some threads take two
    N = min(B, 5000) + 7
    c = _batch(dec, win, N, 1000 * win + B + SEED_SHIFT.get(win, 0), scale=0.3)
    rng = np.random.default_rng(B)
    index = rng.integers(0, N, B).astype(np.int32)                 # repeats, any order
    if B >= 3:
        index[1] = index[0]
    applies = 0
    for use_weight, penalty in itertools.product((True, False), (1.0, 10.0)):
        out, model = _check_model(dec, c, index, penalty, use_weight, f"B={B} win={win} weight={use_weight} penalty={penalty}")
        applies += model["counts"][2]
    assert B < 257 or applies > 0                                  # the penalty applied to some sample
    # without a list: the first B rows in order
    if B <= N:
        sub = dict(c, x=c["x"][:B], y=c["y"][:B], sw=c["sw"][:B], x_d=c["x_d"][:B].contiguous(), y_d=c["y_d"][:B].contiguous(),
                   sw_d=c["sw_d"][:B].contiguous())
        _check_model(dec, sub, None, 10.0, True, f"B={B} win={win} no list")


def test_same_bits_on_any_stream_and_additive_over_the_batch(dec):
    win, B = 5, 70001
    c = _batch(dec, win, 5007, 3, scale=0.3)
    index = np.random.default_rng(1).integers(0, 5007, B).astype(np.int32)
    idx_d = to_dev(index, dec)
    runs = []
    for s in (torch.cuda.Stream(dec.device), torch.cuda.Stream(dec.device), None):
        with torch.cuda.stream(s if s is not None else torch.cuda.current_stream(dec.device)):
            for _ in range(2):
                out = dec.fcn_grad(c["x_d"], c["y_d"], c["w"], win, 10.0, weight=c["sw_d"], index=idx_d, want_p=True)
                runs.append([_bits(out[k], dt) for k, dt in zip(("p", "loss_sum", "grad", "acc", "counts"), DT)])
        torch.cuda.synchronize()
    for r in runs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(r, runs[0]))
    h = B // 2
    a = dec.fcn_grad(c["x_d"], c["y_d"], c["w"], win, 10.0, weight=c["sw_d"], index=idx_d[:h])
    b = dec.fcn_grad(c["x_d"], c["y_d"], c["w"], win, 10.0, weight=c["sw_d"], index=idx_d[h:])
    out, model = _check_model(dec, c, index, 10.0, True, "whole batch")
    mass = FM.pack(model["mass_dW1"], model["mass_dW2"])
    assert np.all(np.abs((a["grad"] + b["grad"] - out["grad"]).cpu().numpy()) <= TREE * mass)
    assert abs((a["loss_sum"] + b["loss_sum"] - out["loss_sum"]).item()) <= TREE * model["abs_loss"]
    assert np.all(np.abs((a["acc"] + b["acc"] - out["acc"]).cpu().numpy()) <= TREE * model["abs_acc"])
    assert torch.equal(a["counts"] + b["counts"], out["counts"])


def test_saturated_and_zero_weights(dec):
    win, N = 5, 300
    # p_y underflows: z1 - z0 = 1e5 k - 30 sum(window) lies beyond +-110 for every sample, so p is exactly (1, 0) or (0, 1)
    c = _batch(dec, win, N, 21, weights=DM.stopping_fcn_weights(win, per_block=1e5, per_metric=30.0))
    z = DM.classifier_logits(c["x"], c["W1"], c["W2"]).astype(np.float64)
    assert np.all(np.abs(z[:, 1] - z[:, 0]) > 110) and np.all(np.isfinite(z))
    for penalty in (1.0, 10.0):
        out, model = _check_model(dec, c, None, penalty, True, f"saturated, penalty {penalty}")
        p = out["p"].cpu().numpy()
        assert set(np.unique(p)) == {0.0, 1.0}
        wrong = p[np.arange(N), c["y"]] == 0
        assert 10 < wrong.sum() < N - 10
        assert not out["grad"].cpu().numpy().any()                   # p_y = 0: no gradient; p_y = 1: p - onehot = 0
        s = c["sw"].astype(np.float64) * np.where((p[:, 0] < p[:, 1]) & (c["y"] == 0), penalty, 1.0)
        want = float(np.sum(-s[wrong] * np.log(FM.FLOOR)))
        assert abs(out["loss_sum"].item() - want) <= TREE * want
    # zero weights: p = 0.5 each, the prediction is "continue" (p0 < p1 is false), and the gradient is the model's
    for name, W1, W2 in (("all zero", 0, 0), ("dense1 zero", 0, 1), ("dense2 zero", 1, 0)):
        base = _batch(dec, win, N, 22, scale=0.3)
        c = _batch(dec, win, N, 22, weights=(base["W1"] * np.float32(W1), base["W2"] * np.float32(W2)))
        out, model = _check_model(dec, c, None, 10.0, True, name)
        assert np.all(out["p"].cpu().numpy() == 0.5) and out["counts"].tolist() == [int((c["y"] == 0).sum()), int(c["y"].sum()), 0]
        g1, g2 = np.split(out["grad"].cpu().numpy(), [36])
        assert g1.any() == bool(W2) and g2.any() == bool(W1)
        assert abs(out["loss_sum"].item() - float(np.sum(c["sw"].astype(np.float64)) * -np.log(np.float64(np.float32(0.5))))) \
            <= TREE * model["abs_loss"]


def test_grad_no_batch_and_refusals(dec):
    win, N = 5, 40
    c = _batch(dec, win, N, 5)
    rc, outs = _abi_grad(dec, c, None, 0, fill=7)
    assert rc == 0 and all(torch.all(t == 7) for t in outs)
    empty = dec.fcn_grad(c["x_d"], c["y_d"], c["w"], win, 10.0, index=to_dev(np.zeros(0, np.int32), dec), want_p=True)
    assert empty["loss_sum"].item() == 0 and not empty["grad"].any() and empty["p"].shape == (0, 2) and not empty["counts"].any()
    err = lambda: dec.L.ldpc_last_error().decode()     # noqa: E731

    def refused(expect, B=N, **kw):
        rc, outs = _abi_grad(dec, c, None, B, fill=7, **kw)
        msg = err()
        assert rc == -1 and msg.startswith("ldpc_fcn_grad: ") and expect in msg, (rc, msg)
        assert all(torch.all(t == 7) for t in outs), "refused, yet an output was written"

    refused("win = 0", win=0, nw=48)
    refused("win = 16", win=16, nw=48)
    refused("n_weights = 47", w=c["w"][:-1])
    refused("n_weights = 48, win = 4 takes 35", win=4)
    refused("fcn_weights is NULL", w=None)
    refused("d_inputs is NULL", x_d=None)
    refused("d_labels is NULL", y_d=None)
    refused("B = -1", B=-1)
    # d_labels is not needed for the forward pass alone
    rc, outs = _abi_grad(dec, c, None, N, want=(1, 0, 0, 0, 0), y_d=None)
    assert rc == 0 and np.array_equal(_bits(outs[0], np.uint32), _bits(_abi_grad(dec, c, None, N)[1][0], np.uint32))
    # the Python layer
    with pytest.raises(ValueError, match="win = 0"):
        dec.fcn_grad(c["x_d"], c["y_d"], c["w"], 0, 10.0)
    with pytest.raises(ValueError, match="weights: 47"):
        dec.fcn_grad(c["x_d"], c["y_d"], c["w"][:-1], win, 10.0)
    with pytest.raises(ValueError, match="inputs"):
        dec.fcn_grad(c["x_d"][:, :5].contiguous(), c["y_d"], c["w"], win, 10.0)
    with pytest.raises(ValueError, match="labels"):
        dec.fcn_grad(c["x_d"], c["y_d"][:7].contiguous(), c["w"], win, 10.0)
    with pytest.raises(ValueError, match="weight"):
        dec.fcn_grad(c["x_d"], c["y_d"], c["w"], win, 10.0, weight=c["sw_d"][:7].contiguous())
    with pytest.raises(ValueError, match="outside the 40 rows"):
        dec.fcn_grad(c["x_d"], c["y_d"], c["w"], win, 10.0, index=to_dev(np.array([3, 40], np.int32), dec))
    with pytest.raises(ValueError, match="outside the 40 rows"):
        dec.fcn_grad(c["x_d"], c["y_d"], c["w"], win, 10.0, index=to_dev(np.array([-1, 4], np.int32), dec))


# ------------------------------------------------------------------------------------------ replay against the scan
PATH = [[0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0], [1, 1, 0, 0, 0, 0], [0, 0, 0, 1, 0, 0],
        [0, 2, 0, 0, 0, 0], [0, 0, 0, 0, 1, 0], [0, 1, 1, 0, 0, 0], [0, 0, 0, 0, 0, 1], [0, 0, 2, 0, 0, 0], [1, 0, 1, 0, 0, 0],
        [0, 1, 0, 1, 0, 0], [1, 0, 0, 1, 0, 0], [0, 0, 1, 1, 0, 0], [0, 1, 0, 0, 1, 0], [1, 0, 0, 0, 1, 0], [0, 0, 0, 2, 0, 0],
        [0, 0, 1, 0, 1, 0], [0, 1, 0, 0, 0, 1]]
# win -> (per_block, per_metric, soft_margin).  Under z1 - z0 = per_block k - per_metric sum(window) and the margin the 64 frames
# below stop after (blocks: frames, by the host classifier, with the closest any p1 comes to the margin)
#    1: {2: 2, 3: 2, 20: 60}, 3.5e-3        5: {5: 35, 6: 2, 20: 27}, 2.8e-3
#    8: {8: 56, 16: 1, 20: 7}, 1.1e-3      15: {15: 9, 16: 1, 20: 54}, 4.7e-3
REPLAY = {1: (0.35, 0.01, 0.5), 5: (0.35, 0.01, 0.32), 8: (0.35, 0.01, 0.2), 15: (2.0, 0.01, 0.12)}


def replay_frames(np_code):
    """64 CCSDS frames at 2.5 dB: ordering values = NMS-4 posteriors, metric = channel values, labels; the 20 blocks."""
    rng = np.random.default_rng(11)
    y, cw = np_oracle.make_frames(np_code.G, 2.5, 64, rng)[:2]
    y = y.astype(np.float32)
    x = np_oracle.nms_sparse(y, np_code.H, 4, np.float32(0.669435))[-1].astype(np.float32)
    _, b = np_oracle.segment_boundaries(64, 6)
    ranges = [range(int(b[i]), int(b[i + 1])) for i in range(6)]
    return x, y, cw, [np_oracle.error_pattern_gen(p, ranges, 64) for p in PATH]


@pytest.mark.parametrize("win", sorted(REPLAY))
def test_replay_of_the_sliding_scan(dec, np_code, win):
    """Windows from hosd_search's block minima, p1 from fcn_grad under the stopping classifier, the reference's lazy loop
    replayed on the host: deep_limit and global_min are ldpc_hosd_sliding's for every frame.  That holds the training
    kernels' forward pass and window order to slide_p1's."""
    from short_ldpc_decoding_osd_amd.ordered_statistics_decoding import _teps_from_matrix
    x, y, cw, blocks = replay_frames(np_code)
    per_block, per_metric, margin = REPLAY[win]
    w1, w2 = DM.stopping_fcn_weights(win, per_block, per_metric)
    w = np.concatenate([w1.ravel(), w2.ravel()])
    teps = to_dev(np.concatenate([_teps_from_matrix(E) for E in blocks]), dec)
    off = to_dev(np.insert(np.cumsum([len(E) for E in blocks]), 0, 0).astype(np.int32), dec)
    xd, yd, lab = to_dev(x, dec), to_dev(y, dec), to_dev(pack_np(cw).view(np.int64), dec)
    front = dec.hosd_front(xd)
    search = dec.hosd_search(xd, yd, front, teps, off, label_bits=lab)
    bm = search["block_min"]
    ok = bm.min(dim=1).values == search["truth"]
    inputs, labels, _ = dec.fcn_windows(bm, ok, win=win)
    p1 = dec.fcn_grad(inputs, labels, w, win, 1.0, want_p=True, want_grad=False)["p"][:, 1].cpu().numpy().reshape(-1, 64)
    assert p1.shape == (len(PATH) - win + 1, 64)
    assert np.all(np.abs(p1 - margin) >= 1e-6)                    # no decision within an ulp of exp of the margin
    slid = dec.hosd_sliding(xd, yd, front, teps, off, win, margin, w, label_bits=lab)
    deep, gmin = slid["deep_limit"].cpu().numpy(), slid["global_min"].cpu().numpy()
    bm_np = bm.cpu().numpy()
    for f in range(64):
        want_deep, want_gmin = FM.replay_sliding(bm_np[f], p1[:, f], win, margin)
        assert deep[f] == want_deep and gmin[f].view(np.uint32) == want_gmin.view(np.uint32), f
    assert len(set(deep.tolist())) >= 3, sorted(set(deep.tolist()))
