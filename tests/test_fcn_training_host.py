"""CPU: the host side of the sliding-window classifier's training stage -- the float64 model of
tests/fcn_training_model.py against torch autograd, the window rule on hand-made records, the NumPy loss and the class
weights of predict_phase, checkpoints through the test stage's restore, the directories, the refusals, the initializer."""
import os

import numpy as np
import pytest
import torch

from tests import fcn_training_model as FM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALIST = os.path.join(ROOT, "short_ldpc_decoding_osd_amd", "data", "CCSDS_ldpc_n128_k64.alist")


@pytest.fixture
def gl_state():
    from short_ldpc_decoding_osd_amd import globalmap as GL
    saved = dict(GL.map)
    yield GL
    GL.map.clear()
    GL.map.update(saved)


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _case(win, B, seed):
    """Random inputs (the rule does not care that real windows are sorted), centred so that both predictions occur under
    random weights -- the penalty applies to some samples and not to others --, with eight rows scaled until p_y
    underflows below 1e-30 for the wrong label."""
    rng = np.random.default_rng(seed)
    D = win + 1
    x = rng.uniform(-10, 10, (B, D)).astype(np.float32)
    W1 = (rng.standard_normal((D, D)) * 0.3).astype(np.float32)
    W2 = (rng.standard_normal((D, 2)) * 0.3).astype(np.float32)
    x[:8] *= np.float32(400.0)
    y = rng.integers(0, 2, B)
    sw = rng.uniform(0.5, 3.0, B).astype(np.float32)
    return x, y, sw, W1, W2


@pytest.mark.parametrize("win", [1, 5, 15])
def test_model_loss_and_gradient_equal_autograd(win):
    x, y, sw, W1, W2 = _case(win, 300, win)
    index = np.random.default_rng(win).integers(0, 300, 500)          # repeats, any order
    index[:16] = np.repeat(np.arange(8), 2)                           # the underflowing rows, twice each
    xb, yb, swb = x[index], y[index], sw[index]
    for penalty in (1.0, 10.0):
        model = FM.loss_grad(xb, yb, swb, W1, W2, penalty)
        a, b = (torch.tensor(w, dtype=torch.float64, requires_grad=True) for w in (W1, W2))
        p = torch.softmax(torch.tensor(xb, dtype=torch.float64) @ a @ b, dim=1)
        yt = torch.tensor(yb)
        pen = torch.where((p[:, 0] < p[:, 1]) & (yt == 0), penalty, 1.0).detach()
        py = p[torch.arange(len(yb)), yt]
        loss = torch.sum(-torch.log(torch.clamp(py, min=FM.FLOOR)) * pen * torch.tensor(swb, dtype=torch.float64))
        loss.backward()
        below = _np(py.detach()) < FM.FLOOR
        applies = (model["pred"] == 1) & (yb == 0)
        assert below.sum() >= 4 and applies.sum() >= 10 and (~applies).sum() >= 10
        assert np.all(model["g"][below] == 0)
        floor_terms = -swb[below].astype(np.float64) * np.where(applies[below], penalty, 1.0) * np.log(FM.FLOOR)
        assert abs(model["loss"] - loss.item()) <= 1e-12 * model["abs_loss"]
        assert model["abs_loss"] >= floor_terms.sum() > 0
        assert np.all(np.abs(model["dW1"] - _np(a.grad)) <= 1e-11 * model["mass_dW1"] + 1e-300)
        assert np.all(np.abs(model["dW2"] - _np(b.grad)) <= 1e-11 * model["mass_dW2"] + 1e-300)
        assert sum(model["counts"]) == len(yb) and model["counts"][2] == applies.sum()
        # a repeated sample counts once per repeat
        twice = FM.loss_grad(np.concatenate([xb, xb]), np.concatenate([yb, yb]), np.concatenate([swb, swb]), W1, W2, penalty)
        assert abs(twice["loss"] - 2 * model["loss"]) <= 1e-12 * twice["abs_loss"]
        assert np.allclose(twice["dW2"], 2 * model["dW2"], rtol=1e-12, atol=1e-12 * model["mass_dW2"].max())


def test_windows_on_hand_made_records(gl_state):
    rec = np.array([[3, 1, 1, 2, 5, 1],        # ties inside a window; the row minimum in several windows
                    [4, 4, 4, 4, 4, 4],        # every window holds the minimum
                    [9, 8, 7, 6, 5, 0.5],      # only the last window
                    [2, 7, 1, 8, 2, 8]], np.float32)
    x, y = FM.windows(rec, [True, True, True, False], 2)
    assert x.shape == (20, 3) and y.shape == (20,)
    assert np.array_equal(x[0::4, :2], [[1, 3], [1, 1], [1, 2], [2, 5], [1, 5]])          # record 0, ascending
    assert np.array_equal(x[:, 2], np.repeat(np.arange(5), 4))                              # window-major
    assert np.array_equal(y.reshape(5, 4).T, [[1, 1, 1, 0, 1], [1, 1, 1, 1, 1], [0, 0, 0, 0, 1], [0, 0, 0, 0, 0]])
    # nblk == win: one window, which always holds the minimum
    x, y = FM.windows(rec, [True, False, True, True], 6)
    assert x.shape == (4, 7) and np.array_equal(y, [1, 0, 1, 1]) and np.all(x[:, 6] == 0)
    assert np.array_equal(x[0, :6], [1, 1, 1, 2, 3, 5])
    # the package's rule on random records with duplicates and +inf: reform_inputs wants finite records
    from short_ldpc_decoding_osd_amd import interval_boundary as IB
    rng = np.random.default_rng(0)
    rec = rng.integers(0, 6, (37, 9)).astype(np.float32)
    ok = rng.integers(0, 2, 37).astype(bool)
    for win in (1, 3, 9):
        wx, wy = FM.windows(rec, ok, win)
        hx, hy = IB._host_windows(rec, ok, win)
        assert np.array_equal(wx.view(np.uint32), hx.view(np.uint32)) and np.array_equal(wy, hy)
    gl_state.dl_training_setting(["prog", "2.7", "2.7", "100", "12", ALIST, "NMS-1"])
    gl_state.set_map('sliding_win_width', 3)
    records = np.concatenate([rec, np.where(ok, 1.0, -1.0)[:, None]], axis=1)
    rx, ry = IB.reform_inputs(records)
    wx, wy = FM.windows(rec, ok, 3)
    assert np.array_equal(_np(rx).view(np.uint32), wx.view(np.uint32)) and np.array_equal(_np(ry), wy)
    records[5, 4] = np.inf
    with pytest.raises(ValueError, match="record 5 .* block 4"):
        IB.reform_inputs(records)
    with pytest.raises(ValueError, match="nblk"):
        IB.reform_inputs(records[:, :3])


def test_calculation_loss_and_class_weights_match_the_model(gl_state):
    from short_ldpc_decoding_osd_amd import predict_phase as PP
    gl_state.set_map('regulation_weight', 10.)
    gl_state.set_map('dl_init_seed', 4)
    rng = np.random.default_rng(1)
    B = 400
    labels = (rng.uniform(size=B) < 0.2).astype(np.uint8)
    perm, lab, weight, one_hot = PP.shuffle_data(np.zeros((B, 6), np.float32), labels, epoch=3)
    want, per_class = FM.class_weights(labels)
    assert np.array_equal(_np(weight).view(np.uint32), want.view(np.uint32)) and _np(weight).dtype == np.float32
    assert np.array_equal(PP.class_weights((int((labels == 0).sum()), int(labels.sum()))), [per_class[0], per_class[1]])
    assert np.array_equal(_np(one_hot), np.stack([labels == 0, labels == 1], 1).astype(np.float32))
    assert perm.dtype == torch.int32 and np.array_equal(np.sort(_np(perm)), np.arange(B))
    assert torch.equal(perm, PP.shuffle_data(None, labels, epoch=3)[0])
    assert not torch.equal(perm, PP.shuffle_data(None, labels, epoch=4)[0])
    gl_state.set_map('dl_init_seed', 5)
    assert not torch.equal(perm, PP.shuffle_data(None, labels, epoch=3)[0])
    p1 = rng.uniform(size=B).astype(np.float32)
    p1[:5] = [0.0, 1.0, 1e-35, 1 - 1e-7, 0.5]
    p = np.stack([np.float32(1) - p1, p1], axis=1)
    got = PP.calculation_loss(p, _np(one_hot), _np(weight))
    model = FM.loss_grad(np.zeros((B, 6)), labels, want, np.zeros((6, 6)), np.zeros((6, 2)), 10.0, p=p)
    assert abs(got - model["loss"]) <= 1e-12 * model["abs_loss"]
    assert got > PP.calculation_loss(p, _np(one_hot), np.zeros(B)) == 0.0


def test_one_class_is_refused(gl_state):
    from short_ldpc_decoding_osd_amd import predict_phase as PP
    for counts in ((0, 5), (7, 0)):
        with pytest.raises(ValueError, match="both label classes"):
            PP.class_weights(counts)
    with pytest.raises(ValueError, match="both label classes"):
        PP.shuffle_data(None, np.zeros(12, np.uint8))
    with pytest.raises(ValueError, match="both label classes"):
        PP.shuffle_data(None, np.ones(12, np.uint8))


@pytest.mark.parametrize("win", [1, 5, 15])
def test_initialize(win):
    from short_ldpc_decoding_osd_amd import nn_net
    fcn = nn_net.Predict_outlier_light(win).initialize(3)
    d = win + 1
    assert fcn.dense1.shape == (d, d) and fcn.dense2.shape == (d, 2)
    assert fcn.dense1.dtype == fcn.dense2.dtype == np.float32
    assert np.all(np.abs(fcn.dense2) <= np.sqrt(6.0 / (d + 2))) and np.abs(fcn.dense2).max() > 0
    assert np.abs(fcn.dense1).max() < 0.05 * 6 and (win == 1 or 0.02 < fcn.dense1.std() < 0.1)
    again = nn_net.Predict_outlier_light(win).initialize(3)
    assert np.array_equal(fcn.packed().view(np.uint32), again.packed().view(np.uint32))
    assert not np.array_equal(fcn.packed(), nn_net.Predict_outlier_light(win).initialize(4).packed())
    assert fcn.packed().size == d * d + 2 * d and nn_net.Predict_outlier_light.TRAINABLE == ("dense1", "dense2")
    assert [v is getattr(fcn, a) for v, a in zip(fcn.trainable_variables(), fcn.TRAINABLE)] == [True, True]
    with pytest.raises(RuntimeError):
        nn_net.Predict_outlier_light(win).trainable_variables()


def test_checkpoint_restores_through_load_fcn_and_resumes_the_optimizer(tmp_path, gl_state):
    from short_ldpc_decoding_osd_amd import nn_net, nn_testing, nn_training, predict_phase as PP, tf_checkpoint
    from short_ldpc_decoding_osd_amd.nms_train import LegacyAdam
    win = 5
    gl_state.set_map('sliding_win_width', win)
    fcn = nn_net.Predict_outlier_light(win).initialize(1)
    opt = LegacyAdam(0.001)
    rng = np.random.default_rng(2)
    for _ in range(3):
        opt.apply_gradients([(rng.standard_normal(getattr(fcn, a).shape).astype(np.float32), a, fcn.__dict__) for a in fcn.TRAINABLE])
    ckpts_dir = str(tmp_path) + "/"
    nn_training.checkpoint_saver(fcn, opt, ckpts_dir, 'ldpc-ckpt', PP.VARIABLE_PATHS)(3)
    names = set(tf_checkpoint.read_checkpoint(ckpts_dir + 'ldpc-ckpt-3'))
    S = nn_testing.VARIABLE_SUFFIX
    assert names == {f"myAwesomeOptimizer/iter{S}"} | {f"myAwesomeModel/{layer}/kernel{tail}{S}" for layer in ("dense1", "dense2")
                                                       for tail in ("", "/.OPTIMIZER_SLOT/myAwesomeOptimizer/m",
                                                                    "/.OPTIMIZER_SLOT/myAwesomeOptimizer/v")}
    restored = nn_testing.load_fcn([ckpts_dir, 'ldpc-ckpt', 'latest'])
    assert np.array_equal(restored.packed().view(np.uint32), fcn.packed().view(np.uint32))
    step, prefix = PP.retore_saved_model(ckpts_dir, 'latest', 'ldpc-ckpt')
    assert step == 3 and prefix.endswith('ldpc-ckpt-3')
    fresh = nn_training.restore_optimizer(LegacyAdam(0.001), prefix, PP.VARIABLE_PATHS)
    assert fresh.iterations == 3 and set(fresh.m) == set(fresh.v) == {"dense1", "dense2"}
    for a in fcn.TRAINABLE:
        assert np.array_equal(fresh.m[a].view(np.uint32), opt.m[a].view(np.uint32))
        assert np.array_equal(fresh.v[a].view(np.uint32), opt.v[a].view(np.uint32))
    # one more step from the restored state equals one more step of the original
    g = [rng.standard_normal(getattr(fcn, a).shape).astype(np.float32) for a in fcn.TRAINABLE]
    opt.apply_gradients([(gi, a, fcn.__dict__) for gi, a in zip(g, fcn.TRAINABLE)])
    fresh.apply_gradients([(gi, a, restored.__dict__) for gi, a in zip(g, fcn.TRAINABLE)])
    assert np.array_equal(restored.packed().view(np.uint32), fcn.packed().view(np.uint32))


def test_training_and_test_stage_name_the_same_classifier_directory(tmp_path, gl_state):
    root = str(tmp_path / "stage") + "/"
    for snr, T, length, order in (("2.7", "12", 30, 3), ("3.25", "8", 12, 2)):
        gl_state.dl_training_setting(["prog", snr, snr, "100", T, ALIST, "NMS-1"])
        gl_state.set_map('dl_training_dir', root)
        gl_state.set_map('decoding_length', length)
        gl_state.set_map('threshold_sum', order)
        trained = gl_state.dl_training_set_predict_model(True)
        gl_state.set_map('training_snr', float(snr))
        assert trained == gl_state.set_predict_model(True) and os.path.isdir(trained[0])
        assert trained[0] == f"{root}ckpts/fcn/{snr}-{snr}dB/{T}th/len-{length}-order-{order}/"
        assert gl_state.dl_training_set_predict_model(False) == gl_state.set_predict_model(False)
        assert "/benchmark/" in gl_state.dl_training_set_predict_model(False)[0]
