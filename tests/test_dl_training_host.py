"""Host side of the DL-OSD training stage: the moment identity the training kernel rests on against torch autograd, the
fresh weights of conv_bitwise, the statistics functions on hand-made values against a per-frame restatement, the pickle
the test stage reads back, and the directories both stages share."""
import os
import pickle
from collections import Counter

import numpy as np
import pytest
import torch

from short_ldpc_decoding_osd_amd import Code
from short_ldpc_decoding_osd_amd import globalmap as GL
from short_ldpc_decoding_osd_amd import nn_net, nn_testing, nn_training
from tests import dl_training_model as TM
from tests import dlosd_model as DM


@pytest.fixture
def gl_state():
    saved = dict(GL.map)
    yield GL
    GL.map.clear()
    GL.map.update(saved)


@pytest.mark.parametrize("L", [7, 8, 13, 64])
def test_moment_identity_equals_autograd(L):
    """g, the moments and the backward pass at m in float64 NumPy == torch float64 autograd of the whole batch loss,
    within 1e-12 of the largest gradient entry."""
    rng = np.random.default_rng(L)
    F, n = 5, 37
    ws = [w.astype(np.float64) for w in DM.random_cnn_weights(rng, L)]
    rows = (rng.standard_normal((F, L, n)) * 3).astype(np.float32)
    labels = rng.integers(0, 2, (F, n))
    model = TM.cnn_loss_grad(rows, labels, ws)
    loss, grads, out = TM.torch_loss_grad(rows, labels, ws)
    assert abs(model["loss"] - loss) <= 1e-12 * abs(loss)
    want, got = TM.pack(grads), TM.pack(model["grads"])
    assert got.shape == want.shape == (145 + 2 * (L - 6),)
    assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))
    # the float64 forward of the model is the network torch evaluates
    x = rows.astype(np.float64).transpose(0, 2, 1).reshape(-1, L)
    assert np.allclose(TM.forward64(x, ws).reshape(F, n), out, rtol=1e-12, atol=1e-12)


def test_initialize_is_glorot_uniform_with_zero_bias():
    L = 13
    nn = nn_net.conv_bitwise(list_length=L, n_dims=128).initialize(seed=3)
    sh = nn.shapes()
    limits = dict(cnv_one=np.sqrt(6 / (3 * 1 + 3 * 8)), cnv_two=np.sqrt(6 / (3 * 8 + 3 * 4)), cnv_three=np.sqrt(6 / (3 * 4 + 3 * 2)),
                  dense_kernel=np.sqrt(6 / (2 * (L - 6) + 1)))
    for name, v in zip(nn.TRAINABLE, nn.trainable_variables()):
        assert v.shape == sh[name] and v.dtype == np.float32
        if name == "dense_bias":
            assert np.all(v == 0)
        else:
            assert np.all(np.abs(v) <= np.float32(limits[name])), name
            assert np.max(np.abs(v)) > 0.5 * limits[name], name      # (24 draws or more: not a narrower distribution)
    assert nn.packed().size == 145 + 2 * (L - 6)
    same = nn_net.conv_bitwise(list_length=L, n_dims=128).initialize(seed=3)
    other = nn_net.conv_bitwise(list_length=L, n_dims=128).initialize(seed=4)
    assert np.array_equal(same.packed(), nn.packed()) and not np.array_equal(other.packed(), nn.packed())
    with pytest.raises(RuntimeError):
        nn_net.conv_bitwise(list_length=L, n_dims=128).trainable_variables()


def _hand_made(code, rng, F):
    """Values with a tie across the MRB boundary (frame 0), zeros and negative zeros (frame 2), many ties (frame 3);
    among random frames some have dependent most-reliable columns, so the elimination exchanges columns."""
    n, k = code.check_matrix_column, code.k
    x = (rng.standard_normal((F, n)) * 2).astype(np.float32)
    labels = rng.integers(0, 2, (F, n)).astype(np.int64)
    order = np.argsort(np.abs(x[0]), kind="stable")
    x[0, order[n - k]] = -np.abs(x[0, order[n - k - 1]])          # |.| tie between sorted positions n-k-1 and n-k
    x[2, :5] = 0.0
    x[2, 5:9] = -0.0
    x[3] = np.round(x[3])                                          # many ties
    return x, labels


def test_statistics_equal_the_per_frame_restatement(gl_state, alist_path):
    code = Code(alist_path)
    gl_state.set_map('code_parameters', code)
    gl_state.set_map('segment_num', 6)
    n, k = code.check_matrix_column, code.k
    rng = np.random.default_rng(11)
    x, labels = _hand_made(code, rng, 40)
    # the tie straddles the boundary and goes to the lower index
    order = np.argsort(np.abs(x[0]), kind="stable")
    assert abs(x[0, order[n - k - 1]]) == abs(x[0, order[n - k]]) and order[n - k - 1] < order[n - k]
    seg, boundary = gl_state.secure_segment_threshold()
    assert int(boundary[-1]) == k
    mrbs, swaps = zip(*(TM.frame_mrb(code, row) for row in x))
    assert max(swaps) > 0, "no frame of the set needs a column exchange"
    # evaluate_MRB_bit
    got = nn_training.evaluate_MRB_bit(x, labels)
    assert isinstance(got, Counter) and got == TM.mrb_bit_counts(x, labels, k)
    assert nn_training.evaluate_MRB_bit(torch.from_numpy(x), torch.from_numpy(labels)) == got
    # evaluate_MRB_pattern on the restatement's MRBs, unsorted as the reference hands them over
    cnt = nn_training.evaluate_MRB_pattern(x, labels, list(mrbs), list(swaps), Counter(), boundary)
    want = Counter(TM.pattern_word(row, lab, mrb, boundary) for row, lab, mrb in zip(x, labels, mrbs))
    assert cnt == want and sum(cnt.values()) == len(x)
    assert all(len(key.split(",")) == 6 for key in cnt)
    # dic_union sums and sorts
    assert nn_training.dic_union({3: 1, 1: 2}, Counter({1: 5, 0: 1})) == {0: 1, 1: 7, 3: 1}
    assert list(nn_training.dic_union({3: 1, 1: 2}, {0: 1})) == [0, 1, 3]


def test_pickle_is_what_the_test_stage_reads(tmp_path, gl_state, alist_path):
    """Six objects in the reference's order under <root>/log/<type>/<lo>-<hi>dB/: query_decoding_path reads the sixth
    and orders its keys by descending ratio."""
    gl_state.dl_training_setting(["prog", "2.7", "2.7", "100", "12", alist_path, "NMS-1"])
    gl_state.set_map('dl_training_dir', str(tmp_path) + "/")     # (the test-stage functions append to it as it stands)
    gl_state.set_map('training_snr', 2.7)
    gl_state.set_map('threshold_sum', 3)
    log_dir = gl_state.dl_training_log_dir()
    assert log_dir == str(tmp_path) + "/log/NMS-1/2.7-2.7dB/" == gl_state.pattern_log_dir()
    os.makedirs(log_dir)
    ratio = Counter({"0,0,0,0,0,0": 0.5, "0,1,0,0,0,0": 0.05, "1,0,0,0,0,0": 0.2, "0,0,1,1,0,0": 0.01, "1,1,1,1,0,0": 0.3})
    with open(log_dir + "dist-error-pattern-model_cnn.pkl", "wb") as fh:
        for obj in (10, {0: 1}, {0: 2}, {0: 3}, Counter({0: 5}), ratio):
            pickle.dump(obj, fh)
    path, nn_type = nn_testing.query_decoding_path([True, False, False], ['model_cnn', 'model_rnn1', 'model_rnn2'], True)
    assert nn_type == 'model_cnn'
    assert path == [[0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0], [0, 0, 1, 1, 0, 0]]   # (order 4 filtered out)


def test_directories_of_training_are_those_of_testing(tmp_path, gl_state, alist_path):
    argv = ["prog", "2.7", "2.7", "100", "12", alist_path, "NMS-1"]
    gl_state.dl_training_setting(argv)
    for key, val in dict(snr_lo=2.7, snr_hi=2.7, unit_batch_size=100, num_iterations=12, selected_decoder_type="NMS-1",
                         epochs=100, initial_learning_rate=0.001, decay_rate=0.95, decay_step=500, termination_step=2000,
                         print_interval=100, record_interval=100, nn_train=True, segment_num=6, threshold_sum=3,
                         decoding_length=30, sliding_win_width=5).items():
        assert gl_state.get_map(key) == val, key
    lr = gl_state.optimizer_setting()
    assert lr(0) == np.float32(0.001) and lr(500) == np.float32(0.001 * 0.95)
    # the reference's default: everything under the working directory
    assert gl_state.dl_training_log_dir() == "./log/NMS-1/2.7-2.7dB/"
    root = str(tmp_path / "run")
    gl_state.set_map('dl_training_dir', root)
    indicators, prefixes = [True, False, False], ['model_cnn', 'model_rnn1', 'model_rnn2']
    info = gl_state.dl_training_logistic_setting(indicators, prefixes)
    assert info == [root + "/ckpts/model_cnn/2.7-2.7dB/12th/", "ldpc-ckpt", "latest"] and os.path.isdir(info[0])
    # a checkpoint written there is the one the test stage restores
    nn = nn_net.conv_bitwise().initialize(1)
    from short_ldpc_decoding_osd_amd.nms_train import LegacyAdam
    opt = LegacyAdam(lr)
    opt.apply_gradients([(np.ones_like(v), a, nn.__dict__) for a, v in zip(nn.TRAINABLE, nn.trainable_variables())])
    nn_training.checkpoint_saver(nn, opt, info[0], info[1])(7)
    gl_state.global_setting(["prog", "2.7", "2.7", "1", "100", "12", alist_path, "NMS-1"], stage="DL")
    gl_state.set_map('dl_training_dir', root + "/")
    assert gl_state.logistic_setting_model(indicators, prefixes) == info
    assert gl_state.pattern_log_dir() == root + "/log/NMS-1/2.7-2.7dB/"
    prefix = nn_testing.retore_saved_model(*[info[0], info[2], info[1]])
    restored = nn_testing.restore_conv_bitwise(nn_net.conv_bitwise(), prefix)
    assert np.array_equal(restored.packed(), nn.packed())
    # ... and the optimizer comes back with its step count and slots
    step, ckpt_f = nn_training.retore_saved_model(info[0], 'latest', info[1])
    assert step == 7 and ckpt_f == prefix
    back = nn_training.restore_optimizer(LegacyAdam(lr), ckpt_f)
    assert back.iterations == 1 and set(back.m) == set(nn.TRAINABLE) == set(back.v)
    for a in nn.TRAINABLE:
        assert np.array_equal(back.m[a], opt.m[a]) and np.array_equal(back.v[a], opt.v[a]) and back.m[a].shape == getattr(nn, a).shape
    assert nn_training.retore_saved_model(str(tmp_path / "none") + "/", 'latest', 'ldpc-ckpt') == (0, None)
    # the retrain file is looked for where the NMS training stage leaves it
    ds = gl_state.dl_training_data_setting(str(tmp_path / "data"))
    assert ds.path == str(tmp_path / "data" / "snr2.7-2.7dB" / "12th" / "NMS-1" / "ldpc-nonzero-retrain.tfrecord")
    assert ds.batch_size == 100 * 13
