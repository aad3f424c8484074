"""Host side of the DL-OSD stage: network restore from TensorFlow bundles (no TensorFlow), the decoding-path pickle
order, the NumPy classifier, and the RNN variants that are not mirrored."""
import pickle
from collections import Counter

import numpy as np
import pytest

from short_ldpc_decoding_osd_amd import globalmap as GL
from short_ldpc_decoding_osd_amd import nn_net, nn_testing, tf_checkpoint
from tests import dlosd_model as DM

SUFFIX = "/.ATTRIBUTES/VARIABLE_VALUE"


@pytest.fixture
def gl_state():
    saved = dict(GL.map)
    yield GL
    GL.map.clear()
    GL.map.update(saved)


def _cnn_bundle(prefix, L, seed=1, **override):
    ws = DM.random_cnn_weights(np.random.default_rng(seed), L)
    names = ("cnv_one/kernel", "cnv_two/kernel", "cnv_three/kernel", "dense/kernel", "dense/bias")
    t = {f"myAwesomeModel/{n}{SUFFIX}": w for n, w in zip(names, ws)}
    t.update({f"myAwesomeModel/{n}{SUFFIX}": v for n, v in override.items()})
    # what the training stage saves besides the model (nn_training.py:371): optimizer state and slots
    t[f"myAwesomeOptimizer/iter{SUFFIX}"] = np.array(120, np.int64)
    t[f"myAwesomeOptimizer/learning_rate{SUFFIX}"] = np.array(1e-3, np.float32)
    t[f"myAwesomeModel/dense/kernel/.OPTIMIZER_SLOT/myAwesomeOptimizer/m{SUFFIX}"] = np.ones((2 * (L - 6), 1), np.float32)
    t[f"myAwesomeModel/activation/alpha{SUFFIX}"] = np.full((L, 1), 0.25, np.float32)   # the unused PReLU
    tf_checkpoint.write_checkpoint(prefix, t)
    return ws


def test_restore_conv_bitwise(tmp_path, gl_state):
    L = 13
    gl_state.set_map('num_iterations', L - 1)
    ws = _cnn_bundle(str(tmp_path / "cnn" / "ldpc-ckpt-40"), L)
    prefix = nn_testing.retore_saved_model(str(tmp_path / "cnn") + "/", "latest", "ldpc-ckpt")
    assert prefix.endswith("ldpc-ckpt-40")
    nn = nn_testing.restore_conv_bitwise(nn_net.conv_bitwise(n_dims=128), prefix)
    assert np.array_equal(nn.packed(), DM.pack_cnn(ws))
    assert nn.packed().size == 24 + 96 + 24 + 2 * (L - 6) + 1
    # a designated step instead of the latest one
    assert nn_testing.retore_saved_model(str(tmp_path / "cnn") + "/", "40", "ldpc-ckpt") == str(tmp_path / "cnn" / "ldpc-ckpt-40")


def test_restore_predict_outlier(tmp_path, gl_state):
    gl_state.set_map('sliding_win_width', 5)
    w1, w2 = DM.random_fcn_weights(np.random.default_rng(2), 5)
    tf_checkpoint.write_checkpoint(str(tmp_path / "fcn" / "ldpc-ckpt-9"), {
        f"myAwesomeModel/dense1/kernel{SUFFIX}": w1, f"myAwesomeModel/dense2/kernel{SUFFIX}": w2,
        f"myAwesomeOptimizer/iter{SUFFIX}": np.array(9, np.int64),
        f"myAwesomeModel/dense2/kernel/.OPTIMIZER_SLOT/myAwesomeOptimizer/v{SUFFIX}": np.zeros((6, 2), np.float32)})
    fcn = nn_testing.load_fcn([str(tmp_path / "fcn") + "/", "ldpc-ckpt", "latest"])
    assert np.array_equal(fcn.dense1, w1) and np.array_equal(fcn.dense2, w2)
    assert np.array_equal(fcn.packed(), np.concatenate([w1.ravel(), w2.ravel()]))


def test_restore_refuses_wrong_shapes(tmp_path, gl_state):
    L = 11
    gl_state.set_map('num_iterations', L - 1)
    _cnn_bundle(str(tmp_path / "a" / "ldpc-ckpt-1"), L, **{"dense/kernel": np.zeros((2 * (L - 5), 1), np.float32)})
    with pytest.raises(ValueError):
        nn_testing.restore_conv_bitwise(nn_net.conv_bitwise(n_dims=128), str(tmp_path / "a" / "ldpc-ckpt-1"))
    _cnn_bundle(str(tmp_path / "b" / "ldpc-ckpt-1"), L, **{"cnv_two/kernel": np.zeros((3, 4, 8), np.float32)})
    with pytest.raises(ValueError):
        nn_testing.restore_conv_bitwise(nn_net.conv_bitwise(n_dims=128), str(tmp_path / "b" / "ldpc-ckpt-1"))
    gl_state.set_map('sliding_win_width', 3)
    tf_checkpoint.write_checkpoint(str(tmp_path / "c" / "ldpc-ckpt-1"), {
        f"myAwesomeModel/dense1/kernel{SUFFIX}": np.zeros((6, 6), np.float32),
        f"myAwesomeModel/dense2/kernel{SUFFIX}": np.zeros((6, 2), np.float32)})
    with pytest.raises(ValueError):
        nn_testing.load_fcn([str(tmp_path / "c") + "/", "ldpc-ckpt", "latest"])
    tf_checkpoint.write_checkpoint(str(tmp_path / "d" / "ldpc-ckpt-1"), {f"myAwesomeModel/dense1/kernel{SUFFIX}": np.zeros((4, 4), np.float32)})
    with pytest.raises(KeyError):
        nn_testing.load_fcn([str(tmp_path / "d") + "/", "ldpc-ckpt", "latest"])
    with pytest.raises(ValueError):                # no restore step: no untrained networks to fall back on
        nn_testing.load_fcn([str(tmp_path / "c") + "/", "ldpc-ckpt", ""])


def test_decoding_path_pickle_order(tmp_path, gl_state):
    gl_state.set_map('selected_decoder_type', 'NMS-1')
    gl_state.set_map('dl_training_dir', str(tmp_path) + "/")
    gl_state.set_map('threshold_sum', 3)
    gl_state.set_map('decoding_length', 5)
    d = tmp_path / "log" / "NMS-1" / "2.7-2.7dB"
    d.mkdir(parents=True)
    cnt = Counter()
    # insertion order matters for ties: the reference's sorted(..., reverse=True) keeps it
    for key, v in (("[0, 0, 0, 0, 0, 0]", 9), ("[0, 1, 0, 0, 0, 0]", 4), ("[1, 0, 0, 0, 0, 0]", 4), ("[2, 2, 0, 0, 0, 0]", 8),
                   ("[0, 0, 1, 0, 0, 0]", 4), ("[1, 1, 0, 0, 0, 0]", 2), ("[0, 0, 0, 1, 0, 0]", 2), ("[0, 0, 0, 0, 1, 0]", 1)):
        cnt[key] = v
    with open(d / "dist-error-pattern-model_cnn.pkl", "wb") as fh:
        for obj in ({}, [1, 2], "x", 3.0, Counter({"a": 1}), cnt):
            pickle.dump(obj, fh)
    path, nn_type = nn_testing.query_decoding_path([True, False, False], ['model_cnn', 'model_rnn1', 'model_rnn2'], True)
    assert nn_type == 'model_cnn'
    assert path == [[0, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0], [1, 1, 0, 0, 0, 0]]
    conv, t = nn_testing.query_convention_path([True], ['model_cnn'], False)
    assert t == 'benchmark' and len(conv) == 20 and conv[:5] == [[0, 0, 0], [0, 0, 1], [0, 1, 0], [1, 0, 0], [0, 0, 2]]


def test_classifier_matches_float64_softmax():
    rng = np.random.default_rng(4)
    for win in (3, 5, 15):
        fcn = nn_net.Predict_outlier_light(win)
        w1, w2 = DM.random_fcn_weights(rng, win)
        fcn.set_weights(w1, w2)
        x = np.concatenate([np.sort(rng.uniform(0, 40, (500, win)), axis=1), rng.integers(0, 25, (500, 1))], axis=1).astype(np.float32)
        p = fcn(x)
        assert p.dtype == np.float32 and p.shape == (500, 2)
        z = x.astype(np.float64) @ w1.astype(np.float64) @ w2.astype(np.float64)
        e = np.exp(z - z.max(axis=1, keepdims=True))
        want = e / e.sum(axis=1, keepdims=True)
        assert np.allclose(p, want, rtol=1e-4, atol=1e-5)
        assert np.array_equal(p[:, 1], DM.classifier_p1(x, w1, w2))      # the device's operation order


def test_rnn_variants_not_mirrored():
    with pytest.raises(NotImplementedError):
        nn_net.rnn_one()
    with pytest.raises(NotImplementedError):
        nn_net.rnn_two()
    with pytest.raises(NotImplementedError):
        nn_testing.NN_gen([["x/", "ldpc-ckpt", "latest"], ["y/", "ldpc-ckpt", "latest"]], [False, True, False])


def test_globalmap_dl_settings(tmp_path, gl_state, alist_path):
    gl_state.global_setting(["prog", "2.0", "3.0", "6", "100", "12", alist_path, "NMS-1"], stage="DL")
    for key, val in dict(threshold_sum=3, segment_num=6, soft_margin=0.9, decoding_length=30, sliding_win_width=5,
                         convention_path=False, termination_threshold=500, training_snr=2.7).items():
        assert gl_state.get_map(key) == val, key
    gl_state.set_map('dl_training_dir', str(tmp_path) + "/")
    info = gl_state.logistic_setting_model([True, False, False], ['model_cnn', 'model_rnn1', 'model_rnn2'])
    assert info == [str(tmp_path) + "/ckpts/model_cnn/2.7-2.7dB/12th/", "ldpc-ckpt", "latest"]
    info = gl_state.set_predict_model(True)
    assert info == [str(tmp_path) + "/ckpts/fcn/2.7-2.7dB/12th/len-30-order-3/", "ldpc-ckpt", "latest"]
