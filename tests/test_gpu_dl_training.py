"""-m gpu: the DL-OSD training stage (nn_training.Training_NN) on a retrain set of real NMS failures built on the device --
40 training steps replayed on the host, the checkpoint through the test stage's restore, resume, the six pickled objects
against the per-frame restatement of tests/dl_training_model.py, the statistics alone on (96,48), and the benchmark path."""
import os
import pickle
import re

import numpy as np
import pytest
import torch

from tests import dl_training_model as TM
from tests import dlosd_model as DM

K, U = TM.K, TM.U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALIST = os.path.join(ROOT, "short_ldpc_decoding_osd_amd", "data", "CCSDS_ldpc_n128_k64.alist")
ALIST_96 = os.path.join(ROOT, "tests", "golden", "LDPC_N96_K48_P8_set0_dmin10.alist")
T, UNIT, BATCHES, STEPS = 12, 100, 20, 40
INDICATORS, PREFIXES = [True, False, False], ['model_cnn', 'model_rnn1', 'model_rnn2']
ALPHA = np.float32(0.669435)


@pytest.fixture
def gl_state():
    from short_ldpc_decoding_osd_amd import globalmap as GL
    saved = dict(GL.map)
    yield GL
    GL.map.clear()
    GL.map.update(saved)


def _settings(GL, alist, root, **extra):
    GL.dl_training_setting(["prog", "2.7", "2.7", str(UNIT), str(T), alist, "NMS-1"])
    GL.set_map('dl_training_dir', str(root) + "/")
    for key, val in extra.items():
        GL.set_map(key, val)


def _retrain_file(alist, data_root, frames, seed):
    """``frames`` failed frames of NMS-12 at 2.7 dB, their trajectories from Decoder.nms(..., want_traj) 32768 channel
    frames at a time, written as the retrain TFRecord where dl_training_data_setting looks for it."""
    from short_ldpc_decoding_osd_amd import Code, data_generating
    from short_ldpc_decoding_osd_amd.runtime import Decoder
    dec = Decoder(Code(alist))
    rows, labels, frame0, chunk = [], [], 0, 32768
    while sum(len(r) for r in rows) < frames:
        assert frame0 < 64 * chunk, "too few failures"
        y, lab = dec.gen_frames(chunk, seed=seed, snr_db=2.7, frame0=frame0)
        res = dec.nms(y, T, ALPHA, want_soft=False, want_traj=True, want_fail=False)
        idx = torch.nonzero((res["hard"] != lab).any(dim=1)).reshape(-1)      # failed = decision differs from the label
        rows.append(torch.cat([y[idx][:, None], res["traj"][:, idx].permute(1, 0, 2)], dim=1).cpu().numpy())
        labels.append(dec.unpack_bits(lab[idx].contiguous()).cpu().numpy())
        frame0 += chunk
    rows, labels = np.concatenate(rows)[:frames], np.concatenate(labels)[:frames]
    d = os.path.join(str(data_root), "snr2.7-2.7dB", f"{T}th", "NMS-1")
    os.makedirs(d, exist_ok=True)
    data_generating.make_tfrecord((rows.reshape(-1, dec.n), np.repeat(labels, T + 1, axis=0)),
                                  out_filename=os.path.join(d, "ldpc-nonzero-retrain.tfrecord"))
    return rows, labels


@pytest.fixture(scope="module")
def retrain(tmp_path_factory):
    d = tmp_path_factory.mktemp("dl_training")
    rows, labels = _retrain_file(ALIST, d / "data", UNIT * BATCHES, seed=31)
    return dict(dir=d, rows=rows, labels=labels)


@pytest.fixture(scope="module")
def trained(retrain):
    """One uninterrupted run of 40 steps with a line and a checkpoint at every step, then the verification pass."""
    import contextlib
    import io
    from short_ldpc_decoding_osd_amd import globalmap as GL
    from short_ldpc_decoding_osd_amd import nn_training
    saved = dict(GL.map)
    try:
        root = retrain["dir"] / "run"
        _settings(GL, ALIST, root, print_interval=1, record_interval=1, termination_step=STEPS)
        ds = GL.dl_training_data_setting(str(retrain["dir"] / "data"))
        info = GL.dl_training_logistic_setting(INDICATORS, PREFIXES)
        text = io.StringIO()
        with contextlib.redirect_stdout(text):
            res = nn_training.Training_NN(ds, info, INDICATORS, PREFIXES, True)
        return dict(res=res, info=info, root=root, out=text.getvalue(), ds=ds)
    finally:
        GL.map.clear()
        GL.map.update(saved)


def _batch(retrain, i):
    sl = slice(i * UNIT, (i + 1) * UNIT)
    return retrain["rows"][sl], retrain["labels"][sl]


def _state(prefix):
    """(weights, m slots, v slots, optimizer step) of a checkpoint of the run."""
    from short_ldpc_decoding_osd_amd import nn_training, tf_checkpoint
    t = tf_checkpoint.read_checkpoint(prefix)
    S = nn_training.VARIABLE_SUFFIX
    paths = list(nn_training.VARIABLE_PATHS.values())
    ws = [t[f"myAwesomeModel/{p}{S}"] for p in paths]
    m = [t[f"myAwesomeModel/{p}/.OPTIMIZER_SLOT/myAwesomeOptimizer/m{S}"] for p in paths]
    v = [t[f"myAwesomeModel/{p}/.OPTIMIZER_SLOT/myAwesomeOptimizer/v{S}"] for p in paths]
    return ws, m, v, int(t[f"myAwesomeOptimizer/iter{S}"])


def _adam_step_bound(g, e, m, v, lr_t, b1=0.9, b2=0.999, eps=1e-7, clip=5e2):
    """Bound on the difference of one clipped Adam update (float32) when its gradient g is known to within e (per entry).
    clip_by_norm is the projection onto the L2 ball, 1-Lipschitz in L2: a clipped entry moves by at most ||e||_2 (+ 4 u of
    the three float32 operations of the clip).  Then dm' <= (1-b1) e + 3 u |m'|, dv' <= (1-b2)(2 |g| e + e^2) + 4 u v', and
    for u = lr_t m' / (sqrt(v') + eps): du <= lr_t [dm' / (s_lo + eps) + |m'| (s - s_lo) / (s_lo + eps)^2] + 4 u |u|,
    s = sqrt(v'), s_lo = sqrt(max(v' - dv', 0)) (the square root is concave: its largest change is downwards)."""
    g, e = np.asarray(g, np.float64), np.asarray(e, np.float64)
    norm, enorm = np.sqrt(np.sum(g * g)), np.sqrt(np.sum(e * e))
    if norm + enorm > clip:
        gc = g * min(1.0, clip / norm)
        e = np.full_like(g, enorm) + 4 * U * np.abs(gc)
        g = gc
    m1 = b1 * np.asarray(m, np.float64) + (1 - b1) * g
    v1 = b2 * np.asarray(v, np.float64) + (1 - b2) * g * g
    dm = (1 - b1) * e + 3 * U * np.abs(m1)
    dv = (1 - b2) * (2 * np.abs(g) * e + e * e) + 4 * U * v1
    s, s_lo = np.sqrt(v1), np.sqrt(np.maximum(v1 - dv, 0))
    upd = lr_t * m1 / (s + eps)
    return lr_t * (dm / (s_lo + eps) + np.abs(m1) * (s - s_lo) / (s_lo + eps) ** 2) + 4 * U * np.abs(upd)


def test_training_steps_equal_the_host_replay(retrain, trained, gl_state):
    """Every logged loss and every weight of the run against a host replay of the same steps: the float64 model of
    tests/dl_training_model.py feeds NumPy Adam.

    How the rounding bound is carried over the steps: it is not carried through the weights.  The run leaves a checkpoint
    at every step, and step t of the replay starts from the run's own state after step t - 1 (weights, Adam slots, step
    count).  So the loss logged at step t is the kernel's loss at weights the model is given exactly, and the bound of
    test_gpu_dia_train's model test holds for it as it stands (2 K u sum |term|); the %.3f line adds half a unit of its
    last digit.  The weights after step t are those of NumPy Adam fed the model's gradient, within the first-order bound
    of ``_adam_step_bound`` for a gradient known to within 2 K u mass (+ u |g| for its cast to float32), plus u |w| for
    the final subtraction.  A free-running replay would need a Lipschitz bound of the gradient in the weights, which this
    network (a product of four layers) does not give cheaply; re-anchoring checks the same 40 steps with a bound that is
    tight at every one of them."""
    from short_ldpc_decoding_osd_amd import nn_net
    res, info = trained["res"], trained["info"]
    history = res["history"]
    assert res["step"] == STEPS and len(history) == STEPS
    logged = {int(a): float(b) for a, b in re.findall(r"^Step:(\d+)  Loss:(-?[\d.]+)$", trained["out"], re.M)}
    assert sorted(logged) == list(range(1, STEPS + 1))
    assert trained["out"].count("Start of epoch") == 2 and "Start of epoch 1:" in trained["out"]
    L = T + 1
    ws = [np.asarray(w) for w in nn_net.conv_bitwise(list_length=L, n_dims=128).initialize(0).trainable_variables()]
    m = [np.zeros_like(w) for w in ws]
    v = [np.zeros_like(w) for w in ws]
    lr0 = np.float32(0.001)
    worst_loss = worst_w = 0.0
    for t in range(1, STEPS + 1):
        rows, labels = _batch(retrain, (t - 1) % BATCHES)
        # the kernel's own float32 out at these weights (the forward is tested bit for bit elsewhere)
        out = DM.cnn_forward(rows, ws)
        model = TM.cnn_loss_grad(rows, labels, ws, out=out)
        lbound = 2 * K * U * model["abs_loss"]
        assert abs(history[t - 1] - model["loss"]) <= lbound, (t, history[t - 1], model["loss"])
        assert abs(logged[t] - model["loss"]) <= lbound + 0.5e-3 + 1e-12 * abs(model["loss"]), t
        worst_loss = max(worst_loss, abs(history[t - 1] - model["loss"]) / lbound)
        masses = TM.grad_masses(L, ws, model["abs_m"], model["abs_g"])
        state = dict(t=t - 1, m=[a.copy() for a in m], v=[a.copy() for a in v])
        new = TM.adam_replay_step(ws, model["grads"], state, lr0)          # (no decay before step 500)
        lr_t = float(lr0) * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        ws_run, m_run, v_run, it = _state(info[0] + f"ldpc-ckpt-{t}")
        assert it == t
        for i in range(5):
            g = np.asarray(model["grads"][i], np.float64)
            e = 2 * K * U * masses[i] + U * np.abs(g)
            bound = _adam_step_bound(g, e, m[i], v[i], lr_t) + U * np.abs(new[i])
            diff = np.abs(ws_run[i].astype(np.float64) - new[i])
            assert np.all(diff <= bound), (t, i, float(np.max(diff / bound)))
            worst_w = max(worst_w, float(np.max(diff / bound)))
        ws, m, v = ws_run, m_run, v_run
    print(f"host replay: worst loss error / bound {worst_loss:.3g}, worst weight error / bound {worst_w:.3g}")
    # training helps: below the first step's loss at the end, and on the first batch when it comes round again
    assert history[STEPS - 1] < history[0] and history[BATCHES] < history[0]


def test_checkpoint_restores_through_the_test_stage(trained, gl_state):
    from short_ldpc_decoding_osd_amd import nn_net, nn_testing
    _settings(gl_state, ALIST, trained["root"], training_snr=2.7)
    info = gl_state.logistic_setting_model(INDICATORS, PREFIXES)
    assert info == trained["info"]
    prefix = nn_testing.retore_saved_model(info[0], info[2], info[1])
    assert prefix.endswith(f"ldpc-ckpt-{STEPS}")
    nn = nn_testing.restore_conv_bitwise(nn_net.conv_bitwise(), prefix)
    assert np.array_equal(nn.packed().view(np.uint32), trained["res"]["nn"].packed().view(np.uint32))


def test_resumed_run_reaches_the_same_bits(retrain, trained, gl_state, capsys):
    from short_ldpc_decoding_osd_amd import nn_training
    root = retrain["dir"] / "resumed"
    _settings(gl_state, ALIST, root, print_interval=10, record_interval=10, termination_step=STEPS // 2)
    info = gl_state.dl_training_logistic_setting(INDICATORS, PREFIXES)
    first = nn_training.Training_NN(trained["ds"], info, INDICATORS, PREFIXES, True)
    assert first["step"] == STEPS // 2 and first["history"] == trained["res"]["history"][:STEPS // 2]
    gl_state.set_map('termination_step', STEPS)
    second = nn_training.Training_NN(trained["ds"], info, INDICATORS, PREFIXES, True)
    out = capsys.readouterr().out
    assert f"ldpc-ckpt-{STEPS // 2}" in out and "Start of epoch 1:" in out
    assert second["step"] == STEPS and second["history"] == trained["res"]["history"][STEPS // 2:]
    a, b = _state(info[0] + f"ldpc-ckpt-{STEPS}"), _state(trained["info"][0] + f"ldpc-ckpt-{STEPS}")
    assert a[3] == b[3] == STEPS
    for i in range(3):
        for x, y in zip(a[i], b[i]):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    # a finished run trains no further
    third = nn_training.Training_NN(trained["ds"], info, INDICATORS, PREFIXES, True)
    assert third["history"] == [] and third["step"] == STEPS


def _check_pickle(GL, code, log_file, batches):
    """The six objects against the restatement applied to the same refined values; the summary ratios to 1e-12."""
    seg, boundary = GL.secure_segment_threshold()
    want = TM.stage_statistics(code, batches, seg, boundary)
    with open(log_file, "rb") as fh:
        got = [pickle.load(fh) for _ in range(6)]
    size, d0, dT, dr, merged, ratio = want["objects"]
    assert got[0] == size and got[1] == d0 and got[2] == dT and got[3] == dr and got[4] == merged
    assert list(got[1]) == sorted(got[1]) and set(got[5]) == set(ratio)
    for key, value in ratio.items():
        assert abs(got[5][key] - value) <= 1e-12 * value, key
    return want


def test_pickled_statistics_equal_the_restatement(retrain, trained, gl_state):
    from short_ldpc_decoding_osd_amd import nn_testing
    _settings(gl_state, ALIST, trained["root"], training_snr=2.7)
    code = gl_state.get_map('code_parameters')
    nn = trained["res"]["nn"]
    assert trained["res"]["log_file"] == str(trained["root"]) + "/log/NMS-1/2.7-2.7dB/dist-error-pattern-model_cnn.pkl"
    batches = []
    for i in range(BATCHES):
        rows, labels = _batch(retrain, i)
        batches.append((rows[:, 0], rows[:, -1], nn(rows), labels))        # the device's refined values
    want = _check_pickle(gl_state, code, trained["res"]["log_file"], batches)
    assert max(want["swaps"]) > 0 and len(want["pattern"]) > 5
    out = trained["out"]
    assert f"Total counts:{UNIT * BATCHES}" in out and f"average swaps:{np.mean(want['swaps']):.4f} " in out
    assert "Summary before GE for model_cnn:" in out and "Summary of decoding_pth:" in out
    path, nn_type = nn_testing.query_decoding_path(INDICATORS, PREFIXES, True)
    assert nn_type == "model_cnn" and len(path) > 0 and all(len(p) == 6 and sum(p) <= 3 for p in path)


def test_benchmark_path_writes_its_pickle(retrain, trained, gl_state, capsys):
    from short_ldpc_decoding_osd_amd import nn_training
    root = retrain["dir"] / "benchmark"
    _settings(gl_state, ALIST, root)
    res = nn_training.Training_NN(trained["ds"], [], [], [], False)
    assert res["log_file"] == str(root) + "/log/NMS-1/2.7-2.7dB/dist-error-pattern-benchmark.pkl" and res["nn"] is None
    batches = []
    for i in range(BATCHES):
        rows, labels = _batch(retrain, i)
        batches.append((rows[:, 0], rows[:, -1], rows[:, -1], labels))
    _check_pickle(gl_state, gl_state.get_map('code_parameters'), res["log_file"], batches)
    assert "Summary before GE for benchmark:" in capsys.readouterr().out and not os.path.exists(str(root) + "/ckpts")


def test_statistics_on_96_48(tmp_path, gl_state):
    """The verification pass alone (nn_train off: fresh weights, no step) on another code: hosd_stage picks the any-shape
    front end."""
    from short_ldpc_decoding_osd_amd import nn_training
    rows, labels = _retrain_file(ALIST_96, tmp_path / "data", 300, seed=32)
    _settings(gl_state, ALIST_96, tmp_path / "run", nn_train=False)
    ds = gl_state.dl_training_data_setting(str(tmp_path / "data"))
    info = gl_state.dl_training_logistic_setting(INDICATORS, PREFIXES)
    res = nn_training.Training_NN(ds, info, INDICATORS, PREFIXES, True)
    assert res["step"] == 0 and res["history"] == [] and not os.path.exists(info[0] + "checkpoint")
    nn = res["nn"]
    batches = [(rows[a:a + UNIT, 0], rows[a:a + UNIT, -1], nn(rows[a:a + UNIT]), labels[a:a + UNIT]) for a in range(0, 300, UNIT)]
    want = _check_pickle(gl_state, gl_state.get_map('code_parameters'), res["log_file"], batches)
    assert want["objects"][0] == 300
