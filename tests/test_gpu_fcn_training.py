"""-m gpu: the sliding-window classifier's training stage (predict_phase.train_sliding_window) on a retrain set of real NMS
failures built on the device -- the records and their pickle against a restatement from osd.block_minima, every training
step against a host replay from the kernel's own gradients, the loss over all windows before and after, the checkpoint
through the test stage (both routes of Testing_OSD), resume, the saved-samples path, and the stage on (96,48) and (121,80)."""
import os
import pickle
import re
from collections import Counter

import numpy as np
import pytest
import torch

from oracle import np_oracle
from tests import dl_training_model as TM
from tests import fcn_training_model as FM
from tests.gpu_util import to_dev

U = TM.U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALIST = os.path.join(ROOT, "short_ldpc_decoding_osd_amd", "data", "CCSDS_ldpc_n128_k64.alist")
ALIST_96 = os.path.join(ROOT, "tests", "golden", "LDPC_N96_K48_P8_set0_dmin10.alist")
ALIST_121 = os.path.join(ROOT, "tests", "golden", "ArrayCode_N121_K80_r0.66.alist")
T, UNIT, BATCHES, STEPS, WIN = 12, 100, 3, 200, 5
INDICATORS, PREFIXES = [True, False, False], ['model_cnn', 'model_rnn1', 'model_rnn2']
ALPHA = np.float32(0.669435)
# a short decoding path: twelve order patterns of weight <= 2 over the six MRB segments, every one with TEPs on all three codes
PATH = [[0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0], [1, 1, 0, 0, 0, 0], [0, 0, 0, 1, 0, 0],
        [0, 2, 0, 0, 0, 0], [0, 0, 0, 0, 1, 0], [0, 1, 1, 0, 0, 0], [0, 0, 0, 0, 0, 1], [0, 0, 2, 0, 0, 0], [1, 0, 1, 0, 0, 0]]
NWIN = len(PATH) - WIN + 1


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
    for key, val in dict(decoding_length=len(PATH), sliding_win_width=WIN, dl_init_seed=0, **extra).items():
        GL.set_map(key, val)


def _retrain_file(alist, data_root, frames, seed):
    """``frames`` failed frames of NMS-12 at 2.7 dB with their trajectories, written as the retrain TFRecord where
    dl_training_data_setting looks for it (the recipe of tests/test_gpu_dl_training.py)."""
    from short_ldpc_decoding_osd_amd import Code, data_generating
    from short_ldpc_decoding_osd_amd.runtime import Decoder
    dec = Decoder(Code(alist))
    rows, labels, frame0, chunk = [], [], 0, 32768
    while sum(len(r) for r in rows) < frames:
        assert frame0 < 64 * chunk, "too few failures"
        y, lab = dec.gen_frames(chunk, seed=seed, snr_db=2.7, frame0=frame0)
        res = dec.nms(y, T, ALPHA, want_soft=False, want_traj=True, want_fail=False)
        idx = torch.nonzero((res["hard"] != lab).any(dim=1)).reshape(-1)[:frames]
        rows.append(torch.cat([y[idx][:, None], res["traj"][:, idx].permute(1, 0, 2)], dim=1).cpu().numpy())
        labels.append(dec.unpack_bits(lab[idx].contiguous()).cpu().numpy())
        frame0 += chunk
    rows, labels = np.concatenate(rows)[:frames], np.concatenate(labels)[:frames]
    d = os.path.join(str(data_root), "snr2.7-2.7dB", f"{T}th", "NMS-1")
    os.makedirs(d, exist_ok=True)
    data_generating.make_tfrecord((rows.reshape(-1, dec.n), np.repeat(labels, T + 1, axis=0)),
                                  out_filename=os.path.join(d, "ldpc-nonzero-retrain.tfrecord"))
    return rows, labels


def _last_row_cnn(nn):
    """Weights under which conv_bitwise returns the last row of the trajectory: tap 2 of channel 0 through the three
    convolutions, then the dense weight of the last position."""
    sh = nn.shapes()
    w = {k: np.zeros(s, np.float32) for k, s in sh.items()}
    w["cnv_one"][2, 0, 0] = w["cnv_two"][2, 0, 0] = w["cnv_three"][2, 0, 0] = 1
    w["dense_kernel"][-2, 0] = 1
    return nn.set_weights(w["cnv_one"], w["cnv_two"], w["cnv_three"], w["dense_kernel"], w["dense_bias"])


def _prepare(GL, root, cnn="random"):
    """What Training_NN leaves for the classifier's stage: a CNN checkpoint (randomly initialised, or the last-row
    network) and the decoding-path pickle, PATH in this order by descending frequency."""
    from short_ldpc_decoding_osd_amd import nn_net, nn_training
    from short_ldpc_decoding_osd_amd.nms_train import LegacyAdam
    info = GL.dl_training_logistic_setting(INDICATORS, PREFIXES)
    nn = nn_net.conv_bitwise()
    nn = nn.initialize(GL.get_map('dl_init_seed')) if cnn == "random" else _last_row_cnn(nn)
    nn_training.checkpoint_saver(nn, LegacyAdam(0.001), info[0], info[1])(0)
    os.makedirs(GL.dl_training_log_dir(), exist_ok=True)
    with open(GL.dl_training_log_dir() + "dist-error-pattern-model_cnn.pkl", "wb") as fh:
        for obj in (1, {}, {}, {}, Counter(), Counter({str(p): float(len(PATH) - i) for i, p in enumerate(PATH)})):
            pickle.dump(obj, fh)
    return info, nn


def _run(GL, root, ds, info, steps, **extra):
    import contextlib
    import io
    from short_ldpc_decoding_osd_amd import predict_phase
    GL.set_map('termination_prediction_step', steps)
    for key, val in extra.items():
        GL.set_map(key, val)
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        res = predict_phase.train_sliding_window([info, GL.dl_training_set_predict_model(True)], INDICATORS, PREFIXES, True,
                                                 selected_ds=ds)
    return res, text.getvalue()


@pytest.fixture(scope="module")
def retrain(tmp_path_factory):
    d = tmp_path_factory.mktemp("fcn_training")
    rows, labels = _retrain_file(ALIST, d / "data", UNIT * BATCHES, seed=41)
    return dict(dir=d, rows=rows, labels=labels)


@pytest.fixture(scope="module")
def trained(retrain):
    """One uninterrupted run of 200 steps with a line and a checkpoint at every step, then the validation pass."""
    from short_ldpc_decoding_osd_amd import globalmap as GL
    saved = dict(GL.map)
    try:
        root = retrain["dir"] / "run"
        _settings(GL, ALIST, root, print_interval=1, record_interval=1)
        ds = GL.dl_training_data_setting(str(retrain["dir"] / "data"))
        info, nn = _prepare(GL, root)
        res, out = _run(GL, root, ds, info, STEPS)
        return dict(res=res, out=out, info=info, fcn_info=GL.dl_training_set_predict_model(True), root=root, ds=ds, nn=nn)
    finally:
        GL.map.clear()
        GL.map.update(saved)


def _records_restated(GL, retrain, nn):
    """query_teps_dis restated per frame on osd.block_minima's arrays, batch by batch."""
    from short_ldpc_decoding_osd_amd import ordered_statistics_decoding as osd_mod
    inst = osd_mod.osd(GL.get_map('code_parameters'))
    teps_list, _ = osd_mod.generate_teps(inst, PATH)
    records, counts = [], [0, 0, 0]
    for i in range(BATCHES):
        rows, labels = retrain["rows"][i * UNIT:(i + 1) * UNIT], retrain["labels"][i * UNIT:(i + 1) * UNIT]
        res = inst.block_minima(rows.reshape(-1, rows.shape[2]), nn(rows), labels, teps_list)
        for bm, truth in zip(res["block_min"], res["truth"]):
            if min(bm) < truth:
                counts[2] += 1
                continue
            located = 1 if min(bm) == truth else -1
            counts[0 if located == 1 else 1] += 1
            records.append(list(bm.astype(np.float64)) + [located])
    return np.asarray(records, dtype=np.float64), tuple(counts)


def test_records_and_summary_equal_the_restatement(retrain, trained, gl_state):
    _settings(gl_state, ALIST, trained["root"])
    res = trained["res"]
    assert res["records_file"] == str(trained["root"]) + f"/log/model_cnn/2.7-2.7dB/order-pattern-len{len(PATH)}-model_cnn.pkl"
    with open(res["records_file"], "rb") as fh:
        summary, records = pickle.load(fh), pickle.load(fh)
        with pytest.raises(EOFError):
            pickle.load(fh)
    want, counts = _records_restated(gl_state, retrain, trained["nn"])
    assert summary == res["summary"] == (3, UNIT * BATCHES) + counts
    assert records.shape == want.shape == (counts[0] + counts[1], len(PATH) + 1) and np.array_equal(records, want)
    # conditions on the fixture (np_oracle's H-form functions on a host model of these frames, which agrees with the device's
    # to a few ulp of the channel values, gave 298 of 300 frames kept, over 260 of them located and about 500 of the 2384
    # windows labelled "stop"): both labels occur, at least half the frames are kept as records
    x, y = FM.windows(records[:, :-1], records[:, -1] != -1, WIN)
    assert 0 < y.sum() < len(y) and len(records) >= UNIT * BATCHES // 2
    assert f"Summary:(order,actual_size,correct,failed,undeteced)={summary}" in trained["out"]
    assert f"Correct:{counts[0]},Failed:{counts[1]},Undetected:{counts[2]}" in trained["out"]
    # one frame of the first batch against the oracle's H-form scan
    _, b = np_oracle.segment_boundaries(64, 6)
    blocks = [np_oracle.error_pattern_gen(p, [range(int(b[i]), int(b[i + 1])) for i in range(6)], 64) for p in PATH]
    order = trained["nn"](retrain["rows"][:UNIT])
    f = 0
    r = np_oracle.hosd_frame(order[f], retrain["rows"][f, 0], retrain["labels"][f], np_oracle.Code(ALIST).H, blocks)
    if r["block_min"].min() >= r["truth"]:
        assert np.array_equal(records[0, :-1].astype(np.float32).view(np.uint32), r["block_min"].view(np.uint32))


def _state(prefix):
    """(weights, m slots, v slots, optimizer step) of a checkpoint of the run."""
    from short_ldpc_decoding_osd_amd import tf_checkpoint
    t = tf_checkpoint.read_checkpoint(prefix)
    S = "/.ATTRIBUTES/VARIABLE_VALUE"
    paths = ("dense1/kernel", "dense2/kernel")
    ws = [t[f"myAwesomeModel/{p}{S}"] for p in paths]
    m = [t[f"myAwesomeModel/{p}/.OPTIMIZER_SLOT/myAwesomeOptimizer/m{S}"] for p in paths]
    v = [t[f"myAwesomeModel/{p}/.OPTIMIZER_SLOT/myAwesomeOptimizer/v{S}"] for p in paths]
    return ws, m, v, int(t[f"myAwesomeOptimizer/iter{S}"])


def _adam_step_bound(g, e, m, v, lr_t, b1=0.9, b2=0.999, eps=1e-7, clip=5e2):
    """Bound on the difference of one clipped Adam update (float32) when its gradient g is known to within e (per entry);
    the derivation is that of tests/test_gpu_dl_training.py: clip_by_norm is 1-Lipschitz in L2 (+ 4 u of its three float32
    operations), dm' <= (1-b1) e + 3 u |m'|, dv' <= (1-b2)(2 |g| e + e^2) + 4 u v', and for u = lr_t m' / (sqrt(v') + eps):
    du <= lr_t [dm' / (s_lo + eps) + |m'| (s - s_lo) / (s_lo + eps)^2] + 4 u |u|, s_lo = sqrt(max(v' - dv', 0))."""
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


def _windows_on_device(dec, trained):
    with open(trained["res"]["records_file"], "rb") as fh:
        pickle.load(fh)
        records = pickle.load(fh)
    x, y = FM.windows(records[:, :-1], records[:, -1] != -1, WIN)
    sw, _ = FM.class_weights(y)
    return to_dev(x, dec), to_dev(y, dec), to_dev(sw, dec), len(y)


def test_training_steps_equal_the_host_replay(trained, gl_state):
    """Step t of the replay starts from the run's own state after step t - 1 (its checkpoint), asks the kernel for the
    gradient at those weights on the step's rows, and applies NumPy Adam: the run's checkpoint after step t holds those
    weights within ``_adam_step_bound`` for a float64 gradient known to within its cast to float32 (u |g|), plus u |w| for
    the final subtraction; the logged loss is the kernel's loss_sum to the three decimals of the line."""
    from short_ldpc_decoding_osd_amd import nn_net, predict_phase
    from short_ldpc_decoding_osd_amd._osd_common import _dec
    _settings(gl_state, ALIST, trained["root"])
    dec = _dec()
    res = trained["res"]
    history = res["history"]
    assert res["step"] == STEPS and len(history) == STEPS
    logged = {int(a): (float(b), float(c)) for a, b, c in
              re.findall(r"^Step:(\d+)  Loss:(-?[\d.]+) Error rate:(-?[\d.]+)$", trained["out"], re.M)}
    assert sorted(logged) == list(range(1, STEPS + 1))
    x_d, y_d, sw_d, N = _windows_on_device(dec, trained)
    per_epoch = -(-N // UNIT)
    assert trained["out"].count("Start of epoch") == -(-STEPS // per_epoch) > 1
    ws = nn_net.Predict_outlier_light(WIN).initialize(0).trainable_variables()
    m, v = [np.zeros_like(w) for w in ws], [np.zeros_like(w) for w in ws]
    worst, right, total = 0.0, 0.0, 0.0
    for t in range(1, STEPS + 1):
        epoch, i = divmod(t - 1, per_epoch)
        perm = predict_phase.shuffle_data(None, y_d, epoch)[0]
        if i == 0:
            right = total = 0.0
        index = perm[i * UNIT:(i + 1) * UNIT].contiguous()
        out = dec.fcn_grad(x_d, y_d, np.concatenate([w.ravel() for w in ws]), WIN, 10.0, weight=sw_d, index=index)
        assert history[t - 1] == out["loss_sum"].item(), t
        assert abs(logged[t][0] - history[t - 1]) <= 0.5e-3 + 1e-12 * abs(history[t - 1]), t
        acc = out["acc"].cpu().numpy()
        right, total = right + acc[0], total + acc[1]
        assert abs(logged[t][1] - (1.0 - right / total)) <= 0.5e-3 + 1e-9, t
        g64 = np.split(out["grad"].cpu().numpy(), [36])
        grads = [g64[0].reshape(6, 6), g64[1].reshape(6, 2)]
        new = TM.adam_replay_step(ws, grads, dict(t=t - 1, m=[a.copy() for a in m], v=[a.copy() for a in v]), np.float32(0.001))
        lr_t = 0.001 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)                # (no decay before step 500)
        ws_run, m_run, v_run, it = _state(trained["fcn_info"][0] + f"ldpc-ckpt-{t}")
        assert it == t
        for k in range(2):
            bound = _adam_step_bound(grads[k], U * np.abs(grads[k]), m[k], v[k], lr_t) + U * np.abs(new[k])
            diff = np.abs(ws_run[k].astype(np.float64) - new[k])
            assert np.all(diff <= bound), (t, k, float(np.max(diff / bound)))
            worst = max(worst, float(np.max(diff / bound)))
        ws, m, v = ws_run, m_run, v_run
    print(f"host replay: worst weight error / bound {worst:.3g}")
    assert np.array_equal(res["fcn"].packed().view(np.uint32), np.concatenate([w.ravel() for w in ws]).view(np.uint32))


def test_training_lowers_the_loss_over_all_windows(trained, gl_state):
    from short_ldpc_decoding_osd_amd import nn_net
    from short_ldpc_decoding_osd_amd._osd_common import _dec
    _settings(gl_state, ALIST, trained["root"])
    dec = _dec()
    x_d, y_d, sw_d, N = _windows_on_device(dec, trained)
    before = dec.fcn_grad(x_d, y_d, nn_net.Predict_outlier_light(WIN).initialize(0).packed(), WIN, 10.0, weight=sw_d, want_grad=False)
    after = dec.fcn_grad(x_d, y_d, trained["res"]["fcn"].packed(), WIN, 10.0, weight=sw_d, want_grad=False)
    assert before["grad"] is None and after["loss_sum"].item() < before["loss_sum"].item()
    print(f"weighted loss over {N} windows: {before['loss_sum'].item():.3f} -> {after['loss_sum'].item():.3f}")
    # the validation pass of the run is this call
    val = trained["res"]["validation"]
    assert (val["S"], val["F1"], val["F2"]) == tuple(after["counts"].cpu().numpy().tolist()) and val["loss"] == after["loss_sum"].item()
    assert val["S"] + val["F1"] + val["F2"] == N and val["dist_labels"] == Counter({0.0: N - int(y_d.sum()), 1.0: int(y_d.sum())})
    log = open(trained["res"]["log_file"]).read()
    assert trained["res"]["log_file"] == str(trained["root"]) + f"/log/fcn/2.7-2.7dB/dB/length-{len(PATH)}prediction-phase-one.txt"
    assert f"S:{val['S']} F1:{val['F1']} F2:{val['F2']}\n" in log and "For Summery of /2.7-2.7dB/dB:" in log
    assert f"Total counts:{N}" in trained["out"] and "Summary of validation:" in trained["out"]


def test_checkpoint_through_the_test_stage(retrain, trained, gl_state, monkeypatch, capsys):
    from short_ldpc_decoding_osd_amd import nn_testing, read_TFdata
    gl_state.global_setting(["prog", "2.7", "2.7", "1", str(UNIT), str(T), ALIST, "NMS-1"], stage="DL")
    for key, val in dict(dl_training_dir=str(trained["root"]) + "/", training_snr=2.7, decoding_length=len(PATH), sliding_win_width=WIN,
                         soft_margin=0.5).items():
        gl_state.set_map(key, val)
    restore_list = [gl_state.logistic_setting_model(INDICATORS, PREFIXES), gl_state.set_predict_model(True)]
    assert restore_list == [trained["info"], trained["fcn_info"]]
    nn, fcn = nn_testing.NN_gen(restore_list, INDICATORS)
    assert np.array_equal(fcn.packed().view(np.uint32), trained["res"]["fcn"].packed().view(np.uint32))
    assert np.array_equal(nn.packed().view(np.uint32), trained["nn"].packed().view(np.uint32))
    assert nn_testing.load_fcn(restore_list[1]).sliding_win_width == WIN
    path = os.path.join(str(retrain["dir"] / "data"), "snr2.7-2.7dB", f"{T}th", "NMS-1", "ldpc-nonzero-retrain.tfrecord")
    results = {}
    for route in ("device", "host"):
        wd = retrain["dir"] / ("osd_" + route)
        wd.mkdir()
        monkeypatch.chdir(wd)
        ds = read_TFdata.data_handler(128, path, UNIT * (T + 1))
        fer, log = nn_testing.Testing_OSD(2.7, ds, restore_list, INDICATORS, PREFIXES, True, route=route)
        lines = open(wd / "log" / "OSD-3-model_cnn.txt").read().splitlines()
        results[route] = (fer, [ln for ln in lines if not ln.startswith("Running time")])
        assert f"Actual decoding path:{len(PATH)}" in capsys.readouterr().out
    assert results["device"] == results["host"] and 0 <= results["device"][0] <= 1


def test_resumed_run_reaches_the_same_bits(retrain, trained, gl_state):
    root = retrain["dir"] / "resumed"
    _settings(gl_state, ALIST, root, print_interval=25, record_interval=25)
    info, _ = _prepare(gl_state, root)
    first, _ = _run(gl_state, root, trained["ds"], info, 50)
    assert first["step"] == 50 and first["history"] == trained["res"]["history"][:50]
    second, out = _run(gl_state, root, trained["ds"], info, STEPS)
    assert "ldpc-ckpt-50" in out and second["step"] == STEPS and second["history"] == trained["res"]["history"][50:]
    fcn_dir = gl_state.dl_training_set_predict_model(True)[0]
    a, b = _state(fcn_dir + f"ldpc-ckpt-{STEPS}"), _state(trained["fcn_info"][0] + f"ldpc-ckpt-{STEPS}")
    assert a[3] == b[3] == STEPS
    for i in range(3):
        for x, y in zip(a[i], b[i]):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    third, _ = _run(gl_state, root, trained["ds"], info, STEPS)          # a finished run trains no further
    assert third["history"] == [] and third["step"] == STEPS
    assert third["validation"]["loss"] == trained["res"]["validation"]["loss"]


def test_saved_samples_train_to_the_same_bits(retrain, trained, gl_state):
    import shutil
    root = retrain["dir"] / "saved"
    _settings(gl_state, ALIST, root, print_interval=50, record_interval=50, regnerate_training_samples=False)
    info, _ = _prepare(gl_state, root)
    with pytest.raises(FileNotFoundError, match="order-pattern-len12-model_cnn.pkl"):
        _run(gl_state, root, None, info, 60)
    dst = str(root) + "/log/model_cnn/2.7-2.7dB/"
    os.makedirs(dst)
    shutil.copy(trained["res"]["records_file"], dst)
    res, out = _run(gl_state, root, None, info, 60)                       # no data set: nothing is generated
    assert res["summary"] == trained["res"]["summary"] and res["history"] == trained["res"]["history"][:60]
    assert "Selectd decoding path" not in out
    a, b = _state(gl_state.dl_training_set_predict_model(True)[0] + "ldpc-ckpt-50"), _state(trained["fcn_info"][0] + "ldpc-ckpt-50")
    assert all(np.array_equal(x, y) for i in range(3) for x, y in zip(a[i], b[i]))
    # a one-class set is refused before any step
    with open(dst + "order-pattern-len12-model_cnn.pkl", "rb") as fh:
        summary, records = pickle.load(fh), pickle.load(fh)
    records[:, -1] = -1
    with open(dst + "order-pattern-len12-model_cnn.pkl", "wb") as fh:
        pickle.dump(summary, fh)
        pickle.dump(records, fh)
    with pytest.raises(ValueError, match="both label classes"):
        _run(gl_state, root, None, info, 70)
    # without a network (DIA false) the samples of the benchmark path are written and no classifier is trained
    from short_ldpc_decoding_osd_amd import predict_phase
    _settings(gl_state, ALIST, retrain["dir"] / "benchmark", convention_path=False)
    os.makedirs(gl_state.dl_training_log_dir(), exist_ok=True)
    shutil.copy(str(trained["root"]) + "/log/NMS-1/2.7-2.7dB/dist-error-pattern-model_cnn.pkl",
                gl_state.dl_training_log_dir() + "dist-error-pattern-benchmark.pkl")
    res = predict_phase.train_sliding_window([[], gl_state.dl_training_set_predict_model(False)], [], [], False, selected_ds=trained["ds"])
    assert res["fcn"] is None and res["step"] == 0 and res["records_file"].endswith("/log/benchmark/2.7-2.7dB/order-pattern-len12-benchmark.pkl")
    assert os.path.exists(res["records_file"]) and res["summary"][1] == UNIT * BATCHES


@pytest.mark.parametrize("alist,family", [(ALIST_96, "hosdx"), (ALIST_121, "hosdw")])
def test_stage_on_other_codes(tmp_path, gl_state, alist, family):
    """The same stage for a few steps where the scan runs through the any-shape and the wide H-form kernels.  The CNN here
    returns the last NMS row, so that some frames are located whatever the code (a random network may order them so badly
    that no window is ever labelled "stop", which the stage refuses)."""
    from short_ldpc_decoding_osd_amd._osd_common import _dec
    frames = 200
    _retrain_file(alist, tmp_path / "data", frames, seed=43)
    _settings(gl_state, alist, tmp_path / "run", print_interval=5, record_interval=5)
    assert _dec().hosd_stage_family() == family
    ds = gl_state.dl_training_data_setting(str(tmp_path / "data"))
    info, _ = _prepare(gl_state, tmp_path / "run", cnn="last row")
    res, out = _run(gl_state, tmp_path / "run", ds, info, 10)
    assert res["step"] == 10 and len(res["history"]) == 10 and all(np.isfinite(res["history"]))
    summary = res["summary"]
    assert summary[1] == frames and sum(summary[2:]) == frames and summary[2] > 0
    val = res["validation"]
    assert val["S"] + val["F1"] + val["F2"] == (summary[2] + summary[3]) * NWIN
    assert "Step:10  Loss:" in out and os.path.exists(gl_state.dl_training_set_predict_model(True)[0] + "ldpc-ckpt-10.index")
