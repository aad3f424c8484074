"""-m gpu: the DL-OSD leg of scripts/snr_sweep.py (`--osd dl --training DIR`) as a command: it finds the networks and the decoding
path in a training directory laid out as scripts/run_dl_osd.py expects it (checkpoints under ckpts/, the dist-error-pattern
pickle under log/), sweeps a point on pipeline.DlOsdPipeline and prints the rates of the 15 counters; `--cpu-check` sends the
last batch's failures through the host route osd.sliding_osd and both sides give the same (S, F, windows, complexity).  The
frames come from the library's generator, so a run decodes the same frames every time."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from tests import dlosd_model as DM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, WIN = 6, 5
PATH = [[0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0], [2, 0, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0],
        [0, 2, 0, 0, 0, 0], [1, 0, 1, 0, 0, 0], [0, 1, 1, 0, 0, 0], [0, 0, 0, 1, 0, 0]]


@pytest.fixture(scope="module")
def training_dir(tmp_path_factory):
    """ckpts/model_cnn/2.7-2.7dB/6th/, ckpts/fcn/2.7-2.7dB/6th/len-30-order-3/ and log/NMS-1/2.7-2.7dB/ with synthetic networks
    under the Keras names and a ten-block path by descending frequency."""
    from short_ldpc_decoding_osd_amd import tf_checkpoint
    d = tmp_path_factory.mktemp("dl_training")
    names = ("cnv_one/kernel", "cnv_two/kernel", "cnv_three/kernel", "dense/kernel", "dense/bias")
    cnn = DM.random_cnn_weights(np.random.default_rng(3), T + 1, scale=0.3)
    tf_checkpoint.write_checkpoint(str(d / "ckpts" / "model_cnn" / "2.7-2.7dB" / f"{T}th" / "ldpc-ckpt-1"),
                                   {f"myAwesomeModel/{k}/.ATTRIBUTES/VARIABLE_VALUE": v for k, v in zip(names, cnn)})
    w1, w2 = DM.stopping_fcn_weights(WIN)
    tf_checkpoint.write_checkpoint(str(d / "ckpts" / "fcn" / "2.7-2.7dB" / f"{T}th" / "len-30-order-3" / "ldpc-ckpt-1"), {
        "myAwesomeModel/dense1/kernel/.ATTRIBUTES/VARIABLE_VALUE": w1,
        "myAwesomeModel/dense2/kernel/.ATTRIBUTES/VARIABLE_VALUE": w2})
    os.makedirs(d / "log" / "NMS-1" / "2.7-2.7dB")
    for nn_type in ("model_cnn", "benchmark"):               # (DIA = False reads the benchmark's statistics)
        with open(d / "log" / "NMS-1" / "2.7-2.7dB" / f"dist-error-pattern-{nn_type}.pkl", "wb") as fh:
            for obj in (0, 0, 0, 0, 0, {str(p): len(PATH) - i for i, p in enumerate(PATH)}):
                pickle.dump(obj, fh)
    return d


def sweep(training_dir, cwd, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "snr_sweep.py"), "--osd", "dl", "--training", str(training_dir), "--snr", "2.5",
           "2.5", "1", "--frames", "2000", "--iters", str(T), "--gen", "hip", "--streams", "2"] + list(extra)
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return lines[0]


def test_sweep_point_with_cpu_check(training_dir, tmp_path):
    out = sweep(training_dir, tmp_path, "--batch", "1000", "--cpu-check", "--cpu-frames", "96")
    print(out)
    assert out["frames"] == 2000 and out["family"] == "hosd" and out["code"] == [128, 64] and out["gen"] == "hip" and out["dia"]
    assert out["path_blocks"] == 10 and out["win"] == WIN and out["macro_batches"] == 2
    assert 0 < out["stage_frames"] == round(out["synd_fail_rate"] * 2000) < 2000 and out["left_out"] == 0
    assert 1.0 <= out["mean_windows"] <= 10 - WIN + 1 and 0 < out["mean_complexity"] <= out["path_teps"] and out["mean_teps"] > 0
    assert 0.0 <= out["fer_end_to_end"] <= 1.0 and out["ber_nms"] > 0 and out["ber_end_to_end"] >= 0
    chk = out["dl_vs_host"]
    assert 0 < chk["frames"] <= 96 and chk["agree"] is True and chk["host"] == chk["device"], chk
    assert chk["host"][0] + chk["host"][1] == chk["frames"]


def test_sweep_point_without_cnn_stops_on_errors(training_dir, tmp_path):
    """DIA = False (the checkpoint of the classifier alone), a capacity below the batch and the stop rule: the point ends on the
    first macro-batch that brings undetected + merged wrong to the threshold."""
    # (the classifier of DIA = False lives under ckpts/fcn as well: run_dl_osd.py passes set_predict_model(True) either way)
    out = sweep(training_dir, tmp_path, "--batch", "500", "--no-dia", "--capacity", "400", "--stop-errors", "1")
    print(out)
    assert not out["dia"] and out["capacity"] == 400 and out["stop_errors"] == 1
    assert out["macro_batches"] < 4 and out["frames"] == 500 * out["macro_batches"]
    assert out["fer_end_to_end"] * out["frames"] >= 1
