#!/usr/bin/env python3
"""Recipe steps 1-2 end to end on the GPU: training file -> NMS training -> values.txt / checkpoint / retrain file.

    python scripts/run_training.py [--snr-lo 2.7 --snr-hi 2.7 --batch 100 --batches 1000 --T 12 --type NMS-1 --steps 1200]
                                   [--alist FILE] [--out DIR] [--seed 0]

Defaults are the reference's (ldpc_128_training.py:14, globalmap.py:28-56).  Under --out: data/snr<lo>-<hi>dB/ (the
training file and <T>th/<type>/ldpc-nonzero-retrain.tfrecord) and ckpts/<type>/<T>th/ (checkpoints, par/values.txt).
The trained weight reaches the test stage through run_stages.py --values <out>/ckpts/<type>/<T>th/par/values.txt."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from short_ldpc_decoding_osd_amd import data_generating, globalmap as GL, training_stage  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--snr-lo", type=float, default=2.7)
    ap.add_argument("--snr-hi", type=float, default=2.7)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--batches", type=int, default=1000)
    ap.add_argument("--T", type=int, default=12)
    ap.add_argument("--type", default="NMS-1")
    ap.add_argument("--steps", type=int, default=1200, help="termination_step")
    ap.add_argument("--alist", default=os.path.join(ROOT, "short_ldpc_decoding_osd_amd", "data", "CCSDS_ldpc_n128_k64.alist"))
    ap.add_argument("--out", default="training_run")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    t0 = time.time()
    GL.training_setting_global(["run_training", a.snr_lo, a.snr_hi, a.batch, a.batches, a.T, a.alist, a.type])
    GL.set_map('termination_step', a.steps)
    code = GL.get_map('code_parameters')
    data_root = os.path.join(a.out, "data")
    data_dir = os.path.join(data_root, f"snr{round(a.snr_lo, 2)}-{round(a.snr_hi, 2)}dB")
    os.makedirs(data_dir, exist_ok=True)
    train_file = os.path.join(data_dir, "ldpc-train-nonzero.tfrecord")
    if not os.path.exists(train_file):      # recipe step 1 (Training_data_gen_128)
        y, labels = data_generating.training_data_generating(code, (a.snr_lo, a.snr_hi), a.batch * a.batches,
                                                             np.random.default_rng(a.seed))
        data_generating.make_tfrecord((y.astype(np.float32), labels), train_file)
    restore_info = GL.training_logistic_setting(a.out)
    Model = training_stage.training_stage(restore_info, data_root)
    retrain = training_stage.post_process_input(Model, data_root)
    print(f"values: {os.path.join(restore_info[2], 'values.txt')}\nretrain file: {retrain}")
    print('Running time:%s seconds!' % (time.time() - t0))


if __name__ == "__main__":
    main()
