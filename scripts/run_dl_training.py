#!/usr/bin/env python3
"""The DL-OSD training stage for the bit-wise CNN, as Main_DL.py drives it (its `reliability_enhance` part), over the
retrain file the NMS training stage leaves (scripts/run_training.py):

    python scripts/run_dl_training.py --data DIR --out DIR [--alist FILE] [--snr 2.7] [--batch 100] [--iters 12]
                                      [--type NMS-1] [--steps N] [--seed 0] [--no-dia]

--data: the root holding snr<lo>-<hi>dB/<T>th/<type>/ldpc-nonzero-retrain.tfrecord; --out: where ckpts/ and log/ go --
pass the same directory to scripts/run_dl_osd.py --training; --steps: termination_step (default 2000, the reference's);
--no-dia: the 'benchmark' statistics of the last NMS iteration, no network.  The sliding-window classifier
(predict_phase.train_sliding_window) is not trained here: its `fcn` checkpoint still comes from elsewhere.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from short_ldpc_decoding_osd_amd import globalmap as GL  # noqa: E402
from short_ldpc_decoding_osd_amd import nn_training as CNN_RNN  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--snr", type=float, default=2.7)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--alist", "--hfile", dest="hfile", default="CCSDS_ldpc_n128_k64.alist")
    ap.add_argument("--type", default="NMS-1")
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-dia", action="store_true")
    a = ap.parse_args()
    T1 = time.process_time()
    GL.dl_training_setting(["prog", str(a.snr), str(a.snr), str(a.batch), str(a.iters), a.hfile, a.type])
    GL.set_map('dl_training_dir', os.path.join(os.path.abspath(a.out), ""))
    GL.set_map('dl_init_seed', a.seed)
    if a.steps is not None:
        GL.set_map('termination_step', a.steps)
    selected_ds = GL.dl_training_data_setting(a.data)
    DIA = not a.no_dia
    restore_info, indicator_list, prefix_list = [], [], []
    if DIA:
        indicator_list = [True, False, False]
        prefix_list = ['model_cnn', 'model_rnn1', 'model_rnn2']
        restore_info = GL.dl_training_logistic_setting(indicator_list, prefix_list)
    res = CNN_RNN.Training_NN(selected_ds, restore_info, indicator_list, prefix_list, DIA)
    print(f"Statistics: {res['log_file']}")
    print('Running time:%s seconds!' % (time.process_time() - T1))


if __name__ == "__main__":
    main()
