#!/usr/bin/env python3
"""The DL-OSD training stage, as Main_DL.py drives it, over the retrain file the NMS training stage leaves
(scripts/run_training.py): the bit-wise CNN and the decoding-path statistics (nn_training.Training_NN), then the
sliding-window early-stop classifier on that path (predict_phase.train_sliding_window):

    python scripts/run_dl_training.py --data DIR --out DIR [--alist FILE] [--snr 2.7] [--batch 100] [--iters 12]
                                      [--type NMS-1] [--steps N] [--seed 0] [--no-dia] [--no-fcn] [--fcn-steps N]

--data: the root holding snr<lo>-<hi>dB/<T>th/<type>/ldpc-nonzero-retrain.tfrecord; --out: where ckpts/ and log/ go --
pass the same directory to scripts/run_dl_osd.py --training, which finds the CNN checkpoint, the decoding-path pickle
and the classifier's `fcn` checkpoint there; --steps: termination_step (default 2000, the reference's); --fcn-steps:
termination_prediction_step (default 2000); --no-fcn: stop after the CNN; --no-dia: the 'benchmark' statistics of the
last NMS iteration and the training samples of the benchmark path, no network.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from short_ldpc_decoding_osd_amd import globalmap as GL  # noqa: E402
from short_ldpc_decoding_osd_amd import nn_training as CNN_RNN  # noqa: E402
from short_ldpc_decoding_osd_amd import predict_phase as Predict  # noqa: E402


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
    ap.add_argument("--no-fcn", action="store_true")
    ap.add_argument("--fcn-steps", type=int, default=None)
    a = ap.parse_args()
    T1 = time.process_time()
    GL.dl_training_setting(["prog", str(a.snr), str(a.snr), str(a.batch), str(a.iters), a.hfile, a.type])
    GL.set_map('dl_training_dir', os.path.join(os.path.abspath(a.out), ""))
    GL.set_map('dl_init_seed', a.seed)
    if a.steps is not None:
        GL.set_map('termination_step', a.steps)
    if a.fcn_steps is not None:
        GL.set_map('termination_prediction_step', a.fcn_steps)
    selected_ds = GL.dl_training_data_setting(a.data)
    DIA = not a.no_dia
    restore_info, indicator_list, prefix_list = [], [], []
    if DIA:
        indicator_list = [True, False, False]
        prefix_list = ['model_cnn', 'model_rnn1', 'model_rnn2']
        restore_info = GL.dl_training_logistic_setting(indicator_list, prefix_list)
    res = CNN_RNN.Training_NN(selected_ds, restore_info, indicator_list, prefix_list, DIA)
    print(f"Statistics: {res['log_file']}")
    if GL.get_map('prediction_order_pattern') and not a.no_fcn:
        restore_list = [restore_info, GL.dl_training_set_predict_model(DIA)]
        res = Predict.train_sliding_window(restore_list, indicator_list, prefix_list, DIA, selected_ds=selected_ds)
        print(f"Training samples: {res['records_file']}")
        if res['fcn'] is not None:
            print(f"Classifier: {restore_list[1][0]} after {res['step']} steps; validation: {res['log_file']}")
    print('Running time:%s seconds!' % (time.process_time() - T1))


if __name__ == "__main__":
    main()
