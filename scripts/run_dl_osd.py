#!/usr/bin/env python3
"""The DL-OSD test stage, as Main_DL_OSD.py drives it, over the retest files scripts/run_stages.py writes:

    python scripts/run_dl_osd.py --data DIR --training DIR [--snr-lo 2.0 --snr-hi 3.0 --snr-num 6] [--batch 100]
                                 [--iters 12] [--type NMS-1] [--no-dia] [--convention-path] [--route device|host]
                                 [--alist FILE]

--data: the root holding <type>/<T>th/<snr>dB/ldpc-nonzero-retest.tfrecord (run_stages.py's output directory);
--training: the training stage's directory (ckpts/ with the CNN and classifier checkpoints, log/ with the
dist-error-pattern pickle); --alist: the code definition (default: the CCSDS (128,64) code; any code the H-form kernels
serve, e.g. LDPC_N96_K48_P8_set0_dmin10.alist).  The log goes to ./log/OSD-<order_sum>-<nn>.txt as in the reference.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from short_ldpc_decoding_osd_amd import globalmap as GL  # noqa: E402
from short_ldpc_decoding_osd_amd import nn_testing as NN_test, read_TFdata  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", required=True)
    ap.add_argument("--training", required=True)
    ap.add_argument("--snr-lo", type=float, default=2.0)
    ap.add_argument("--snr-hi", type=float, default=3.0)
    ap.add_argument("--snr-num", type=int, default=6)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--alist", "--hfile", dest="hfile", default="CCSDS_ldpc_n128_k64.alist")
    ap.add_argument("--type", default="NMS-1")
    ap.add_argument("--no-dia", action="store_true")
    ap.add_argument("--convention-path", action="store_true")
    ap.add_argument("--route", default="device", choices=("device", "host"))
    a = ap.parse_args()
    T1 = time.process_time()
    GL.global_setting(["prog", str(a.snr_lo), str(a.snr_hi), str(a.snr_num), str(a.batch), str(a.iters), a.hfile, a.type],
                      stage="DL")
    GL.set_map('dl_training_dir', os.path.join(os.path.abspath(a.training), ""))
    GL.set_map('convention_path', a.convention_path)
    DIA = not a.no_dia
    indicator_list = [True, False, False]
    prefix_list = ['model_cnn', 'model_rnn1', 'model_rnn2']
    restore_list = [GL.logistic_setting_model(indicator_list, prefix_list), GL.set_predict_model(True)]
    L = a.iters + 1
    snr_list = np.linspace(a.snr_lo, a.snr_hi, a.snr_num)
    FER_list = []
    log_filename = None
    for snr in snr_list:
        snr = round(float(snr), 2)
        f = os.path.join(a.data, a.type, f"{a.iters}th", f"{snr}dB", "ldpc-nonzero-retest.tfrecord")
        ds = read_TFdata.data_handler(GL.get_map('code_parameters').check_matrix_column, f, a.batch * L)
        FER, log_filename = NN_test.Testing_OSD(snr, ds, restore_list, indicator_list, prefix_list, DIA, route=a.route)
        FER_list.append((snr, FER))
    soft_margin = GL.get_map('soft_margin')
    print(f'Summary of FER:{FER_list} soft_margin:{soft_margin}')
    if log_filename:
        with open(log_filename, 'a+') as fh:
            fh.write(f'\n Summary of FER for soft_margin={soft_margin}:{FER_list}')
    print('Running time:%s seconds!' % (time.process_time() - T1))


if __name__ == "__main__":
    main()
