"""The DL-OSD test stage without TensorFlow (LDPC_128/DL_OSD_Testing_serial/nn_testing.py).

``Testing_OSD`` keeps the reference's arguments, console and log lines, log file name, return value and termination
rule (stop after the batch on which the failure count reaches 'termination_threshold').  Per batch of retest rows the
default route stays on the device: the bit-wise CNN (``ldpc_dia_cnn``), the front end (``ldpc_hosd_front``) and the
block scan with the sliding-window early stop (``ldpc_hosd_sliding``) -- no per-frame host work; beyond (128,64) the
``ldpc_hosdx_*`` or ``ldpc_hosdw_*`` calls of the same names, as ``runtime.Decoder.hosd_stage`` picks.  ``route="host"`` is
the cross-check: every block on the device, then the reference's window loop replayed on the host frame by frame with
the NumPy classifier (``osd.sliding_osd``).

The networks are restored from TensorFlow checkpoint bundles by ``tf_checkpoint`` (no TensorFlow).
"""
from __future__ import annotations

import os
import pickle
import re
import time

import numpy as np
import torch

from . import globalmap as GL
from . import nn_net as CRNN_DEF
from . import ordered_statistics_decoding as OSD_mod
from . import tf_checkpoint
from .ordered_statistics_decoding import filter_order_patterns, generate_teps  # noqa: F401  (nn_testing.py:110-148)

VARIABLE_SUFFIX = "/.ATTRIBUTES/VARIABLE_VALUE"
ROOT_NAME = "myAwesomeModel"


def retore_saved_model(restore_ckpts_dir, restore_step, ckpt_nm):
    """:25-36 -> the checkpoint prefix ('latest' = the one the directory's ``checkpoint`` file names)."""
    print("Ready to restore a saved latest or designated model!")
    if restore_step == 'latest':
        ckpt_f = tf_checkpoint.latest_checkpoint(restore_ckpts_dir)
        if ckpt_f is None:
            raise FileNotFoundError(f"{restore_ckpts_dir}: no 'checkpoint' state file with a model_checkpoint_path")
    else:
        ckpt_f = restore_ckpts_dir + ckpt_nm + '-' + str(restore_step)
    print('Loading wgt file: ' + ckpt_f)
    return ckpt_f


def _model_variables(prefix):
    """{layer/variable: array} of the model object of a bundle; optimizer entries and slots are ignored."""
    out = {}
    for name, value in tf_checkpoint.read_checkpoint(prefix).items():
        if not name.startswith(ROOT_NAME + "/") or not name.endswith(VARIABLE_SUFFIX) or ".OPTIMIZER_SLOT" in name:
            continue
        out[name[len(ROOT_NAME) + 1: -len(VARIABLE_SUFFIX)]] = value
    return out


def _need(variables, key, prefix):
    if key not in variables:
        raise KeyError(f"{prefix}: no '{ROOT_NAME}/{key}{VARIABLE_SUFFIX}' variable in the bundle")
    return variables[key]


def restore_conv_bitwise(nn, prefix):
    v = _model_variables(prefix)
    return nn.set_weights(_need(v, "cnv_one/kernel", prefix), _need(v, "cnv_two/kernel", prefix),
                          _need(v, "cnv_three/kernel", prefix), _need(v, "dense/kernel", prefix), _need(v, "dense/bias", prefix))


def restore_predict_outlier(fcn, prefix):
    v = _model_variables(prefix)
    return fcn.set_weights(_need(v, "dense1/kernel", prefix), _need(v, "dense2/kernel", prefix))


def _restore_prefix(info, what):
    ckpts_dir, ckpt_nm, restore_step = info
    if not restore_step:
        raise ValueError(f"{what}: no restore step given -- the mirror has no freshly initialised networks to fall back on")
    return retore_saved_model(ckpts_dir, restore_step, ckpt_nm)


def load_fcn(info):
    """The sliding-window classifier from [ckpts_dir, ckpt_nm, restore_step] (:54-61)."""
    fcn = CRNN_DEF.Predict_outlier_light(GL.get_map('sliding_win_width'))
    return restore_predict_outlier(fcn, _restore_prefix(info, "Predict_outlier_light"))


def NN_gen(restore_list, indicator_list):   # noqa: N802
    """:38-62 -> (nn, fcn).  The first true indicator picks the network: [CNN, RNN1, RNN2]."""
    constructors = [CRNN_DEF.conv_bitwise, CRNN_DEF.rnn_one, CRNN_DEF.rnn_two]
    idx = next((i for i, e in enumerate(indicator_list) if e), None)
    if idx is None:
        raise ValueError("NN_gen: no network selected in indicator_list")
    nn = constructors[idx]()
    restore_conv_bitwise(nn, _restore_prefix(restore_list[0], "conv_bitwise"))
    return nn, load_fcn(restore_list[1])


def _nn_type(indicator_list, prefix_list, DIA):
    if DIA:
        for i, element in enumerate(indicator_list):
            if element:
                return prefix_list[i]
    return 'benchmark'


def query_convention_path(indicator_list, prefix_list, DIA):
    """:65-82 -> (decoding path, nn_type)."""
    return OSD_mod.query_convention_path(), _nn_type(indicator_list, prefix_list, DIA)


def query_decoding_path(indicator_list, prefix_list, DIA):
    """:84-108: the 6th object of ``dist-error-pattern-<nn_type>.pkl``, patterns by descending frequency (ties in the
    dictionary's order), filtered by ``filter_order_patterns``."""
    nn_type = _nn_type(indicator_list, prefix_list, DIA)
    file_name = GL.pattern_log_dir() + "dist-error-pattern-" + nn_type + ".pkl"
    with open(file_name, "rb") as fh:
        for _ in range(5):
            pickle.load(fh)
        pattern_dict = pickle.load(fh)
    string_pattern = sorted(pattern_dict, key=pattern_dict.get, reverse=True)
    decoding_path = [[int(d) for d in re.findall(r"\w+", element)] for element in string_pattern]
    return filter_order_patterns(decoding_path), nn_type


def calculate_loss(inputs, labels):
    """:120-125: sum of sigmoid cross-entropy with logits = -inputs (TensorFlow's stable form, f32)."""
    x = -np.asarray(inputs, dtype=np.float32)
    z = np.asarray(labels, dtype=np.float32)
    ce = np.maximum(x, 0) - x * z + np.log1p(np.exp(-np.abs(x)))
    return np.float32(ce.astype(np.float32).sum(dtype=np.float32))


def calculate_list_cross_entropy_ber(input_list, labels):
    """:127-136 -> (cross-entropy per input, bit errors per input)."""
    labels = np.asarray(labels)
    ce, ber = [], []
    for x in input_list:
        ce.append(calculate_loss(x, labels))
        hard = np.where(np.asarray(x) > 0, 0, 1)
        ber.append(int((hard != labels).sum()))
    return ce, ber


def Testing_OSD(snr, selected_ds, restore_list, indicator_list, prefix_list, DIA, route="device"):   # noqa: N802
    """:159-236 -> (FER, log file name).  ``route``: "device" (CNN -> front -> sliding scan, all on the GPU) or "host"
    (all blocks on the device, the window loop replayed on the host)."""
    if route not in ("device", "host"):
        raise ValueError(f"route must be 'device' or 'host', not {route!r}")
    start_time = time.process_time()
    code = GL.get_map('code_parameters')
    order_sum = GL.get_map('threshold_sum')
    soft_margin = GL.get_map('soft_margin')
    osd_instance = OSD_mod.osd(code)
    if GL.get_map('convention_path'):
        residual_path, nn_type = query_convention_path(indicator_list, prefix_list, DIA)
    else:
        residual_path, nn_type = query_decoding_path(indicator_list, prefix_list, DIA)
    print(f'Actual decoding path:{len(residual_path)}', residual_path)
    teps_list, acc_block_size = generate_teps(osd_instance, residual_path)
    tep_info = (teps_list, acc_block_size)
    if DIA:
        nn, fcn = NN_gen(restore_list, indicator_list)
    else:
        # the reference reaches `fcn` undefined here (NameError); the window loop still needs the classifier
        if not restore_list or len(restore_list) < 2:
            raise ValueError("Testing_OSD with DIA=False still needs the sliding-window classifier: "
                             "restore_list = [cnn_info (unused), fcn_info]")
        nn, fcn = None, load_fcn(restore_list[1])
    logdir = './log/'
    os.makedirs(logdir, exist_ok=True)
    log_filename = logdir + 'OSD-' + str(order_sum) + '-' + nn_type + '.txt'
    list_length = GL.get_map('num_iterations') + 1

    input_list = list(selected_ds.as_numpy_iterator())
    num_counter = len(input_list)
    fail_sum = correct_sum = windows_sum = complexity_sum = actual_size = 0
    cross_entropy_list_sum = [0.] * (list_length + 1)
    ber_list_sum = [0] * (list_length + 1)
    for i in range(num_counter):
        if DIA:
            rows, inputs, labels = nn.preprocessing_inputs(input_list[i])
            if route == "device":          # the refined values stay on the device for the scan
                ordering = nn(torch.from_numpy(rows).to(OSD_mod._dec().device))
                new_inputs = ordering.cpu().numpy()
            else:
                new_inputs = ordering = nn(rows)
        else:
            labels = input_list[i][1][0::list_length]
            new_inputs = ordering = input_list[i][0][0::list_length]
        actual_size += labels.shape[0]
        input_data_list = [input_list[i][0][j::list_length] for j in range(list_length)]
        input_data_list.append(new_inputs)
        cross_entropy_list, ber_list = calculate_list_cross_entropy_ber(input_data_list, labels)
        cross_entropy_list_sum = [a + b for a, b in zip(cross_entropy_list, cross_entropy_list_sum)]
        ber_list_sum = [a + b for a, b in zip(ber_list, ber_list_sum)]
        if route == "device":
            correct_counter, fail_counter, windows_size, complexity_size = osd_instance.sliding_osd_device(
                fcn, input_list[i][0], ordering, labels, tep_info)
        else:
            correct_counter, fail_counter, windows_size, complexity_size = osd_instance.sliding_osd(
                fcn, input_list[i][0], new_inputs, labels, tep_info)
        correct_sum += correct_counter
        fail_sum += fail_counter
        windows_sum += windows_size
        complexity_sum += complexity_size
        if (i + 1) % 10 == 0:
            average_size = round(complexity_sum / actual_size, 4)
            wins_size = round(windows_sum / actual_size, 4)
            print(f'\nFor {snr:.1f}dB order_sum:{order_sum} len:{len(residual_path)} soft_margin:{soft_margin}:')
            print(f'Selected actual path:{residual_path}')
            print(f'--> S/F:{correct_sum} /{fail_sum} Avr TEPs:{average_size} Wins:{wins_size}')
            average_loss_list = [cross_entropy_list_sum[j] / actual_size for j in range(list_length + 1)]
            average_ber_list = [ber_list_sum[j] / (actual_size * code.check_matrix_column) for j in range(list_length + 1)]
            formatted_floats_ce = [" ".join(["{:.3f}".format(value) for value in average_loss_list])]
            formatted_floats_ber = [" ".join(["{:.3f}".format(value) for value in average_ber_list])]
            print(f'avr CE per itr:\n{formatted_floats_ce} \nBER:{formatted_floats_ber}')
            T2 = time.process_time()
            print(f'Running time:{T2 - start_time} seconds with mean time {(T2 - start_time) / actual_size:.4f}!')
        if i == num_counter - 1 or fail_sum >= GL.get_map('termination_threshold'):
            break
    T2 = time.process_time()
    actual_size = max(actual_size, 1)
    FER = round(fail_sum / actual_size, 5)
    average_size = round(complexity_sum / actual_size, 4)
    wins_size = round(windows_sum / actual_size, 4)
    average_loss_list = [cross_entropy_list_sum[j] / actual_size for j in range(list_length + 1)]
    average_ber_list = [ber_list_sum[j] / (actual_size * code.check_matrix_column) for j in range(list_length + 1)]
    print('\nFor %.1fdB (order_sum:%d) ' % (snr, order_sum) + nn_type + ':\n')
    print('----> S:' + str(correct_sum) + ' F:' + str(fail_sum) + '\n')
    print(f'FER:{FER}--> S/F:{correct_sum} /{fail_sum} Avr TEPs:{average_size} Wins:{wins_size}')
    formatted_floats_ce = [" ".join(["{:.3f}".format(value) for value in average_loss_list])]
    formatted_floats_ber = [" ".join(["{:.3f}".format(value) for value in average_ber_list])]
    print(f'avr CE per itr:\n{formatted_floats_ce} \nBER:{formatted_floats_ber}')
    print(f'Running time:{T2 - start_time} seconds with mean time {(T2 - start_time) / actual_size:.4f}!')
    with open(log_filename, 'a+') as f:
        f.write(f'For {snr:.1f}dB order_sum:{order_sum} len:{len(residual_path)} soft_margin:{soft_margin}:\n')
        f.write(f'Selected actual path:{residual_path}\n')
        f.write('----> S:' + str(correct_sum) + ' F:' + str(fail_sum) + '\n')
        f.write(f'FER:{FER}--> S/F:{correct_sum} /{fail_sum} Avr TEPs:{average_size} Wins:{wins_size}\n')
        f.write(f'avr CE per itr:\n{formatted_floats_ce} \nBER:{formatted_floats_ber}\n')
        f.write(f'Running time:{T2 - start_time} seconds with mean time {(T2 - start_time) / actual_size:.4f}!\n')
    return FER, log_filename
