"""Training of the sliding-window early-stop classifier without TensorFlow
(LDPC_128/DL_Training_serial/predict_phase.py).

``train_sliding_window`` keeps the reference's arguments, console lines and files.  The windows live on the device
(``interval_boundary.reform_inputs`` -> ``ldpc_fcn_windows``); per step the weighted, penalised cross-entropy of one
mini-batch of windows and the gradient of both kernels come from one call of the HIP training kernel
(``Predict_outlier_light.loss_and_grads`` -> ``ldpc_fcn_grad``) on ``index = permutation[i*B:(i+1)*B]``, and the host
applies ``clip_by_norm(., 5e2)`` per variable and the legacy Adam of ``nms_train`` to the (win+1)^2 + 2(win+1) weights.
Checkpoints are TensorFlow bundles under the names ``nn_testing.load_fcn`` reads, with the optimizer's ``iter`` and its
``m`` / ``v`` slots, so that a resumed run continues bit for bit.

Where this differs from the reference, on purpose:
- The l2 ``kernel_regularizer`` declared on ``dense1`` has no effect in the reference's hand-written loop (``model.losses``
  is never added to the loss) and has none here.
- The epoch's permutation comes from a ``torch.Generator`` seeded with ('dl_init_seed', epoch), so a resumed run repeats
  it and continues inside the epoch where it stopped; the reference reshuffles with TensorFlow's global generator and
  restarts the epoch.  The windows are not moved: a step reads its rows through the permutation.
- With ``DIA`` false the reference falls over at the undefined ``fcn``.  Here the samples and their pickle are written
  and the function returns without a classifier.
- The validation pass is one device call over all windows, so its per-ten-batches progress lines are not printed.
The gradient rules are not pinned against TensorFlow.
"""
from __future__ import annotations

import math
import os
import pickle
from collections import Counter

import numpy as np
import torch

from . import globalmap as GL
from . import interval_boundary as Boundary
from . import nn_net as CRNN_DEF
from .nms_train import LegacyAdam, clip_by_norm
from .nn_training import checkpoint_saver, restore_optimizer, retore_saved_model  # noqa: F401  (:34-49)
from .nn_testing import restore_predict_outlier

VARIABLE_PATHS = {"dense1": "dense1/kernel", "dense2": "dense2/kernel"}   # attribute of Predict_outlier_light -> object path
CLIP_NORM = 5e2   # :211
PROB_FLOOR = np.float32(1e-30)   # :123


def class_weights(class_count):
    """:113-119: N / (num_classes * count_c) in float32 for the two classes; ValueError where one of them is empty (the
    reference would train a one-output softmax target against two outputs there: nothing to learn)."""
    counts = [int(c) for c in class_count]
    if len(counts) != 2 or min(counts) <= 0:
        raise ValueError(f"sliding-window training needs both label classes, got counts {counts} (continue, stop)")
    total = np.float32(sum(counts))
    return np.array([total / (np.float32(2) * np.float32(c)) for c in counts], dtype=np.float32)


def shuffle_data(matrix, labels, epoch=0):
    """:104-120 -> (permutation [N] int32, labels, weight_samples [N] f32, one_hot_matrix [N, 2] f32), on the device of
    ``labels``.  The permutation is drawn from a ``torch.Generator`` seeded with ('dl_init_seed', epoch); the rows are not
    moved -- sample j of the shuffled set is row permutation[j], and the last two results are in ROW order."""
    labels = labels if isinstance(labels, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(labels))
    n = labels.shape[0]
    if matrix is not None and len(matrix) != n:
        raise ValueError(f"shuffle_data: {len(matrix)} rows of inputs for {n} labels")
    gen = torch.Generator(device=labels.device)
    gen.manual_seed((int(GL.get_map('dl_init_seed', 0)) << 20) + int(epoch))
    permutation = torch.randperm(n, generator=gen, device=labels.device).to(torch.int32)
    is_stop = labels != 0
    ones = int(is_stop.sum())
    cw = class_weights((n - ones, ones))
    weight_samples = torch.where(is_stop, float(cw[1]), float(cw[0])).to(torch.float32)
    one_hot_matrix = torch.stack([~is_stop, is_stop], dim=1).to(torch.float32)
    return permutation, labels, weight_samples, one_hot_matrix


def calculation_loss(soft_output, one_hot_labels, batch_weight):
    """:121-135 restated in NumPy float64 on the given float32 probabilities: sum_b w_b pen_b (-log max(p[b][y_b], 1e-30)),
    pen_b = 'regulation_weight' where the prediction is "stop" (p0 < p1) and the truth is "continue", else 1.  The
    training loop's loss is the kernel's; this is the same sum on the host, for checks and for reading a run."""
    p = np.maximum(np.asarray(soft_output, dtype=np.float32), PROB_FLOOR).astype(np.float64)
    one_hot = np.asarray(one_hot_labels, dtype=np.float64)
    ce = np.sum(-np.log(p) * one_hot, axis=-1)
    penalty = np.where((p[:, 0] < p[:, 1]) & (one_hot[:, 0] == 1), float(GL.get_map('regulation_weight')), 1.0)
    return float(np.sum(ce * penalty * np.asarray(batch_weight, dtype=np.float64)))


def _validation_log_file():
    """:273-276 (the reference's snr_info carries its own slashes and 'dB', hence the 'dB/' directory below it)."""
    log_dir = GL._dl_stage_root() + 'log/fcn/' + GL._dl_stage_snr_info() + 'dB/'
    os.makedirs(log_dir, exist_ok=True)
    return log_dir + 'length-' + str(GL.get_map('decoding_length')) + 'prediction-phase-one.txt'


def train_sliding_window(restore_list, indicator_list, prefix_list, DIA, selected_ds=None):   # noqa: N803
    """:137-281.  Builds (or, with 'regnerate_training_samples' false, reads) the records of the decoding path, forms the
    windows, trains ``Predict_outlier_light`` on mini-batches of 'unit_batch_size' windows up to
    'termination_prediction_step', validates over all windows and appends the summary to
    ``log/fcn/<lo>-<hi>dB/dB/length-<decoding_length>prediction-phase-one.txt``.  ``selected_ds``: the cached retrain set
    (default: ``GL.dl_training_data_setting(GL 'dl_training_data_root')``).  Fresh weights come from
    ``Predict_outlier_light.initialize(GL 'dl_init_seed', default 0)`` where there is no checkpoint to resume from.
    Returns dict(step, history = the loss of every step taken, fcn, records_file, log_file, summary, validation =
    dict(S, F1, F2, loss, dist_samples, dist_labels)); with DIA false fcn / log_file / validation are None."""
    restore_info, restore_predict_info = restore_list
    print_interval = GL.get_map('print_interval')
    record_interval = GL.get_map('record_interval')
    batch_size = GL.get_map('unit_batch_size')
    decoding_length = GL.get_map('decoding_length')
    snr_info = '/' + GL._dl_stage_snr_info()
    if GL.get_map('convention_path'):
        residual_path, nn_type = Boundary.query_convention_path(indicator_list, prefix_list, DIA)
    else:
        residual_path, nn_type = Boundary.query_decoding_path(indicator_list, prefix_list, DIA)
    file_name = Boundary.records_file(nn_type)
    if GL.get_map('regnerate_training_samples'):
        if selected_ds is None:
            selected_ds = GL.dl_training_data_setting(GL.get_map('dl_training_data_root'))
        saved_summary, records_matrix = Boundary.query_samples(selected_ds, restore_info, residual_path, nn_type,
                                                               (indicator_list, DIA))
    else:
        if not os.path.exists(file_name):
            raise FileNotFoundError(f"{file_name}: no saved training samples (run once with 'regnerate_training_samples')")
        with open(file_name, "rb") as fh:
            saved_summary = pickle.load(fh)
            records_matrix = pickle.load(fh)
    print(f'Summary:(order,actual_size,correct,failed,undeteced)={saved_summary}')
    result = dict(step=0, history=[], fcn=None, records_file=file_name, log_file=None, summary=saved_summary, validation=None)
    if not DIA:
        return result
    volume_inputs, volume_labels = Boundary.reform_inputs(records_matrix)
    if not isinstance(volume_inputs, torch.Tensor):
        raise RuntimeError("train_sliding_window: no GPU -- the classifier is trained by the HIP kernel only")
    sliding_win_width = GL.get_map('sliding_win_width')
    penalty = float(GL.get_map('regulation_weight'))
    epochs = GL.get_map('epochs')
    fcn = CRNN_DEF.Predict_outlier_light(sliding_win_width)
    optimizer = LegacyAdam(GL.optimizer_setting())
    ckpts_dir, ckpt_nm, restore_step = restore_predict_info
    step, ckpt_f, history = 0, None, []
    if restore_step:
        print('Load the previous saved model from disk!')
        step, ckpt_f = retore_saved_model(ckpts_dir, restore_step, ckpt_nm)
    if ckpt_f is not None:
        restore_predict_outlier(fcn, ckpt_f)
        restore_optimizer(optimizer, ckpt_f, VARIABLE_PATHS)
    else:
        fcn.initialize(GL.get_map('dl_init_seed', 0))
    manager_save = checkpoint_saver(fcn, optimizer, ckpts_dir, ckpt_nm, VARIABLE_PATHS)
    total = volume_inputs.shape[0]
    # the class weights do not depend on the permutation: one pass, which also refuses a one-class set before any step
    _, _, weight_samples, _ = shuffle_data(None, volume_labels, 0)
    num_counter = math.ceil(total / batch_size)
    start_epoch = step // num_counter
    residual = step % num_counter
    jump_loop = False
    if step < GL.get_map('termination_prediction_step') and start_epoch < epochs and GL.get_map('nn_train'):
        for epoch in range(start_epoch, epochs):
            print("\nStart of epoch %d:" % epoch)
            permutation = shuffle_data(None, volume_labels, epoch)[0]
            right = weight_sum = 0.0                     # the weighted CategoricalAccuracy of the epoch so far
            for i in range(residual, num_counter):
                step = step + 1
                index = permutation[i * batch_size:(i + 1) * batch_size]
                loss, grads, acc, _ = fcn.loss_and_grads(volume_inputs, volume_labels, weight_samples, index, penalty)
                history.append(loss)
                optimizer.apply_gradients([(clip_by_norm(g, CLIP_NORM), attr, fcn.__dict__)
                                           for g, attr in zip(grads, fcn.TRAINABLE)])
                right += acc[0]
                weight_sum += acc[1]
                if step % print_interval == 0:
                    print('Step:%d  Loss:%.3f Error rate:%.3f' % (step, loss, 1.0 - right / weight_sum))
                if step % record_interval == 0:
                    manager_save(step)
                if step >= GL.get_map('termination_prediction_step'):
                    jump_loop = True
                    break
            residual = 0
            if jump_loop:
                break
        manager_save(step)   # the latest setting

    # verifying trained pars from start to end: one pass over all windows
    from ._osd_common import _dec
    out = _dec().fcn_grad(volume_inputs, volume_labels, fcn.packed(), sliding_win_width, penalty, weight=weight_samples,
                          want_grad=False)
    success_sum, fail_sum1, fail_sum2 = (int(c) for c in out["counts"].cpu().numpy())
    ones = int((volume_labels != 0).sum())
    cw = class_weights((total - ones, ones))
    dist_samples = Counter({float(cw[0]): total - ones, float(cw[1]): ones})
    dist_labels = Counter({0.0: total - ones, 1.0: ones})
    actual_size = total
    success_rate, fail_rate1, fail_rate2 = success_sum / actual_size, fail_sum1 / actual_size, fail_sum2 / actual_size
    print('Summary of validation:')
    print(f'Total counts:{actual_size}')
    print(f'dist_samples:{dist_samples}')
    print(f'dist_labels:{dist_labels}')
    print(f'S:{success_sum} F1:{fail_sum1} F2:{fail_sum2}')
    print(f'Success rate:{success_rate:.4f} FR1:{fail_rate1:.4f} FR2:{fail_rate2:.4f}')
    log_file = _validation_log_file()
    with open(log_file, "a+") as f:
        f.write('\nFor Summery of ' + snr_info + 'dB:\n')
        f.write(f'dist_samples:{dist_samples}\n')
        f.write(f'dist_labels:{dist_labels}\n')
        f.write(f'S:{success_sum} F1:{fail_sum1} F2:{fail_sum2}\n')
        f.write(f'Success rate:{success_rate:.4f} FR1:{fail_rate1:.4f} FR2:{fail_rate2:.4f}\n')
    result.update(step=step, history=history, fcn=fcn, log_file=log_file,
                  validation=dict(S=success_sum, F1=fail_sum1, F2=fail_sum2, loss=float(out["loss_sum"].item()),
                                  dist_samples=dist_samples, dist_labels=dist_labels))
    return result
