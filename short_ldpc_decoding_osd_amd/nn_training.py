"""The DL-OSD training stage without TensorFlow (LDPC_128/DL_Training_serial/nn_training.py): training of the bit-wise
CNN on the retrain set and the statistics pass that leaves the decoding-path pickle for the test stage.

``Training_NN`` keeps the reference's arguments, console lines and files.  Per step the loss and the gradient of every
weight come from one call of the HIP training kernel (``conv_bitwise.loss_and_grads`` -> ``ldpc_dia_cnn_grad``); the
host applies ``clip_by_norm(., 5e2)`` per variable and the legacy Adam of ``nms_train`` to the 145 + 2(L-6) weights.
Checkpoints are TensorFlow bundles under the names ``nn_testing.restore_conv_bitwise`` reads, with the optimizer's
``iter`` and its ``m`` / ``v`` slots, so that a resumed run continues bit for bit.  The gradient rules are not pinned
against TensorFlow.

The verification pass (:418-498) stays on the device per batch: refined values from ``ldpc_dia_cnn``, stable sorts and
gathers as torch ops (ascending |value|, ties to the lower index -- the rule of ``ldpc_hosd_front``), and the
elimination of ``stat_pro_osd`` through ``Decoder.hosd_stage("front")``; only the per-frame counts reach the host.
The statistics functions run where their tensors live; NumPy input is taken as a host tensor.
"""
from __future__ import annotations

import math
import os
import pickle
from collections import Counter

import numpy as np
import torch

from . import globalmap as GL
from . import nn_net as CRNN_DEF
from . import tf_checkpoint
from .nms_train import LegacyAdam, clip_by_norm
from .nn_testing import ROOT_NAME, VARIABLE_SUFFIX, calculate_loss, restore_conv_bitwise  # noqa: F401  (calculate_loss: :293-297)

OPTIMIZER_NAME = "myAwesomeOptimizer"
# attribute of conv_bitwise -> object path of its variable under the model (tf.train.Checkpoint(myAwesomeModel=nn), :371)
VARIABLE_PATHS = {"cnv_one": "cnv_one/kernel", "cnv_two": "cnv_two/kernel", "cnv_three": "cnv_three/kernel",
                  "dense_kernel": "dense/kernel", "dense_bias": "dense/bias"}
CLIP_NORM = 5e2   # :400


def _tensor(x, dtype=None):
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    return t if dtype is None else t.to(dtype)


def _reliability_order(values):
    """Ascending |value|, stable: ties go to the lower index."""
    return torch.argsort(values.abs(), dim=-1, stable=True)


def evaluate_MRB_bit(updated_inputs, labels):   # noqa: N802
    """:323-333 -> Counter of the number of hard-decision errors among each frame's k most reliable bits."""
    code = GL.get_map('code_parameters')
    x = _tensor(updated_inputs)
    lab = _tensor(labels).to(x.device, torch.int64)
    order_index = _reliability_order(x)[:, -code.k:]
    order_inputs_hard = (torch.gather(x, 1, order_index) <= 0).to(torch.int64)
    cmp_result = (order_inputs_hard != torch.gather(lab, 1, order_index)).sum(dim=-1)
    return Counter(cmp_result.cpu().numpy().tolist())


def dic_union(dicA, dicB):   # noqa: N803
    """:335-341."""
    for key, value in dicB.items():
        if key in dicA:
            dicA[key] += value
        else:
            dicA[key] = value
    return dict(sorted(dicA.items(), key=lambda d: d[0]))


def stat_pro_osd(inputs, labels):
    """:549-575 -> (updated MRB [F, k] int64: positions in the reliability order, ascending -- the reference returns them
    unsorted and sorts them in evaluate_MRB_pattern --, swap count per frame: the MRB entries that came from below n-k).
    The elimination is the device front end of the DL-OSD test stage for this code."""
    from ._osd_common import _dec
    dec = _dec()
    code = GL.get_map('code_parameters')
    n, k = code.check_matrix_column, code.k
    x = _tensor(inputs, torch.float32).to(dec.device).contiguous()
    uidx = dec.hosd_stage("front")(x)[1]
    updated_MRB = uidx[:, n - k:n].to(torch.int64)   # noqa: N806
    swap_len_list = (updated_MRB < n - k).sum(dim=-1).cpu().numpy().tolist()
    return updated_MRB, swap_len_list


def evaluate_MRB_pattern(inputs, labels, updated_mrb_list, swap_len_list, pattern_cnt, boundary_MRB):   # noqa: N802, N803
    """:524-546: errors per MRB segment of every frame, counted under the key ','.join(counts)."""
    x = _tensor(inputs)
    lab = _tensor(labels).to(x.device, torch.int64)
    order_index = _reliability_order(x)
    order_inputs = torch.gather(x, 1, order_index)
    order_labels = torch.gather(lab, 1, order_index)
    if not isinstance(updated_mrb_list, torch.Tensor):
        updated_mrb_list = torch.from_numpy(np.stack([np.asarray(e, dtype=np.int64) for e in updated_mrb_list]))
    reorder_index = torch.sort(updated_mrb_list.to(x.device, torch.int64).reshape(x.shape[0], -1), dim=-1).values
    reorder_inputs_hard = (torch.gather(order_inputs, 1, reorder_index) <= 0).to(torch.int64)
    diff_matrix = (reorder_inputs_hard != torch.gather(order_labels, 1, reorder_index)).to(torch.int64)
    bounds = [int(b) for b in boundary_MRB]
    compound_block = torch.stack([diff_matrix[:, bounds[i]:bounds[i + 1]].sum(dim=-1) for i in range(len(bounds) - 1)], dim=-1)
    for row in compound_block.cpu().numpy():
        pattern_cnt[','.join(map(str, row))] += 1
    return pattern_cnt


def generate_pattern_dist(inputs, labels, pattern_cnt, boundary_MRB):   # noqa: N803
    """:518-521."""
    updated_MRB_list, swap_len_list = stat_pro_osd(inputs, labels)   # noqa: N806
    pattern_cnt = evaluate_MRB_pattern(inputs, labels, updated_MRB_list, swap_len_list, pattern_cnt, boundary_MRB)
    return pattern_cnt, swap_len_list


# ------------------------------------------------------------------------------------------------------ checkpoints
def checkpoint_tensors(nn, optimizer, paths=None):
    """The bundle of tf.train.Checkpoint(myAwesomeModel=nn, myAwesomeOptimizer=optimizer) (:371): the variables (``paths``:
    attribute -> object path; default the five of conv_bitwise), the optimizer's step count and its m / v slot of every
    variable that has one."""
    t = {f"{OPTIMIZER_NAME}/iter{VARIABLE_SUFFIX}": np.array(optimizer.iterations, np.int64)}
    for attr, path in (VARIABLE_PATHS if paths is None else paths).items():
        t[f"{ROOT_NAME}/{path}{VARIABLE_SUFFIX}"] = getattr(nn, attr).copy()
        for slot, store in (("m", optimizer.m), ("v", optimizer.v)):
            if attr in store:
                t[f"{ROOT_NAME}/{path}/.OPTIMIZER_SLOT/{OPTIMIZER_NAME}/{slot}{VARIABLE_SUFFIX}"] = store[attr].copy()
    return t


def checkpoint_saver(nn, optimizer, ckpts_dir, ckpt_nm, paths=None):
    """CheckpointManager.save stand-in: writes ``<ckpts_dir>/<ckpt_nm>-<step>`` and the ``checkpoint`` state file (every
    checkpoint is kept; the reference keeps the last five)."""
    def save(checkpoint_number):
        return tf_checkpoint.write_checkpoint(os.path.join(ckpts_dir, f"{ckpt_nm}-{checkpoint_number}"),
                                              checkpoint_tensors(nn, optimizer, paths))
    return save


def retore_saved_model(restore_ckpts_dir, restore_step, ckpt_nm):
    """:278-291 -> (start step, checkpoint prefix), or (0, None) where the directory holds no checkpoint yet."""
    print("Ready to restore a saved latest or designated model!")
    if restore_step == 'latest':
        ckpt_f = tf_checkpoint.latest_checkpoint(restore_ckpts_dir)
    else:
        ckpt_f = restore_ckpts_dir + ckpt_nm + '-' + str(restore_step)
    if ckpt_f is None or not os.path.exists(ckpt_f + ".index"):
        print('Error, no qualified file found')
        return 0, None
    print('Loading wgt file: ' + ckpt_f)
    return int(ckpt_f.split('-')[-1]), ckpt_f


def restore_optimizer(optimizer, prefix, paths=None):
    """The optimizer's step count and slots from a bundle of ``checkpoint_tensors`` (``paths`` as there)."""
    tensors = tf_checkpoint.read_checkpoint(prefix)
    key = f"{OPTIMIZER_NAME}/iter{VARIABLE_SUFFIX}"
    if key in tensors:
        optimizer.iterations = int(tensors[key])
    for attr, path in (VARIABLE_PATHS if paths is None else paths).items():
        for slot, store in (("m", optimizer.m), ("v", optimizer.v)):
            key = f"{ROOT_NAME}/{path}/.OPTIMIZER_SLOT/{OPTIMIZER_NAME}/{slot}{VARIABLE_SUFFIX}"
            if key in tensors:
                store[attr] = np.asarray(tensors[key], dtype=np.float32).copy()
    return optimizer


def _selected(indicator_list, prefix_list=None):
    idx = next((i for i, e in enumerate(indicator_list) if e), None)
    if idx is None:
        raise ValueError("no network selected in indicator_list")
    nn = [CRNN_DEF.conv_bitwise, CRNN_DEF.rnn_one, CRNN_DEF.rnn_two][idx]()
    return nn, (prefix_list[idx] if prefix_list is not None else None)


def NN_gen(restore_info, indicator_list):   # noqa: N802
    """:500-516 -> the selected network, restored from [ckpts_dir, ckpt_nm, restore_step] when a step is named."""
    nn, _ = _selected(indicator_list)
    ckpts_dir, ckpt_nm, restore_step = restore_info
    if restore_step:
        _, ckpt_f = retore_saved_model(ckpts_dir, restore_step, ckpt_nm)
        if ckpt_f is None:
            raise FileNotFoundError(f"{ckpts_dir}: no checkpoint to restore the network from")
        restore_conv_bitwise(nn, ckpt_f)
    return nn


# ------------------------------------------------------------------------------------------------------- the stage
def _device_batch(nn, batch, device):
    """One cached batch -> (rows [F, L, n] f32, labels [F, n] int64) on the device (preprocessing_inputs, nn_net.py)."""
    rows, _, labels = nn.preprocessing_inputs(batch)
    return torch.from_numpy(rows).to(device), torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int64)).to(device)


def Training_NN(selected_ds, restore_info, indicator_list, prefix_list, DIA=False):   # noqa: N802, N803
    """:345-498.  Trains the selected network (DIA) on the cached batches, then runs the verification pass over them
    and pickles its six objects to ``<root>/log/<type>/<lo>-<hi>dB/dist-error-pattern-<prefix>.pkl``; with DIA false
    (the 'benchmark' path) there is no network and the statistics are those of the last NMS iteration.  Fresh weights
    come from ``conv_bitwise.initialize(GL 'dl_init_seed', default 0)`` where there is no checkpoint to resume from.
    Returns dict(step, history = the loss of every step taken, nn, log_file)."""
    from ._osd_common import _dec
    dec = _dec()
    list_length =GL.get_map('num_iterations') + 1
    print_interval = GL.get_map('print_interval')
    record_interval = GL.get_map('record_interval')
    prefix = 'benchmark'
    input_list = list(selected_ds.as_numpy_iterator())
    num_counter = len(input_list)
    nn, step, history = None, 0, []
    if DIA:
        epochs = GL.get_map('epochs')
        nn, prefix = _selected(indicator_list, prefix_list)
        optimizer = LegacyAdam(GL.optimizer_setting())
        ckpts_dir, ckpt_nm, restore_step = restore_info
        ckpt_f = None
        if restore_step:
            print('Load the previous saved model from disk!')
            step, ckpt_f = retore_saved_model(ckpts_dir, restore_step, ckpt_nm)
        if ckpt_f is not None:
            restore_conv_bitwise(nn, ckpt_f)
            restore_optimizer(optimizer, ckpt_f)
        else:
            nn.initialize(GL.get_map('dl_init_seed', 0))
        manager_save = checkpoint_saver(nn, optimizer, ckpts_dir, ckpt_nm)
        start_epoch = step // num_counter
        residual = step % num_counter
        jump_loop = False
        if GL.get_map('nn_train') and step < GL.get_map('termination_step'):
            for epoch in range(start_epoch, epochs):
                print("\nStart of epoch %d:" % epoch)
                for i in range(residual, num_counter):
                    rows, labels = _device_batch(nn, input_list[i], dec.device)
                    step = step + 1
                    loss, grads = nn.loss_and_grads(rows, labels)
                    history.append(loss)
                    optimizer.apply_gradients([(clip_by_norm(g, CLIP_NORM), attr, nn.__dict__)
                                               for g, attr in zip(grads, nn.TRAINABLE)])
                    if step % print_interval == 0:
                        print('Step:%d  Loss:%.3f' % (step, loss))
                    if step % record_interval == 0:
                        manager_save(step)
                    if step >= GL.get_map('termination_step'):
                        jump_loop = True
                        break
                residual = 0
                if jump_loop:
                    break
            manager_save(step)   # the latest setting

    # verifying trained pars from start to end
    dic_sum, dic_sum_initial, dic_sum_end = {}, {}, {}
    actual_size = 0
    pattern_cnt = Counter()
    swap_list = []
    loss_sum = 0.
    segment_size_list, boundary_MRB = GL.secure_segment_threshold()   # noqa: N806
    for i in range(num_counter):
        feats = torch.from_numpy(np.ascontiguousarray(input_list[i][0], dtype=np.float32)).to(dec.device)
        labels = torch.from_numpy(np.ascontiguousarray(input_list[i][1][list_length - 1::list_length], dtype=np.int64)).to(dec.device)
        first, last = feats[0::list_length].contiguous(), feats[list_length - 1::list_length].contiguous()
        updated_inputs = nn(feats) if DIA else last
        loss_sum += calculate_loss(updated_inputs.cpu().numpy(), labels.cpu().numpy())
        actual_size += updated_inputs.shape[0]
        dic_sum = dic_union(dic_sum, evaluate_MRB_bit(updated_inputs, labels))
        dic_sum_initial = dic_union(dic_sum_initial, evaluate_MRB_bit(first, labels))
        dic_sum_end = dic_union(dic_sum_end, evaluate_MRB_bit(last, labels))
        pattern_cnt, swap_len_list = generate_pattern_dist(updated_inputs, labels, pattern_cnt, boundary_MRB)
        swap_list += swap_len_list
        if (i + 1) % 100 == 0:
            print(dic_sum)
    merged_counter = Counter()
    for key, value in pattern_cnt.items():
        merged_counter[sum(int(d) for d in key.split(','))] += value
    updated_counter = Counter({key: value / math.prod(math.comb(int(s), int(d)) for s, d in zip(segment_size_list, key.split(',')))
                               for key, value in pattern_cnt.items()})
    average_loss = loss_sum / max(actual_size, 1)
    average_swaps = sum(swap_list) / max(len(swap_list), 1)
    print(f'Total counts:{actual_size}')
    print(f'average swaps:{average_swaps:.4f} \naverage loss:{average_loss:.4f}')
    print('Summary for 0-th dist:', dic_sum_initial)
    print('Summary for T-th dist:', dic_sum_end)
    print('Summary before GE for ' + prefix + ':', dic_sum)
    print('Summary of after GE for ' + prefix + ':', merged_counter)
    print(f'Summary of decoding_pth:\n{pattern_cnt}')
    print('Summary of decoding_pth:')
    for key, value in updated_counter.most_common():
        print(f'{key}: {value:.4f}')
    log_dir = GL.dl_training_log_dir()
    os.makedirs(log_dir, exist_ok=True)
    log_file = log_dir + "dist-error-pattern-" + prefix + ".pkl"
    with open(log_file, "wb") as fh:
        for obj in (actual_size, dic_sum_initial, dic_sum_end, dic_sum, merged_counter, updated_counter):
            pickle.dump(obj, fh)
    return dict(step=step, history=history, nn=nn, log_file=log_file)
