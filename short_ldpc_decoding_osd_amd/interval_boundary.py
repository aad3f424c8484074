"""Training samples of the sliding-window early-stop classifier without TensorFlow
(LDPC_128/DL_Training_serial/interval_boundary.py): the records of ``query_samples`` / ``query_teps_dis`` and the windows
of ``reform_inputs``.

A record is one frame's block minima over the decoding path plus ``locate_phase`` (1: the overall minimum is the label's
metric, -1: it is not); a frame whose overall minimum lies below the label's metric is "undetected" and dropped.  The
per-frame work -- reliability sort, elimination, the scan of every TEP block, the label's metric -- is the H-form front
end and block scan of the test stage (``Decoder.hosd_stage``); the comparison with the label's metric and the compaction
of the kept frames stay on the device, and only the records and three counts reach the host, for the pickle.  The windows
are built by ``ldpc_fcn_windows`` from a record matrix, so a pickle read from disk and fresh records take the same path.
"""
from __future__ import annotations

import os
import pickle
import re

import numpy as np
import torch

from . import globalmap as GL
from . import ordered_statistics_decoding as OSD_mod
from .nn_testing import _nn_type
from .nn_training import NN_gen  # noqa: F401  (:149-166)
from .ordered_statistics_decoding import filter_order_patterns, generate_teps  # noqa: F401  (:138-147, :252-265)


def query_convention_path(indicator_list, prefix_list, DIA):   # noqa: N803
    """:90-105 -> (decoding path, nn_type)."""
    return OSD_mod.query_convention_path(), _nn_type(indicator_list, prefix_list, DIA)


def query_decoding_path(indicator_list, prefix_list, DIA):   # noqa: N803
    """:107-136: the 6th object of the ``dist-error-pattern-<nn_type>.pkl`` that ``Training_NN`` left under this stage's own
    log directory, patterns by descending frequency (ties in the dictionary's order), filtered by
    ``filter_order_patterns``."""
    nn_type = _nn_type(indicator_list, prefix_list, DIA)
    with open(GL.dl_training_log_dir() + "dist-error-pattern-" + nn_type + ".pkl", "rb") as fh:
        for _ in range(5):
            pickle.load(fh)
        pattern_dict = pickle.load(fh)
    string_pattern = sorted(pattern_dict, key=pattern_dict.get, reverse=True)
    decoding_path = [[int(d) for d in re.findall(r"\w+", element)] for element in string_pattern]
    return filter_order_patterns(decoding_path), nn_type


def records_file(nn_type):
    """``log/<nn_type>/<lo>-<hi>dB/order-pattern-len<decoding_length>-<nn_type>.pkl`` under the stage's root (:213-217)."""
    logdir = GL._dl_stage_root() + 'log/' + nn_type + '/' + GL._dl_stage_snr_info()
    return logdir + 'order-pattern-len' + str(GL.get_map('decoding_length')) + '-' + nn_type + ".pkl"


_scan = {}   # the osd instance whose device copy of the TEP blocks serves the current tep_info


def _scan_instance(teps_list):
    if _scan.get("teps") is not teps_list:
        _scan.update(teps=teps_list, osd=OSD_mod.osd(GL.get_map('code_parameters')))
    return _scan["osd"]


def query_teps_dis(original_inputs, updated_inputs, labels, tep_info):
    """:267-334 for one batch -> (record matrix [kept, nblk + 1] float64, (success, fail, undetected)).
    ``updated_inputs`` order the positions (NumPy or a device tensor), ``original_inputs`` (trajectory row 0) carry the
    metric.  The front end and the scan of all blocks run per frame on the device; overall minimum < the label's metric:
    undetected, dropped; otherwise the nblk block minima, then locate_phase = 1 where the two are equal, else -1."""
    dec = OSD_mod._dec()
    teps_list, _ = tep_info
    osd_instance = _scan_instance(teps_list)
    if isinstance(updated_inputs, torch.Tensor):
        order = updated_inputs.to(device=dec.device, dtype=torch.float32).contiguous()
    else:
        order = torch.from_numpy(np.ascontiguousarray(updated_inputs, dtype=np.float32)).to(dec.device)
    metric = torch.from_numpy(np.ascontiguousarray(original_inputs, dtype=np.float32)).to(dec.device)
    lab = dec.pack_bits(torch.from_numpy(np.ascontiguousarray(labels).astype(np.uint8)).to(dec.device))
    teps, off = osd_instance._device_blocks(dec, teps_list)
    front = dec.hosd_stage("front")(order)
    out = dec.hosd_stage("search")(order, metric, front, teps, off, label_bits=lab, want_arg=False, want_best=False)
    block_min, truth = out["block_min"], out["truth"]
    overall = block_min.min(dim=1).values
    kept = (overall >= truth).to(torch.uint8)                    # not undetected (:317-320)
    index, count = dec.compact(kept)
    located = torch.where(overall == truth, 1.0, -1.0).to(torch.float64)
    n_kept = int(count.item())
    sel = index[:n_kept].long()
    records = torch.cat([block_min[sel].to(torch.float64), located[sel][:, None]], dim=1).cpu().numpy()
    success = int((records[:, -1] > -1).sum())
    return records, (success, n_kept - success, order.shape[0] - n_kept)


def query_samples(selected_ds, restore_info, residual_path, nn_type, option_tuple):
    """:168-221 -> (saved_summary, records_matrix), also pickled, in this order, to ``records_file(nn_type)``:
    saved_summary = (threshold_sum, frames, correct, failed, undetected), records_matrix [R, nblk + 1].  The ordering
    values are the CNN's output (DIA) or the last NMS row; the metric values are row 0."""
    code = GL.get_map('code_parameters')
    order_sum = GL.get_map('threshold_sum')
    print('Selectd decoding path:\n', residual_path)
    indicator_list, DIA = option_tuple   # noqa: N806
    osd_instance = OSD_mod.osd(code)
    teps_list, boundary_error_patterns = generate_teps(osd_instance, residual_path)
    tep_info = (teps_list, boundary_error_patterns)
    nn = NN_gen(restore_info, indicator_list) if DIA else None
    list_length = GL.get_map('num_iterations') + 1
    input_list = list(selected_ds.as_numpy_iterator())
    fail_sum = correct_sum = undetect_sum = validate_size = 0
    record_list = []
    for i, batch in enumerate(input_list):
        labels = batch[1][0::list_length]
        if DIA:
            rows, original_inputs, _ = nn.preprocessing_inputs(batch)
            updated_inputs = nn(torch.from_numpy(rows).to(OSD_mod._dec().device))     # stays on the device for the scan
        else:
            original_inputs = batch[0][0::list_length]
            updated_inputs = batch[0][list_length - 1::list_length]
        validate_size += updated_inputs.shape[0]
        records, cf_counter = query_teps_dis(original_inputs, updated_inputs, labels, tep_info)
        record_list.append(records)
        correct_sum += cf_counter[0]
        fail_sum += cf_counter[1]
        undetect_sum += cf_counter[2]
        if (i + 1) % 2 == 0:
            print(correct_sum, fail_sum, undetect_sum)
    file_name = records_file(nn_type)
    os.makedirs(os.path.dirname(file_name), exist_ok=True)
    saved_summary = (order_sum, validate_size, correct_sum, fail_sum, undetect_sum)
    records_matrix = np.concatenate(record_list, axis=0) if record_list else np.zeros((0, len(teps_list) + 1))
    print(f'Correct:{correct_sum},Failed:{fail_sum},Undetected:{undetect_sum}')
    with open(file_name, "wb") as fh:
        pickle.dump(saved_summary, fh)
        pickle.dump(records_matrix, fh)
    return saved_summary, records_matrix


def _host_windows(block_min, success, win):
    """:224-249 in NumPy (inspection of a pickle on a host without a GPU; training always runs on the device)."""
    nwin = block_min.shape[1] - win + 1
    row_min = block_min.min(axis=1)
    inputs, labels = [], []
    for i in range(nwin):
        window = block_min[:, i:i + win]
        labels.append(((window.min(axis=1) == row_min) & success).astype(np.uint8))
        inputs.append(np.concatenate([np.sort(window, axis=1), np.full((len(window), 1), np.float32(i))], axis=1))
    return np.concatenate(inputs).astype(np.float32), np.concatenate(labels)


def reform_inputs(records_matrix):
    """:224-249 -> (volume_inputs [(nblk-win+1)*R, win+1] f32, volume_labels [(nblk-win+1)*R] uint8), window-major (row
    i*R + r): the window of 'sliding_win_width' block minima at position i in ascending order, then float(i); the label is
    1 where the window holds the record's minimum and locate_phase != -1.  Device tensors through ``Decoder.fcn_windows``
    where there is a GPU (NumPy arrays from the same rule on a host without one).  A record with a non-finite block
    minimum -- an order pattern that has no TEP on this code gives +inf -- raises ValueError naming the block."""
    records = np.asarray(records_matrix)
    win = GL.get_map('sliding_win_width')
    if records.ndim != 2 or records.shape[1] - 1 < win:
        raise ValueError(f"reform_inputs: records of shape {records.shape}: need [R, nblk + 1] with nblk >= the window of {win}")
    bad = np.argwhere(~np.isfinite(records[:, :-1]))
    if len(bad):
        raise ValueError(f"reform_inputs: record {bad[0][0]} has a non-finite minimum in block {bad[0][1]} "
                         "(an order pattern of the decoding path has no TEP on this code)")
    block_min = np.ascontiguousarray(records[:, :-1], dtype=np.float32)
    success = records[:, -1] != -1
    if not torch.cuda.is_available():
        return _host_windows(block_min, success, win)
    dec = OSD_mod._dec()
    inputs, labels, _ = dec.fcn_windows(torch.from_numpy(block_min).to(dec.device), torch.from_numpy(success).to(dec.device), win=win)
    return inputs, labels
