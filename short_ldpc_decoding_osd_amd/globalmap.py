"""Process-wide settings dictionary with the reference's ``globalmap`` surface
(LDPC_128/Ldpc_128_testing/globalmap.py:8-22; stage settings PB_OSD/globalmap.py:26-47,
FS_OSD/globalmap.py:28-50).  The decoders read the same keys the reference reads:
'code_parameters', 'num_iterations', 'selected_decoder_type', 'order_limit',
'termination_num_threshlod' (sic), 'd_min', 'tau_psc', 'pb_osd', 'fs_osd', 'convention_osd',
'miracle_view'; the DL-OSD stage's keys (DL_OSD_Testing_serial/globalmap.py:28-54, ``stage="DL"``):
'convention_path', 'termination_threshold', 'threshold_sum', 'training_snr', 'segment_num',
'soft_margin', 'decoding_length', 'sliding_win_width'; the DL-OSD training stage's settings and directories
(DL_Training_serial/globalmap.py:28-64, :87-106, :140-159) are the ``dl_training_*`` functions.  Unlike the reference a
missing key raises KeyError instead of printing.
"""
from __future__ import annotations

import os

map = {}  # noqa: A001  (name kept from the reference)


def set_map(key, value):
    map[key] = value


def del_map(key):
    map.pop(key, None)


def get_map(key, default=KeyError):
    if key == "all":
        return map
    if key in map:
        return map[key]
    if default is KeyError:
        raise KeyError(f"globalmap: key '{key}' was never set")
    return default


def global_setting(argv, stage="PB"):
    """Positional settings of the OSD stages: ``prog snr_lo snr_hi snr_num unit_batch T Hfile type``
    (PB_OSD/globalmap.py:26-47, FS_OSD/globalmap.py:28-50) with the reference's defaults."""
    from .fill_matrix_info import Code

    set_map('snr_lo', float(argv[1]))
    set_map('snr_hi', float(argv[2]))
    set_map('snr_num', int(argv[3]))
    set_map('unit_batch_size', int(argv[4]))
    set_map('num_iterations', int(argv[5]))
    set_map('H_filename', argv[6])
    set_map('selected_decoder_type', argv[7])
    set_map('ALL_ZEROS_CODEWORD_TRAINING', False)
    set_map('code_parameters', Code(get_map('H_filename')))
    set_map('order_limit', 3)
    set_map('termination_num_threshlod', 100)
    set_map('miracle_view', False)
    set_map('convention_osd', False)
    if stage.upper() == "DL":
        set_map('print_interval', 100)
        set_map('record_interval', 100)
        set_map('convention_path', False)
        set_map('termination_threshold', 500)
        set_map('threshold_sum', 3)
        set_map('training_snr', 2.7)
        set_map('segment_num', 6)
        set_map('soft_margin', 0.9)
        set_map('decoding_length', 30)
        set_map('sliding_win_width', 5)
    elif stage.upper() == "FS":
        set_map('fs_osd', True)
        set_map('d_min', 14)
        set_map('tau_psc', 30)
    else:
        set_map('pb_osd', True)


# ---- DL-OSD stage: where the training stage left its checkpoints and statistics (DL_OSD_Testing_serial/globalmap.py:78-117).
# 'dl_training_dir' (default: the reference's '../DL_Training_serial/') roots them.
def _training_root():
    return get_map('dl_training_dir', '../DL_Training_serial/')


def _snr_info():
    t = get_map('training_snr')
    return '/' + str(t) + '-' + str(t) + 'dB/'


def secure_segment_threshold():
    """:57-76 (segment sizes, MRB boundaries)."""
    from .ordered_statistics_decoding import secure_segment_threshold as sst
    return sst()


def logistic_setting_model(indicator_list, prefix_list):
    """:78-95 -> [ckpts_dir, 'ldpc-ckpt', 'latest'] of the selected network (the directory is created)."""
    prefix = next(prefix_list[i] for i, e in enumerate(indicator_list) if e)
    ckpts_dir = _training_root() + 'ckpts/' + prefix + _snr_info() + str(get_map('num_iterations')) + 'th' + '/'
    os.makedirs(ckpts_dir, exist_ok=True)
    return [ckpts_dir, 'ldpc-ckpt', 'latest']


def set_predict_model(DIA):   # noqa: N803
    """:96-117 -> [ckpts_dir, 'ldpc-ckpt', 'latest'] of the sliding-window classifier (the directory is created)."""
    nn_type = 'fcn' if DIA else 'benchmark'
    ckpts_dir = (_training_root() + 'ckpts/' + nn_type + _snr_info() + str(get_map('num_iterations')) + 'th/len-'
                 + str(get_map('decoding_length')) + '-order-' + str(get_map('threshold_sum')) + '/')
    os.makedirs(ckpts_dir, exist_ok=True)
    return [ckpts_dir, 'ldpc-ckpt', 'latest']


def pattern_log_dir():
    """Directory of ``dist-error-pattern-<nn>.pkl`` (nn_testing.py:96-99: the 2.7-2.7 dB statistics)."""
    return _training_root() + 'log/' + get_map('selected_decoder_type') + '/2.7-2.7dB/'


# ---- DL-OSD training stage (DL_Training_serial/globalmap.py).  It writes under 'dl_training_dir' too (default: the working
# directory, as the reference does), so a run rooted at R is what the test-stage functions above find with
# dl_training_dir = R and training_snr = snr_lo = snr_hi.
def dl_training_setting(argv):
    """Positional settings of the DL-OSD training stage: ``prog snr_lo snr_hi unit_batch T Hfile type`` (:28-64) with the
    reference's defaults."""
    from .fill_matrix_info import Code

    set_map('snr_lo', float(argv[1]))
    set_map('snr_hi', float(argv[2]))
    set_map('unit_batch_size', int(argv[3]))
    set_map('num_iterations', int(argv[4]))
    set_map('H_filename', argv[5])
    set_map('selected_decoder_type', argv[6])
    set_map('ALL_ZEROS_CODEWORD_TRAINING', False)
    set_map('epochs', 100)
    set_map('initial_learning_rate', 0.001)
    set_map('decay_rate', 0.95)
    set_map('decay_step', 500)
    set_map('termination_step', 2000)
    set_map('termination_prediction_step', 2000)
    set_map('threshold_sum', 3)
    set_map('code_parameters', Code(get_map('H_filename')))
    set_map('convention_path', False)
    set_map('print_interval', 100)
    set_map('record_interval', 100)
    set_map('nn_train', True)
    set_map('segment_num', 6)
    set_map('reliability_enhance', False)
    set_map('prediction_order_pattern', True)
    set_map('regulation_weight', 10.)
    set_map('decoding_length', 30)
    set_map('regnerate_training_samples', True)
    set_map('sliding_win_width', 5)


def _dl_stage_root():
    return os.path.join(get_map('dl_training_dir', './'), '')


def _dl_stage_snr_info():
    return str(round(get_map('snr_lo'), 2)) + '-' + str(round(get_map('snr_hi'), 2)) + 'dB/'


def dl_training_logistic_setting(indicator_list, prefix_list):
    """:87-106 -> [ckpts_dir, 'ldpc-ckpt', 'latest'] of the network being trained (the directory is created)."""
    prefix = next(prefix_list[i] for i, e in enumerate(indicator_list) if e)
    ckpts_dir = _dl_stage_root() + 'ckpts/' + prefix + '/' + _dl_stage_snr_info() + str(get_map('num_iterations')) + 'th/'
    os.makedirs(ckpts_dir, exist_ok=True)
    return [ckpts_dir, 'ldpc-ckpt', 'latest']


def dl_training_set_predict_model(DIA):   # noqa: N803
    """:107-124 -> [ckpts_dir, 'ldpc-ckpt', 'latest'] of the sliding-window classifier being trained (the directory is
    created): the directory ``set_predict_model(DIA)`` resolves with the same root and training_snr = snr_lo = snr_hi.
    The reference names no restore step here; 'latest' resumes a run where the directory holds a checkpoint."""
    nn_type = 'fcn' if DIA else 'benchmark'
    ckpts_dir = (_dl_stage_root() + 'ckpts/' + nn_type + '/' + _dl_stage_snr_info() + str(get_map('num_iterations')) + 'th/len-'
                 + str(get_map('decoding_length')) + '-order-' + str(get_map('threshold_sum')) + '/')
    os.makedirs(ckpts_dir, exist_ok=True)
    return [ckpts_dir, 'ldpc-ckpt', 'latest']


def dl_training_log_dir():
    """Where Training_NN leaves ``dist-error-pattern-<nn>.pkl`` (nn_training.py:489)."""
    return _dl_stage_root() + 'log/' + get_map('selected_decoder_type') + '/' + _dl_stage_snr_info()


def dl_training_data_setting(data_root):
    """The cached retrain set (:140-159): ``<data_root>/snr<lo>-<hi>dB/<T>th/<type>/ldpc-*-retrain.tfrecord`` -- where
    ``training_stage.post_process_input`` writes it -- in batches of unit_batch_size frames (T + 1 rows each);
    ``data_root`` stands for the reference's '../Training_data_gen_<n>/data'."""
    from .read_TFdata import data_handler
    code = get_map('code_parameters')
    list_length = get_map('num_iterations') + 1
    name = 'ldpc-allzero-retrain.tfrecord' if get_map('ALL_ZEROS_CODEWORD_TRAINING') else 'ldpc-nonzero-retrain.tfrecord'
    path = os.path.join(data_root, 'snr' + _dl_stage_snr_info()[:-1], str(get_map('num_iterations')) + 'th',
                        get_map('selected_decoder_type'), name)
    return data_handler(code.check_matrix_column, path, get_map('unit_batch_size') * list_length)


def training_setting_global(argv):
    """Settings of the NMS training stage: ``prog snr_lo snr_hi unit_batch num_batch_train T Hfile type``
    (Ldpc_128_training/globalmap.py:28-56) with the reference's defaults."""
    from .fill_matrix_info import Code

    set_map('snr_lo', float(argv[1]))
    set_map('snr_hi', float(argv[2]))
    set_map('unit_batch_size', int(argv[3]))
    set_map('num_batch_train', int(argv[4]))
    set_map('num_iterations', int(argv[5]))
    set_map('H_filename', argv[6])
    set_map('selected_decoder_type', argv[7])
    set_map('loss_process_indicator', True)
    set_map('ALL_ZEROS_CODEWORD_TRAINING', False)
    set_map('epochs', 100)
    set_map('initial_learning_rate', 0.01)
    set_map('decay_rate', 0.95)
    set_map('decay_step', 500)
    set_map('termination_step', 1200)
    set_map('code_parameters', Code(get_map('H_filename')))
    set_map('print_interval', 50)
    set_map('record_interval', 50)


def training_logistic_setting(root='.'):
    """[ckpts_dir, ckpt_nm, ckpts_dir_par, restore_step] of the training stage (Ldpc_128_training/globalmap.py:58-68)."""
    import os
    T, decoder_type = get_map('num_iterations'), get_map('selected_decoder_type')
    ckpts_dir = os.path.join(root, 'ckpts', decoder_type, f'{T}th') + os.sep
    ckpts_dir_par = os.path.join(ckpts_dir, 'par') + os.sep
    os.makedirs(ckpts_dir_par, exist_ok=True)
    return [ckpts_dir, 'ldpc-ckpt', ckpts_dir_par, 'latest']


def training_setting():
    """[start_step, multiplier, train_steps] (Ldpc_128_training/globalmap.py:70-77)."""
    return [0, 1, get_map('num_batch_train') * get_map('epochs')]


def training_data_setting(code, unit_batch_size, data_root):
    """(retrain directory, training dataset) (Ldpc_128_training/globalmap.py:79-99); ``data_root`` stands for the
    reference's '../Training_data_gen_<n>/data'."""
    import os

    from .read_TFdata import data_handler
    n, T, decoder_type = code.check_matrix_column, get_map('num_iterations'), get_map('selected_decoder_type')
    data_dir = os.path.join(data_root, f"snr{round(get_map('snr_lo'), 2)}-{round(get_map('snr_hi'), 2)}dB")
    name = 'ldpc-train-allzero.tfrecord' if get_map('ALL_ZEROS_CODEWORD_TRAINING') else 'ldpc-train-nonzero.tfrecord'
    gen_data_dir = os.path.join(data_dir, f'{T}th', decoder_type) + os.sep
    os.makedirs(gen_data_dir, exist_ok=True)
    return gen_data_dir, data_handler(n, os.path.join(data_dir, name), unit_batch_size)


def optimizer_setting():
    """ExponentialDecay(initial_learning_rate, decay_step, decay_rate, staircase=True) (Ldpc_128_training/globalmap.py:101-107)."""
    from .nms_train import ExponentialDecay
    return ExponentialDecay(get_map('initial_learning_rate'), get_map('decay_step'), get_map('decay_rate'), staircase=True)
