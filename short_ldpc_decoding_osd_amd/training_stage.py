"""Training stage with the reference's names (LDPC_128/Ldpc_128_training/training_stage.py), on the HIP training kernel."""
import os

from . import globalmap as GL
from . import ms_decoder_dense as Decoder_module
from .nms_train import LegacyAdam
from .tf_checkpoint import latest_checkpoint, load_checkpoint


def training_stage(restore_info, data_root):
    """Build the model and the optimiser, restore the latest checkpoint if there is one, train (training_stage.py:12-39)."""
    unit_batch_size = GL.get_map('unit_batch_size')
    code = GL.get_map('code_parameters')
    _, iterator = GL.training_data_setting(code, unit_batch_size, data_root)
    start_info = GL.training_setting()
    exponential_decay = GL.optimizer_setting()
    Model = Decoder_module.Decoding_model()
    optimizer = LegacyAdam(exponential_decay)
    ckpts_dir, ckpt_nm, ckpts_dir_par, restore_step = restore_info
    if restore_step and os.path.isdir(ckpts_dir) and latest_checkpoint(ckpts_dir):
        prefix = latest_checkpoint(ckpts_dir)
        load_checkpoint(Model, prefix)
        start_info[0] = int(prefix.split('-')[-1]) + 1
        print('Loading wgt file: ' + prefix)
    log_info = (None, Decoder_module.checkpoint_saver(Model, ckpts_dir, ckpt_nm))
    if GL.get_map('loss_process_indicator'):
        Model = Decoder_module.training_block(start_info, Model, optimizer, exponential_decay, iterator, log_info, restore_info)
    return Model


def post_process_input(Model, data_root):
    """Failed-decoding trajectories of the training set -> ``<data_dir>/<T>th/<type>/ldpc-*-retrain.tfrecord``
    (training_stage.py:41-56); returns the file name."""
    unit_batch_size = GL.get_map('unit_batch_size')
    code = GL.get_map('code_parameters')
    data_dir, iterator = GL.training_data_setting(code, unit_batch_size, data_root)
    GL.set_map('loss_process_indicator', False)
    buffer_list = Decoder_module.postprocess_training(Model, iterator)
    file_name = 'ldpc-allzero-retrain.tfrecord' if GL.get_map('ALL_ZEROS_CODEWORD_TRAINING') else 'ldpc-nonzero-retrain.tfrecord'
    retrain_file_dir = data_dir + file_name
    Decoder_module.save_decoded_data(buffer_list[0], buffer_list[1], retrain_file_dir)
    print("Collecting targeted cases of decoding is finished!")
    return retrain_file_dir
