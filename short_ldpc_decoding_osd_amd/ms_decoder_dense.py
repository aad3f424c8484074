"""NMS training with the reference's names (LDPC_128/Ldpc_128_training/ms_decoder_dense.py), without TensorFlow.

``Decoding_model.call`` runs ONE kernel (ldpc_nms_train_grad) that decodes the batch, computes the loss and its gradient;
the gradient of the stored weights is kept for ``training_block`` in place of tf.GradientTape.  The weights are plain
float32 [1] arrays holding the STORED (pre-softplus) values, as in the checkpoint and in ``ms_test.Decoder_Layer``.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import globalmap as GL
from . import nms_train
from .ms_test import RowBuffer
from .runtime import default_decoder
from .tf_checkpoint import VARIABLE_SUFFIX, write_checkpoint

VARIABLE_NAMES = {   # attribute -> Keras variable name (Decoder_Layer.build :74-91; the layer is "decoder__layer" in the graph)
    "shared_check_weight": "decoder_check_normalized factor",
    "shared_bit_weight": "decoder_bit_normalized factor",
    "shared_bit_weight1": "decoder_bit_normalized factor1",
    "shared_bit_weight2": "decoder_bit_normalized factor2",
}


class Decoder_Layer:
    """``Decoder_Layer`` (ms_decoder_dense.py:63-241): trainable stored weights of NMS-1/2/3."""

    def __init__(self, initial_value=-0.048):
        self.decoder_type = GL.get_map('selected_decoder_type')
        self.num_iterations = GL.get_map('num_iterations')
        self.code = GL.get_map('code_parameters')
        self.feature_len = self.code.max_chk_degree - 1
        self.initials = initial_value
        self.build(None)

    def build(self, input_shape):
        if self.decoder_type not in nms_train.STORED_NAMES:
            raise NotImplementedError(f"decoder type '{self.decoder_type}': training covers NMS-1/2/3 "
                                      "(NMS-r, compute_cv1 and its dense network, is out of scope)")
        for attr in self.trainable_names:
            setattr(self, attr, np.full([1], self.initials, dtype=np.float32))

    @property
    def trainable_names(self):
        return nms_train.STORED_NAMES[self.decoder_type]

    @property
    def variables(self):
        """[(Keras variable name, attribute)] in creation order (Model.variables of the reference)."""
        return [("decoder__layer/" + VARIABLE_NAMES[a] + ":0", a) for a in self.trainable_names]

    def stored(self):
        return {a: np.float32(getattr(self, a)[0]) for a in self.trainable_names}

    def get_weights(self):
        return [getattr(self, a).copy() for a in self.trainable_names]

    def effective_weights(self):
        return nms_train.effective(self.decoder_type, self.stored())


class Decoding_model:
    """``Decoding_model`` (ms_decoder_dense.py:24-61)."""

    def __init__(self):
        self.layer = Decoder_Layer()
        self.grads = None        # {attribute: dL/dw} of the last call

    @property
    def variables(self):
        return self.layer.variables

    def loss_and_grads(self, soft_input, labels):
        """-> (soft_output_list [y, out_1..out_T], loss, {attribute: dL/dstored}) from one ldpc_nms_train_grad launch."""
        layer = self.layer
        dec = default_decoder(layer.code)
        y = torch.from_numpy(np.ascontiguousarray(soft_input, dtype=np.float32)).to(dec.device)
        lab = dec.pack_bits(torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int64)).to(dec.device))
        T = layer.num_iterations
        alpha, w_in, w_out = layer.effective_weights()
        res = dec.nms_grad(y, lab, T, np.full(max(T, 1), alpha, np.float32), w_in, w_out, want_loss=False, want_grad=False,
                           want_traj=T > 0)
        traj = res["traj"].cpu().numpy() if T > 0 else np.zeros((0,) + tuple(y.shape), np.float32)
        soft_output_list = [np.asarray(soft_input, dtype=np.float32)] + [traj[t] for t in range(T)]
        loss = float(res["loss_sum"].cpu().numpy()[0])
        grads = nms_train.stored_grads(layer.decoder_type, layer.stored(), res["grad_sum"].cpu().numpy())
        return soft_output_list, loss, grads

    def call(self, inputs):
        """inputs = (soft_input, labels, ...) -> (soft_output_list, labels, loss)  (:29-31, Decoder_Layer.call)."""
        soft_input, labels = inputs[0], inputs[1]
        soft_output_list, loss, self.grads = self.loss_and_grads(soft_input, labels)
        return soft_output_list, labels, loss

    __call__ = call

    def get_eval(self, soft_output_list, labels):
        """(FER, BER, index[F,1]) of the last posterior (:49-61)."""
        soft = np.asarray(soft_output_list[-1])
        err = (soft < 0) != np.asarray(labels).astype(bool)
        fer_data = err.any(axis=1)
        index = np.flatnonzero(fer_data).reshape(-1, 1)
        return fer_data.sum() / soft.shape[0], err.sum() / (soft.shape[0] * soft.shape[1]), index

    def collect_failed_input_output(self, soft_output_list, labels, index):
        """T + 1 rows per listed frame (:33-42): row 0 the channel values, row t the posterior after iteration t."""
        idx = np.asarray(index).reshape(-1)
        rows = np.stack([np.asarray(s)[idx] for s in soft_output_list], axis=1).reshape(-1, np.asarray(soft_output_list[0]).shape[1])
        return RowBuffer(rows), RowBuffer(np.asarray(labels)[idx], repeat=len(soft_output_list))

    def collect_failed_input_output2(self, soft_output_list, labels, index):
        """T rows per listed frame (:43-52): the posterior after iteration t minus the channel values."""
        idx = np.asarray(index).reshape(-1)
        y = np.asarray(soft_output_list[0])[idx]
        rows = np.stack([np.asarray(s)[idx] - y for s in soft_output_list[1:]], axis=1).reshape(-1, y.shape[1])
        return RowBuffer(rows), RowBuffer(np.asarray(labels)[idx], repeat=len(soft_output_list) - 1)


def checkpoint_tensors(Model):
    """The bundle names tf.train.Checkpoint(myAwesomeModel=Model) gives the weights (training_stage.py:22)."""
    return {f"myAwesomeModel/layer/{a}{VARIABLE_SUFFIX}": getattr(Model.layer, a).copy() for a in Model.layer.trainable_names}


def write_values(path, step, Model):
    """One values.txt record (ms_decoder_dense.py:338-346): header line, then name + str(value) back to back."""
    with open(path, 'a+') as f:
        f.write("For all layers at the %4d-th step:\n" % step)
        for name, attr in Model.variables:
            f.write(name + ' ' + str(getattr(Model.layer, attr)))
        f.write('\n')


def save_decoded_data(buffer_inputs, buffer_labels, file_dir):
    """The retrain file (:255-263) through the whole-file TFRecord codec."""
    from . import data_generating as Data_gen

    def as_array(buf):
        return buf.materialize() if isinstance(buf, RowBuffer) else np.stack(buf)

    info, label = as_array(buffer_inputs), as_array(buffer_labels)
    print(" Data for retraining  with %d cases to be stored " % info.shape[0])
    Data_gen.make_tfrecord((info, label), out_filename=file_dir)
    print("Data storing finished!")


def postprocess_training(Model, iterator):
    """Failed-frame trajectories of every batch (:266-285): the rows come from ldpc_nms_traj_rows on the failures."""
    layer = Model.layer
    dec = default_decoder(layer.code)
    T = layer.num_iterations
    alpha, w_in, w_out = layer.effective_weights()
    a = np.full(max(T, 1), alpha, np.float32)
    rows_all, labels_all = [], []
    for i, inputs in enumerate(iterator.as_numpy_iterator()):
        if not (i + 1) % 100:
            print("Total ", i + 1, " batches are processed!")
        y = torch.from_numpy(np.ascontiguousarray(inputs[0], dtype=np.float32)).to(dec.device)
        labels = np.asarray(inputs[1], dtype=np.int64)
        lab = dec.pack_bits(torch.from_numpy(labels).to(dec.device))
        res = dec.nms(y, T, a, w_in, w_out, want_soft=False, want_fail=False)
        # failed = decision differs from the label (get_eval :49-61), not the syndrome
        wrong = (res["hard"] != lab).any(dim=1).to(torch.uint8)
        index, count = dec.compact(wrong)
        nf = int(count.cpu()[0])
        if nf:
            rows = dec.nms_traj_rows(y, index, count, nf, T, a, w_in, w_out)
            rows_all.append(rows[:nf].reshape(-1, dec.n).cpu().numpy())
            labels_all.append(labels[index[:nf].cpu().numpy()])
    n = layer.code.check_matrix_column
    rows = np.concatenate(rows_all) if rows_all else np.zeros((0, n), np.float32)
    labels = np.concatenate(labels_all) if labels_all else np.zeros((0, n), np.int64)
    return RowBuffer(rows), RowBuffer(labels, repeat=T + 1)


def training_block(start_info, Model, optimizer, exponential_decay, selected_ds, log_info, restore_info):
    """The training loop (:288-355): ``multiplier`` batches per step, mean gradient, clip_by_norm(g, 5) per variable,
    legacy Adam; the reference's log line every print_interval steps (and a checkpoint), a values.txt record every
    record_interval steps; stops at min(train_steps, termination_step).  ``log_info`` = (summary writer -- unused, there
    are no TensorBoard summaries --, checkpoint saver or None: called with the step)."""
    input_list = list(selected_ds.as_numpy_iterator())
    num_counter = len(input_list)
    start_step, multiplier, train_steps = start_info
    _, manager_current = log_info
    ckpts_dir, ckpt_nm, ckpts_dir_par, restore_step = restore_info
    batch_index = start_step
    termination_indicator = False
    start_step = start_step % num_counter
    print_interval, record_interval = GL.get_map('print_interval'), GL.get_map('record_interval')
    history = []
    while True:
        for i in range(start_step, num_counter):
            loss_mini_total = fer_mini_total = ber_mini_total = 0.0
            grads_mini_total = None
            for _ in range(multiplier):
                soft_output_list, label, loss = Model(input_list[i])
                fer, ber, _ = Model.get_eval(soft_output_list, label)
                loss_mini_total += loss
                fer_mini_total += fer
                ber_mini_total += ber
                grads = Model.grads
                grads_mini_total = dict(grads) if grads_mini_total is None else {k: grads_mini_total[k] + grads[k] for k in grads}
            capped = [(nms_train.clip_by_norm(np.float32(grads_mini_total[attr] / multiplier).reshape(1), 5), attr, Model.layer.__dict__)
                      for _, attr in Model.variables]
            optimizer.apply_gradients(capped)
            history.append(loss_mini_total / multiplier)
            batch_index = batch_index + 1
            if batch_index % print_interval == 0 or batch_index == train_steps - 1:
                print("Step%4d: lr:%.4f Loss:%.4f FER:%.4f BER:%.4f" % (batch_index, exponential_decay(batch_index), loss_mini_total / multiplier,
                                                                        fer_mini_total / multiplier, ber_mini_total / multiplier))
                if manager_current is not None:
                    manager_current(batch_index)
            if batch_index % record_interval == 0:
                print("For all layers at the %4d-th step:" % batch_index)
                for _, attr in Model.variables:
                    print(str(getattr(Model.layer, attr)))
                if ckpts_dir_par:
                    write_values(os.path.join(ckpts_dir_par, 'values.txt'), batch_index, Model)
            if batch_index >= min(train_steps, GL.get_map('termination_step')):
                termination_indicator = True
                break
            if batch_index % num_counter == 0:
                start_step = 0
        if termination_indicator:
            break
        start_step = 0
    print("Final selected parameters:")
    for weight in Model.layer.get_weights():
        print(weight)
    Model.history = history
    return Model


def checkpoint_saver(Model, ckpts_dir, ckpt_nm):
    """CheckpointManager.save stand-in: writes ``<ckpts_dir>/<ckpt_nm>-<step>`` with the ``checkpoint`` state file."""
    def save(step):
        write_checkpoint(os.path.join(ckpts_dir, f"{ckpt_nm}-{step}"), checkpoint_tensors(Model))
    return save
