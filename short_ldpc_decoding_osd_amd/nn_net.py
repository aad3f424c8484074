"""The DL-OSD stage's networks without TensorFlow (LDPC_128/DL_OSD_Testing_serial/nn_net.py).

``conv_bitwise`` (:174-211) refines each bit's LLR from its (T+1)-long NMS trajectory; its forward pass is the HIP
kernel behind ``ldpc_dia_cnn``.  ``Predict_outlier_light`` (:136-149) is the sliding-window early-stop classifier; the
device form lives in ``ldpc_hosd_sliding`` and ``__call__`` here is a NumPy f32 form in the same operation order, so the
host replay of ``ordered_statistics_decoding.osd.sliding_osd`` can use it.  Weights are NumPy arrays in the Keras
layouts, restored from the training stage's checkpoints by ``nn_testing.NN_gen``.  Both networks are trained here too:
``loss_and_grads`` of either class is one call of its HIP training kernel (``ldpc_dia_cnn_grad``, ``ldpc_fcn_grad``).

Float order (shared with the kernels, include/ldpc_osd.h): every output of a Conv1D or Dense layer is a sequential f32
sum over its flattened input index (Conv1D: (tap, in-channel), tap-major), starting from the first product, then
+ bias where the layer has one.  The classifier's softmax subtracts the larger logit: p_c = e_c / (e0 + e1),
e_c = exp(z_c - max(z)).  The PReLU that ``conv_bitwise`` constructs is never applied in its ``call`` and is not here.
"""
from __future__ import annotations

import numpy as np
import torch

from . import globalmap as GL

F32 = np.float32


def _checked(name, value, shape):
    a = np.asarray(value, dtype=F32)
    if a.shape != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {a.shape}")
    return np.ascontiguousarray(a)


def _seq_matmul(x, w):
    """x [B, d_in] . w [d_in, d_out] as sequential f32 sums over the input index, starting from the first product."""
    acc = x[:, 0:1] * w[0][None, :]
    for i in range(1, w.shape[0]):
        acc = acc + x[:, i:i + 1] * w[i][None, :]
    return acc


class conv_bitwise:   # noqa: N801  (name kept from the reference)
    """Conv1D 1->8, 8->4, 4->2 (kernel 3, valid, no bias), Flatten, Dense(2(L-6) -> 1) + bias, per bit."""

    VARIABLES = ("cnv_one", "cnv_two", "cnv_three", "dense")

    def __init__(self, list_length=None, n_dims=None):
        code = GL.get_map('code_parameters', None)
        self.list_length = int(GL.get_map('num_iterations') + 1 if list_length is None else list_length)
        self.n_dims = int(code.check_matrix_column if n_dims is None else n_dims)
        if self.list_length < 7:
            raise ValueError(f"conv_bitwise: trajectories of {self.list_length} values; three valid convolutions need >= 7")
        self.cnv_one = self.cnv_two = self.cnv_three = self.dense_kernel = self.dense_bias = None

    def shapes(self):
        return dict(cnv_one=(3, 1, 8), cnv_two=(3, 8, 4), cnv_three=(3, 4, 2),
                    dense_kernel=(2 * (self.list_length - 6), 1), dense_bias=(1,))

    def set_weights(self, cnv_one, cnv_two, cnv_three, dense_kernel, dense_bias):
        sh = self.shapes()
        self.cnv_one = _checked("cnv_one/kernel", cnv_one, sh["cnv_one"])
        self.cnv_two = _checked("cnv_two/kernel", cnv_two, sh["cnv_two"])
        self.cnv_three = _checked("cnv_three/kernel", cnv_three, sh["cnv_three"])
        self.dense_kernel = _checked("dense/kernel", dense_kernel, sh["dense_kernel"])
        self.dense_bias = _checked("dense/bias", dense_bias, sh["dense_bias"])
        return self

    def packed(self):
        """The weight vector of ``ldpc_dia_cnn``: conv1, conv2, conv3, dense kernel, dense bias (Keras layouts)."""
        if self.cnv_one is None:
            raise RuntimeError("conv_bitwise: no weights (restore a checkpoint or call set_weights)")
        return np.concatenate([self.cnv_one.ravel(), self.cnv_two.ravel(), self.cnv_three.ravel(),
                               self.dense_kernel.ravel(), self.dense_bias.ravel()]).astype(F32)

    TRAINABLE = ("cnv_one", "cnv_two", "cnv_three", "dense_kernel", "dense_bias")   # attributes, in the packed order

    def initialize(self, seed=0):
        """Fresh weights with the Keras defaults of the layers: ``glorot_uniform`` kernels -- uniform on [-a, a],
        a = sqrt(6 / (fan_in + fan_out)), fan_in = 3 in and fan_out = 3 out for a Conv1D of kernel 3, (in, out) for the
        Dense layer -- and a zero bias.  Drawn from ``numpy.random.default_rng(seed)``: the distribution is TensorFlow's,
        the random stream is not, so a run does not reproduce a TensorFlow run weight for weight."""
        rng = np.random.default_rng(seed)
        sh = self.shapes()
        drawn = {}
        for name in ("cnv_one", "cnv_two", "cnv_three", "dense_kernel"):
            shape = sh[name]
            receptive = int(np.prod(shape[:-2]))
            limit = np.sqrt(6.0 / (receptive * shape[-2] + receptive * shape[-1]))
            drawn[name] = rng.uniform(-limit, limit, size=shape).astype(F32)
        return self.set_weights(drawn["cnv_one"], drawn["cnv_two"], drawn["cnv_three"], drawn["dense_kernel"],
                                np.zeros(sh["dense_bias"], F32))

    def trainable_variables(self):
        """[conv1, conv2, conv3, dense kernel, dense bias]: the arrays themselves, in the packed order."""
        if self.cnv_one is None:
            raise RuntimeError("conv_bitwise: no weights (initialize, restore a checkpoint or call set_weights)")
        return [getattr(self, a) for a in self.TRAINABLE]

    def loss_and_grads(self, rows, labels):
        """The training step's loss (nn_training.py:293-297 of the training stage) on the retrain rows ([F, L, n] or
        [F*L, n]; NumPy or a device tensor) against ``labels`` [F, n], and its gradient: (loss as a float, one float32
        array per trainable variable, unpacked from the f64 gradient of ``ldpc_dia_cnn_grad``).  One synchronisation."""
        from ._osd_common import _dec
        dec = _dec()
        if not isinstance(rows, torch.Tensor):
            rows = torch.from_numpy(np.ascontiguousarray(rows, dtype=F32)).to(dec.device)
        rows = rows.reshape(-1, self.list_length, self.n_dims).contiguous()
        if not isinstance(labels, torch.Tensor):
            labels = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int64)).to(dec.device)
        loss_sum, grad, _ = dec.dia_cnn_grad(rows, dec.pack_bits(labels.contiguous()), self.packed())
        both = torch.cat([loss_sum, grad]).cpu().numpy()
        grads, at = [], 1
        for v in self.trainable_variables():
            grads.append(both[at:at + v.size].reshape(v.shape).astype(F32))
            at += v.size
        return float(both[0]), grads

    def preprocessing_inputs(self, input_slice):
        """:198-211 without the transpose -> (rows [F, L, n] f32, channel values [F, n], labels [F, n])."""
        original_input, original_label = np.asarray(input_slice[0]), np.asarray(input_slice[1])
        rows = np.ascontiguousarray(original_input, dtype=F32).reshape(-1, self.list_length, self.n_dims)
        return rows, original_input[0::self.list_length], original_label[0::self.list_length]

    def __call__(self, rows):
        """Refined values [F, n] of the retest rows ([F, L, n] or [F*L, n]).  A device tensor gives a device tensor;
        NumPy input gives NumPy output."""
        from ._osd_common import _dec
        dec = _dec()
        if isinstance(rows, torch.Tensor):
            return dec.dia_cnn(rows.reshape(-1, self.list_length, self.n_dims).contiguous(), self.packed())
        x = torch.from_numpy(np.ascontiguousarray(rows, dtype=F32).reshape(-1, self.list_length, self.n_dims)).to(dec.device)
        return dec.dia_cnn(x, self.packed()).cpu().numpy()


class Predict_outlier_light:   # noqa: N801
    """Dense(w+1 -> w+1, no bias, linear), Dense(w+1 -> 2, no bias, softmax) on the sorted window + its index."""

    VARIABLES = ("dense1", "dense2")

    def __init__(self, sliding_win_width):
        self.sliding_win_width = int(sliding_win_width)
        self.input_width = self.sliding_win_width + 1
        self.dense1 = self.dense2 = None

    def shapes(self):
        return dict(dense1=(self.input_width, self.input_width), dense2=(self.input_width, 2))

    def set_weights(self, dense1, dense2):
        sh = self.shapes()
        self.dense1 = _checked("dense1/kernel", dense1, sh["dense1"])
        self.dense2 = _checked("dense2/kernel", dense2, sh["dense2"])
        return self

    def packed(self):
        """The classifier weights of ``ldpc_hosd_sliding``: dense1 then dense2, row-major."""
        if self.dense1 is None:
            raise RuntimeError("Predict_outlier_light: no weights (restore a checkpoint or call set_weights)")
        return np.concatenate([self.dense1.ravel(), self.dense2.ravel()]).astype(F32)

    TRAINABLE = ("dense1", "dense2")   # attributes, in the packed order

    def initialize(self, seed=0):
        """Fresh weights with the initializers of the reference's layers (nn_net.py of the training stage): ``dense1``
        RandomNormal(stddev 0.05), ``dense2`` the Keras default glorot_uniform, uniform on [-a, a] with
        a = sqrt(6 / (win + 1 + 2)).  Drawn from ``numpy.random.default_rng(seed)``: the distributions are TensorFlow's,
        the random stream is not."""
        rng = np.random.default_rng(seed)
        d = self.input_width
        limit = np.sqrt(6.0 / (d + 2))
        return self.set_weights((rng.standard_normal((d, d)) * 0.05).astype(F32),
                                rng.uniform(-limit, limit, size=(d, 2)).astype(F32))

    def trainable_variables(self):
        """[dense1 kernel, dense2 kernel]: the arrays themselves, in the packed order."""
        if self.dense1 is None:
            raise RuntimeError("Predict_outlier_light: no weights (initialize, restore a checkpoint or call set_weights)")
        return [getattr(self, a) for a in self.TRAINABLE]

    def loss_and_grads(self, inputs, labels, weight=None, index=None, penalty=1.0):
        """One training step's loss and gradients on the device (``Decoder.fcn_grad`` -> ldpc_fcn_grad): the windows
        ``inputs`` [N, win+1] f32 / ``labels`` [N] uint8 / per-sample ``weight`` [N] f32 are device tensors, ``index``
        [B] int32 names the rows of the batch (valid by the caller's construction; default: every row).  Returns (loss
        as a float, [dW1, dW2] float32 in the Keras shapes, acc = (sum of the weights where the prediction is right, sum
        of the weights), counts = (S, F1, F2)).  The l2 kernel_regularizer the reference declares on ``dense1`` never
        reaches its hand-written loss (model.losses is not added there), so it has no part here.  One synchronisation."""
        from ._osd_common import _dec
        out = _dec().fcn_grad(inputs, labels, self.packed(), self.sliding_win_width, penalty, weight=weight, index=index,
                              check_index=False)
        both = torch.cat([out["loss_sum"], out["acc"], out["grad"]]).cpu().numpy()
        d = self.input_width
        grads = [both[3:3 + d * d].reshape(d, d).astype(F32), both[3 + d * d:].reshape(d, 2).astype(F32)]
        return float(both[0]), grads, (float(both[1]), float(both[2])), tuple(int(c) for c in out["counts"].cpu().numpy())

    def __call__(self, inputs):
        x = np.asarray(inputs, dtype=F32).reshape(-1, self.input_width)
        with np.errstate(over="ignore", invalid="ignore"):     # (windows of empty blocks hold inf)
            z = _seq_matmul(_seq_matmul(x, self.dense1), self.dense2)
            m = np.where(z[:, 1] > z[:, 0], z[:, 1], z[:, 0])
            e = np.exp(z - m[:, None]).astype(F32)
        return (e / (e[:, 0:1] + e[:, 1:2])).astype(F32)


class rnn_one:   # noqa: N801
    """The RNN variants of the reference (nn_net.py) are not mirrored."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError("rnn_one: only the bit-wise CNN (conv_bitwise) is mirrored")


class rnn_two:   # noqa: N801
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("rnn_two: only the bit-wise CNN (conv_bitwise) is mirrored")
