"""NMS training on the GPU without TensorFlow (recipe step 2, LDPC_128/Ldpc_128_training).

The loss of ``Decoding_model`` and its gradient come from one HIP launch (``Decoder.nms_grad``, ldpc_nms_train_grad);
what remains on the host acts on 1-3 scalars and is written out here in NumPy:

- ``NMSLoss``: a ``torch.autograd.Function`` over the kernel, so any torch optimiser can train the effective factors;
- ``stored_grads``: the gradient of the STORED weights (Decoder_Layer.build, ms_decoder_dense.py:74-91) by the chain
  rule through softplus (d softplus(w) = sigmoid(w)); NMS-1/2/3 share one alpha over all iterations, so its gradient is
  the sum over t;
- ``LegacyAdam``, ``ExponentialDecay``, ``clip_by_norm``: the optimiser of training_stage.py:20 and globalmap.py:96-101
  (tf.keras.optimizers.legacy.Adam, ExponentialDecay(0.01, 500, 0.95, staircase=True), tf.clip_by_norm(g, 5)).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .weights import softplus32

STORED_NAMES = {            # Decoder_Layer.build: the trainable variables of each type, in creation order
    "NMS-1": ("shared_check_weight",),
    "NMS-2": ("shared_bit_weight", "shared_check_weight"),
    "NMS-3": ("shared_bit_weight1", "shared_bit_weight2", "shared_check_weight"),
}


def sigmoid32(x):
    x = np.float32(x)
    return np.float32(1.0) / (np.float32(1.0) + np.float32(np.exp(-x)))


def effective(decoder_type, stored):
    """stored weights {name: float32} -> effective (alpha, w_in, w_out) (ms_decoder_dense.py:121-131, :205-206, :219-224)."""
    alpha = softplus32(stored["shared_check_weight"])
    w_in = w_out = np.float32(1.0)
    if decoder_type == "NMS-2":
        w_in = w_out = softplus32(stored["shared_bit_weight"])
    elif decoder_type == "NMS-3":
        w_in, w_out = softplus32(stored["shared_bit_weight1"]), softplus32(stored["shared_bit_weight2"])
    elif decoder_type != "NMS-1":
        raise NotImplementedError(f"decoder type '{decoder_type}': training covers NMS-1/2/3 (NMS-r is out of scope)")
    return alpha, w_in, w_out


def stored_grads(decoder_type, stored, grad_eff):
    """grad_eff = [dL/dalpha_0..T-1, dL/dw_in, dL/dw_out] (float64) -> {stored name: dL/dw} by the chain rule."""
    g = np.asarray(grad_eff, dtype=np.float64)
    T = g.shape[0] - 2
    sig = lambda name: float(sigmoid32(stored[name]))              # noqa: E731
    out = {"shared_check_weight": sig("shared_check_weight") * float(math.fsum(g[:T]))}
    if decoder_type == "NMS-2":
        out["shared_bit_weight"] = sig("shared_bit_weight") * (g[T] + g[T + 1])
    elif decoder_type == "NMS-3":
        out["shared_bit_weight1"] = sig("shared_bit_weight1") * g[T]
        out["shared_bit_weight2"] = sig("shared_bit_weight2") * g[T + 1]
    return out


class NMSLoss(torch.autograd.Function):
    """loss = sum over frames, iterations and bits of the reference's cross entropy (ms_decoder_dense.py:210-215).

    ``NMSLoss.apply(llr, label_bits, alpha, w_in, w_out, decoder)``: llr [B, n] f32 and label_bits [B, words] int64 on the
    decoder's device; alpha a tensor [T] of effective factors, w_in / w_out 0-d tensors.  The backward pass returns the
    kernel's gradient for alpha, w_in and w_out, None for the channel values and labels (no gradient flows into them)."""

    @staticmethod
    def forward(ctx, llr, label_bits, alpha, w_in, w_out, decoder):
        T = int(alpha.shape[0])
        a = alpha.detach().to("cpu", torch.float32).numpy()
        res = decoder.nms_grad(llr, label_bits, T, a, float(w_in), float(w_out), want_loss=False, want_grad=False,
                               want_sums=True)
        ctx.save_for_backward(res["grad_sum"])
        ctx.dtypes = (alpha.dtype, w_in.dtype, w_out.dtype)
        ctx.devices = (alpha.device, w_in.device, w_out.device)
        return res["loss_sum"][0].to(alpha.device, alpha.dtype)

    @staticmethod
    def backward(ctx, g):
        (gs,) = ctx.saved_tensors
        T = gs.shape[0] - 2
        g = g.to(gs.device, torch.float64)
        ga, gi, go = gs[:T] * g, gs[T] * g, gs[T + 1] * g
        (da, di, do), (va, vi, vo) = ctx.dtypes, ctx.devices
        return None, None, ga.to(va, da), gi.to(vi, di), go.to(vo, do), None


def clip_by_norm(g, clip_norm=5.0):
    """tf.clip_by_norm for one variable: g * clip / max(||g||_2, clip)."""
    g = np.asarray(g, dtype=np.float32)
    l2 = np.float32(np.sqrt(np.sum(g * g, dtype=np.float32)))
    if l2 <= np.float32(clip_norm):
        return g
    return (g * np.float32(clip_norm) / l2).astype(np.float32)


class ExponentialDecay:
    """tf.keras.optimizers.schedules.ExponentialDecay: lr0 * rate ** (step / steps), floor of the ratio when staircase."""

    def __init__(self, initial_learning_rate=0.01, decay_steps=500, decay_rate=0.95, staircase=True):
        self.lr0, self.steps, self.rate, self.staircase = float(initial_learning_rate), int(decay_steps), float(decay_rate), staircase

    def __call__(self, step):
        p = float(step) / self.steps
        if self.staircase:
            p = math.floor(p)
        return np.float32(self.lr0 * self.rate ** p)


class LegacyAdam:
    """tf.keras.optimizers.legacy.Adam (epsilon 1e-7, no amsgrad) on float32 scalars:
    m = b1 m + (1 - b1) g,  v = b2 v + (1 - b2) g^2,  lr_t = lr sqrt(1 - b2^t) / (1 - b1^t),  w -= lr_t m / (sqrt(v) + eps)
    with t the 1-based count of applied steps; ``learning_rate`` is a number or a schedule called with t - 1."""

    def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7):
        self.learning_rate, self.b1, self.b2, self.eps = learning_rate, np.float32(beta_1), np.float32(beta_2), np.float32(epsilon)
        self.iterations = 0
        self.m, self.v = {}, {}

    def lr(self, step):
        return np.float32(self.learning_rate(step) if callable(self.learning_rate) else self.learning_rate)

    def apply_gradients(self, grads_and_vars):
        """grads_and_vars: iterable of (gradient, name, params dict); params[name] is updated in place (float32)."""
        lr = self.lr(self.iterations)
        t = np.float32(self.iterations + 1)
        one = np.float32(1.0)
        lr_t = np.float32(lr * np.float32(np.sqrt(one - self.b2 ** t)) / (one - self.b1 ** t))
        for g, name, params in grads_and_vars:
            g = np.asarray(g, dtype=np.float32)
            m = self.m.get(name, np.zeros_like(g))
            v = self.v.get(name, np.zeros_like(g))
            m = (self.b1 * m + (one - self.b1) * g).astype(np.float32)
            v = (self.b2 * v + (one - self.b2) * g * g).astype(np.float32)
            self.m[name], self.v[name] = m, v
            w = np.asarray(params[name], dtype=np.float32)
            params[name] = (w - lr_t * m / (np.sqrt(v) + self.eps)).astype(np.float32)
        self.iterations += 1
