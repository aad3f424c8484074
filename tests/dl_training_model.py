"""Float64 NumPy model of the DL-OSD training stage, for the tests.

The gradient (``cnn_loss_grad``) is what ``ldpc_dia_cnn_grad`` rests on: conv_bitwise has no activation, so
out = bias + sum_r E[r] x[r]; with g = dloss/dout = y - sigmoid(-out) the batch gradient is the back-propagation of the
network at the single pseudo-input m[r] = sum_{f,v} g x[r] with upstream gradient 1 (``backprop_at``), and
dloss/dbias = sum g.  ``torch_loss_grad`` is the same loss through torch autograd, with no use of that identity.

The statistics (``mrb_bit_counts``, ``frame_mrb``, ``pattern_word``, ``stage_statistics``) restate
DL_Training_serial/nn_training.py:323-333 and :418-575 of the reference one frame at a time: a stable ascending sort of
|value| (ties to the lower index), ``Code.gf2elim`` on the reordered H, the recorded column exchanges replayed on
0..n-1.
"""
import math
from collections import Counter

import numpy as np

F64 = np.float64
U = 2.0 ** -24      # float32 unit roundoff
# Length of the float32 chain behind one product g x[r] of the training kernel (and behind one loss term): the sigmoid
# 1 / (1 + exp(-t)) -- or log1p(exp(-|z|)) -- counted as 8, as tests/test_gpu_nms_train.py counts a transcendental chain,
# plus the product (the loss term: plus its one addition).  Selecting the sign of g and negating out are exact; every sum
# is float64, and 3e6 terms of float64 rounding (3e6 * 2^-53 = 4e-10) are nothing next to K u = 5e-7.
K = 8 + 1


def _conv_fwd(x, w):
    """x [P, cin], w [3][cin][cout] -> [P-2, cout]."""
    P = x.shape[0]
    return sum(x[t:P - 2 + t] @ w[t] for t in range(3))


def _conv_bwd(x, w, dy):
    """-> (dw, dx) of y = _conv_fwd(x, w) under upstream dy."""
    P = x.shape[0]
    dw = np.stack([x[t:P - 2 + t].T @ dy for t in range(3)])
    dx = np.zeros_like(x)
    for t in range(3):
        dx[t:P - 2 + t] += dy @ w[t].T
    return dw, dx


def forward64(x, ws):
    """x [N, L] -> out [N] in float64 (any summation order: the inputs of the exact-forward test make every order exact)."""
    w1, w2, w3, wd, b = [np.asarray(w, F64) for w in ws]
    h = np.asarray(x, F64)[:, :, None]
    for w in (w1, w2, w3):
        P = h.shape[1]
        h = sum(h[:, t:P - 2 + t] @ w[t] for t in range(3))
    return h.reshape(h.shape[0], -1) @ wd[:, 0] + b[0]


def backprop_at(m, ws):
    """Gradient of (out - bias) at the input m [L] with respect to (w1, w2, w3, wd): [dw1, dw2, dw3, dwd]."""
    w1, w2, w3, wd, _ = [np.asarray(w, F64) for w in ws]
    x0 = np.asarray(m, F64)[:, None]
    c1 = _conv_fwd(x0, w1)
    c2 = _conv_fwd(c1, w2)
    c3 = _conv_fwd(c2, w3)
    dwd = c3.reshape(-1, 1).copy()
    dw3, dc2 = _conv_bwd(c2, w3, wd.reshape(-1, 2))
    dw2, dc1 = _conv_bwd(c1, w2, dc2)
    dw1, _ = _conv_bwd(x0, w1, dc1)
    return [dw1, dw2, dw3, dwd]


def loss_terms(out, y):
    """TF's stable sigmoid_cross_entropy_with_logits at logits -out, and g = dloss/dout, both float64 per element."""
    out, y = np.asarray(out, F64), np.asarray(y, F64)
    z = -out
    with np.errstate(over="ignore"):
        term = np.maximum(z, 0) - z * y + np.log1p(np.exp(-np.abs(z)))
        q = np.where(y > 0, out, z)
        s = 1.0 / (1.0 + np.exp(-q))
    return term, np.where(y > 0, s, -s)


def cnn_loss_grad(rows, labels, ws, out=None, chunk=4096):
    """rows [F, L, n], labels [F, n] 0/1 -> dict(loss, grads [5 arrays], m [L], sg, and the masses of the rounding bound:
    abs_m[r] = sum |g x[r]|, abs_g = sum |g|, abs_loss = sum |term|).  ``out`` [F, n]: the refined values to take the
    loss at (the kernel's own float32 ones); None = the float64 forward.  Frames are processed ``chunk`` at a time."""
    F, L, n = rows.shape
    m, abs_m = np.zeros(L), np.zeros(L)
    sg = abs_g = loss = abs_loss = 0.0
    for a in range(0, F, chunk):
        x = np.asarray(rows[a:a + chunk], F64).transpose(0, 2, 1).reshape(-1, L)
        o = forward64(x, ws) if out is None else np.asarray(out[a:a + chunk], F64).reshape(-1)
        term, g = loss_terms(o, np.asarray(labels[a:a + chunk]).reshape(-1))
        gx = g[:, None] * x
        m += gx.sum(0)
        abs_m += np.abs(gx).sum(0)
        sg += g.sum()
        abs_g += np.abs(g).sum()
        loss += term.sum()
        abs_loss += np.abs(term).sum()
    grads = backprop_at(m, ws) + [np.array([sg])]
    return dict(loss=loss, grads=grads, m=m, sg=sg, abs_m=abs_m, abs_g=abs_g, abs_loss=abs_loss)


def filter_derivatives(L, ws):
    """dE[r]/dtheta for every r: a list over r of [dw1, dw2, dw3, dwd] (the gradient at the r-th unit vector)."""
    return [backprop_at(np.eye(L)[r], ws) for r in range(L)]


def grad_masses(L, ws, abs_m, abs_g):
    """Per weight theta: sum_r |dE[r]/dtheta| abs_m[r] (bias: abs_g), the L1 mass of the products that reach theta."""
    dE = filter_derivatives(L, ws)
    return [sum(np.abs(dE[r][i]) * abs_m[r] for r in range(L)) for i in range(4)] + [np.array([abs_g])]


def pack(arrays):
    return np.concatenate([np.asarray(a, F64).ravel() for a in arrays])


def torch_loss_grad(rows, labels, ws):
    """The loss and its gradient by torch float64 autograd: conv1d x3 -> flatten position-major -> dense ->
    binary_cross_entropy_with_logits(-out, y, 'sum')."""
    import torch
    import torch.nn.functional as Fn
    F, L, n = rows.shape
    P = [torch.tensor(np.asarray(w, F64), requires_grad=True) for w in ws]
    x = torch.tensor(np.asarray(rows, F64).transpose(0, 2, 1).reshape(-1, L))
    h = x[:, None, :]
    for w in P[:3]:
        h = Fn.conv1d(h, w.permute(2, 1, 0))     # Keras [tap][in][out] -> torch [out][in][tap]
    h = h.permute(0, 2, 1).reshape(x.shape[0], -1)
    out = (h @ P[3])[:, 0] + P[4]
    y = torch.tensor(np.asarray(labels, F64).reshape(-1))
    loss = Fn.binary_cross_entropy_with_logits(-out, y, reduction="sum")
    grads = [g.numpy() for g in torch.autograd.grad(loss, P)]
    return float(loss.detach()), grads, out.detach().numpy().reshape(F, n)


# ------------------------------------------------------------------------------------------- NumPy Adam (host replay)
def adam_replay_step(ws, grads, state, lr, clip=5e2, b1=0.9, b2=0.999, eps=1e-7):
    """One step of the training loop's host part, restated: per-variable clip_by_norm, then legacy Adam in float32.
    ``state``: dict(t, m, v), updated in place; returns the new float32 weights."""
    f32 = np.float32
    state["t"] += 1
    t = f32(state["t"])
    lr_t = f32(f32(lr) * f32(np.sqrt(f32(1) - f32(b2) ** t)) / (f32(1) - f32(b1) ** t))
    new = []
    for i, (w, g) in enumerate(zip(ws, grads)):
        g = np.asarray(g, f32)
        l2 = f32(np.sqrt(np.sum(g * g, dtype=f32)))
        if l2 > f32(clip):
            g = (g * f32(clip) / l2).astype(f32)
        m = (f32(b1) * state["m"][i] + (f32(1) - f32(b1)) * g).astype(f32)
        v = (f32(b2) * state["v"][i] + (f32(1) - f32(b2)) * g * g).astype(f32)
        state["m"][i], state["v"][i] = m, v
        new.append((np.asarray(w, f32) - lr_t * m / (np.sqrt(v) + f32(eps))).astype(f32))
    return new


# ------------------------------------------------------------------------------------------------------ statistics
def _stable_order(values):
    return np.argsort(np.abs(np.asarray(values)), kind="stable")


def mrb_bit_counts(values, labels, k):
    """evaluate_MRB_bit (:323-333): Counter of the number of hard-decision errors among each frame's k most reliable bits."""
    cnt = Counter()
    for x, lab in zip(np.asarray(values), np.asarray(labels)):
        o = _stable_order(x)[-k:]
        cnt[int(np.sum((x[o] <= 0).astype(int) != lab[o].astype(int)))] += 1
    return cnt


def frame_mrb(code, x):
    """stat_pro_osd (:549-575) for one frame -> (updated_MRB [k] positions in the reliability order, swap count)."""
    n, k = code.check_matrix_column, code.k
    o = _stable_order(x)
    H = np.ascontiguousarray(np.asarray(code.H)[:, o]).astype(np.int32)
    _, record = code.gf2elim(H)
    index_order = np.arange(n)
    for a, b in record:
        index_order[a], index_order[b] = index_order[b], index_order[a]
    mrb = index_order[-k:]
    return mrb, int(np.sum(mrb < n - k))


def pattern_word(x, lab, mrb, boundary):
    """evaluate_MRB_pattern (:524-546) for one frame: errors per MRB segment, joined with commas."""
    o = _stable_order(x)
    pos = o[np.sort(mrb)]
    diff = ((np.asarray(x)[pos] <= 0).astype(int) != np.asarray(lab)[pos].astype(int)).astype(int)
    return ",".join(str(int(diff[boundary[i]:boundary[i + 1]].sum())) for i in range(len(boundary) - 1))


def stage_statistics(code, batches, seg_sizes, boundary):
    """The six pickled objects of Training_NN's verification pass (:418-498) from ``batches`` = [(first row [F, n],
    last row, refined values, labels)], plus the mean swap count."""
    k = code.k
    size, swaps = 0, []
    d0, dT, dr, pattern = Counter(), Counter(), Counter(), Counter()
    for first, last, refined, labels in batches:
        size += len(refined)
        d0.update(mrb_bit_counts(first, labels, k))
        dT.update(mrb_bit_counts(last, labels, k))
        dr.update(mrb_bit_counts(refined, labels, k))
        for x, lab in zip(refined, labels):
            mrb, ns = frame_mrb(code, x)
            swaps.append(ns)
            pattern[pattern_word(x, lab, mrb, boundary)] += 1
    merged = Counter()
    for key, value in pattern.items():
        merged[sum(int(d) for d in key.split(","))] += value
    ratio = Counter({key: value / math.prod(math.comb(int(s), int(d)) for s, d in zip(seg_sizes, key.split(",")))
                     for key, value in pattern.items()})
    srt = lambda c: dict(sorted(c.items()))      # noqa: E731
    return dict(objects=(size, srt(d0), srt(dT), srt(dr), merged, ratio), swaps=swaps, pattern=pattern)
