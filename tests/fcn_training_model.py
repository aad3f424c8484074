"""Float64 NumPy restatements of the sliding-window classifier's training stage, for the tests.

windows:       reform_inputs (interval_boundary.py:224-249 of the reference's training stage), literally: for window position
               i = 0 .. nblk-win the window record[i:i+win]; label 1 when min(window) == min(record) and the record's
               locate_phase is not -1; input the ascending window then float(i); window-major (row i*R + r).
class_weights: shuffle_data (predict_phase.py:113-119): N / (num_classes * count_c), float32, one weight per sample.
loss_grad:     calculation_loss (:121-135) and its gradient by the chain rule, written out:
                 s_b = sw_b pen_b,  pen_b = penalty where p0 < p1 and y_b = 0, else 1 (a constant: it sits under a where)
                 loss = sum_b -s_b log max(p[b][y_b], 1e-30)
                 dloss/dz_c = g_c = s_b (p_c - [c == y_b]) where p[b][y_b] >= 1e-30, else 0
                 (softmax Jacobian times -1/p_y; the maximum passes no gradient below the floor)
                 z = (x W1) W2:  dW1 = x^T (g W2^T) = m W2^T,  dW2 = (x W1)^T g = W1^T m,  m = x^T g.
               With ``p`` given (the kernel's own float32 probabilities) the forward pass is not recomputed, so the only
               differences left to a float64 implementation are the roundings of its sums: the masses returned are the L1
               sums those roundings are relative to.
replay_sliding: the lazy loop of sliding_osd (ordered_statistics_decoding.py:187-218 of the test stage) on a table of
               p1 per window position.
"""
import numpy as np

F32 = np.float32
FLOOR = float(np.float32(1e-30))


def windows(records, success, win):
    records = np.asarray(records, dtype=F32)
    success = np.asarray(success).astype(bool)
    R, nblk = records.shape
    rows = records.astype(np.float64).tolist()      # (float32 values are exact in float64: the comparisons are the same)
    row_min = [min(row) for row in rows] if nblk else []
    inputs, labels = [], []
    for i in range(nblk - win + 1):
        for r in range(R):
            window = rows[r][i:i + win]
            labels.append(1 if (min(window) == row_min[r] and success[r]) else 0)
            inputs.append(sorted(window) + [float(i)])
    return np.asarray(inputs, dtype=F32).reshape(-1, win + 1), np.asarray(labels, dtype=np.uint8)


def class_weights(labels):
    labels = np.asarray(labels).astype(np.int64)
    classes = np.unique(labels)
    n, nc = F32(len(labels)), F32(len(classes))
    w = {int(c): n / (nc * F32(np.sum(labels == c))) for c in classes}
    return np.asarray([w[int(y)] for y in labels], dtype=F32), w


def forward64(x, W1, W2):
    z = np.asarray(x, np.float64) @ np.asarray(W1, np.float64) @ np.asarray(W2, np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def loss_grad(x, y, sw, W1, W2, penalty, p=None):
    x = np.asarray(x, np.float64)
    y = np.asarray(y).astype(np.int64)
    B = len(y)
    sw = np.ones(B) if sw is None else np.asarray(sw, np.float64)
    W1, W2 = np.asarray(W1, np.float64), np.asarray(W2, np.float64)
    p = forward64(x, W1, W2) if p is None else np.asarray(p, np.float64)
    pred = (p[:, 0] < p[:, 1]).astype(np.int64)
    s = sw * np.where((pred == 1) & (y == 0), float(penalty), 1.0)
    py = p[np.arange(B), y]
    terms = -s * np.log(np.maximum(py, FLOOR))
    onehot = np.stack([y == 0, y == 1], axis=1).astype(np.float64)
    g = np.where((py >= FLOOR)[:, None], s[:, None] * (p - onehot), 0.0)
    m = x.T @ g                                   # [D, 2]
    abs_m = np.abs(x).T @ np.abs(g)
    return dict(loss=float(terms.sum()), dW1=m @ W2.T, dW2=W1.T @ m, m=m, g=g, p=p, pred=pred,
                acc=(float(np.sum(sw[pred == y])), float(np.sum(sw))),
                counts=(int(np.sum(y == pred)), int(np.sum(y > pred)), int(np.sum(y < pred))),
                abs_loss=float(np.abs(terms).sum()), abs_acc=float(np.abs(sw).sum()),
                mass_dW1=abs_m @ np.abs(W2).T, mass_dW2=np.abs(W1).T @ abs_m)


def pack(dW1, dW2):
    return np.concatenate([np.asarray(dW1).ravel(), np.asarray(dW2).ravel()])


def replay_sliding(block_min, p1, win, soft_margin):
    """One frame: ``p1[k]`` is the classifier's output on window k.  -> (deep_limit, global_min)."""
    block_min = np.asarray(block_min, dtype=F32)
    global_min = min(block_min[:win])
    deep_limit = win
    for k in range(len(block_min) - win + 1):
        deep_limit = k + win
        if k != 0 and block_min[win + k - 1] > global_min:
            continue
        global_min = min(global_min, min(block_min[k:k + win]))
        if float(p1[k]) > soft_margin:
            break
    return deep_limit, F32(global_min)
