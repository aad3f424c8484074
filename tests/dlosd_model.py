"""NumPy restatements of the DL-OSD stage's networks in the pinned float order of include/ldpc_osd.h, for the tests.

cnn_forward: conv_bitwise.call (nn_net.py:184-197) on retest rows [F, L, n]; every conv output a sequential f32 sum over
the flattened (tap, in-channel) index, tap-major, from the first product; the dense output the sequential sum over the
flattened (position, channel) index from the first product, then + bias.
classifier_p1: Predict_outlier_light (nn_net.py:136-149) on [B, win+1]: h = x.W1, z = h.W2 (sequential sums from the
first product), p1 = e1 / (e0 + e1), e_c = exp(z_c - max z).
"""
import numpy as np

F32 = np.float32


def cnn_sizes(L):
    return (3, 1, 8), (3, 8, 4), (3, 4, 2), (2 * (L - 6), 1), (1,)


def random_cnn_weights(rng, L, scale=0.5):
    return [(rng.standard_normal(s) * scale).astype(F32) for s in cnn_sizes(L)]


def pack_cnn(ws):
    return np.concatenate([np.asarray(w, F32).ravel() for w in ws])


def _conv(x, w):
    """x [B, P, cin], w [3][cin][cout] -> [B, P-2, cout], sequential over (tap, cin)."""
    P, cin = x.shape[1], x.shape[2]
    out = None
    for t in range(3):
        for i in range(cin):
            term = x[:, t:P - 2 + t, i:i + 1] * w[t, i][None, None, :]
            out = term if out is None else out + term
    return out


def cnn_forward(rows, ws):
    """rows [F, L, n] f32 -> [F, n] f32."""
    w1, w2, w3, wd, b = [np.asarray(w, F32) for w in ws]
    F, L, n = rows.shape
    x = np.ascontiguousarray(np.asarray(rows, F32).transpose(0, 2, 1)).reshape(F * n, L, 1)
    c = _conv(_conv(_conv(x, w1), w2), w3)          # [F*n, L-6, 2]
    flat = c.reshape(F * n, -1)
    acc = flat[:, 0] * wd[0, 0]
    for j in range(1, flat.shape[1]):
        acc = acc + flat[:, j] * wd[j, 0]
    return (acc + b[0]).reshape(F, n).astype(F32)


def _seq(x, w):
    acc = x[:, 0:1] * w[0][None, :]
    for i in range(1, w.shape[0]):
        acc = acc + x[:, i:i + 1] * w[i][None, :]
    return acc


def classifier_logits(x, w1, w2):
    return _seq(_seq(np.asarray(x, F32), np.asarray(w1, F32)), np.asarray(w2, F32))


def classifier_p1(x, w1, w2):
    z = classifier_logits(x, w1, w2)
    m = np.where(z[:, 1] > z[:, 0], z[:, 1], z[:, 0])
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(z - m[:, None]).astype(F32)
        return (e[:, 1] / (e[:, 0] + e[:, 1])).astype(F32)


def random_fcn_weights(rng, win, scale=0.05):
    d = win + 1
    return (rng.standard_normal((d, d)) * scale).astype(F32), (rng.standard_normal((d, 2)) * scale).astype(F32)


def stopping_fcn_weights(win, per_block=0.35, per_metric=0.01):
    """A classifier whose logit difference grows with the window index and falls with the window's metrics:
    z1 - z0 = per_block * k - per_metric * sum(window), so the stop fires at a depth that depends on the frame."""
    d = win + 1
    w1 = np.eye(d, dtype=F32)
    w2 = np.zeros((d, 2), F32)
    w2[:win, 1] = -per_metric
    w2[win, 1] = per_block
    return w1, w2


class Classifier:
    """``fcn`` for np_oracle.sliding_window_decide; records every p1 it returns with its logit difference."""

    def __init__(self, w1, w2):
        self.w1, self.w2 = np.asarray(w1, F32), np.asarray(w2, F32)
        self.p1, self.dz = [], []

    def __call__(self, x):
        with np.errstate(invalid="ignore", over="ignore"):
            p = classifier_p1(x, self.w1, self.w2)
            z = classifier_logits(x, self.w1, self.w2)
            self.dz.extend((z[:, 1].astype(np.float64) - z[:, 0]).tolist())
        self.p1.extend(p.tolist())
        return np.stack([1 - p, p], axis=1)

    def near(self, margin, tol=1e-6):
        """Decisions whose p1 lies within ``tol`` of the margin, where an ulp of exp could move it across.  A logit
        difference beyond 110 (or NaN / inf) saturates p1 to 0 or 1 exactly in any f32 exp (exp(-110) is below the
        smallest denormal), so those are not counted."""
        return sum(1 for p, d in zip(self.p1, self.dz) if abs(p - margin) < tol and np.isfinite(d) and abs(d) <= 110)

    def packed(self):
        return np.concatenate([self.w1.ravel(), self.w2.ravel()]).astype(F32)
