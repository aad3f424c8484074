"""Test helper: float64 reverse-mode restatement of the NMS training gradient on the edge list.

The forward pass runs in float32 in the generic kernel's order (and is checked against ``np_oracle.nms_dense``); every
decision the gradient depends on -- which edges top_k picks (ties to the lower variable index), which edges receive m1
and which m2 (an edge tied with m1 receives m2, so its gradient goes to the m2 edge), which checks hold a zero
vc (S = 0), which magnitudes the clip passes -- is taken from those float32 values.  The backward pass then runs in
float64 under TensorFlow's rules for the reference's ops (ldpc_nms_train.hip spells them out).

``grad_model`` returns per frame: loss, grad [T+2] = dL/dalpha_0..T-1, dL/dw_in, dL/dw_out, and mass [T+2], the same
reverse sweep with every term replaced by its absolute value (the L1 contribution mass a rounding bound scales with).
"""
import numpy as np

from oracle import np_oracle

F32 = np.float32


class Graph:
    """Padded edge lists of H: checks [m, dc] -> variable (pad -1), variables [n, dv] -> (check, row position) (pad -1)."""

    def __init__(self, H):
        H = np.asarray(H)
        self.m, self.n = H.shape
        rows = [np.flatnonzero(H[c]) for c in range(self.m)]
        self.deg = np.array([len(r) for r in rows])
        dc = max(1, self.deg.max())
        self.chk_var = np.full((self.m, dc), -1, np.int64)
        for c, r in enumerate(rows):
            self.chk_var[c, :len(r)] = r
        cols = [[(c, int(np.flatnonzero(rows[c] == v)[0])) for c in np.flatnonzero(H[:, v])] for v in range(self.n)]
        dv = max(1, max(len(x) for x in cols))
        self.var_chk = np.full((self.n, dv), -1, np.int64)
        self.var_pos = np.full((self.n, dv), -1, np.int64)
        for v, lst in enumerate(cols):
            for q, (c, j) in enumerate(lst):
                self.var_chk[v, q], self.var_pos[v, q] = c, j
        self.valid = self.chk_var >= 0

    def var_sum(self, x):
        """[B, m, dc] -> [B, n]: per variable, its edges in ascending check order (the kernel's order)."""
        B = x.shape[0]
        acc = np.zeros((B, self.n), x.dtype)
        for q in range(self.var_chk.shape[1]):
            ok = self.var_chk[:, q] >= 0
            val = x[:, np.maximum(self.var_chk[:, q], 0), np.maximum(self.var_pos[:, q], 0)]
            acc = np.where(ok[None], acc + val, acc).astype(x.dtype)
        return acc

    def gather(self, x):
        """[B, n] -> [B, m, dc] (0 on padding)."""
        return np.where(self.valid[None], x[:, np.maximum(self.chk_var, 0)], 0).astype(x.dtype)


def forward32(g, y, T, alpha, w_in, w_out):
    """float32 forward in the kernel's order; returns (outs [y, soft_1..soft_T], per-iteration records)."""
    y = np.asarray(y, F32)
    B = y.shape[0]
    alpha = np.broadcast_to(np.asarray(alpha, F32), (T,))
    w_in, w_out = F32(w_in), F32(w_out)
    cv = np.zeros((B, g.m, g.chk_var.shape[1]), F32)
    outs, recs = [y], []
    inf = F32(np.inf)
    for t in range(T):
        tot = (g.var_sum(cv) + y * w_in).astype(F32)
        vc = np.where(g.valid[None], g.gather(tot) - cv, F32(0)).astype(F32)
        a = np.where(g.valid[None], np.abs(vc), inf).astype(F32)
        srt = np.sort(a, axis=2)
        m1 = srt[:, :, 0:1]
        m2 = srt[:, :, 1:2] if a.shape[2] > 1 else np.full_like(m1, inf)
        m1s = (alpha[t] * np.minimum(m1, F32(1e30))).astype(F32)
        m2s = np.where(m1 == 0, F32(0), alpha[t] * np.minimum(m2, F32(1e30))).astype(F32)
        mag = np.where(a > m1, m1s, m2s).astype(F32)
        sbit = (vc.view(np.uint32) >> 31) & np.where(g.valid[None], 1, 0).astype(np.uint32)
        par = np.bitwise_xor.reduce(sbit, axis=2, keepdims=True)
        neg = (par ^ sbit).astype(bool)
        cv = np.where(g.valid[None], np.where(neg, -mag, mag), F32(0)).astype(F32)
        # decisions: top_k on the clipped magnitudes, ties to the lower row position
        cl = np.minimum(a, F32(1e30))
        cl = np.where(g.valid[None], cl, inf)
        j1 = np.argmin(cl, axis=2)
        cl2 = cl.copy()
        np.put_along_axis(cl2, j1[..., None], inf, axis=2)
        j2 = np.argmin(cl2, axis=2)
        has2 = (g.deg >= 2)[None]
        recs.append(dict(vc=vc, j1=j1, j2=j2, has2=np.broadcast_to(has2, j1.shape), zero=(m1[..., 0] == 0),
                         le=g.valid[None] & ~(a > m1)))     # the edges that received m2 (m1 edge and its ties)
        outs.append((g.var_sum(cv) + w_out * y).astype(F32))
    return outs, recs


def grad_model(H, y, bits, T, alpha, w_in=1.0, w_out=1.0, check_dense=True):
    """-> dict(loss [B], grad [B, T+2], mass [B, T+2], outs) in float64 (outs: the float32 posteriors)."""
    g = Graph(H)
    y = np.asarray(y, F32)
    bits = np.asarray(bits, np.float64)
    B = y.shape[0]
    alpha32 = np.broadcast_to(np.asarray(alpha, F32), (T,))
    outs, recs = forward32(g, y, T, alpha32, w_in, w_out)
    if check_dense:
        dense = np_oracle.nms_dense(y, np.asarray(H), T, alpha32, w_in, w_out)
        for t in range(T + 1):
            assert np.array_equal(outs[t], dense[t]), f"edge-list forward differs from nms_dense at t={t}"
    y64 = y.astype(np.float64)
    loss = np.zeros(B)
    gsoft = []
    for t in range(1, T + 1):
        x = -outs[t].astype(np.float64)
        loss += (np.maximum(x, 0) - x * bits + np.log1p(np.exp(-np.abs(x)))).sum(axis=1)
        s = outs[t].astype(np.float64)       # z - sigmoid(-s) without cancellation: sigmoid(s) for z = 1, -sigmoid(-s) for z = 0
        with np.errstate(over="ignore"):     # exp(1e30-scale) = inf gives the limit, 0 or 1
            gsoft.append(np.where(bits == 1, 1.0 / (1.0 + np.exp(-s)), -1.0 / (1.0 + np.exp(s))))
    grad = np.zeros((B, T + 2))
    mass = np.zeros((B, T + 2))
    shape = (B, g.m, g.chk_var.shape[1])
    gcv, acv = np.zeros(shape), np.zeros(shape)
    bidx = np.arange(B)[:, None]
    cidx = np.arange(g.m)[None, :]
    for t in range(T - 1, -1, -1):
        r = recs[t]
        gs = gsoft[t]
        gcv = gcv + g.gather(gs)
        acv = acv + g.gather(np.abs(gs))
        grad[:, T + 1] += (gs * y64).sum(axis=1)
        mass[:, T + 1] += np.abs(gs * y64).sum(axis=1)
        vc = r["vc"]
        sb = ((vc.view(np.uint32) >> 31) & 1).astype(np.int64) * g.valid[None]
        par = np.bitwise_xor.reduce(sb, axis=2, keepdims=True)
        s = np.where((sb ^ par) == 1, -1.0, 1.0) * g.valid[None]
        live = ~r["zero"]
        G = gcv * s
        j1, j2 = r["j1"], r["j2"]
        le = r["le"]
        G2 = np.where(le, G, 0).sum(axis=2)
        G1 = np.where(le, 0, G).sum(axis=2)
        A2 = np.where(le, acv, 0).sum(axis=2)
        A1 = np.where(le, 0, acv).sum(axis=2)
        a = np.abs(vc).astype(np.float64)
        r1 = a[bidx, cidx, j1]
        r2 = np.where(r["has2"], a[bidx, cidx, j2], np.inf)
        m1c, m2c = np.minimum(r1, 1e30), np.minimum(r2, 1e30)
        grad[:, t] = np.where(live, m1c * G1 + m2c * G2, 0).sum(axis=1)
        mass[:, t] = np.where(live, m1c * A1 + m2c * A2, 0).sum(axis=1)
        al = float(alpha32[t])
        sgn = np.where(vc < 0, -1.0, 1.0)
        gvc, avc = np.zeros(shape), np.zeros(shape)
        ok1 = live & (r1 <= 1e30)
        ok2 = live & r["has2"] & (r2 <= 1e30)
        gvc[bidx, cidx, j1] = np.where(ok1, sgn[bidx, cidx, j1] * al * G1, 0)
        avc[bidx, cidx, j1] = np.where(ok1, abs(al) * A1, 0)
        j2c = np.where(r["has2"], j2, j1)
        gvc[bidx, cidx, j2c] += np.where(ok2, sgn[bidx, cidx, j2c] * al * G2, 0)
        avc[bidx, cidx, j2c] += np.where(ok2, abs(al) * A2, 0)
        gtot = g.var_sum(gvc)
        atot = g.var_sum(avc)
        grad[:, T] += (gtot * y64).sum(axis=1)
        mass[:, T] += (atot * np.abs(y64)).sum(axis=1)
        gcv = (g.gather(gtot) - gvc) * g.valid[None]
        acv = (g.gather(atot) + avc) * g.valid[None]
    return dict(loss=loss, grad=grad, mass=mass, outs=outs)


def loss64(H, y, bits, T, alpha, w_in=1.0, w_out=1.0):
    """The loss with the forward pass in float64 throughout (for finite differences): [B]."""
    g = Graph(H)
    y = np.asarray(y, np.float64)
    bits = np.asarray(bits, np.float64)
    alpha = np.broadcast_to(np.asarray(alpha, np.float64), (T,))
    cv = np.zeros((y.shape[0], g.m, g.chk_var.shape[1]))
    loss = np.zeros(y.shape[0])
    for t in range(T):
        tot = g.var_sum(cv) + y * w_in
        vc = np.where(g.valid[None], g.gather(tot) - cv, 0)
        a = np.where(g.valid[None], np.minimum(np.abs(vc), 1e30), np.inf)
        srt = np.sort(a, axis=2)
        m1, m2 = srt[:, :, 0:1], np.minimum(srt[:, :, 1:2], 1e30)     # (a check with one edge: the reference's padding, 1e30)
        S = np.prod(np.where(g.valid[None], np.sign(vc), 1), axis=2, keepdims=True)
        mag = np.where(a > m1, m1, m2)
        cv = np.where(g.valid[None], alpha[t] * mag * S * np.sign(vc), 0)
        soft = g.var_sum(cv) + w_out * y
        x = -soft
        loss += (np.maximum(x, 0) - x * bits + np.log1p(np.exp(-np.abs(x)))).sum(axis=1)
    return loss
