"""CPU: the float64 gradient model of tests/nms_grad_model.py (finite differences, torch autograd of a dense op-for-op
restatement with TensorFlow's tie rule), the host optimiser of nms_train.py, and the training stage's files (values.txt,
checkpoint bundle, training data)."""
import numpy as np
import pytest
import torch

from oracle import np_oracle
from tests.nms_grad_model import Graph, forward32, grad_model, loss64


@pytest.fixture(scope="module")
def code(np_code):
    return np_code


def _frames(code, snr, B, seed):
    return np_oracle.make_frames(np.asarray(code.G), snr, B, np.random.default_rng(seed))


def _min_gap(H, y, T, alpha, w_in, w_out, rows=None):
    """Per frame: smallest |vc| and smallest gap between the three smallest |vc| of any check (float32 forward); ``rows``:
    the checks looked at (all by default)."""
    g = Graph(H)
    _, recs = forward32(g, y, T, alpha, w_in, w_out)
    small, gap = np.full(y.shape[0], np.inf), np.full(y.shape[0], np.inf)
    for r in recs:
        a = np.where(g.valid[None], np.abs(r["vc"]), np.inf)
        s = np.sort(a, axis=2)[:, slice(None) if rows is None else rows]
        small = np.minimum(small, s[:, :, 0].min(axis=1))
        with np.errstate(invalid="ignore"):     # a check with fewer than three edges: inf - inf, no gap to speak of
            d = np.stack([s[:, :, 1] - s[:, :, 0], s[:, :, 2] - s[:, :, 1]])
        gap = np.minimum(gap, np.where(np.isnan(d), np.inf, d).min(axis=(0, 2)))
    return small, gap


def check_finite_differences(H, y, cw, w_in, w_out, min_share=0.0, rows=None):
    """The model's gradient against central differences of loss64 on the frames of (y, cw) with a decision gap;
    ``min_share``: the share of the frames that must qualify; ``rows``: the checks the gap rule looks at."""
    T = 4
    alpha = np.array([0.7, 0.6, 0.8, 0.65], np.float32)
    small, gap = _min_gap(H, y, T, alpha, w_in, w_out, rows)
    ok = (small > 1e-3) & (gap > 1e-3)                           # no near-zero vc, no near-ties: smooth around the point
    assert ok.mean() >= min_share, ok.mean()
    keep = np.flatnonzero(ok)[:6]
    assert keep.size >= 3
    y, cw = y[keep], cw[keep]
    r = grad_model(H, y, cw, T, alpha, w_in, w_out)
    assert np.allclose(r["loss"], loss64(H, y, cw, T, alpha, w_in, w_out), rtol=1e-6)
    h = 1e-6

    def fd(da=None, di=0.0, do=0.0):
        ap = alpha.astype(np.float64) + (da if da is not None else 0)
        am = alpha.astype(np.float64) - (da if da is not None else 0)
        return (loss64(H, y, cw, T, ap, w_in + di, w_out + do) - loss64(H, y, cw, T, am, w_in - di, w_out - do)) / (2 * h)

    for t in range(T):
        e = np.zeros(T)
        e[t] = h
        assert np.allclose(r["grad"][:, t], fd(da=e), rtol=2e-5, atol=1e-5 * r["mass"][:, t].max())
    assert np.allclose(r["grad"][:, T], fd(di=h), rtol=2e-5, atol=1e-5 * r["mass"][:, T].max())
    assert np.allclose(r["grad"][:, T + 1], fd(do=h), rtol=2e-5, atol=1e-5 * r["mass"][:, T + 1].max())


@pytest.mark.parametrize("w_in,w_out", [(1.0, 1.0), (0.9, 1.1)])
def test_model_matches_finite_differences(code, w_in, w_out):
    y, cw = _frames(code, 2.0, 200, 1)
    check_finite_differences(np.asarray(code.H), y, cw, w_in, w_out)


def _torch_loss(H, y, bits, T, alpha, w_in, w_out):
    """Dense op-for-op restatement of compute_vc / compute_cv2 / marginalize / calculation_loss
    (ms_decoder_dense.py:121-134, :177-208, :217-226, :210-215) in float64 with TF's gradient rules: the sign matrix is
    detached (tf.stop_gradient), clip is min/max, top_k(k=2) takes the largest decisions with ties to the LOWER
    column index first (a stable sort), and the cross entropy is TF's select form."""
    Hf = torch.as_tensor(H, dtype=torch.float64)
    y = torch.as_tensor(y, dtype=torch.float64)
    z = torch.as_tensor(bits, dtype=torch.float64)
    B, n = y.shape
    cv = torch.zeros((B,) + tuple(Hf.shape), dtype=torch.float64)
    back = torch.where(Hf == 0, torch.tensor(-1e30 - 1, dtype=torch.float64), torch.tensor(0.0, dtype=torch.float64))
    loss = 0.0
    for t in range(T):
        tot = cv.sum(dim=1) + y * w_in
        vc = tot[:, None, :] * Hf - cv
        sgn = torch.sign((1 - Hf)[None] + vc).detach()
        out_sign = (torch.prod(sgn, dim=2, keepdim=True) * Hf) * sgn
        a = torch.clamp(torch.abs(vc), 0.0, 1e30)
        decision = -torch.abs(a) + back[None]
        order = torch.sort(-decision.detach(), dim=2, stable=True).indices[:, :, :2]
        part = torch.gather(decision, 2, order)
        m1 = (-part[:, :, 0:1]) * Hf
        m2 = (-part[:, :, 1:2]) * Hf
        mag = torch.where(a > m1, m1, m2)
        cv = alpha[t] * mag * out_sign
        soft = cv.sum(dim=1) + w_out * y
        x = -soft
        # tf.nn.sigmoid_cross_entropy_with_logits as TF writes it (two selects on x >= 0): its gradient at x = 0 is
        # 0.5 - z, where clamp / abs would give 1 - z
        cond = x >= 0
        relu, neg_abs = torch.where(cond, x, torch.zeros_like(x)), torch.where(cond, -x, x)
        loss = loss + (relu - x * z + torch.log1p(torch.exp(neg_abs))).sum()
    return loss


def check_torch_autograd(H, y, cw, ties):
    """The model's batch gradient against torch autograd of _torch_loss; ``ties``: on quantised channel values."""
    if ties:        # quantised channel values: equal |vc| in a check, resolved by the lower variable index
        y = (np.round(y * 4) / 4).astype(np.float32)
        y[y == 0] = 0.25
    T = 3
    alpha = np.array([0.75, 0.5, 0.625], np.float32)     # exact binary fractions: the float64 forward meets the same ties
    w_in, w_out = 1.0, 0.75
    g = Graph(H)
    _, recs = forward32(g, y, T, alpha, w_in, w_out)
    if ties:
        srt = [np.sort(np.where(g.valid[None], np.abs(r["vc"]), np.inf), axis=2) for r in recs]
        tied = any(np.any((s[:, :, 0] == s[:, :, 1]) & np.isfinite(s[:, :, 1])) for s in srt)   # (inf: fewer than two edges)
        assert tied, "the crafted frames must hold ties"
    a = torch.tensor(alpha.astype(np.float64), requires_grad=True)
    wi = torch.tensor(w_in, dtype=torch.float64, requires_grad=True)
    wo = torch.tensor(w_out, dtype=torch.float64, requires_grad=True)
    loss = _torch_loss(H, y, cw, T, a, wi, wo)
    loss.backward()
    r = grad_model(H, y, cw, T, alpha, w_in, w_out)
    tot = r["grad"].sum(axis=0)
    mass = r["mass"].sum(axis=0)
    # the model's forward is float32, torch's float64: the two differ by float32 rounding (a few 1e-7 relative)
    assert abs(loss.item() - r["loss"].sum()) <= 1e-6 * loss.item()
    got = np.concatenate([a.grad.numpy(), [wi.grad.item(), wo.grad.item()]])
    assert np.all(np.abs(got - tot) <= 1e-5 * mass), (got, tot)


@pytest.mark.parametrize("ties", [False, True])
def test_model_matches_torch_autograd(code, ties):
    y, cw = _frames(code, 2.5, 4, 11)
    check_torch_autograd(np.asarray(code.H), y, cw, ties)


def test_adam_decay_clip_by_hand():
    from short_ldpc_decoding_osd_amd.nms_train import ExponentialDecay, LegacyAdam, clip_by_norm
    d = ExponentialDecay(0.01, 500, 0.95, staircase=True)
    assert d(0) == np.float32(0.01) and d(499) == np.float32(0.01) and d(500) == np.float32(0.0095)
    assert d(1200) == np.float32(0.01 * 0.95 ** 2)
    assert np.array_equal(clip_by_norm(np.float32([3.0]), 5), np.float32([3.0]))
    assert np.array_equal(clip_by_norm(np.float32([-12.0]), 5), np.float32([-5.0]))
    opt = LegacyAdam(0.01)
    p = {"w": np.float32([-0.048])}
    g1, g2 = 2.0, -1.0
    opt.apply_gradients([(np.float32([g1]), "w", p)])
    # step 1: m = 0.1 g, v = 0.001 g^2, lr_t = lr sqrt(0.001) / 0.1  ->  w -= lr (g / |g|) (up to eps)
    m, v = 0.1 * g1, 0.001 * g1 * g1
    lr_t = 0.01 * np.sqrt(1 - 0.999) / (1 - 0.9)
    w = -0.048 - lr_t * m / (np.sqrt(v) + 1e-7)
    assert abs(p["w"][0] - w) <= 1e-7
    opt.apply_gradients([(np.float32([g2]), "w", p)])
    m, v = 0.9 * m + 0.1 * g2, 0.999 * v + 0.001 * g2 * g2
    lr_t = 0.01 * np.sqrt(1 - 0.999 ** 2) / (1 - 0.9 ** 2)
    w = w - lr_t * m / (np.sqrt(v) + 1e-7)
    assert abs(p["w"][0] - w) <= 1e-7
    assert opt.iterations == 2


def test_stored_gradient_chain_rule():
    from short_ldpc_decoding_osd_amd.nms_train import stored_grads
    ge = np.array([1.0, 2.0, 3.0, 0.5, -0.25])          # T = 3
    s = {"shared_check_weight": np.float32(-0.048), "shared_bit_weight1": np.float32(0.3), "shared_bit_weight2": np.float32(-0.2),
         "shared_bit_weight": np.float32(0.1)}
    sig = lambda x: 1 / (1 + np.exp(-float(np.float32(x))))       # noqa: E731
    g1 = stored_grads("NMS-1", s, ge)
    assert set(g1) == {"shared_check_weight"} and abs(g1["shared_check_weight"] - 6.0 * sig(-0.048)) < 1e-6
    g2 = stored_grads("NMS-2", s, ge)
    assert abs(g2["shared_bit_weight"] - 0.25 * sig(0.1)) < 1e-6
    g3 = stored_grads("NMS-3", s, ge)
    assert abs(g3["shared_bit_weight1"] - 0.5 * sig(0.3)) < 1e-6 and abs(g3["shared_bit_weight2"] + 0.25 * sig(-0.2)) < 1e-6


@pytest.fixture
def training_globals(alist_path):
    from short_ldpc_decoding_osd_amd import globalmap as GL
    GL.training_setting_global(["t", 2.7, 2.7, 100, 10, 12, alist_path, "NMS-3"])
    return GL


def test_values_txt_round_trip(tmp_path, training_globals):
    from short_ldpc_decoding_osd_amd import ms_decoder_dense, weights
    M = ms_decoder_dense.Decoding_model()
    M.layer.shared_check_weight = np.float32([0.123])
    M.layer.shared_bit_weight1 = np.float32([-0.5])
    p = str(tmp_path / "values.txt")
    ms_decoder_dense.write_values(p, 50, M)
    M.layer.shared_check_weight = np.float32([0.25])
    ms_decoder_dense.write_values(p, 100, M)
    step, var = weights.parse_values_txt(p)
    assert step == 100 and var["decoder__layer/decoder_check_normalized factor:0"][0] == np.float32(0.25)
    step, var = weights.parse_values_txt(p, 50)
    assert var["decoder__layer/decoder_check_normalized factor:0"][0] == np.float32(0.123)
    assert var["decoder__layer/decoder_bit_normalized factor1:0"][0] == np.float32(-0.5)
    assert len(var) == 3


def test_checkpoint_round_trip_into_test_model(tmp_path, training_globals):
    from short_ldpc_decoding_osd_amd import ms_decoder_dense, ms_test
    from short_ldpc_decoding_osd_amd.tf_checkpoint import load_checkpoint
    M = ms_decoder_dense.Decoding_model()
    M.layer.shared_check_weight = np.float32([0.321])
    M.layer.shared_bit_weight1 = np.float32([0.5])
    M.layer.shared_bit_weight2 = np.float32([-0.75])
    ms_decoder_dense.checkpoint_saver(M, str(tmp_path), "ldpc-ckpt")(50)
    R = ms_test.Decoding_model()
    done = load_checkpoint(R, str(tmp_path))
    assert set(done) == {"shared_check_weight", "shared_bit_weight1", "shared_bit_weight2"}
    assert R.layer.shared_check_weight[0] == np.float32(0.321) and R.layer.shared_bit_weight2[0] == np.float32(-0.75)


def test_nms_r_is_refused(alist_path):
    from short_ldpc_decoding_osd_amd import globalmap as GL, ms_decoder_dense
    GL.training_setting_global(["t", 2.7, 2.7, 100, 10, 12, alist_path, "NMS-r"])
    with pytest.raises(NotImplementedError):
        ms_decoder_dense.Decoding_model()


def test_training_data_generating(training_globals):
    from short_ldpc_decoding_osd_amd import data_generating
    code = training_globals.get_map('code_parameters')
    y, lab = data_generating.training_data_generating(code, (2.7, 2.7), 4000, np.random.default_rng(3))
    H = np.asarray(code.H)
    assert not np.any((lab @ H.T) % 2)                          # codewords of the code
    x = np.where(lab == 0, y, -y)                                # back to the noise
    sigma = np.sqrt(1. / (2 * (64 / 128) * 10 ** (2.7 / 10)))
    assert abs(x.mean() - 1.0) < 0.01 and abs(x.std() - sigma) < 0.01
    # snr_lo != snr_hi: the weighted-sigma mean and spread
    y2, lab2 = data_generating.training_data_generating(code, (1.0, 4.0), 4000, np.random.default_rng(3))
    x2 = np.where(lab2 == 0, y2, -y2)
    s_lo, s_hi = (np.sqrt(1. / (2 * 0.5 * 10 ** (snr / 10))) for snr in (1.0, 4.0))
    assert 2 / s_lo ** 2 < x2.mean() < 2 / s_hi ** 2 and x2.std() > 0     # the mean of 2 / sigma^2 over the band
