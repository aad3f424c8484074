"""-m gpu: ldpc_nms_train_grad (csrc/ldpc_nms_train.hip) -- its decoder outputs against ldpc_nms_decode (both kernels)
and the C oracle bit for bit, its loss and gradient against the float64 model of tests/nms_grad_model.py within a
rounding bound, the per-frame values independent of the batch, the batch sums deterministic, and the error paths."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import c_oracle, np_oracle
from tests.gpu_util import pack_np, to_dev, words_np
from tests.nms_grad_model import grad_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24      # float32 unit roundoff


def rel_bound(T, n=128, dc=8, dv=5):
    """Relative bound (times the L1 contribution mass) of the kernel's float32 loss / gradient against the float64 model.

    The kernel's forward pass is the model's float32 forward bit for bit (tested below), so the difference is the
    rounding of the float32 backward and of the sums.  A term reaches a per-frame gradient through, per iteration, at most
    dv additions into dL/dcv, dc additions of the check's sum, 2 multiplications (sign, alpha), dv additions of dL/dtot
    and 1 subtraction, chained over T iterations, then a lane's running sum over its ceil(n/64) T or ceil(m/64) T terms
    and 6 butterfly additions; the sigmoid / exp / log1p of a term add a few ulps (counted as 8).  By the standard bound
    |error| <= K u (1 + O(K u)) mass with K the longest such chain; twice that covers the O(K u) term and float32's
    round-to-nearest of the model's inputs."""
    K = T * (2 * dv + dc + 3) + T * math.ceil(n / 64) + 6 + 8
    return 2 * K * U


TYPES = {"NMS-1": (0.669435, 1.0, 1.0), "NMS-2": (0.7, 0.9, 0.9), "NMS-3": (0.62, 0.85, 1.2)}


@pytest.fixture(scope="module")
def dec():
    from short_ldpc_decoding_osd_amd import Code
    from short_ldpc_decoding_osd_amd.runtime import Decoder
    return Decoder(Code())


def _frames(dec, snr, B, seed, quantise=False):
    rng = np.random.default_rng(seed)
    y, cw = np_oracle.make_frames(dec.code.G, snr, B, rng)
    if quantise:        # ties in |vc| and zero channel values (S = 0 rows)
        y = (np.round(y * 2) / 2).astype(np.float32)
        y[:, ::17] = 0.0
    return y, cw


def _alphas(T, base):
    return np.array([base * (1 + 0.03 * (t % 5)) for t in range(T)], np.float32)


@pytest.mark.parametrize("dtype", list(TYPES))
@pytest.mark.parametrize("T", [0, 1, 5, 12])
def test_decoder_outputs_equal_nms_decode_and_oracle(dec, dtype, T):
    base, w_in, w_out = TYPES[dtype]
    alpha = _alphas(T, base)
    sizes = [1, 100, 333, 4096]
    for i, snr in enumerate([1.0, 2.7, 4.0]):
        B = sizes[(i + T) % 4]
        for quant in (False, True):
            y, cw = _frames(dec, snr, B, 100 * T + 10 * i + quant, quantise=quant)
            yd, lab = to_dev(y, dec), to_dev(pack_np(cw).view(np.int64), dec)
            res = dec.nms_grad(yd, lab, T, alpha, w_in, w_out, want_traj=True, want_hard=True, want_fail=True)
            for kernel in (1, 2):
                ref = dec.nms(yd, T, alpha if T else 1.0, w_in, w_out, want_traj=True, kernel=kernel)
                torch.cuda.synchronize()
                if T:   # the generic kernel's bits; QC16 may differ in the sign of a zero (array_equal compares values)
                    got, want = res["traj"].cpu().numpy(), ref["traj"].cpu().numpy()
                    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) if kernel == 1 else np.array_equal(got, want)
                assert np.array_equal(words_np(res["hard"]), words_np(ref["hard"]))
                assert np.array_equal(res["fail"].cpu().numpy(), ref["fail"].cpu().numpy())
            soft_o, traj_o = c_oracle.nms(dec.code.H, y, T, alpha if T else 1.0, w_in, w_out, want_traj=True)
            hard_o, fail_o, _ = c_oracle.evaluate(dec.code.H, soft_o, None)
            if T:
                assert np.array_equal(res["traj"].cpu().numpy(), traj_o[1:])
            assert np.array_equal(words_np(res["hard"]), pack_np(hard_o))
            assert np.array_equal(res["fail"].cpu().numpy(), fail_o)


@pytest.mark.parametrize("dtype", list(TYPES))
@pytest.mark.parametrize("T,quant,snr", [(1, False, 2.7), (5, True, 1.0), (12, False, 2.7), (12, True, 4.0)])
def test_loss_and_gradient_within_bound_of_model(dec, dtype, T, quant, snr):
    base, w_in, w_out = TYPES[dtype]
    alpha = _alphas(T, base)
    y, cw = _frames(dec, snr, 64, 7 * T + quant, quantise=quant)
    res = dec.nms_grad(to_dev(y, dec), to_dev(pack_np(cw).view(np.int64), dec), T, alpha, w_in, w_out)
    torch.cuda.synchronize()
    model = grad_model(dec.code.H, y, cw, T, alpha, w_in, w_out)
    bound = rel_bound(T)
    loss = res["loss"].cpu().numpy().astype(np.float64)
    assert np.all(np.abs(loss - model["loss"]) <= bound * model["loss"] + 1e-30)
    grad = res["grad"].cpu().numpy().astype(np.float64)
    err = np.abs(grad - model["grad"])
    assert np.all(err <= bound * model["mass"] + 1e-30), float(np.max(err / np.maximum(model["mass"], 1e-30)))


def test_per_frame_values_do_not_depend_on_the_batch(dec):
    T, alpha = 12, _alphas(12, 0.669435)
    y, cw = _frames(dec, 2.7, 4096, 5)
    lab = pack_np(cw).view(np.int64)
    full = dec.nms_grad(to_dev(y, dec), to_dev(lab, dec), T, alpha)
    torch.cuda.synchronize()
    for f in (0, 1, 2047, 4095):
        one = dec.nms_grad(to_dev(y[f:f + 1], dec), to_dev(lab[f:f + 1], dec), T, alpha)
        torch.cuda.synchronize()
        assert np.array_equal(one["grad"].cpu().numpy().view(np.uint32), full["grad"][f:f + 1].cpu().numpy().view(np.uint32))
        assert np.array_equal(one["loss"].cpu().numpy().view(np.uint32), full["loss"][f:f + 1].cpu().numpy().view(np.uint32))


def test_batch_sums_are_deterministic_and_exact(dec):
    T, alpha = 12, _alphas(12, 0.669435)
    y, cw = _frames(dec, 2.7, 5000, 9)
    yd, lab = to_dev(y, dec), to_dev(pack_np(cw).view(np.int64), dec)
    runs = []
    for s in (torch.cuda.Stream(dec.device), torch.cuda.Stream(dec.device), None):
        with torch.cuda.stream(s if s is not None else torch.cuda.current_stream(dec.device)):
            for _ in range(2):
                r = dec.nms_grad(yd, lab, T, alpha)
                runs.append((r["loss_sum"].cpu().numpy(), r["grad_sum"].cpu().numpy(), r["loss"].cpu().numpy(), r["grad"].cpu().numpy()))
        torch.cuda.synchronize()
    for r in runs[1:]:
        assert np.array_equal(r[0].view(np.uint64), runs[0][0].view(np.uint64))
        assert np.array_equal(r[1].view(np.uint64), runs[0][1].view(np.uint64))
    ls, gs, loss, grad = runs[0]
    assert abs(ls[0] - math.fsum(loss.astype(np.float64))) <= 1e-12 * abs(ls[0])
    for k in range(T + 2):
        want = math.fsum(grad[:, k].astype(np.float64))
        assert abs(gs[k] - want) <= 1e-12 * max(abs(want), math.fsum(np.abs(grad[:, k]).astype(np.float64)))
    # sums without per-frame outputs (scratch inside the call) are the same bits
    r = dec.nms_grad(yd, lab, T, alpha, want_loss=False, want_grad=False)
    torch.cuda.synchronize()
    assert np.array_equal(r["grad_sum"].cpu().numpy().view(np.uint64), gs.view(np.uint64))


def test_nmsloss_autograd_returns_kernel_gradient(dec):
    from short_ldpc_decoding_osd_amd.nms_train import NMSLoss
    T = 5
    y, cw = _frames(dec, 2.7, 100, 3)
    yd, lab = to_dev(y, dec), to_dev(pack_np(cw).view(np.int64), dec)
    w = torch.tensor([-0.048], dtype=torch.float64, requires_grad=True)
    alpha = torch.nn.functional.softplus(w).expand(T)
    w_in = torch.tensor(1.0, dtype=torch.float64)
    w_out = torch.tensor(1.0, dtype=torch.float64)
    loss = NMSLoss.apply(yd, lab, alpha, w_in, w_out, dec)
    loss.backward()
    a32 = np.full(T, np.float32(alpha[0].item()), np.float32)
    ref = dec.nms_grad(yd, lab, T, a32)
    torch.cuda.synchronize()
    gs = ref["grad_sum"].cpu().numpy()
    assert loss.item() == ref["loss_sum"].cpu().numpy()[0]
    want = math.fsum(gs[:T]) / (1 + math.exp(0.048))
    assert abs(w.grad.item() - want) <= 1e-12 * abs(want)


def test_error_paths(dec):
    import ctypes as C
    from short_ldpc_decoding_osd_amd import Code, _lib
    from short_ldpc_decoding_osd_amd.runtime import Decoder
    y, cw = _frames(dec, 2.7, 4, 1)
    yd, lab = to_dev(y, dec), to_dev(pack_np(cw).view(np.int64), dec)
    with pytest.raises(_lib.LdpcError, match="T=65"):
        dec.nms_grad(yd, lab, 65, np.ones(65, np.float32))
    a = np.ones(4, np.float32)
    ap = a.ctypes.data_as(C.POINTER(C.c_float))
    s = C.c_void_p(torch.cuda.current_stream(dec.device).cuda_stream)
    args = [None] * 7
    assert dec.L.ldpc_nms_train_grad(dec._ctx, None, C.c_void_p(lab.data_ptr()), 4, 4, ap, 1.0, 1.0, *args, s) == -1
    assert dec.L.ldpc_nms_train_grad(dec._ctx, C.c_void_p(yd.data_ptr()), None, 4, 4, ap, 1.0, 1.0, *args, s) == -1
    assert dec.L.ldpc_nms_train_grad(dec._ctx, C.c_void_p(yd.data_ptr()), C.c_void_p(lab.data_ptr()), 4, 4, None, 1.0, 1.0, *args, s) == -1
    assert dec.L.ldpc_nms_train_grad(None, C.c_void_p(yd.data_ptr()), C.c_void_p(lab.data_ptr()), 4, 4, ap, 1.0, 1.0, *args, s) == -1
    # CCSDS fits at T = 64 (115 KiB per frame); WiMAX (1056, 880) does not
    T = 64
    res = dec.nms_grad(yd, lab, T, np.full(T, 0.669435, np.float32), want_traj=True)
    torch.cuda.synchronize()
    ref = dec.nms(yd, T, 0.669435, want_traj=True, kernel=1)
    torch.cuda.synchronize()
    assert np.array_equal(res["traj"].cpu().numpy(), ref["traj"].cpu().numpy())
    wimax = Decoder(Code(os.path.join(ROOT, "tests", "golden", "wimax_1056_0.83.alist")), dec.device)
    yw = torch.zeros((2, wimax.n), dtype=torch.float32, device=dec.device)
    lw = torch.zeros((2, wimax.words), dtype=torch.int64, device=dec.device)
    with pytest.raises(_lib.LdpcError, match=r"needs \d+ B of LDS") as e:
        wimax.nms_grad(yw, lw, T, np.full(T, 0.669435, np.float32))
    assert "(-5)" in str(e.value)
    # the same code at a short T fits and decodes as ldpc_nms_decode does
    res = wimax.nms_grad(yw + 0.5, lw, 2, np.full(2, 0.7, np.float32), want_traj=True)
    ref = wimax.nms(yw + 0.5, 2, 0.7, want_traj=True)
    torch.cuda.synchronize()
    assert np.array_equal(res["traj"].cpu().numpy(), ref["traj"].cpu().numpy())
