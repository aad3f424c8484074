"""-m gpu: ldpc_dia_cnn_grad (csrc/ldpc_dia.hip) -- its refined values against ldpc_dia_cnn bit for bit with every subset
of the nullable outputs, its loss and gradient against the float64 model of tests/dl_training_model.py within a derived
rounding bound (and, on inputs whose float32 forward is exact, against torch autograd), many elements per thread,
determinism and batch independence, saturated / zero inputs, and the refusals."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import dl_training_model as TM
from tests import dlosd_model as DM
from tests.gpu_util import pack_np, to_dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, U = TM.K, TM.U      # the float32 chain length behind one product / loss term, and the unit roundoff
CODES = {"ccsds": None, "96_48": "LDPC_N96_K48_P8_set0_dmin10.alist", "121_80": "ArrayCode_N121_K80_r0.66.alist"}
SHAPES = [("ccsds", L, F) for L in (7, 8, 13, 64) for F in (1, 3, 100)] + [("96_48", 13, 3), ("121_80", 13, 3)]
# dia_grad_kernel's workgroup: 256 threads up to L = 22, 128 up to L = 46, 64 beyond -- both sides of either switch point
SHAPES += [("ccsds", L, F) for L in (22, 23, 46, 47) for F in (3, 100)]


@pytest.fixture(scope="module")
def decs():
    from short_ldpc_decoding_osd_amd import Code
    from short_ldpc_decoding_osd_amd.runtime import Decoder
    made = {}

    def get(name):
        if name not in made:
            made[name] = Decoder(Code(os.path.join(ROOT, "tests", "golden", CODES[name])) if CODES[name] else Code())
        return made[name]
    return get


def _case(dec, L, F, seed, scale=0.5):
    rng = np.random.default_rng(seed)
    ws = DM.random_cnn_weights(rng, L, scale=scale)
    rows = (rng.standard_normal((F, L, dec.n)) * 3).astype(np.float32)
    labels = rng.integers(0, 2, (F, dec.n)).astype(np.int64)
    return ws, rows, labels


def _abi(dec, rows_d, lab_d, w, L, F, want_out=True, want_loss=True, want_grad=True, stream=None, fill=None):
    """The C call itself with any subset of the outputs; -> (rc, out, loss_sum, grad) as device tensors / None."""
    w = np.ascontiguousarray(w, np.float32) if w is not None else None
    nw = w.size if w is not None else 145 + 2 * (L - 6)
    mk = (lambda shape, dt: torch.full(shape, fill, dtype=dt, device=dec.device)) if fill is not None else dec.empty
    out = mk((max(F, 1), dec.n), torch.float32) if want_out else None
    ls = mk((1,), torch.float64) if want_loss else None
    gs = mk((nw,), torch.float64) if want_grad else None
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None     # noqa: E731
    s = C.c_void_p(torch.cuda.current_stream(dec.device).cuda_stream) if stream is None else stream
    rc = dec.L.ldpc_dia_cnn_grad(dec._ctx, p(rows_d), p(lab_d), F, L, w.ctypes.data_as(C.POINTER(C.c_float)) if w is not None else None,
                                 nw, p(out), p(ls), p(gs), s)
    return rc, out, ls, gs


def _bits(t, dt):
    return t.cpu().numpy().view(dt)


def _check_against_model(dec, rows, labels, ws, what):
    """The kernel's loss and gradient against the float64 model fed the kernel's own float32 out.  Per weight theta the
    difference is bounded by 2 K u sum_r |dE[r]/dtheta| sum_{f,v} |g x[r]| (bias: 2 K u sum |g|), the loss by
    2 K u sum |term| (K: the chain counted in tests/dl_training_model.py; the factor 2 covers the O(K u) term).  Prints the
    worst error / bound ratio; returns (loss_sum, grad, out) as NumPy."""
    L = rows.shape[1]
    lab = to_dev(pack_np(labels).view(np.int64), dec)
    loss_sum, grad, out = dec.dia_cnn_grad(to_dev(rows, dec), lab, DM.pack_cnn(ws), want_out=True)
    loss_sum, grad, out = loss_sum.cpu().numpy(), grad.cpu().numpy(), out.cpu().numpy()
    model = TM.cnn_loss_grad(rows, labels, ws, out=out)
    mass = TM.pack(TM.grad_masses(L, ws, model["abs_m"], model["abs_g"]))
    err, bound = np.abs(grad - TM.pack(model["grads"])), 2 * K * U * mass
    lerr, lbound = abs(loss_sum[0] - model["loss"]), 2 * K * U * model["abs_loss"]
    worst = float(np.max(err / np.maximum(bound, 1e-300)))
    print(f"{what}: worst gradient error / bound {worst:.3g}, loss error / bound {lerr / max(lbound, 1e-300):.3g}")
    assert np.all(np.isfinite(grad)) and np.isfinite(loss_sum[0])
    assert np.all(err <= bound), worst
    assert lerr <= lbound, (loss_sum[0], model["loss"])
    return loss_sum, grad, out, model


# ------------------------------------------------------------------------------------------------ 1. forward, nullables
@pytest.mark.parametrize("code,L,F", SHAPES)
def test_out_equals_dia_cnn_with_every_subset_of_outputs(decs, code, L, F):
    dec = decs(code)
    ws, rows, labels = _case(dec, L, F, 100 * L + F)
    w = DM.pack_cnn(ws)
    rows_d, lab_d = to_dev(rows, dec), to_dev(pack_np(labels).view(np.int64), dec)
    assert (F * dec.n) % 256 != 0 or code == "ccsds"
    want = _bits(dec.dia_cnn(rows_d, w), np.uint32)
    rc, out, ls, gs = _abi(dec, rows_d, lab_d, w, L, F)
    assert rc == 0 and np.array_equal(_bits(out, np.uint32), want)
    full = (_bits(ls, np.uint64), _bits(gs, np.uint64))
    for wo, wl, wg in [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (0, 0, 0)]:
        rc, out, ls, gs = _abi(dec, rows_d, lab_d, w, L, F, wo, wl, wg)
        assert rc == 0
        if wo:
            assert np.array_equal(_bits(out, np.uint32), want), (wo, wl, wg)
        if wl:
            assert np.array_equal(_bits(ls, np.uint64), full[0]), (wo, wl, wg)
        if wg:
            assert np.array_equal(_bits(gs, np.uint64), full[1]), (wo, wl, wg)
    # the Python layer returns the same bits
    loss_sum, grad, out = dec.dia_cnn_grad(rows_d, lab_d, w, want_out=True)
    assert np.array_equal(_bits(out, np.uint32), want) and np.array_equal(_bits(loss_sum, np.uint64), full[0])
    assert np.array_equal(_bits(grad, np.uint64), full[1]) and dec.dia_cnn_grad(rows_d, lab_d, w)[2] is None


def test_no_frames_writes_nothing(decs):
    dec = decs("ccsds")
    L = 13
    w = DM.pack_cnn(DM.random_cnn_weights(np.random.default_rng(0), L))
    rc, out, ls, gs = _abi(dec, None, None, w, L, 0, fill=7.0)
    torch.cuda.synchronize()
    assert rc == 0 and torch.all(out == 7) and torch.all(ls == 7) and torch.all(gs == 7)
    # the Python layer reports the empty sums as zeros
    loss_sum, grad, out = dec.dia_cnn_grad(dec.empty((0, L, dec.n), torch.float32), dec.empty((0, dec.words), torch.int64), w, want_out=True)
    assert loss_sum.item() == 0 and grad.shape == (w.size,) and not grad.any() and out.shape == (0, dec.n)


# ------------------------------------------------------------------------------------------------ 2. the rounding bound
@pytest.mark.parametrize("code,L,F", [s for s in SHAPES if s[2] in (3, 100)])
def test_loss_and_gradient_within_bound_of_model(decs, code, L, F):
    dec = decs(code)
    ws, rows, labels = _case(dec, L, F, 7 * L + F)
    _check_against_model(dec, rows, labels, ws, f"{code} L={L} F={F}")


# ------------------------------------------------------------------------------------------------ 3. exact forward
@pytest.mark.parametrize("L", [7, 13, 23, 47])
def test_exact_forward_gradient_equals_autograd(decs, L):
    """Weights that are multiples of 1/8 in [-1, 1] and rows that are multiples of 1/4 in [-8, 8]: every product and
    partial sum of the forward pass is a multiple of 2^-14, exact in float32 while it stays below 2^10 (the outputs of
    these draws stay below 2^8 up to L = 13, reach 270 at L = 23 and 703 at L = 47), so out is the float64 forward --
    asserted below.  The gradient then equals torch autograd (no moment identity) within the bound of the model test.
    L = 23 and 47 run the 128- and the 64-thread workgroup of dia_grad_kernel."""
    dec = decs("ccsds")
    rng = np.random.default_rng(L)
    F = 100
    ws = [(rng.integers(-8, 9, s) / 8).astype(np.float32) for s in DM.cnn_sizes(L)]
    rows = (rng.integers(-32, 33, (F, L, dec.n)) / 4).astype(np.float32)
    labels = rng.integers(0, 2, (F, dec.n)).astype(np.int64)
    loss_sum, grad, out, model = _check_against_model(dec, rows, labels, ws, f"exact forward L={L}")
    loss, grads, out64 = TM.torch_loss_grad(rows, labels, ws)
    assert np.array_equal(out.astype(np.float64), out64)
    mass = TM.pack(TM.grad_masses(L, ws, model["abs_m"], model["abs_g"]))
    assert np.all(np.abs(grad - TM.pack(grads)) <= 2 * K * U * mass)
    assert abs(loss_sum[0] - loss) <= 2 * K * U * model["abs_loss"]


# ------------------------------------------------------------------------------------------------ 4. elements per thread
def test_many_elements_per_thread(decs):
    """F n = 3 * (4096 workgroups * 256 threads) + 38528: most threads take four elements, the rest three; 89 MB of
    rows, generated on the device; the model runs on the host 4096 frames at a time."""
    dec = decs("ccsds")
    L, F = 7, 24877
    assert F * dec.n > 3 * 4096 * 256 and (F * dec.n) % (4096 * 256) != 0 and F * L * dec.n * 4 < 100e6
    gen = torch.Generator(device=dec.device).manual_seed(5)
    rows_d = torch.randn((F, L, dec.n), generator=gen, device=dec.device, dtype=torch.float32) * 3
    labels_d = torch.randint(0, 2, (F, dec.n), generator=gen, device=dec.device, dtype=torch.int64)
    ws = DM.random_cnn_weights(np.random.default_rng(5), L)
    loss_sum, grad, out = dec.dia_cnn_grad(rows_d, dec.pack_bits(labels_d), DM.pack_cnn(ws), want_out=True)
    assert torch.equal(out, dec.dia_cnn(rows_d, DM.pack_cnn(ws)))
    rows, labels, out = rows_d.cpu().numpy(), labels_d.cpu().numpy(), out.cpu().numpy()
    model = TM.cnn_loss_grad(rows, labels, ws, out=out)
    mass = TM.pack(TM.grad_masses(L, ws, model["abs_m"], model["abs_g"]))
    err, bound = np.abs(grad.cpu().numpy() - TM.pack(model["grads"])), 2 * K * U * mass
    print(f"many elements per thread: worst gradient error / bound {float(np.max(err / bound)):.3g}")
    assert np.all(err <= bound)
    assert abs(loss_sum.cpu().numpy()[0] - model["loss"]) <= 2 * K * U * model["abs_loss"]


# ------------------------------------------------------------------------------------------------ 5. determinism
def test_deterministic_on_any_stream_and_additive_over_the_batch(decs):
    _deterministic_and_additive(decs("ccsds"), 13, 5000)     # 2500 workgroups: the finish kernel's lanes sum 39 or 40 partials each


def test_deterministic_and_additive_with_the_128_thread_workgroup(decs):
    _deterministic_and_additive(decs("ccsds"), 23, 2500)     # L = 23: workgroups of 128, 2500 of them again


def _deterministic_and_additive(dec, L, F):
    ws, rows, labels = _case(dec, L, F, 9)
    w = DM.pack_cnn(ws)
    rows_d, lab_d = to_dev(rows, dec), to_dev(pack_np(labels).view(np.int64), dec)
    runs = []
    for s in (torch.cuda.Stream(dec.device), torch.cuda.Stream(dec.device), None):
        with torch.cuda.stream(s if s is not None else torch.cuda.current_stream(dec.device)):
            for _ in range(2):
                loss_sum, grad, _ = dec.dia_cnn_grad(rows_d, lab_d, w)
                runs.append((_bits(loss_sum, np.uint64), _bits(grad, np.uint64)))
        torch.cuda.synchronize()
    for r in runs[1:]:
        assert np.array_equal(r[0], runs[0][0]) and np.array_equal(r[1], runs[0][1])
    # grad(F frames) = grad(first half) + grad(second half) within the float64 rounding of the trees: 1e-12 of the L1
    # mass of the products that reach the weight (the halves run other tree shapes)
    h = F // 2
    la, ga, _ = dec.dia_cnn_grad(rows_d[:h].contiguous(), lab_d[:h].contiguous(), w)
    lb, gb, _ = dec.dia_cnn_grad(rows_d[h:].contiguous(), lab_d[h:].contiguous(), w)
    ls, gs, out = dec.dia_cnn_grad(rows_d, lab_d, w, want_out=True)
    model = TM.cnn_loss_grad(rows, labels, ws, out=out.cpu().numpy())
    mass = TM.pack(TM.grad_masses(L, ws, model["abs_m"], model["abs_g"]))
    assert np.all(np.abs((ga + gb - gs).cpu().numpy()) <= 1e-12 * mass)
    assert abs((la + lb - ls).cpu().numpy()[0]) <= 1e-12 * model["abs_loss"]


# ------------------------------------------------------------------------------------------------ 6. extremes
def _saturated_case(dec, L):
    """Two frames of +-1e4 under large weights: |out| is far beyond 750, where float64's sigmoid is exactly 0 or 1 too."""
    rng = np.random.default_rng(42)
    ws = DM.random_cnn_weights(rng, L, scale=2.0)
    rows = np.empty((2, L, dec.n), np.float32)
    rows[0] = 1e4
    rows[1] = -1e4
    rows[:, :, ::3] *= -1
    return ws, rows


@pytest.mark.parametrize("labels_kind", ["zeros", "ones", "random"])
def test_saturated_rows(decs, labels_kind):
    dec = decs("ccsds")
    L = 7
    ws, rows = _saturated_case(dec, L)
    rng = np.random.default_rng(1)
    labels = dict(zeros=np.zeros((2, dec.n), np.int64), ones=np.ones((2, dec.n), np.int64),
                  random=rng.integers(0, 2, (2, dec.n)).astype(np.int64))[labels_kind]
    loss_sum, grad, out, model = _check_against_model(dec, rows, labels, ws, f"saturated, labels {labels_kind}")
    assert np.all(np.isfinite(out)) and np.all(np.abs(out) > 750) and (out > 0).any() and (out < 0).any()
    # g is exactly 0 or +-1 in the model (float64 saturates beyond 750), and so in the kernel: the products +-1e4 and
    # their float64 sums are exact, so the bias gradient is the model's integer and the moments are the model's
    _, g = TM.loss_terms(out, labels)
    assert set(np.unique(g)) <= {-1.0, 0.0, 1.0}
    assert grad[-1] == model["sg"] == float(np.sum(g))


@pytest.mark.parametrize("labels_kind", ["zeros", "ones"])
def test_zero_rows_and_constant_labels(decs, labels_kind):
    """All-zero rows: out = bias everywhere, every moment is 0, so only the bias has a gradient: F n g(bias)."""
    dec = decs("ccsds")
    L, F = 8, 3
    ws = DM.random_cnn_weights(np.random.default_rng(2), L)
    rows = np.zeros((F, L, dec.n), np.float32)
    rows[1] = -0.0
    labels = np.full((F, dec.n), 1 if labels_kind == "ones" else 0, np.int64)
    loss_sum, grad, out, model = _check_against_model(dec, rows, labels, ws, f"zero rows, labels {labels_kind}")
    assert np.all(out == ws[4][0])
    assert np.all(grad[:-1] == 0) and grad[-1] != 0 and np.sign(grad[-1]) == (1 if labels_kind == "ones" else -1)
    # moderate random rows under constant labels
    ws, rows, _ = _case(dec, L, 50, 77)
    _check_against_model(dec, rows, np.full((50, dec.n), labels[0, 0], np.int64), ws, f"random rows, labels {labels_kind}")


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_name_the_call_and_the_argument(decs):
    dec = decs("ccsds")
    L, F = 13, 4
    ws, rows, labels = _case(dec, L, F, 3)
    w = DM.pack_cnn(ws)
    rows_d, lab_d = to_dev(rows, dec), to_dev(pack_np(labels).view(np.int64), dec)
    err = lambda: dec.L.ldpc_last_error().decode()     # noqa: E731

    def refused(expect, *args, **kw):
        rc, out, ls, gs = _abi(dec, *args, fill=7.0, **kw)
        torch.cuda.synchronize()
        msg = err()
        assert rc == -1 and msg.startswith("ldpc_dia_cnn_grad: ") and expect in msg, (rc, msg)
        assert torch.all(out == 7) and torch.all(ls == 7) and torch.all(gs == 7), "refused, yet an output was written"

    refused("L = 6", rows_d, lab_d, np.zeros(145, np.float32), 6, F)
    refused("L = 65", rows_d, lab_d, np.zeros(145 + 2 * 59, np.float32), 65, F)
    refused("n_weights = 158", rows_d, lab_d, w[:-1], L, F)
    refused("weights is NULL", rows_d, lab_d, None, L, F)
    refused("d_rows is NULL", None, lab_d, w, L, F)
    refused("d_label_bits is NULL", rows_d, None, w, L, F)
    refused("F = -1", rows_d, lab_d, w, L, -1)
    # the Python layer refuses mismatched frames before the call
    with pytest.raises(ValueError, match="label_bits"):
        dec.dia_cnn_grad(rows_d, lab_d[:2].contiguous(), w)
