"""-m gpu: the H-form OSD primitives for short codes of any shape (ldpc_hosdx_front / _search / _sliding) against the
(128,64) kernels on the CCSDS code, and against the NumPy model (tests/hosdx_model.py) on (96,48), (64,32) and the synthetic
shape edges of tests/osd_shapes.BOTH.  Unless stated otherwise every comparison is array_equal on bit patterns."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import np_oracle
from tests import dlosd_model as DM
from tests import hosdx_model as HM
from tests import osd_shapes
from tests.gpu_util import to_dev

pytestmark = pytest.mark.gpu

REAL = {"96_48": "LDPC_N96_K48_P8_set0_dmin10.alist", "64_32": "code1.alist"}
FRONT_KEYS = ("lri", "uidx", "M", "nswaps")
SEARCH_KEYS = ("block_min", "block_arg", "truth", "cw", "metric", "best")
SLIDE_KEYS = ("deep_limit", "global_min", "truth", "success", "cw", "metric", "best", "teps")
_decoders = {}


def _decoder(key, H=None, path=None):
    from short_ldpc_decoding_osd_amd import Code
    from short_ldpc_decoding_osd_amd.runtime import Decoder
    if key not in _decoders:
        code = Code(H=np.array(H)) if H is not None else (Code(path) if path else Code())
        _decoders[key] = Decoder(code)
    return _decoders[key]


def real(golden_dir, which):
    """(decoder, H, G) of a real code of the reference."""
    path = os.path.join(golden_dir, REAL[which])
    c = np_oracle.Code(path)
    dec = _decoder(which, path=path)
    assert dec.hosdx_supported and (dec.n, dec.k) == tuple(int(v) for v in which.split("_"))
    return dec, c.H, c.G


def bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_same(got, want, keys, what=""):
    for key in keys:
        assert np.array_equal(bits(got[key]), bits(want[key])), (key, what)


def device_inputs(dec, x, y, cw, blocks):
    teps, off = HM.table(blocks)
    return dict(x=to_dev(x, dec), y=to_dev(y, dec), lab=to_dev(HM.pack_cw(np.asarray(cw)).view(np.int64), dec),
                teps=to_dev(teps, dec), off=to_dev(off, dec), nblk=len(off) - 1)


def run_search(dec, d):
    """hosdx_front + hosdx_search -> the dict of HM.packed."""
    lri, uidx, M, ns = dec.hosdx_front(d["x"])
    out = dec.hosdx_search(d["x"], d["y"], (lri, uidx, M), d["teps"], d["off"], label_bits=d["lab"])
    torch.cuda.synchronize()
    return dict(out, lri=lri, uidx=uidx, M=M, nswaps=ns)


def model(x, y, cw, H, blocks):
    return HM.packed([HM.hosdx_frame(x[f], y[f], cw[f], H, blocks) for f in range(len(x))], len(blocks))


# --------------------------------------------------------------------------------------------- parity on (128,64)
def test_parity_with_the_128_64_kernels(np_code):
    dec = _decoder("ccsds")
    assert dec.hosdx_supported and dec._hosd_fam() == "hosd"
    x, y, cw = HM.refined_frames(np_code.H, np_code.G, 2.0, 256, 31)
    x[3, 10] = x[3, 77] = 0.0
    x[4, :] = np.float32(0.5) * np.sign(x[4, :])
    y[5, 20] = 0.0
    d = device_inputs(dec, x, y, cw, HM.path_blocks(64, 2))
    assert int(d["off"][-1]) == 2081
    old, new = dec.hosd_front(d["x"]), dec.hosdx_front(d["x"])
    for a, b, key in zip(old, new, FRONT_KEYS):
        assert torch.equal(a, b), key
    so = dec.hosd_search(d["x"], d["y"], old, d["teps"], d["off"], label_bits=d["lab"])
    sn = dec.hosdx_search(d["x"], d["y"], new, d["teps"], d["off"], label_bits=d["lab"])
    assert_same(sn, so, SEARCH_KEYS)
    win = 3
    for w1, w2 in (DM.stopping_fcn_weights(win), DM.random_fcn_weights(np.random.default_rng(2), win)):
        fw = np.concatenate([w1.ravel(), w2.ravel()])
        for group in (0, 1):
            lo = dec.hosd_sliding(d["x"], d["y"], old, d["teps"], d["off"], win, 0.9, fw, label_bits=d["lab"], group=group)
            ln = dec.hosdx_sliding(d["x"], d["y"], new, d["teps"], d["off"], win, 0.9, fw, label_bits=d["lab"], group=group)
            assert_same(ln, lo, SLIDE_KEYS, group)


# ------------------------------------------------------------------------------------- oracle parity on the real codes
@pytest.mark.parametrize("snr", [1.0, 3.0])
@pytest.mark.parametrize("which", sorted(REAL))
def test_real_codes_match_the_model(golden_dir, which, snr):
    dec, H, G = real(golden_dir, which)
    x, y, cw = HM.refined_frames(H, G, snr, 64, 100 + int(10 * snr))
    blocks = HM.path_blocks(dec.k, 2)
    got = run_search(dec, device_inputs(dec, x, y, cw, blocks))
    assert_same(got, model(x, y, cw, H, blocks), FRONT_KEYS + SEARCH_KEYS, which)


# ------------------------------------------------------------------------------------------------------- shape edges
@pytest.mark.parametrize("name", HM.STRUCTURES)
@pytest.mark.parametrize("k,n", osd_shapes.BOTH)
def test_shape_edges_match_the_model(k, n, name):
    H, _ = HM.code(k, n, name)
    dec = _decoder(("edge", k, n, name), H=H)
    assert dec.hosdx_supported and (dec.n, dec.k, dec.m) == (n, k, n - k)
    for mode in HM.MODES:
        c = HM.edge_case(k, n, name, mode)
        assert len(c["x"]) == HM.FRAMES
        got = run_search(dec, device_inputs(dec, np.array(c["x"]), np.array(c["y"]), c["cw"], c["blocks"]))
        assert got["cw"].shape == (HM.FRAMES, (n + 63) // 64)
        assert_same(got, c["want"], FRONT_KEYS + SEARCH_KEYS, (k, n, name, mode))


# ----------------------------------------------------------------------------------------------------- raw-call helpers
def _buffers(dec, rows, nblk, fill=0xA5):
    def buf(shape, dtype):
        t = torch.empty(shape, dtype=dtype, device=dec.device)
        t.view(torch.uint8).fill_(fill)
        return t
    return dict(lri=buf((rows, 128), torch.uint8), uidx=buf((rows, 128), torch.uint8), M=buf((rows, 64), torch.int64),
                nswaps=buf((rows,), torch.int32), block_min=buf((rows, nblk), torch.float32),
                block_arg=buf((rows, nblk), torch.int32), truth=buf((rows,), torch.float32),
                cw=buf((rows, dec.words), torch.int64), metric=buf((rows,), torch.float32), best=buf((rows,), torch.int32),
                deep_limit=buf((rows,), torch.int32), global_min=buf((rows,), torch.float32),
                success=buf((rows,), torch.uint8), teps=buf((rows,), torch.int32))


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def raw_front(dec, d, F, b, null=()):
    g = lambda key: None if key in null else _p(b[key])   # noqa: E731
    return dec.L.ldpc_hosdx_front(dec._ctx, _p(d["x"]), F, g("lri"), g("uidx"), g("M"), g("nswaps"), dec._stream())


def raw_search(dec, d, F, b, null=()):
    g = lambda key: None if key in null else _p(b[key])   # noqa: E731
    return dec.L.ldpc_hosdx_search(dec._ctx, _p(d["x"]), _p(d["y"]), F, g("lri"), g("uidx"), g("M"), _p(d["teps"]), _p(d["off"]),
                                   d["nblk"], _p(d["lab"]), g("block_min"), g("block_arg"), g("truth"), g("cw"), g("metric"),
                                   g("best"), dec._stream())


def raw_sliding(dec, d, F, b, win, margin, fw, group=0, null=()):
    g = lambda key: None if key in null else _p(b[key])   # noqa: E731
    fw = np.ascontiguousarray(fw, np.float32)
    return dec.L.ldpc_hosdx_sliding(dec._ctx, _p(d["x"]), _p(d["y"]), F, g("lri"), g("uidx"), g("M"), _p(d["teps"]), _p(d["off"]),
                                    d["nblk"], win, float(margin), fw.ctypes.data_as(C.POINTER(C.c_float)), fw.size, group,
                                    _p(d["lab"]), g("deep_limit"), g("global_min"), g("truth"), g("success"), g("cw"),
                                    g("metric"), g("best"), g("teps"), dec._stream())


# ---------------------------------------------------------------------------------------------------- untouched bytes
@pytest.mark.parametrize("k,n", [(5, 12), (48, 65), (33, 64)])
def test_pads_are_zero_and_nothing_beyond_F_is_written(k, n):
    H, _ = HM.code(k, n, "random_dense")
    dec = _decoder(("edge", k, n, "random_dense"), H=H)
    c = HM.edge_case(k, n, "random_dense", "float")
    F, extra, m = HM.FRAMES, 3, n - k
    d = device_inputs(dec, np.array(c["x"]), np.array(c["y"]), c["cw"], c["blocks"])
    b = _buffers(dec, F + extra, d["nblk"])
    fw = np.concatenate([a.ravel() for a in DM.stopping_fcn_weights(2)])
    assert raw_front(dec, d, F, b) == 0 and raw_search(dec, d, F, b) == 0
    torch.cuda.synchronize()
    first = {key: b[key].clone() for key in FRONT_KEYS + SEARCH_KEYS}
    assert_same({key: v[:F] for key, v in first.items()}, c["want"], FRONT_KEYS + SEARCH_KEYS)
    assert raw_sliding(dec, d, F, b, 2, 0.9, fw) == 0
    torch.cuda.synchronize()
    lri, uidx, M = (b[key].cpu().numpy() for key in ("lri", "uidx", "M"))
    assert not lri[:F, n:].any() and not uidx[:F, n:].any()
    Mu = M[:F].view(np.uint64)
    assert not Mu[:, m:].any() and (k == 64 or not (Mu >> np.uint64(k)).any())
    for key, t in b.items():
        assert (t[F:].contiguous().view(torch.uint8) == 0xA5).all(), key
    # dirty pads on the way in change nothing
    b2 = _buffers(dec, F + extra, d["nblk"])
    for key in ("lri", "uidx", "M"):
        b2[key][:F] = b[key][:F]
    b2["lri"][:F, n:] = 0xEE
    b2["uidx"][:F, n:] = 0xEE
    b2["M"][:F, m:] = -1
    if k < 64:
        b2["M"][:F, :m] |= -(1 << k)
    assert raw_search(dec, d, F, b2) == 0
    torch.cuda.synchronize()
    assert_same({key: b2[key][:F] for key in SEARCH_KEYS}, c["want"], SEARCH_KEYS)


# ----------------------------------------------------------------------------------------------------- nullable outputs
def test_every_nullable_output_alone(golden_dir):
    dec, H, G = real(golden_dir, "96_48")
    x, y, cw = HM.refined_frames(H, G, 2.0, 16, 7)
    d = device_inputs(dec, x, y, cw, HM.path_blocks(48, 1))
    fw = np.concatenate([a.ravel() for a in DM.stopping_fcn_weights(2)])
    F = 16
    full = _buffers(dec, F, d["nblk"])
    assert raw_front(dec, d, F, full) == 0 and raw_search(dec, d, F, full) == 0
    torch.cuda.synchronize()
    ref_search = {key: full[key].clone() for key in FRONT_KEYS + SEARCH_KEYS}
    assert raw_sliding(dec, d, F, full, 2, 0.9, fw) == 0
    torch.cuda.synchronize()
    ref_slide = {key: full[key].clone() for key in SLIDE_KEYS}
    cases = [("front", ("nswaps",))] + [("search", (key,)) for key in ("block_arg", "truth", "cw", "metric", "best")] \
        + [("sliding", (key,)) for key in SLIDE_KEYS]
    for call, null in cases:
        b = _buffers(dec, F, d["nblk"], fill=0x5A)
        for key in ("lri", "uidx", "M"):
            if call != "front":
                b[key].copy_(full[key])
        rc = {"front": lambda: raw_front(dec, d, F, b, null), "search": lambda: raw_search(dec, d, F, b, null),
              "sliding": lambda: raw_sliding(dec, d, F, b, 2, 0.9, fw, null=null)}[call]()
        assert rc == 0, (call, null)
        torch.cuda.synchronize()
        keys, ref = {"front": (FRONT_KEYS, ref_search), "search": (SEARCH_KEYS, ref_search), "sliding": (SLIDE_KEYS, ref_slide)}[call]
        assert_same(b, ref, [key for key in keys if key not in null], (call, null))
        assert (b[null[0]].view(torch.uint8) == 0x5A).all(), (call, null)


# ------------------------------------------------------------------------------------- several frames per workgroup
def test_several_frames_per_wavefront_and_workgroup(golden_dir):
    """The front end's grid takes 8192 x 4 frames in one pass, the scans' 8192 (grid_for in ldpc_hosd.hip): above that a
    wavefront / a workgroup takes several frames in turn.  The whole batch equals its grid-sized slices, and a sample of
    every trip equals the model."""
    dec, H, G = real(golden_dir, "96_48")
    front_grid, scan_grid = 8192 * 4, 8192
    Ff, Fs = 2 * front_grid + 7, 2 * scan_grid + 5
    rng = np.random.default_rng(12)
    y, cw = np_oracle.make_frames(G, 2.0, Ff, rng)[:2]
    y = np.ascontiguousarray(y, np.float32)
    x = np.ascontiguousarray(y + np.float32(0.5) * rng.standard_normal(y.shape).astype(np.float32), dtype=np.float32)
    blocks = HM.path_blocks(48, 1)
    d = device_inputs(dec, x, y, cw, blocks)
    whole = dec.hosdx_front(d["x"])
    parts = [dec.hosdx_front(d["x"][lo:lo + front_grid]) for lo in range(0, Ff, front_grid)]
    for i, key in enumerate(FRONT_KEYS):
        assert torch.equal(whole[i], torch.cat([p[i] for p in parts])), key
    sl = lambda t, lo, hi: t[lo:hi].contiguous()   # noqa: E731
    ws = dec.hosdx_search(d["x"][:Fs], d["y"][:Fs], tuple(t[:Fs] for t in whole), d["teps"], d["off"], label_bits=d["lab"][:Fs])
    fw = np.concatenate([a.ravel() for a in DM.stopping_fcn_weights(2)])
    wl = dec.hosdx_sliding(d["x"][:Fs], d["y"][:Fs], tuple(t[:Fs] for t in whole), d["teps"], d["off"], 2, 0.9, fw,
                           label_bits=d["lab"][:Fs])
    for lo in range(0, Fs, scan_grid):
        hi = min(lo + scan_grid, Fs)
        fr = tuple(sl(t, lo, hi) for t in whole)
        ps = dec.hosdx_search(sl(d["x"], lo, hi), sl(d["y"], lo, hi), fr, d["teps"], d["off"], label_bits=sl(d["lab"], lo, hi))
        assert_same({key: ws[key][lo:hi] for key in SEARCH_KEYS}, ps, SEARCH_KEYS, lo)
        pl = dec.hosdx_sliding(sl(d["x"], lo, hi), sl(d["y"], lo, hi), fr, d["teps"], d["off"], 2, 0.9, fw,
                               label_bits=sl(d["lab"], lo, hi))
        assert_same({key: wl[key][lo:hi] for key in SLIDE_KEYS}, pl, SLIDE_KEYS, lo)
    torch.cuda.synchronize()
    sel = np.array([t * scan_grid + w for t in range(3) for w in (0, 1, scan_grid // 2, scan_grid - 1) if t * scan_grid + w < Fs]
                   + [front_grid, 2 * front_grid - 1, 2 * front_grid, Ff - 1])
    want = model(x[sel], y[sel], cw[sel], H, blocks)
    st = torch.from_numpy(sel).to(dec.device)
    assert_same({key: whole[i][st] for i, key in enumerate(FRONT_KEYS)}, want, FRONT_KEYS)
    inside = np.flatnonzero(sel < Fs)
    si = st[torch.from_numpy(inside).to(dec.device)]
    assert_same({key: ws[key][si] for key in SEARCH_KEYS}, {key: want[key][inside] for key in SEARCH_KEYS}, SEARCH_KEYS)


# --------------------------------------------------------------------------------------------------- large table route
def test_work_item_form_on_an_order3_table(golden_dir):
    dec, H, G = real(golden_dir, "96_48")
    blocks = HM.path_blocks(48, 3)
    x, y, cw = HM.refined_frames(H, G, 1.0, 8, 3)
    d = device_inputs(dec, x, y, cw, blocks)
    assert int(d["off"][-1]) > 2304 and int(d["teps"][:, 3].max()) == 3        # beyond kHosdLdsTeps, weight 3: work items
    assert_same(run_search(dec, d), model(x, y, cw, H, blocks), FRONT_KEYS + SEARCH_KEYS)


# ---------------------------------------------------------------------------------------------------------- sliding stop
def early_fcn_weights(win, per_min, per_block=0.6):
    """z1 - z0 = per_min * min(window) + per_block * k: a frame whose first window is poor stops at once, the others go on
    until a later block improves on the minimum -- stops at both ends and in between on paths as short as these."""
    w1, w2 = np.eye(win + 1, dtype=np.float32), np.zeros((win + 1, 2), np.float32)
    w2[0, 1], w2[win, 1] = per_min, per_block
    return w1, w2


def _sliding_case(dec, H, G, blocks, win, w1, w2, margin, frames, seed):
    x, y, cw = HM.refined_frames(H, G, 1.0, frames, seed)
    nblk = len(blocks)
    off = np.insert(np.cumsum([len(E) for E in blocks]), 0, 0)
    exp = dict(deep_limit=np.zeros(frames, np.int32), global_min=np.zeros(frames, np.float32), success=np.zeros(frames, np.uint8))
    rows, near = [], 0
    for f in range(frames):
        r = HM.hosdx_frame(x[f], y[f], cw[f], H, blocks)
        fcn = DM.Classifier(w1, w2)
        s, wn, _, g = np_oracle.sliding_window_decide(r["block_min"], r["truth"], fcn, win, margin, off)
        near += fcn.near(margin) if margin < 1.0 else 0
        deep = wn + win - 1
        exp["deep_limit"][f], exp["global_min"][f], exp["success"][f] = deep, g, s
        rows.append(HM.hosdx_frame(x[f], y[f], cw[f], H, blocks[:deep]))
    assert near == 0, f"{near} classifier outputs within 1e-6 of the margin"
    exp["cw"] = HM.pack_cw(np.stack([r["codeword"] for r in rows]))
    exp["metric"] = np.array([r["metric"] for r in rows], np.float32)
    exp["best"] = np.array([r["best_index"] for r in rows], np.int32)
    d = device_inputs(dec, x, y, cw, blocks)
    front = dec.hosdx_front(d["x"])
    fw = np.concatenate([w1.ravel(), w2.ravel()])
    for group in (0, 1, nblk):
        out = dec.hosdx_sliding(d["x"], d["y"], front, d["teps"], d["off"], win, margin, fw, label_bits=d["lab"], group=group)
        torch.cuda.synchronize()
        assert_same(out, exp, ("deep_limit", "global_min", "success", "cw", "metric", "best"), (win, margin, group))
    return exp


@pytest.mark.parametrize("win", [1, 3])
@pytest.mark.parametrize("which", ["96_48", "5_12"])
def test_sliding_stop_matches_the_oracle(golden_dir, which, win):
    if which == "96_48":
        dec, H, G = real(golden_dir, which)
        blocks, frames = HM.path_blocks(48, 2), 24
    else:
        H, G = HM.code(5, 12, "random_dense")
        dec = _decoder(("edge", 5, 12, "random_dense"), H=H)
        blocks, frames = [E for E in HM.path_blocks(5, 2) if len(E)], 48
    assert len(blocks) >= 3
    sw, rw = DM.stopping_fcn_weights(win), DM.random_fcn_weights(np.random.default_rng(win), win)
    ew = early_fcn_weights(win, 0.3 if which == "96_48" else 2.5)
    depths = set()
    for (w1, w2), margin in ((sw, 0.9), (ew, 0.9), (rw, 0.9), (rw, 0.0), (sw, 1.0)):
        exp = _sliding_case(dec, H, G, blocks, win, w1, w2, margin, frames, 50 + win)
        if w1 is ew[0]:
            depths |= set(exp["deep_limit"].tolist())
        if margin == 1.0:
            assert (exp["deep_limit"] == len(blocks)).all()
    assert len(depths) > 1, depths


# -------------------------------------------------------------------------------------------------------------- refusals
def _refused_decoders(golden_dir):
    H70, _ = osd_shapes.context_graph(70, 87)
    return [(_decoder("array60", path=os.path.join(golden_dir, "ArrayCode_N121_K60_r0.50.alist")), r"66 rows.*n-k = 61.*\(121,60\)"),
            (_decoder("array80", path=os.path.join(golden_dir, "ArrayCode_N121_K80_r0.66.alist")), r"rows.*n-k = 41.*\(121,80\)"),
            (_decoder("wide70", H=H70), r"17 rows.*n-k = 17.*\(87,70\)")]


def test_refusals(golden_dir):
    from short_ldpc_decoding_osd_amd import _lib
    fw = np.concatenate([a.ravel() for a in DM.stopping_fcn_weights(2)])
    for dec, tail in _refused_decoders(golden_dir):
        assert not dec.hosdx_supported
        x = torch.zeros((4, dec.n), dtype=torch.float32, device=dec.device)
        front = (torch.zeros((4, 128), dtype=torch.uint8, device=dec.device), torch.zeros((4, 128), dtype=torch.uint8, device=dec.device),
                 torch.zeros((4, 64), dtype=torch.int64, device=dec.device))
        teps = torch.zeros((3, 4), dtype=torch.uint8, device=dec.device)
        off = torch.tensor([0, 1, 3], dtype=torch.int32, device=dec.device)
        msg = r"\(-5\).*1 <= k <= 64 and an H of exactly n-k <= 64 rows.*" + tail
        with pytest.raises(_lib.LdpcError, match="ldpc_hosdx_front.*" + msg):
            dec.hosd_front(x)
        with pytest.raises(_lib.LdpcError, match="ldpc_hosdx_search.*" + msg):
            dec.hosd_search(x, x, front, teps, off)
        with pytest.raises(_lib.LdpcError, match="ldpc_hosdx_sliding.*" + msg):
            dec.hosd_sliding(x, x, front, teps, off, 2, 0.9, fw)


def test_argument_errors_and_empty_batch(golden_dir):
    from short_ldpc_decoding_osd_amd import _lib
    dec, H, G = real(golden_dir, "96_48")
    x, y, cw = HM.refined_frames(H, G, 2.0, 4, 1)
    d = device_inputs(dec, x, y, cw, HM.path_blocks(48, 1))
    b = _buffers(dec, 4, d["nblk"])
    fw = np.concatenate([a.ravel() for a in DM.stopping_fcn_weights(2)])
    with pytest.raises(_lib.LdpcError, match=r"\(-5\).*need n=128, m=k=64; this code is n=96 m=48 k=48"):
        _lib.check(dec.L.ldpc_hosd_front(dec._ctx, _p(d["x"]), 4, _p(b["lri"]), _p(b["uidx"]), _p(b["M"]), None, None), "ldpc_hosd_front")
    for key in ("lri", "uidx", "M"):
        with pytest.raises(_lib.LdpcError, match=rf"\(-1\).*ldpc_hosdx_front: d_{key} is NULL"):
            _lib.check(raw_front(dec, d, 4, b, null=(key,)))
        with pytest.raises(_lib.LdpcError, match=rf"\(-1\).*ldpc_hosdx_search: d_{key} is NULL"):
            _lib.check(raw_search(dec, d, 4, b, null=(key,)))
        with pytest.raises(_lib.LdpcError, match=rf"\(-1\).*ldpc_hosdx_sliding: d_{key} is NULL"):
            _lib.check(raw_sliding(dec, d, 4, b, 2, 0.9, fw, null=(key,)))
    with pytest.raises(_lib.LdpcError, match=r"\(-1\).*ldpc_hosdx_search: d_block_min is NULL"):
        _lib.check(raw_search(dec, d, 4, b, null=("block_min",)))
    with pytest.raises(_lib.LdpcError, match=r"\(-1\).*ldpc_hosdx_search: d_order_llr is NULL"):
        _lib.check(raw_search(dec, dict(d, x=None), 4, b))
    torch.cuda.synchronize()
    for key, t in b.items():                                     # all of it refused before any launch
        assert (t.view(torch.uint8) == 0xA5).all(), key
    none = dict(x=None, y=None, lab=None, teps=None, off=None, nblk=d["nblk"])
    nob = {key: None for key in b}
    assert raw_front(dec, none, 0, nob) == 0 and raw_search(dec, none, 0, nob) == 0
    assert raw_sliding(dec, none, 0, nob, 2, 0.9, fw) == 0
    e = dec.empty((0, 96), torch.float32)
    assert dec.hosd_front(e)[0].shape == (0, 128)


# --------------------------------------------------------------------------------------------------------- graph capture
def test_graph_capture_front_and_sliding(golden_dir):
    dec, H, G = real(golden_dir, "96_48")
    x, y, cw = HM.refined_frames(H, G, 1.0, 128, 9)
    d = device_inputs(dec, x, y, cw, HM.path_blocks(48, 2))
    fw = np.concatenate([a.ravel() for a in early_fcn_weights(3, 0.3)])

    def step():
        fr = dec.hosd_front(d["x"])
        out = dec.hosd_sliding(d["x"], d["y"], fr, d["teps"], d["off"], 3, 0.9, fw, label_bits=d["lab"])
        return dict(out, lri=fr[0], uidx=fr[1], M=fr[2], nswaps=fr[3])

    eager = {key: v.clone() for key, v in step().items()}
    torch.cuda.synchronize()
    s = torch.cuda.Stream(dec.device)
    s.wait_stream(torch.cuda.current_stream(dec.device))
    with torch.cuda.stream(s):
        step()                                     # warm-up on the capture stream
    torch.cuda.current_stream(dec.device).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = step()
    g.replay()
    torch.cuda.synchronize()
    for key, v in eager.items():
        assert torch.equal(out[key], v), key
    assert len(torch.unique(eager["deep_limit"])) > 1
