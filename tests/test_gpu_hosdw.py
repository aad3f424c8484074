"""-m gpu: the wide H-form OSD primitives (ldpc_hosdw_front / _search / _sliding: k up to 127, an H with redundant rows)
against the any-shape kernels wherever those serve the code, and against the NumPy model (tests/hosdw_model.py) on the two
array codes, on structured codes with k > 64 and on constructed redundant-row codes at the shape edges.  Unless stated
otherwise every comparison is array_equal on bit patterns."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import np_oracle
from tests import dlosd_model as DM
from tests import hosdw_model as WM
from tests import hosdx_model as HM
from tests.test_gpu_hosdx import FRONT_KEYS, SEARCH_KEYS, SLIDE_KEYS, _p, assert_same, device_inputs, early_fcn_weights

pytestmark = pytest.mark.gpu

ARRAY_SNRS, REDUNDANT = WM.ARRAY_SNRS, WM.REDUNDANT
WIDE_SHAPES = ((65, 66), (65, 128), (70, 87), (100, 108), (112, 128), (127, 128))
_decoders = {}


def _decoder(key, H=None, path=None):
    from short_ldpc_decoding_osd_amd import Code
    from short_ldpc_decoding_osd_amd.runtime import Decoder
    if key not in _decoders:
        code = Code(H=np.array(H)) if H is not None else (Code(path) if path else Code())
        _decoders[key] = Decoder(code)
    return _decoders[key]


def array_decoder(golden_dir, which, reverse=False):
    if not reverse:
        return _decoder(which, path=os.path.join(golden_dir, WM.ARRAY[which]))
    H = np_oracle.Code(os.path.join(golden_dir, WM.ARRAY[which])).H
    return _decoder((which, "reversed"), H=np.ascontiguousarray(H[::-1]))


def run_front(dec, d):
    return dict(zip(FRONT_KEYS, dec.hosdw_front(d["x"])))


def run_search(dec, d):
    """hosdw_front + hosdw_search -> the dict of WM.packed."""
    fr = run_front(dec, d)
    out = dec.hosdw_search(d["x"], d["y"], (fr["lri"], fr["uidx"], fr["M"]), d["teps"], d["off"], label_bits=d["lab"])
    torch.cuda.synchronize()
    return dict(out, **fr)


def fcn(w):
    return np.concatenate([a.ravel() for a in w])


# ------------------------------------------------------------------------------------------ parity with ldpc_hosdx_*
@pytest.mark.parametrize("which", ["128_64", "96_48", "64_32", (5, 12), (33, 64), (64, 65)])
def test_parity_with_the_any_shape_kernels(golden_dir, np_code, which):
    if which == "128_64":
        dec, H, G = _decoder("ccsds"), np_code.H, np_code.G
    elif isinstance(which, str):
        path = os.path.join(golden_dir, {"96_48": "LDPC_N96_K48_P8_set0_dmin10.alist", "64_32": "code1.alist"}[which])
        c = np_oracle.Code(path)
        dec, H, G = _decoder(which, path=path), c.H, c.G
    else:
        H, G = HM.code(*which, "random_dense")
        dec = _decoder(("edge",) + which, H=H)
    assert dec.hosdx_supported and dec.hosdw_supported and dec.hosd_stage_family() != "hosdw"
    x, y, cw = HM.refined_frames(H, G, 2.0, 48, 31)
    x[3, : dec.n // 2] = np.float32(0.5) * np.sign(x[3, : dec.n // 2])
    y[5, 2] = 0.0
    blocks = [E for E in HM.path_blocks(dec.k, 2) if len(E)] if dec.k > 4 else list(HM.edge_blocks(dec.k))
    d = device_inputs(dec, x, y, cw, blocks)
    old, new = dec.hosdx_front(d["x"]), dec.hosdw_front(d["x"])
    for a, b, key in zip(old, new, FRONT_KEYS):
        if key == "M":
            assert b.shape == (48, 128) and torch.equal(a, b[:, :64]) and not b[:, 64:].any()
        else:
            assert torch.equal(a, b), key
    so = dec.hosdx_search(d["x"], d["y"], old, d["teps"], d["off"], label_bits=d["lab"])
    sn = dec.hosdw_search(d["x"], d["y"], new, d["teps"], d["off"], label_bits=d["lab"])
    assert_same(sn, so, SEARCH_KEYS)
    win = min(3, d["nblk"])
    for w in (DM.stopping_fcn_weights(win), DM.random_fcn_weights(np.random.default_rng(2), win)):
        for group in (0, 1):
            lo = dec.hosdx_sliding(d["x"], d["y"], old, d["teps"], d["off"], win, 0.9, fcn(w), label_bits=d["lab"], group=group)
            ln = dec.hosdw_sliding(d["x"], d["y"], new, d["teps"], d["off"], win, 0.9, fcn(w), label_bits=d["lab"], group=group)
            assert_same(ln, lo, SLIDE_KEYS, group)


# ------------------------------------------------------------------------------------------------------- array codes
@pytest.mark.parametrize("snr", ARRAY_SNRS)
@pytest.mark.parametrize("which", sorted(WM.ARRAY))
def test_array_codes_match_the_model(golden_dir, which, snr):
    dec = array_decoder(golden_dir, which)
    assert dec.hosdw_supported and not dec.hosdx_supported and dec.hosd_stage_family() == "hosdw"
    c = WM.array_case(golden_dir, which, snr)
    assert (dec.n, dec.k, dec.m) == (121, c["G"].shape[0], c["H"].shape[0])
    got = run_search(dec, device_inputs(dec, c["x"], c["y"], c["cw"], c["blocks"]))
    assert_same(got, WM.packed(c["results"], len(c["blocks"])), FRONT_KEYS + SEARCH_KEYS, (which, snr))
    b1 = HM.path_blocks(dec.k, 1)                                    # the order-1 path on the first frames
    got = run_search(dec, device_inputs(dec, c["x"][:12], c["y"][:12], c["cw"][:12], b1))
    assert_same(got, WM.model(c["x"][:12], c["y"][:12], c["cw"][:12], c["H"], b1), FRONT_KEYS + SEARCH_KEYS, (which, snr, 1))


def test_row_order_of_H_decides_the_exchanges(golden_dir):
    """A context on (121,60) with the rows of H reversed equals the model of the reversed H, and its front-end results differ
    from those of H as given on exactly the frames where the models differ."""
    a, r = WM.array_case(golden_dir, "121_60", ARRAY_SNRS[0]), WM.array_case(golden_dir, "121_60", ARRAY_SNRS[0], reverse=True)
    da, dr = array_decoder(golden_dir, "121_60"), array_decoder(golden_dir, "121_60", reverse=True)
    d = device_inputs(dr, r["x"], r["y"], r["cw"], r["blocks"])
    got_r = run_search(dr, d)
    want_a, want_r = WM.packed(a["results"], len(a["blocks"])), WM.packed(r["results"], len(r["blocks"]))
    assert_same(got_r, want_r, FRONT_KEYS + SEARCH_KEYS)
    got_a = run_front(da, device_inputs(da, a["x"], a["y"], a["cw"], a["blocks"]))
    differ = np.array([(want_a[key][f] != want_r[key][f]).any() for f in range(len(a["x"])) for key in ("uidx", "M")]).reshape(-1, 2).any(1)
    assert 0 < differ.sum() < len(differ)
    seen = ((got_a["uidx"] != got_r["uidx"]).any(1) | (got_a["M"] != got_r["M"]).any(1)).cpu().numpy()
    assert np.array_equal(seen, differ)


# ----------------------------------------------------------------------------------------------------- sliding stop
def _sliding_case(dec, c, frames, win, w, margin):
    """tests/test_gpu_hosdx.py's _sliding_case on the first ``frames`` frames of a model case."""
    H, blocks = c["H"], c["blocks"]
    m = H.shape[1] - dec.k
    x, y, cw = c["x"][:frames], c["y"][:frames], c["cw"][:frames]
    off = np.insert(np.cumsum([len(E) for E in blocks]), 0, 0)
    exp = dict(deep_limit=np.zeros(frames, np.int32), global_min=np.zeros(frames, np.float32), success=np.zeros(frames, np.uint8))
    rows, near = [], 0
    for f in range(frames):
        r = c["results"][f]
        net = DM.Classifier(*w)
        s, wn, _, g = np_oracle.sliding_window_decide(r["block_min"], r["truth"], net, win, margin, off)
        near += net.near(margin) if margin < 1.0 else 0
        deep = wn + win - 1
        exp["deep_limit"][f], exp["global_min"][f], exp["success"][f] = deep, g, s
        rows.append(r if deep == len(blocks) else WM.hosdw_frame(x[f], y[f], cw[f], H, blocks[:deep], m))
    assert near == 0, f"{near} classifier outputs within 1e-6 of the margin"
    exp["cw"] = HM.pack_cw(np.stack([r["codeword"] for r in rows]))
    exp["metric"] = np.array([r["metric"] for r in rows], np.float32)
    exp["best"] = np.array([r["best_index"] for r in rows], np.int32)
    d = device_inputs(dec, x, y, cw, blocks)
    front = dec.hosdw_front(d["x"])
    for group in (0, 1, len(blocks)):
        out = dec.hosdw_sliding(d["x"], d["y"], front, d["teps"], d["off"], win, margin, fcn(w), label_bits=d["lab"], group=group)
        torch.cuda.synchronize()
        assert_same(out, exp, ("deep_limit", "global_min", "success", "cw", "metric", "best"), (win, margin, group))
    return exp


@pytest.mark.parametrize("win", [2, 3])
@pytest.mark.parametrize("which", sorted(WM.ARRAY))
def test_sliding_stop_matches_the_oracle(golden_dir, which, win):
    dec = array_decoder(golden_dir, which)
    c = WM.array_case(golden_dir, which, ARRAY_SNRS[0])
    sw, ew = DM.stopping_fcn_weights(win), early_fcn_weights(win, 0.3)
    depths = set()
    for w, margin in ((sw, 0.9), (ew, 0.9), (sw, 1.0)):
        exp = _sliding_case(dec, c, 16, win, w, margin)
        if w is ew:
            depths |= set(exp["deep_limit"].tolist())
        if margin == 1.0:
            assert (exp["deep_limit"] == len(c["blocks"])).all()
    assert len(depths) > 1, depths


# ------------------------------------------------------------------------------------------------ k > 64, full rank
@pytest.mark.parametrize("name", HM.STRUCTURES)
@pytest.mark.parametrize("k,n", WIDE_SHAPES)
def test_high_rate_shapes_match_the_model(k, n, name):
    H, _ = HM.code(k, n, name)
    dec = _decoder(("wide", k, n, name), H=H)
    assert dec.hosdw_supported and not dec.hosdx_supported and (dec.n, dec.k, dec.m) == (n, k, n - k)
    for mode in HM.MODES:
        c = WM.case(k, n, name, mode)
        assert len(c["x"]) == WM.FRAMES
        got = run_search(dec, device_inputs(dec, np.array(c["x"]), np.array(c["y"]), c["cw"], c["blocks"]))
        assert got["cw"].shape == (WM.FRAMES, (n + 63) // 64) and got["M"].shape == (WM.FRAMES, 128)
        assert_same(got, c["want"], FRONT_KEYS + SEARCH_KEYS, (k, n, name, mode))


def test_both_scan_forms_are_covered():
    sizes = {k: sum(len(E) for E in WM.wide_blocks(k)) for k, _ in WIDE_SHAPES}
    assert min(sizes.values()) <= 2304 < max(sizes.values()) < 6000      # kHosdLdsTeps: per-thread runs below, work items above


# -------------------------------------------------------------------------------------- redundant rows at the edges
@pytest.mark.parametrize("k,n,R,style", REDUNDANT)
def test_redundant_rows_match_the_model(k, n, R, style):
    for name in ("random_dense", "equal_cols"):
        H, _ = WM.redundant(k, n, name, R, style)
        dec = _decoder(("redundant", k, n, R, style, name), H=H)
        assert dec.hosdw_supported and not dec.hosdx_supported and (dec.n, dec.k, dec.m) == (n, k, R)
        for mode in ("float", "grid"):
            c = WM.case(k, n, name, mode, R, style)
            got = run_search(dec, device_inputs(dec, np.array(c["x"]), np.array(c["y"]), c["cw"], c["blocks"]))
            assert_same(got, c["want"], FRONT_KEYS + SEARCH_KEYS, (k, n, R, style, name, mode))


# ----------------------------------------------------------------------------------------------------- raw-call helpers
def _buffers(dec, rows, nblk, fill=0xA5):
    def buf(shape, dtype):
        t = torch.empty(shape, dtype=dtype, device=dec.device)
        t.view(torch.uint8).fill_(fill)
        return t
    return dict(lri=buf((rows, 128), torch.uint8), uidx=buf((rows, 128), torch.uint8), M=buf((rows, 128), torch.int64),
                nswaps=buf((rows,), torch.int32), block_min=buf((rows, nblk), torch.float32),
                block_arg=buf((rows, nblk), torch.int32), truth=buf((rows,), torch.float32),
                cw=buf((rows, dec.words), torch.int64), metric=buf((rows,), torch.float32), best=buf((rows,), torch.int32),
                deep_limit=buf((rows,), torch.int32), global_min=buf((rows,), torch.float32),
                success=buf((rows,), torch.uint8), teps=buf((rows,), torch.int32))


def raw_front(dec, d, F, b, null=()):
    g = lambda key: None if key in null else _p(b[key])   # noqa: E731
    return dec.L.ldpc_hosdw_front(dec._ctx, _p(d["x"]), F, g("lri"), g("uidx"), g("M"), g("nswaps"), dec._stream())


def raw_search(dec, d, F, b, null=()):
    g = lambda key: None if key in null else _p(b[key])   # noqa: E731
    return dec.L.ldpc_hosdw_search(dec._ctx, _p(d["x"]), _p(d["y"]), F, g("lri"), g("uidx"), g("M"), _p(d["teps"]), _p(d["off"]),
                                   d["nblk"], _p(d["lab"]), g("block_min"), g("block_arg"), g("truth"), g("cw"), g("metric"),
                                   g("best"), dec._stream())


def raw_sliding(dec, d, F, b, win, margin, fw, group=0, null=()):
    g = lambda key: None if key in null else _p(b[key])   # noqa: E731
    fw = np.ascontiguousarray(fw, np.float32)
    return dec.L.ldpc_hosdw_sliding(dec._ctx, _p(d["x"]), _p(d["y"]), F, g("lri"), g("uidx"), g("M"), _p(d["teps"]), _p(d["off"]),
                                    d["nblk"], win, float(margin), fw.ctypes.data_as(C.POINTER(C.c_float)), fw.size, group,
                                    _p(d["lab"]), g("deep_limit"), g("global_min"), g("truth"), g("success"), g("cw"),
                                    g("metric"), g("best"), g("teps"), dec._stream())


# ---------------------------------------------------------------------------------------------------- untouched bytes
@pytest.mark.parametrize("k,n,R", [(5, 12, 9), (70, 87, None), (33, 64, 65)])
def test_pads_are_zero_and_nothing_beyond_F_is_written(k, n, R):
    c = WM.case(k, n, "random_dense", "float", R)
    dec = _decoder(("pads", k, n, R), H=c["H"])
    F, extra, m = WM.FRAMES, 3, n - k
    d = device_inputs(dec, np.array(c["x"]), np.array(c["y"]), c["cw"], c["blocks"])
    b = _buffers(dec, F + extra, d["nblk"])
    assert raw_front(dec, d, F, b) == 0 and raw_search(dec, d, F, b) == 0
    torch.cuda.synchronize()
    first = {key: b[key].clone() for key in FRONT_KEYS + SEARCH_KEYS}
    assert_same({key: v[:F] for key, v in first.items()}, c["want"], FRONT_KEYS + SEARCH_KEYS)
    assert raw_sliding(dec, d, F, b, 2, 0.9, fcn(DM.stopping_fcn_weights(2))) == 0
    torch.cuda.synchronize()
    lri, uidx, M = (b[key].cpu().numpy() for key in ("lri", "uidx", "M"))
    assert not lri[:F, n:].any() and not uidx[:F, n:].any()
    Mu = M[:F].view(np.uint64)
    assert not Mu[:, m:64].any() and not Mu[:, 64 + m:].any()
    lo, hi = min(k, 64), max(k - 64, 0)
    assert (lo == 64 or not (Mu[:, :64] >> np.uint64(lo)).any()) and (not (Mu[:, 64:] >> np.uint64(hi)).any() if hi else not Mu[:, 64:].any())
    for key, t in b.items():
        assert (t[F:].contiguous().view(torch.uint8) == 0xA5).all(), key
    # dirty pads on the way in change nothing
    b2 = _buffers(dec, F + extra, d["nblk"])
    for key in ("lri", "uidx", "M"):
        b2[key][:F] = b[key][:F]
    b2["lri"][:F, n:] = 0xEE
    b2["uidx"][:F, n:] = 0xEE
    b2["M"][:F, m:64] = -1
    b2["M"][:F, 64 + m:] = -1
    if lo < 64:
        b2["M"][:F, :m] |= -(1 << lo)
    if hi < 64:
        b2["M"][:F, 64:64 + m] |= -(1 << hi)
    assert raw_search(dec, d, F, b2) == 0
    torch.cuda.synchronize()
    assert_same({key: b2[key][:F] for key in SEARCH_KEYS}, c["want"], SEARCH_KEYS)


# ----------------------------------------------------------------------------------------------------- nullable outputs
def test_every_nullable_output_alone(golden_dir):
    dec = array_decoder(golden_dir, "121_80")
    c = WM.array_case(golden_dir, "121_80", ARRAY_SNRS[0])
    F = 16
    d = device_inputs(dec, c["x"][:F], c["y"][:F], c["cw"][:F], HM.path_blocks(80, 1))
    fw = fcn(DM.stopping_fcn_weights(2))
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
    """The front end's grid takes 8192 x 4 frames in one pass, the scans' 8192 (grid_for in ldpc_hosd.hip), and nothing
    but the frame count sets it: above that a wavefront / a workgroup takes several frames in turn.  The whole batch
    equals its grid-sized slices, and a sample of every trip equals the model."""
    dec = array_decoder(golden_dir, "121_80")
    c = np_oracle.Code(os.path.join(golden_dir, WM.ARRAY["121_80"]))
    front_grid, scan_grid = 8192 * 4, 8192
    Ff, Fs = front_grid + 7, scan_grid + 5
    rng = np.random.default_rng(12)
    y, cw = np_oracle.make_frames(c.G, 2.0, Ff, rng)[:2]
    y = np.ascontiguousarray(y, np.float32)
    x = np.ascontiguousarray(y + np.float32(0.5) * rng.standard_normal(y.shape).astype(np.float32), dtype=np.float32)
    blocks = HM.path_blocks(80, 1)
    d = device_inputs(dec, x, y, cw, blocks)
    whole = dec.hosdw_front(d["x"])
    parts = [dec.hosdw_front(d["x"][lo:lo + front_grid]) for lo in range(0, Ff, front_grid)]
    for i, key in enumerate(FRONT_KEYS):
        assert torch.equal(whole[i], torch.cat([p[i] for p in parts])), key
    sl = lambda t, lo, hi: t[lo:hi].contiguous()   # noqa: E731
    fw = fcn(DM.stopping_fcn_weights(2))
    args = lambda lo, hi: (sl(d["x"], lo, hi), sl(d["y"], lo, hi), tuple(sl(t, lo, hi) for t in whole), d["teps"], d["off"])   # noqa: E731
    ws = dec.hosdw_search(*args(0, Fs), label_bits=sl(d["lab"], 0, Fs))
    wl = dec.hosdw_sliding(*args(0, Fs), 2, 0.9, fw, label_bits=sl(d["lab"], 0, Fs))
    for lo in range(0, Fs, scan_grid):
        hi = min(lo + scan_grid, Fs)
        ps = dec.hosdw_search(*args(lo, hi), label_bits=sl(d["lab"], lo, hi))
        assert_same({key: ws[key][lo:hi] for key in SEARCH_KEYS}, ps, SEARCH_KEYS, lo)
        pl = dec.hosdw_sliding(*args(lo, hi), 2, 0.9, fw, label_bits=sl(d["lab"], lo, hi))
        assert_same({key: wl[key][lo:hi] for key in SLIDE_KEYS}, pl, SLIDE_KEYS, lo)
    torch.cuda.synchronize()
    sel = np.array([0, 1, scan_grid - 1, scan_grid, Fs - 1, front_grid - 1, front_grid, Ff - 1])
    want = WM.model(x[sel], y[sel], cw[sel], c.H, blocks)
    st = torch.from_numpy(sel).to(dec.device)
    assert_same({key: whole[i][st] for i, key in enumerate(FRONT_KEYS)}, want, FRONT_KEYS)
    inside = np.flatnonzero(sel < Fs)
    si = st[torch.from_numpy(inside).to(dec.device)]
    assert_same({key: ws[key][si] for key in SEARCH_KEYS}, {key: want[key][inside] for key in SEARCH_KEYS}, SEARCH_KEYS)


# --------------------------------------------------------------------------------------------------- large table route
def test_work_item_form_on_an_order3_table(golden_dir):
    dec = array_decoder(golden_dir, "121_80")
    c = WM.array_case(golden_dir, "121_80", ARRAY_SNRS[0])
    blocks = HM.path_blocks(80, 3)
    x, y, cw = c["x"][:12], c["y"][:12], c["cw"][:12]
    d = device_inputs(dec, x, y, cw, blocks)
    assert int(d["off"][-1]) > 2304 and int(d["teps"][:, 3].max()) == 3 and int(d["teps"][:, :3].max()) == 79
    assert_same(run_search(dec, d), WM.model(x, y, cw, c["H"], blocks), FRONT_KEYS + SEARCH_KEYS)


# -------------------------------------------------------------------------------------------------------------- refusals
def test_refusal_names_the_entry_point_and_the_shape(golden_dir):
    from short_ldpc_decoding_osd_amd import _lib
    dec = _decoder("wimax", path=os.path.join(golden_dir, "wimax_1056_0.83.alist"))
    assert not dec.hosdw_supported and not dec.hosdx_supported
    x = torch.zeros((4, dec.n), dtype=torch.float32, device=dec.device)
    front = (torch.zeros((4, 128), dtype=torch.uint8, device=dec.device), torch.zeros((4, 128), dtype=torch.uint8, device=dec.device),
             torch.zeros((4, 128), dtype=torch.int64, device=dec.device))
    teps = torch.zeros((3, 4), dtype=torch.uint8, device=dec.device)
    off = torch.tensor([0, 1, 3], dtype=torch.int32, device=dec.device)
    msg = rf"\(-5\).*n <= 128, an H of 1 <= R <= 127 rows and 1 <= n-k <= 64; this H has {dec.m} rows, n-k = {dec.n - dec.k}, " \
          rf"code \({dec.n},{dec.k}\)"
    assert dec.n == 1056
    with pytest.raises(_lib.LdpcError, match="ldpc_hosdw_front.*" + msg):
        dec.hosdw_front(x)
    with pytest.raises(_lib.LdpcError, match="ldpc_hosdw_search.*" + msg):
        dec.hosdw_search(x, x, front, teps, off)
    with pytest.raises(_lib.LdpcError, match="ldpc_hosdw_sliding.*" + msg):
        dec.hosdw_sliding(x, x, front, teps, off, 2, 0.9, fcn(DM.stopping_fcn_weights(2)))
    with pytest.raises(_lib.LdpcError, match="ldpc_hosdw_front"):
        dec.hosd_stage("front")(x)                                  # the stage's selector lands on the same refusal


def test_argument_errors_and_empty_batch(golden_dir):
    from short_ldpc_decoding_osd_amd import _lib
    dec = array_decoder(golden_dir, "121_60")
    c = WM.array_case(golden_dir, "121_60", ARRAY_SNRS[0])
    d = device_inputs(dec, c["x"][:4], c["y"][:4], c["cw"][:4], HM.path_blocks(60, 1))
    b = _buffers(dec, 4, d["nblk"])
    fw = fcn(DM.stopping_fcn_weights(2))
    for key in ("lri", "uidx", "M"):
        with pytest.raises(_lib.LdpcError, match=rf"\(-1\).*ldpc_hosdw_front: d_{key} is NULL"):
            _lib.check(raw_front(dec, d, 4, b, null=(key,)))
        with pytest.raises(_lib.LdpcError, match=rf"\(-1\).*ldpc_hosdw_search: d_{key} is NULL"):
            _lib.check(raw_search(dec, d, 4, b, null=(key,)))
        with pytest.raises(_lib.LdpcError, match=rf"\(-1\).*ldpc_hosdw_sliding: d_{key} is NULL"):
            _lib.check(raw_sliding(dec, d, 4, b, 2, 0.9, fw, null=(key,)))
    with pytest.raises(_lib.LdpcError, match=r"\(-1\).*ldpc_hosdw_search: d_block_min is NULL"):
        _lib.check(raw_search(dec, d, 4, b, null=("block_min",)))
    with pytest.raises(_lib.LdpcError, match=r"\(-1\).*ldpc_hosdw_search: d_order_llr is NULL"):
        _lib.check(raw_search(dec, dict(d, x=None), 4, b))
    with pytest.raises(_lib.LdpcError, match=r"\(-5\).*ldpc_hosdw_search: 1025 TEP blocks, at most 1024"):
        _lib.check(raw_search(dec, dict(d, nblk=1025), 4, b))
    with pytest.raises(_lib.LdpcError, match=r"\(-1\).*ldpc_hosdw_sliding: bad arguments"):
        _lib.check(raw_sliding(dec, d, 4, b, 16, 0.9, fw))
    with pytest.raises(ValueError, match="hosdw takes M"):
        dec.hosdw_search(d["x"], d["y"], (b["lri"], b["uidx"], b["M"][:, :64].contiguous()), d["teps"], d["off"])
    torch.cuda.synchronize()
    for key, t in b.items():                                     # all of it refused before any launch
        assert (t.view(torch.uint8) == 0xA5).all(), key
    none = dict(x=None, y=None, lab=None, teps=None, off=None, nblk=d["nblk"])
    nob = {key: None for key in b}
    assert raw_front(dec, none, 0, nob) == 0 and raw_search(dec, none, 0, nob) == 0
    assert raw_sliding(dec, none, 0, nob, 2, 0.9, fw) == 0
    assert dec.hosdw_front(dec.empty((0, 121), torch.float32))[2].shape == (0, 128)


# --------------------------------------------------------------------------------------------------------- graph capture
def test_graph_capture_front_and_sliding(golden_dir):
    dec = array_decoder(golden_dir, "121_60")
    c = WM.array_case(golden_dir, "121_60", ARRAY_SNRS[0])
    d = device_inputs(dec, c["x"], c["y"], c["cw"], c["blocks"])
    fw = fcn(early_fcn_weights(3, 0.3))

    def step():
        fr = dec.hosdw_front(d["x"])
        out = dec.hosdw_sliding(d["x"], d["y"], fr, d["teps"], d["off"], 3, 0.9, fw, label_bits=d["lab"])
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
