"""-m gpu: the long H-form OSD primitives (ldpc_hosdl_front / _search / _sliding: n <= 384, an H of at most 192 rows, k <= 192)
against the NumPy model (tests/hosdl_model.py) at the shape edges, on redundant-row codes and on the (384,192) code of
tests/golden, against the reference-made elimination fixture, and against the wide kernels wherever those serve the code.
Unless stated otherwise every comparison is array_equal on bit patterns."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import np_oracle
from tests import dlosd_model as DM
from tests import hosdl_model as LM
from tests import hosdw_model as WM
from tests import hosdx_model as HM
from tests.test_gpu_hosdx import FRONT_KEYS, SEARCH_KEYS, SLIDE_KEYS, _p, device_inputs, early_fcn_weights

pytestmark = pytest.mark.gpu

# Frames per trip of each kernel, from its launcher (ldpc_hosdl.h): kHosdlFrontGrid workgroups of one wavefront for the front
# end, kHosdlScanGrid workgroups for the scans, one frame each per trip.
FRONT_GRID, SCAN_GRID = 32768, 8192
_decoders = {}


def _decoder(key, H=None, path=None):
    from short_ldpc_decoding_osd_amd import Code
    from short_ldpc_decoding_osd_amd.runtime import Decoder
    if key not in _decoders:
        code = Code(H=np.array(H)) if H is not None else (Code(path) if path else Code())
        _decoders[key] = Decoder(code)
    return _decoders[key]


def bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_same(got, want, keys, what=""):
    for key in keys:
        assert np.array_equal(bits(got[key]), bits(want[key])), (key, what)


def golden_decoder(golden_dir):
    return _decoder("golden384", path=os.path.join(golden_dir, LM.GOLDEN_ALIST))


def run_front(dec, d):
    return dict(zip(FRONT_KEYS, dec.hosdl_front(d["x"])))


def run_search(dec, d):
    """hosdl_front + hosdl_search -> the dict of LM.packed."""
    fr = run_front(dec, d)
    out = dec.hosdl_search(d["x"], d["y"], (fr["lri"], fr["uidx"], fr["M"]), d["teps"], d["off"], label_bits=d["lab"])
    torch.cuda.synchronize()
    return dict(out, **fr)


def fcn(w):
    return np.concatenate([a.ravel() for a in w])


def check_case(dec, c, what):
    n, k = dec.n, dec.k
    m = n - k
    got = run_search(dec, device_inputs(dec, np.array(c["x"]), np.array(c["y"]), c["cw"], c["blocks"]))
    F = len(c["x"])
    assert got["cw"].shape == (F, (n + 63) // 64) and got["lri"].shape == (F, 64 * ((n + 63) // 64))
    assert got["M"].shape == (F, 64 * ((m + 63) // 64), (k + 63) // 64)
    assert_same(got, c["want"], FRONT_KEYS + SEARCH_KEYS, what)


# ------------------------------------------------------------------------------------------------ full rank, shape edges
@pytest.mark.parametrize("name", HM.STRUCTURES)
@pytest.mark.parametrize("k,n", LM.SHAPES_ALL)
def test_shape_edges_match_the_model(k, n, name):
    H, _ = HM.code(k, n, name)
    dec = _decoder(("edge", k, n, name), H=H)
    assert dec.hosdl_supported and not dec.hosdw_supported and dec.hosd_stage_family() == "hosdl" and (dec.n, dec.k, dec.m) == (n, k, n - k)
    for mode in HM.MODES:
        check_case(dec, LM.case(k, n, name, mode), (k, n, name, mode))


@pytest.mark.parametrize("k,n", LM.SHAPES_DENSE)
def test_more_shape_edges_match_the_model(k, n):
    H, _ = HM.code(k, n, "random_dense")
    dec = _decoder(("edge", k, n, "random_dense"), H=H)
    assert dec.hosdl_supported and (dec.n, dec.k, dec.m) == (n, k, n - k)
    for mode in ("float", "extreme"):
        check_case(dec, LM.case(k, n, "random_dense", mode), (k, n, mode))


# ------------------------------------------------------------------------------------------------------ redundant rows
@pytest.mark.parametrize("k,n,R,style", LM.REDUNDANT)
def test_redundant_rows_match_the_model(k, n, R, style):
    H, _ = WM.redundant(k, n, "random_dense", R, style)
    dec = _decoder(("redundant", k, n, R, style), H=H)
    assert dec.hosdl_supported and (dec.n, dec.k, dec.m) == (n, k, R)
    m = n - k
    for mode in ("float", "grid"):
        c = LM.case(k, n, "random_dense", mode, R, style)
        steps = [i for r in c["results"] for i, _ in r["deletions"]]
        assert len(steps) == (R - m) * len(c["results"])            # every redundant row is deleted in every frame
        check_case(dec, c, (k, n, R, style, mode))


def test_deletions_cross_the_row_words():
    """The premise of the redundant-row cases, from the model's ``deletions``: rows are deleted while more than 64 and more than
    128 rows are left, at pivot steps in more than one third of the loop, before and after the last pivot, and with the move of
    the later rows crossing both row-word boundaries.  (The reference's rule exchanges a zero row downwards whenever the column
    has a 1 below it, so every deletion happens within the last few steps whatever the position of the redundant row in H.)"""
    left, steps, cross, early, late = set(), set(), set(), 0, 0
    for k, n, R, style in LM.REDUNDANT:
        for r in LM.case(k, n, "random_dense", "float", R, style)["results"]:
            left |= {(rows - 1) // 64 for _, rows in r["deletions"]}
            steps |= {i // 64 for i, _ in r["deletions"]}
            cross |= {(i // 64, (rows - 1) // 64) for i, rows in r["deletions"] if i // 64 < (rows - 1) // 64}
            early += sum(1 for i, _ in r["deletions"] if i < n - k - 1)       # pivots still to come after the deletion
            late += sum(1 for i, _ in r["deletions"] if i == n - k)           # the rows left after the last pivot
    assert left == {0, 1, 2} and len(steps) >= 2 and early > 0 and late > 0
    assert {(0, 1), (1, 2)} <= cross                                          # the rows above the deleted one move across a word


# ------------------------------------------------------------------------------------------------- both forms of the scan
def heavy_blocks(k):
    """Order 0, the singles, 2500 sampled pairs and 400 sampled triples: more than kHosdLdsTeps TEPs, weight 3 among them."""
    rng = np.random.default_rng(77 + k)
    out = [np.zeros((1, k), np.int64), np.eye(k, dtype=np.int64)]
    for weight, count in ((2, 2500), (3, 400)):
        E = np.zeros((count, k), np.int64)
        for r in range(count):
            E[r, rng.choice(k, size=weight, replace=False)] = 1
        out.append(E)
    return tuple(out)


def test_both_scan_forms_on_the_largest_shape():
    k, n = 192, 384
    H, _ = HM.code(k, n, "random_dense")
    dec = _decoder(("edge", k, n, "random_dense"), H=H)
    c = LM.case(k, n, "random_dense", "float")
    x, y, cw = np.array(c["x"]), np.array(c["y"]), c["cw"]
    d = device_inputs(dec, x, y, cw, c["blocks"])                    # the per-thread-run form
    assert int(d["off"][-1]) <= 2304 and int(d["teps"][:, 3].max()) == 2 and d["nblk"] <= 128 and int(d["teps"][:, :3].max()) == k - 1
    assert_same(run_search(dec, d), c["want"], FRONT_KEYS + SEARCH_KEYS, "runs")
    blocks = heavy_blocks(k)                                         # the work-item form
    d = device_inputs(dec, x, y, cw, blocks)
    assert int(d["off"][-1]) > 2304 and int(d["teps"][:, 3].max()) == 3
    assert_same(run_search(dec, d), LM.model(x, y, cw, H, blocks, n - k), FRONT_KEYS + SEARCH_KEYS, "work items")
    pairs = blocks[:3]                                               # ... taken for its size alone
    d = device_inputs(dec, x[:4], y[:4], cw[:4], pairs)
    assert int(d["off"][-1]) > 2304 and int(d["teps"][:, 3].max()) == 2
    assert_same(run_search(dec, d), LM.model(x[:4], y[:4], cw[:4], H, pairs, n - k), FRONT_KEYS + SEARCH_KEYS, "large table")


# ------------------------------------------------------------------------------------------------------ the golden code
@pytest.mark.parametrize("snr", [1.5, 3.0])
def test_golden_code_matches_the_model(golden_dir, snr):
    dec = golden_decoder(golden_dir)
    assert (dec.n, dec.k, dec.m) == (384, 192, 192) and dec.hosd_stage_family() == "hosdl"
    c = LM.golden_case(golden_dir, snr)
    got = run_search(dec, device_inputs(dec, c["x"], c["y"], c["cw"], c["blocks"]))
    assert_same(got, LM.packed(c["results"], len(c["blocks"])), FRONT_KEYS + SEARCH_KEYS, snr)


def test_long_elimination_matches_the_reference_fixture(golden_dir):
    """The front end on the fixture's own ordering values: lri, the exchange count and M as the reference's routine left
    them (tests/golden/gf2elim_hform_long.npz, made by tests/tools/gen_gf2elim_hform_long.py)."""
    z = np.load(os.path.join(golden_dir, "gf2elim_hform_long.npz"))
    sets = [(golden_decoder(golden_dir), "g")]
    if "r_H" in z.files:
        sets.append((_decoder("fixture_redundant", H=z["r_H"]), "r"))
    for dec, p in sets:
        x = np.ascontiguousarray(z[p + "_x"], np.float32)
        n, k = dec.n, dec.k
        m = n - k
        lri, uidx, M, ns = (t.cpu().numpy() for t in dec.hosdl_front(torch.from_numpy(x).to(dec.device)))
        assert np.array_equal(lri[:, :n].astype(np.int64), z[p + "_order"].astype(np.int64))
        assert np.array_equal(ns, z[p + "_nswaps"].astype(np.int32))
        for f in range(len(x)):
            idx = np.arange(n)
            for a, b in z[p + "_swaps"][f][:ns[f]]:
                idx[a], idx[b] = idx[b], idx[a]
            mrb = idx[m:]
            sw = np.argsort(mrb, kind="stable")
            assert np.array_equal(uidx[f, :n].astype(np.int64), np.concatenate([idx[:m], mrb[sw]])), (p, f)
            Mref = np.unpackbits(z[p + "_M"][f], axis=1, bitorder="little")[:m, :k][:, sw]
            assert np.array_equal(M[f].view(np.uint64), LM.pack_M(Mref)), (p, f)


# ------------------------------------------------------------------------------------------- superset of ldpc_hosdw_*
@pytest.mark.parametrize("which", ["128_64", "96_48", "64_32", "121_60", "121_80", (127, 128, 6)])
def test_superset_of_the_wide_kernels(golden_dir, np_code, which):
    if which == "128_64":
        dec, H, G = _decoder("ccsds"), np_code.H, np_code.G
    elif isinstance(which, str):
        name = {"96_48": "LDPC_N96_K48_P8_set0_dmin10.alist", "64_32": "code1.alist"}.get(which) or WM.ARRAY[which]
        c = np_oracle.Code(os.path.join(golden_dir, name))
        dec, H, G = _decoder(which, path=os.path.join(golden_dir, name)), c.H, c.G
    else:
        H, G = WM.redundant(which[0], which[1], "random_dense", which[2], "copies")
        dec = _decoder(("superset",) + which, H=H)
    assert dec.hosdw_supported and dec.hosdl_supported and dec.hosd_stage_family() != "hosdl"
    n, k = dec.n, dec.k
    m = n - k
    F = 24
    x, y, cw = HM.refined_frames(H, G, 2.0, F, 31)
    x[3, : n // 2] = np.float32(0.5) * np.sign(x[3, : n // 2])
    y[5, 2] = 0.0
    blocks = [E for E in HM.path_blocks(k, 2) if len(E)]
    d = device_inputs(dec, x, y, cw, blocks)
    old, new = dec.hosdw_front(d["x"]), dec.hosdl_front(d["x"])
    conv = LM.from_wide(old[0].cpu().numpy(), old[1].cpu().numpy(), old[2].cpu().numpy(), n, m, k)
    for a, b, key in zip(conv, new[:3], FRONT_KEYS):
        assert np.array_equal(a, b.cpu().numpy().view(a.dtype)), key
    assert torch.equal(old[3], new[3])
    so = dec.hosdw_search(d["x"], d["y"], old, d["teps"], d["off"], label_bits=d["lab"])
    sn = dec.hosdl_search(d["x"], d["y"], new, d["teps"], d["off"], label_bits=d["lab"])
    assert_same(sn, so, SEARCH_KEYS)
    win = min(3, d["nblk"])
    for w in (DM.stopping_fcn_weights(win), DM.random_fcn_weights(np.random.default_rng(2), win)):
        for group in (0, 1):
            lo = dec.hosdw_sliding(d["x"], d["y"], old, d["teps"], d["off"], win, 0.9, fcn(w), label_bits=d["lab"], group=group)
            ln = dec.hosdl_sliding(d["x"], d["y"], new, d["teps"], d["off"], win, 0.9, fcn(w), label_bits=d["lab"], group=group)
            assert_same(ln, lo, SLIDE_KEYS, group)


# ------------------------------------------------------------------------------------------------------------- sliding
def slide_blocks(k):
    """Order 0, the singles in 16 blocks, an empty block and three blocks of 300 sampled pairs: 21 blocks."""
    rng = np.random.default_rng(500 + k)
    eye = np.eye(k, dtype=np.int64)
    out = [np.zeros((1, k), np.int64)] + [eye[lo:lo + k // 16] for lo in range(0, k, k // 16)][:16] + [np.zeros((0, k), np.int64)]
    for _ in range(3):
        E = np.zeros((300, k), np.int64)
        for r in range(300):
            E[r, rng.choice(k, size=2, replace=False)] = 1
        out.append(E)
    return tuple(out)


_slide_cases = {}


def slide_case(k, n):
    if (k, n) not in _slide_cases:
        H, G = HM.code(k, n, "random_dense")
        x, y, cw = HM.refined_frames(H, G, 1.0, 8, 900 + n)
        blocks = slide_blocks(k)
        results = [WM.hosdw_frame(x[f], y[f], cw[f], H, blocks, n - k) for f in range(len(x))]
        _slide_cases[(k, n)] = dict(H=H, x=x, y=y, cw=cw, blocks=blocks, results=results)
    return _slide_cases[(k, n)]


def _sliding_expect(c, win, w, margin):
    H, blocks = c["H"], c["blocks"]
    n = H.shape[1]
    m = H.shape[0]
    frames = len(c["x"])
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
        rows.append(r if deep == len(blocks) else WM.hosdw_frame(c["x"][f], c["y"][f], c["cw"][f], H, blocks[:deep], m))
    assert near == 0, f"{near} classifier outputs within 1e-6 of the margin"
    assert n == len(rows[0]["codeword"])
    exp["cw"] = HM.pack_cw(np.stack([r["codeword"] for r in rows]))
    exp["metric"] = np.array([r["metric"] for r in rows], np.float32)
    exp["best"] = np.array([r["best_index"] for r in rows], np.int32)
    exp["teps_least"] = off[exp["deep_limit"]].astype(np.int32)
    return exp


@pytest.mark.parametrize("win", [1, 3, 15])
@pytest.mark.parametrize("k,n", [(192, 384), (64, 129)])
def test_sliding_matches_the_model(k, n, win):
    c = slide_case(k, n)
    dec = _decoder(("edge", k, n, "random_dense"), H=c["H"])
    d = device_inputs(dec, c["x"], c["y"], c["cw"], c["blocks"])
    nblk = d["nblk"]
    front = dec.hosdl_front(d["x"])
    depths = set()
    for w, margin in ((early_fcn_weights(win, 5.0), 0.9), (DM.stopping_fcn_weights(win), 0.9), (early_fcn_weights(win, 0.3), 0.9),
                      (DM.stopping_fcn_weights(win, 0.8, 0.0), 0.9), (DM.stopping_fcn_weights(win), 1.0)):
        exp = _sliding_expect(c, win, w, margin)
        depths |= set(exp["deep_limit"].tolist())
        if margin == 1.0:
            assert (exp["deep_limit"] == nblk).all()
        outs = []
        for group in (0, 1, nblk):
            out = dec.hosdl_sliding(d["x"], d["y"], front, d["teps"], d["off"], win, margin, fcn(w), label_bits=d["lab"], group=group)
            torch.cuda.synchronize()
            assert_same(out, exp, ("deep_limit", "global_min", "success", "cw", "metric", "best"), (win, margin, group))
            assert (out["teps"].cpu().numpy() >= exp["teps_least"]).all()
            outs.append(out)
        assert (outs[2]["teps"].cpu().numpy() == int(d["off"][-1])).all()      # one group: every TEP is scanned
        for o in outs[1:]:
            assert_same(o, outs[0], [key for key in SLIDE_KEYS if key != "teps"], (win, margin))
    # (with win = 15 of 21 blocks the decisions after the first are on the pair blocks, which the reference's rule passes over)
    assert win in depths and nblk in depths and (win == 15 or any(win < v < nblk for v in depths)), depths


# ------------------------------------------------------------------------------------------------------- raw-call helpers
def _buffers(dec, rows, nblk, fill=0xA5):
    def buf(shape, dtype):
        t = torch.empty(shape, dtype=dtype, device=dec.device)
        t.view(torch.uint8).fill_(fill)
        return t
    itail, mtail = dec._hosdl_layout()
    return dict(lri=buf((rows,) + itail, torch.int16), uidx=buf((rows,) + itail, torch.int16), M=buf((rows,) + mtail, torch.int64),
                nswaps=buf((rows,), torch.int32), block_min=buf((rows, nblk), torch.float32),
                block_arg=buf((rows, nblk), torch.int32), truth=buf((rows,), torch.float32),
                cw=buf((rows, dec.words), torch.int64), metric=buf((rows,), torch.float32), best=buf((rows,), torch.int32),
                deep_limit=buf((rows,), torch.int32), global_min=buf((rows,), torch.float32),
                success=buf((rows,), torch.uint8), teps=buf((rows,), torch.int32))


def raw_front(dec, d, F, b, null=()):
    g = lambda key: None if key in null else _p(b[key])   # noqa: E731
    return dec.L.ldpc_hosdl_front(dec._ctx, _p(d["x"]), F, g("lri"), g("uidx"), g("M"), g("nswaps"), dec._stream())


def raw_search(dec, d, F, b, null=()):
    g = lambda key: None if key in null else _p(b[key])   # noqa: E731
    return dec.L.ldpc_hosdl_search(dec._ctx, _p(d["x"]), _p(d["y"]), F, g("lri"), g("uidx"), g("M"), _p(d["teps"]), _p(d["off"]),
                                   d["nblk"], _p(d["lab"]), g("block_min"), g("block_arg"), g("truth"), g("cw"), g("metric"),
                                   g("best"), dec._stream())


def raw_sliding(dec, d, F, b, win, margin, fw, group=0, null=()):
    g = lambda key: None if key in null else _p(b[key])   # noqa: E731
    fw = np.ascontiguousarray(fw, np.float32)
    return dec.L.ldpc_hosdl_sliding(dec._ctx, _p(d["x"]), _p(d["y"]), F, g("lri"), g("uidx"), g("M"), _p(d["teps"]), _p(d["off"]),
                                    d["nblk"], win, float(margin), fw.ctypes.data_as(C.POINTER(C.c_float)), fw.size, group,
                                    _p(d["lab"]), g("deep_limit"), g("global_min"), g("truth"), g("success"), g("cw"),
                                    g("metric"), g("best"), g("teps"), dec._stream())


# ---------------------------------------------------------------------------------------------------- untouched bytes
@pytest.mark.parametrize("k,n,R", [(5, 12, None), (108, 300, None), (64, 129, 66)])
def test_pads_are_zero_and_nothing_beyond_F_is_written(k, n, R):
    c = LM.case(k, n, "random_dense", "float", R)
    dec = _decoder(("pads", k, n, R), H=c["H"])
    F, extra, m = LM.FRAMES, 3, n - k
    d = device_inputs(dec, np.array(c["x"]), np.array(c["y"]), c["cw"], c["blocks"])
    b = _buffers(dec, F + extra, d["nblk"])
    assert raw_front(dec, d, F, b) == 0 and raw_search(dec, d, F, b) == 0
    torch.cuda.synchronize()
    assert_same({key: b[key][:F] for key in FRONT_KEYS + SEARCH_KEYS}, c["want"], FRONT_KEYS + SEARCH_KEYS)
    assert raw_sliding(dec, d, F, b, 2, 0.9, fcn(DM.stopping_fcn_weights(2))) == 0
    torch.cuda.synchronize()
    for key, t in b.items():
        assert (t[F:].contiguous().view(torch.uint8) == 0xA5).all(), key
    # dirty pads on the way in change nothing
    b2 = _buffers(dec, F + extra, d["nblk"])
    for key in ("lri", "uidx", "M"):
        b2[key][:F] = b[key][:F]
    b2["lri"][:F, n:] = 0x6EEE
    b2["uidx"][:F, n:] = 0x6EEE
    b2["M"][:F, m:] = -1
    Wk = (k + 63) // 64
    if k % 64:
        b2["M"][:F, :m, Wk - 1] |= -(1 << (k % 64))
    assert raw_search(dec, d, F, b2) == 0
    torch.cuda.synchronize()
    assert_same({key: b2[key][:F] for key in SEARCH_KEYS}, c["want"], SEARCH_KEYS)


# ----------------------------------------------------------------------------------------------------------- contract
def test_every_nullable_output_alone():
    c = LM.case(64, 129, "random_dense", "float")
    dec = _decoder(("edge", 64, 129, "random_dense"), H=c["H"])
    F = LM.FRAMES
    d = device_inputs(dec, np.array(c["x"]), np.array(c["y"]), c["cw"], c["blocks"])
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
    # without labels: no truth, and d_truth is refused
    nolab = dict(d, lab=None)
    b = _buffers(dec, F, d["nblk"], fill=0x5A)
    for key in ("lri", "uidx", "M"):
        b[key].copy_(full[key])
    from short_ldpc_decoding_osd_amd import _lib
    with pytest.raises(_lib.LdpcError, match=r"\(-1\).*ldpc_hosdl_search: d_truth needs d_label_bits"):
        _lib.check(raw_search(dec, nolab, F, b))
    with pytest.raises(_lib.LdpcError, match=r"\(-1\).*ldpc_hosdl_sliding: d_truth / d_success need d_label_bits"):
        _lib.check(raw_sliding(dec, nolab, F, b, 2, 0.9, fw))
    assert raw_search(dec, nolab, F, b, null=("truth",)) == 0
    torch.cuda.synchronize()
    assert_same(b, ref_search, [key for key in SEARCH_KEYS if key != "truth"], "no labels")


def test_refusal_names_the_entry_point_and_the_shape(golden_dir):
    from short_ldpc_decoding_osd_amd import _lib
    wimax = _decoder("wimax", path=os.path.join(golden_dir, "wimax_1056_0.83.alist"))
    k193 = _decoder(("edge", 193, 200), H=HM.code(193, 200, "random_dense")[0])
    m193 = _decoder(("edge", 7, 200), H=HM.code(7, 200, "random_dense")[0])
    fw = fcn(DM.stopping_fcn_weights(2))
    for dec in (wimax, k193, m193):
        assert not dec.hosdl_supported and not dec.hosdw_supported and dec.hosd_stage_family() == "hosdw"
        x = torch.zeros((4, dec.n), dtype=torch.float32, device=dec.device)
        itail, mtail = dec._hosdl_layout()
        front = (torch.zeros((4,) + itail, dtype=torch.int16, device=dec.device), torch.zeros((4,) + itail, dtype=torch.int16, device=dec.device),
                 torch.zeros((4,) + mtail, dtype=torch.int64, device=dec.device))
        teps = torch.zeros((3, 4), dtype=torch.uint8, device=dec.device)
        off = torch.tensor([0, 1, 3], dtype=torch.int32, device=dec.device)
        msg = rf"\(-5\).*n <= 384, an H of 1 <= R <= 192 rows, 1 <= n-k <= 192 and 1 <= k <= 192; this H has {dec.m} rows, " \
              rf"n-k = {dec.n - dec.k}, code \({dec.n},{dec.k}\)"
        with pytest.raises(_lib.LdpcError, match="ldpc_hosdl_front.*" + msg):
            dec.hosdl_front(x)
        with pytest.raises(_lib.LdpcError, match="ldpc_hosdl_search.*" + msg):
            dec.hosdl_search(x, x, front, teps, off)
        with pytest.raises(_lib.LdpcError, match="ldpc_hosdl_sliding.*" + msg):
            dec.hosdl_sliding(x, x, front, teps, off, 2, 0.9, fw)
        with pytest.raises(_lib.LdpcError, match="ldpc_hosdw_front"):
            dec.hosd_stage("front")(x)                                  # the stage's selector stays on the older refusal


def test_argument_errors_and_empty_batch():
    from short_ldpc_decoding_osd_amd import _lib
    c = LM.case(64, 129, "random_dense", "float")
    dec = _decoder(("edge", 64, 129, "random_dense"), H=c["H"])
    d = device_inputs(dec, np.array(c["x"][:4]), np.array(c["y"][:4]), c["cw"][:4], c["blocks"])
    b = _buffers(dec, 4, d["nblk"])
    fw = fcn(DM.stopping_fcn_weights(2))
    for key in ("lri", "uidx", "M"):
        with pytest.raises(_lib.LdpcError, match=rf"\(-1\).*ldpc_hosdl_front: d_{key} is NULL"):
            _lib.check(raw_front(dec, d, 4, b, null=(key,)))
        with pytest.raises(_lib.LdpcError, match=rf"\(-1\).*ldpc_hosdl_search: d_{key} is NULL"):
            _lib.check(raw_search(dec, d, 4, b, null=(key,)))
        with pytest.raises(_lib.LdpcError, match=rf"\(-1\).*ldpc_hosdl_sliding: d_{key} is NULL"):
            _lib.check(raw_sliding(dec, d, 4, b, 2, 0.9, fw, null=(key,)))
    with pytest.raises(_lib.LdpcError, match=r"\(-1\).*ldpc_hosdl_front: d_lri is NULL"):      # the first one in order
        _lib.check(raw_front(dec, d, 4, b, null=("lri", "uidx", "M")))
    with pytest.raises(_lib.LdpcError, match=r"\(-1\).*ldpc_hosdl_search: d_block_min is NULL"):
        _lib.check(raw_search(dec, d, 4, b, null=("block_min",)))
    with pytest.raises(_lib.LdpcError, match=r"\(-1\).*ldpc_hosdl_search: d_order_llr is NULL"):
        _lib.check(raw_search(dec, dict(d, x=None), 4, b))
    with pytest.raises(_lib.LdpcError, match=r"\(-5\).*ldpc_hosdl_search: 1025 TEP blocks, at most 1024"):
        _lib.check(raw_search(dec, dict(d, nblk=1025), 4, b))
    with pytest.raises(_lib.LdpcError, match=r"\(-5\).*ldpc_hosdl_sliding: 1025 TEP blocks, at most 1024"):
        _lib.check(raw_sliding(dec, dict(d, nblk=1025), 4, b, 2, 0.9, fw))
    with pytest.raises(_lib.LdpcError, match=r"\(-1\).*ldpc_hosdl_sliding: bad arguments"):
        _lib.check(raw_sliding(dec, d, 4, b, 16, 0.9, fw))
    with pytest.raises(ValueError, match="hosdl takes M"):
        dec.hosdl_search(d["x"], d["y"], (b["lri"], b["uidx"], b["M"][:, :, 0].contiguous()), d["teps"], d["off"])
    with pytest.raises(ValueError, match="hosdl takes lri"):
        dec.hosdl_search(d["x"], d["y"], (b["lri"].view(torch.uint8), b["uidx"], b["M"]), d["teps"], d["off"])
    torch.cuda.synchronize()
    for key, t in b.items():                                     # all of it refused before any launch
        assert (t.view(torch.uint8) == 0xA5).all(), key
    none = dict(x=None, y=None, lab=None, teps=None, off=None, nblk=d["nblk"])
    nob = {key: None for key in b}
    assert raw_front(dec, none, 0, nob) == 0 and raw_search(dec, none, 0, nob) == 0
    assert raw_sliding(dec, none, 0, nob, 2, 0.9, fw) == 0
    assert dec.hosdl_front(dec.empty((0, 129), torch.float32))[2].shape == (0, 128, 1)


def test_graph_capture_front_and_sliding():
    c = slide_case(64, 129)
    dec = _decoder(("edge", 64, 129, "random_dense"), H=c["H"])
    d = device_inputs(dec, c["x"], c["y"], c["cw"], c["blocks"])
    fw = fcn(early_fcn_weights(3, 0.3))

    def step():
        fr = dec.hosdl_front(d["x"])
        out = dec.hosdl_sliding(d["x"], d["y"], fr, d["teps"], d["off"], 3, 0.9, fw, label_bits=d["lab"])
        se = dec.hosdl_search(d["x"], d["y"], fr, d["teps"], d["off"], label_bits=d["lab"])
        return dict(out, lri=fr[0], uidx=fr[1], M=fr[2], nswaps=fr[3], block_min=se["block_min"], block_arg=se["block_arg"])

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


# ------------------------------------------------------------------------------------- several frames per workgroup
def test_several_frames_per_wavefront_and_workgroup():
    """On (5,12): three trips of the front end's grid and of the scans' grids.  The whole batch equals its grid-sized slices,
    and a sample stratified over the trips equals the model."""
    k, n = 5, 12
    H, G = HM.code(k, n, "random_dense")
    dec = _decoder(("edge", k, n, "random_dense"), H=H)
    Ff, Fs = 2 * FRONT_GRID + 7, 2 * SCAN_GRID + 5
    assert -(-Ff // FRONT_GRID) == 3 and -(-Fs // SCAN_GRID) == 3
    rng = np.random.default_rng(12)
    y, cw = np_oracle.make_frames(G, 2.0, Ff, rng)[:2]
    y = np.ascontiguousarray(y, np.float32)
    x = np.ascontiguousarray(y + np.float32(0.5) * rng.standard_normal(y.shape).astype(np.float32), dtype=np.float32)
    blocks = HM.edge_blocks(k)
    d = device_inputs(dec, x, y, cw, blocks)
    whole = dec.hosdl_front(d["x"])
    parts = [dec.hosdl_front(d["x"][lo:lo + FRONT_GRID]) for lo in range(0, Ff, FRONT_GRID)]
    for i, key in enumerate(FRONT_KEYS):
        assert torch.equal(whole[i], torch.cat([p[i] for p in parts])), key
    sl = lambda t, lo, hi: t[lo:hi].contiguous()   # noqa: E731
    fw = fcn(DM.stopping_fcn_weights(2))
    args = lambda lo, hi: (sl(d["x"], lo, hi), sl(d["y"], lo, hi), tuple(sl(t, lo, hi) for t in whole), d["teps"], d["off"])   # noqa: E731
    big = tuple(np.concatenate([E] * 600) for E in blocks)      # the work-item form: 600 copies of every block, > 2304 TEPs
    db = device_inputs(dec, x[:Fs], y[:Fs], cw[:Fs], big)
    assert int(db["off"][-1]) > 2304
    ws = dec.hosdl_search(*args(0, Fs), label_bits=sl(d["lab"], 0, Fs))
    wt = dec.hosdl_search(*args(0, Fs)[:3], db["teps"], db["off"], label_bits=sl(d["lab"], 0, Fs))
    wl = dec.hosdl_sliding(*args(0, Fs), 2, 0.9, fw, label_bits=sl(d["lab"], 0, Fs))
    for lo in range(0, Fs, SCAN_GRID):
        hi = min(lo + SCAN_GRID, Fs)
        ps = dec.hosdl_search(*args(lo, hi), label_bits=sl(d["lab"], lo, hi))
        assert_same({key: ws[key][lo:hi] for key in SEARCH_KEYS}, ps, SEARCH_KEYS, lo)
        pt = dec.hosdl_search(*args(lo, hi)[:3], db["teps"], db["off"], label_bits=sl(d["lab"], lo, hi))
        assert_same({key: wt[key][lo:hi] for key in SEARCH_KEYS}, pt, SEARCH_KEYS, lo)
        pl = dec.hosdl_sliding(*args(lo, hi), 2, 0.9, fw, label_bits=sl(d["lab"], lo, hi))
        assert_same({key: wl[key][lo:hi] for key in SLIDE_KEYS}, pl, SLIDE_KEYS, lo)
    torch.cuda.synchronize()
    # the copies change no minimum and no first-minimum codeword: the work-item form agrees with the run form on those
    assert_same(wt, ws, ("truth", "cw", "metric"))
    sel = np.array(sorted({t * g + w for g, top in ((SCAN_GRID, Fs), (FRONT_GRID, Ff)) for t in range(3) for w in (0, g // 2, g - 1)
                           if t * g + w < top} | {Fs - 1, Ff - 1}))
    want = LM.model(x[sel], y[sel], cw[sel], H, blocks, n - k)
    st = torch.from_numpy(sel).to(dec.device)
    assert_same({key: whole[i][st] for i, key in enumerate(FRONT_KEYS)}, want, FRONT_KEYS)
    inside = np.flatnonzero(sel < Fs)
    si = st[torch.from_numpy(inside).to(dec.device)]
    assert_same({key: ws[key][si] for key in SEARCH_KEYS}, {key: want[key][inside] for key in SEARCH_KEYS}, SEARCH_KEYS)
