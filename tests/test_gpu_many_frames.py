"""-m gpu: exact parity when a workgroup decodes several frames in turn.  Every OSD / H-form kernel runs a capped grid and
loops over the frames b, b + grid, b + 2 grid, ... (one pass = one trip); from the second trip on a frame runs on the LDS
the previous one left, and the register-resident order-2 kernels prefetch a later frame's perm / P' / index.  Each test
here asserts that its frame count gives at least three trips of the kernel it targets (TRIPS below), then compares the
outputs with the oracle (every frame, or a sample stratified over the trips) and with the same frames decoded in calls of
at most one trip each (no workgroup gets a second frame)."""
import math

import numpy as np
import pytest
import torch

from oracle import c_oracle, np_oracle
from tests import dlosd_model as DM
from tests import nms_graphs as Z
from tests import osd_adversary as adv
from tests.gpu_util import pack_np, to_dev, words_np
from tests.nms_grad_model import grad_model
from tests.test_gpu_dlosd import _blocks, _check_sliding
from tests.test_gpu_hosd import PATH
from tests.test_gpu_nms_train import rel_bound
from tests.test_gpu_osd import _rows_packed

pytestmark = pytest.mark.gpu
ALPHA0 = 0.669435

# Frames per trip of each kernel (frames a full grid takes in one pass), from its launcher.  "cu" = the device's CU count.
TRIPS = {
    "osd_fused2r": lambda cu: cu * 16 * 6,    # ldpc_osd.hip grid2r(), one frame per workgroup
    "osd_search2r": lambda cu: cu * 16 * 6,   # ldpc_osd.hip grid2r()
    "osd_front": lambda cu: 65536,            # ldpc_osd.hip launch_front(): frame_grid(), one wavefront per workgroup
    "osd_search2": lambda cu: 65536,          # ldpc_osd.hip frame_grid() (readlane order-2 scan)
    "osd_search<1>": lambda cu: 65536,        # ldpc_osd.hip frame_grid() (table scan, orders 2 and 3)
    "osd_fs": lambda cu: 65536,               # ldpc_osd.hip frame_grid()
    "osd_search<4>": lambda cu: 4096 * 4,     # ldpc_osd.hip osd_grid(), 4 waves per workgroup (orders 0 and 1)
    "osd_ge": lambda cu: 4096 * 4,            # ldpc_osd.hip osd_grid()
    "osd_tep_eval": lambda cu: 4096 * 4,      # ldpc_osd.hip osd_grid()
    "index_guard": lambda cu: 1024 * 256,     # ldpc_osd.hip guarded_index(), one entry per thread
    "hosd_front": lambda cu: 8192 * 4,        # ldpc_hosd.hip:243 grid_for(F, 4)
    "hosd_search": lambda cu: 8192,           # ldpc_hosd.hip:243 grid_for(F, 1), one frame per workgroup
    "hosd_sliding": lambda cu: 8192,          # ldpc_hosd.hip:243 grid_for(F, 1)
    "nms_generic": lambda cu: 8192 * 4,       # ldpc_nms.hip:443, 4 waves per workgroup
    "nms_train": lambda cu: 32768 // 2 * 2,   # ldpc_nms_train.hip:288, 32768 / waves workgroups of waves frames; waves = 2 below
}
COMPACT_FPT8_ABOVE = 256 * 1024 * 2           # ldpc_util.hip:218: compact_kernel<EVAL, 8> above this many flags


@pytest.fixture(scope="module")
def dec():
    from short_ldpc_decoding_osd_amd import Code
    from short_ldpc_decoding_osd_amd.runtime import Decoder
    return Decoder(Code())


def per_trip(dec, kernel):
    cu = torch.cuda.get_device_properties(dec.device).multi_processor_count
    return TRIPS[kernel](cu)


def assert_trips(dec, kernel, frames, want=3):
    """The premise: ``frames`` frames take at least ``want`` trips of ``kernel``'s grid."""
    t = -(-int(frames) // per_trip(dec, kernel))
    assert t >= want, f"{frames} frames are {t} trip(s) of {kernel} ({per_trip(dec, kernel)} frames per trip), {want} wanted"
    return t


def stratified(n, grid, rng, extra=200, tail=64):
    """Frame positions for an oracle sample: workgroups 0, grid/2 and grid-1 of every trip, the last ``tail`` frames and
    ``extra`` random ones (ascending, unique)."""
    pos = [k * grid + w for k in range(-(-n // grid)) for w in (0, grid // 2, grid - 1)]
    pos += list(range(max(n - tail, 0), n)) + rng.integers(0, n, size=extra).tolist()
    return np.unique(np.array([p for p in pos if p < n], dtype=np.int64))


def device_frames(dec, B, snr, seed):
    """B AWGN frames generated on the device: (y [B,128] f32, codewords [B,128] f32 0/1)."""
    g = torch.Generator(device=dec.device).manual_seed(seed)
    G = to_dev(dec.code.G, dec, torch.float32)
    cw = (torch.randint(0, 2, (B, 64), device=dec.device, generator=g).to(torch.float32) @ G).remainder(2)
    sigma = np_oracle.snr_to_sigma(snr, 64, 128)
    y = ((1 - 2 * cw) * (1 + sigma * torch.randn((B, 128), device=dec.device, generator=g))).contiguous()
    return y, cw


def check_conv(out, ref, n=None, tag=""):
    n = len(ref["best"]) if n is None else n
    assert np.array_equal(words_np(out["cw"])[:n], pack_np(ref["codeword"])), tag
    assert np.array_equal(out["best"].cpu().numpy()[:n], ref["best"]), tag
    assert np.array_equal(out["metric"].cpu().numpy()[:n].view(np.uint32), ref["metric"].view(np.uint32)), tag
    assert (out["ntep"].cpu().numpy()[:n] == ref["teps_size"]).all(), tag


def assert_same(a, b, keys, tag=""):
    for k in keys:
        assert torch.equal(a[k], b[k]), (tag, k)


# ---------------------------------------------------------------------------------------- conventional OSD, NMS failures
@pytest.fixture(scope="module")
def failures(dec):
    """The NMS-10 failures of 131 072 frames at 1.0 dB as listed by compact (capacity F = 131 072 > count), a few hundred
    crafted deep-exchange frames (tests/osd_adversary.py) laid over listed frames spread through the list."""
    B = 131072
    y, cw = device_frames(dec, B, 1.0, 2026)
    res = dec.nms(y, 10, ALPHA0)
    index, count = dec.compact(res["fail"])
    nf = int(count.cpu()[0])
    idx = index[:nf].to(torch.int64)
    s = adv.crafted_sets(dec.code.G, dec.code.H)
    cy = np.concatenate([s["g"][0], s["g_ties"][0]])
    ccw = np.concatenate([s["g"][1], s["g_ties"][1]])
    reps = 8
    at = idx[torch.linspace(0, nf - 1, reps * len(cy), device=dec.device).round().to(torch.int64)]
    y[at] = to_dev(np.tile(cy, (reps, 1)), dec)
    cw[at] = to_dev(np.tile(ccw, (reps, 1)), dec, torch.float32)
    yh = y[idx].cpu().numpy()
    cwh = cw[idx].to(torch.uint8).cpu().numpy()
    return dict(B=B, y=y, index=index, count=count, nf=nf, yh=yh, cwh=cwh, label=dec.pack_bits(cw.to(torch.int64)),
                crafted_pos=np.searchsorted(idx.cpu().numpy(), at.cpu().numpy()), ref={})


def oracle_conv(fx, dec, order):
    if order not in fx["ref"]:
        fx["ref"][order] = c_oracle.conv_osd(dec.code.G, fx["yh"], fx["cwh"], order)
    return fx["ref"][order]


@pytest.mark.parametrize("order", [0, 1, 2])
def test_conventional_on_nms_failures(dec, failures, order):
    fx = failures
    B, nf, y, index, count = fx["B"], fx["nf"], fx["y"], fx["index"], fx["count"]
    assert nf > 100000
    ref = oracle_conv(fx, dec, order)
    assert ref["nswaps"][fx["crafted_pos"]].max() >= 40        # the crafted frames are in the list and exchange deeply
    routes = {"default": dec.osd_decode(y, order, index=index, count=count, F=B)}
    perm, parity, ns = dec.osd_front(y, index=index, count=count, F=B)
    routes["front_then_search"] = dec.osd_search(y, perm, parity, dec.osd_params(order), index=index, count=count, F=B)
    if order == 2:
        assert_trips(dec, "osd_fused2r", nf, 4)
        assert_trips(dec, "osd_search2r", nf, 4)
    else:
        assert_trips(dec, "osd_search<4>", nf, 4)
    torch.cuda.synchronize()
    assert np.array_equal(ns.cpu().numpy()[:nf], ref["nswaps"])
    for name, o in routes.items():
        check_conv(o, ref, nf, (name, order))
    c = dec.osd_counts(routes["default"]["cw"], fx["label"], index=index, count=count, ntep=routes["default"]["ntep"], F=B)
    c = c.cpu().numpy()
    assert c[0] == nf and c[1] == int((~ref["correct"]).sum()) and c[2] == nf * ref["teps_size"]


@pytest.fixture(scope="module")
def raw_frames(dec):
    """About 200 000 raw channel frames at 2.5 dB (no index), held on the device and on the host."""
    F = 200000
    y, cw = device_frames(dec, F, 2.5, 31)
    return dict(F=F, y=y, yh=y.cpu().numpy(), cwh=cw.to(torch.uint8).cpu().numpy())


def test_order2_scans_on_raw_frames(dec, raw_frames):
    """Order 2 on every route, the 65 536-frame grids (table scan, readlane scan, front end) at 4 trips."""
    fr = raw_frames
    F, y = fr["F"], fr["y"]
    for k in ("osd_search<1>", "osd_search2", "osd_front"):
        assert_trips(dec, k, F, 4)
    assert_trips(dec, "osd_fused2r", F, 4)
    perm, parity, ns = dec.osd_front(y)
    routes = {"table": dec.osd_decode(y, 2, params=dec.osd_params(2, table_scan=True)),
              "readlane": dec.osd_decode(y, 2, params=dec.osd_params(2, readlane_scan=True)),
              "default": dec.osd_decode(y, 2),
              "front_then_search": dec.osd_search(y, perm, parity, dec.osd_params(2))}
    torch.cuda.synchronize()
    ref = c_oracle.conv_osd(dec.code.G, fr["yh"], fr["cwh"], 2)
    assert np.array_equal(ns.cpu().numpy(), ref["nswaps"])
    for name, o in routes.items():
        check_conv(o, ref, F, name)


def sliced(fn, F, step):
    """fn(lo, hi) -> dict of tensors for frames lo..hi-1, called in slices of ``step``; the slices concatenated."""
    parts = [fn(lo, min(lo + step, F)) for lo in range(0, F, step)]
    return {k: torch.cat([p[k] for p in parts]) for k in parts[0] if parts[0][k] is not None}


def test_order3_table_slices_and_sample(dec, raw_frames):
    fr = raw_frames
    F, y = fr["F"], fr["y"]
    grid = per_trip(dec, "osd_search<1>")
    assert_trips(dec, "osd_search<1>", F, 3)
    whole = dec.osd_decode(y, 3)
    parts = sliced(lambda lo, hi: dec.osd_decode(y[lo:hi], 3), F, grid)
    torch.cuda.synchronize()
    assert_same(whole, parts, ("cw", "metric", "best", "ntep"), "order 3")
    sel = stratified(F, grid, np.random.default_rng(3))
    ref = c_oracle.conv_osd(dec.code.G, fr["yh"][sel], fr["cwh"][sel], 3)
    check_conv({k: v[torch.from_numpy(sel).to(dec.device)] for k, v in whole.items()}, ref, tag="order 3")
    assert ref["teps_size"] == 43745


@pytest.mark.parametrize("order", [2, 3])
def test_fs_slices_and_sample(dec, raw_frames, order):
    from short_ldpc_decoding_osd_amd import _lib
    fr = raw_frames
    F, y = fr["F"], fr["y"]
    grid = per_trip(dec, "osd_fs")
    assert_trips(dec, "osd_fs", F, 3)
    sel = stratified(F, grid, np.random.default_rng(10 + order))
    seld = torch.from_numpy(sel).to(dec.device)
    ref = c_oracle.fs_osd(dec.code.G, fr["yh"][sel], fr["cwh"][sel], order)
    depths = set()
    for quirk in (1, 0):
        p = dec.osd_params(order, _lib.OSD_FS, fs_reference_quirk=quirk)
        whole = dec.osd_decode(y, order, params=p)
        parts = sliced(lambda lo, hi: dec.osd_decode(y[lo:hi], order, params=p), F, grid)
        torch.cuda.synchronize()
        assert_same(whole, parts, ("cw", "metric", "best", "ntep"), (order, quirk))
        depths |= set(torch.unique(whole["ntep"]).cpu().tolist())
        o = {k: v[seld] for k, v in whole.items()}
        assert np.array_equal(o["ntep"].cpu().numpy(), ref["num_teps"]), (order, quirk)
        want_cw = ref["codeword_ref"] if quirk else ref["codeword_hit"]
        want_m = ref["metric_ref"] if quirk else ref["metric_hit"]
        assert np.array_equal(words_np(o["cw"]), pack_np(want_cw)), (order, quirk)
        assert np.array_equal(o["metric"].cpu().numpy().view(np.uint32), want_m.view(np.uint32)), (order, quirk)
        if quirk:
            assert np.array_equal(o["best"].cpu().numpy(), ref["best_index"]), order
    assert len(depths) > 2        # frames stop at different depths: a short frame shares a workgroup with a longer one


# ---------------------------------------------------------------------------------------- caller-made frame lists
@pytest.mark.parametrize("kind", ["reversed", "shuffled_repeats"])
def test_caller_lists_on_register_kernels(dec, failures, kind):
    """Non-monotone source indices through the index prefetch (srcc) of osd_fused2r and osd_search2r: the outputs equal
    those of the ascending run, permuted the same way."""
    fx = failures
    nf, y = fx["nf"], fx["y"]
    asc = fx["index"][:nf].contiguous()
    if kind == "reversed":
        pos = np.arange(nf - 1, -1, -1)
    else:
        rng = np.random.default_rng(5)
        pos = np.concatenate([rng.permutation(nf), rng.integers(0, nf, size=nf // 3)])
        rng.shuffle(pos)
    posd = torch.from_numpy(pos).to(dec.device)
    lst = asc[posd].contiguous()
    assert_trips(dec, "osd_fused2r", len(pos), 4)
    base = dec.osd_decode(y, 2, index=asc)
    got = {"fused": dec.osd_decode(y, 2, index=lst)}
    perm, parity, _ = dec.osd_front(y, index=lst)
    got["front_then_search"] = dec.osd_search(y, perm, parity, dec.osd_params(2), index=lst)
    torch.cuda.synchronize()
    want = {k: v[posd] for k, v in base.items()}
    for name, o in got.items():
        assert_same(o, want, ("cw", "metric", "best", "ntep"), (kind, name))
    check_conv(base, oracle_conv(fx, dec, 2), nf, "ascending")


def test_checked_frame_list_beyond_one_guard_stride(dec, failures):
    """osd_params(y_frames=...): the guard kernel strides over a list of more than 2 x 262 144 entries; entries out of range
    (some in the third stride) become frame 0 and are counted."""
    fx = failures
    nf, y, B = fx["nf"], fx["y"], fx["B"]
    asc = fx["index"][:nf].contiguous()
    n = 3 * per_trip(dec, "index_guard") + 1000
    assert_trips(dec, "index_guard", n, 4)
    rng = np.random.default_rng(8)
    pos = rng.integers(0, nf, size=n)
    lst = asc[torch.from_numpy(pos).to(dec.device)]
    bad = np.array([5, n // 2, 2 * per_trip(dec, "index_guard") + 17, n - 1])
    lst[torch.from_numpy(bad).to(dec.device)] = to_dev(np.array([-1, B, B + 12345, -7], np.int32), dec)
    before = dec.osd_index_errors()
    out = dec.osd_decode(y, 2, index=lst.contiguous(), params=dec.osd_params(2, y_frames=B))
    base = dec.osd_decode(y, 2, index=asc)
    zero = dec.osd_decode(y, 2, index=torch.zeros(1, dtype=torch.int32, device=dec.device))
    torch.cuda.synchronize()
    assert dec.osd_index_errors() - before == len(bad)
    good = np.setdiff1d(np.arange(n), bad)
    gd = torch.from_numpy(good).to(dec.device)
    bd = torch.from_numpy(bad).to(dec.device)
    pd = torch.from_numpy(pos[good]).to(dec.device)
    for k in ("cw", "metric", "best", "ntep"):
        assert torch.equal(out[k][gd], base[k][pd]), k
        assert torch.equal(out[k][bd], zero[k].expand_as(out[k][bd])), k


# ---------------------------------------------------------------------------------------- GE and one-TEP evaluation
def test_ge_above_three_trips(dec):
    """ldpc_osd_ge on 70 000 matrices: column-permuted G (the reliability orders of frames) with osd_adversary.ge_matrices
    tiled across the trips; slice invariance on all, gf2elim on a stratified sample."""
    n = 70000
    grid = per_trip(dec, "osd_ge")
    assert_trips(dec, "osd_ge", n, 4)
    y, _ = device_frames(dec, n, 1.5, 12)
    perm = torch.argsort(-y.abs(), dim=1, stable=True)
    G = to_dev(dec.code.G, dec, torch.uint8)
    M = G[:, perm].permute(1, 0, 2).contiguous()                              # [n, 64, 128], M[f] = G[:, perm[f]]
    rows = dec.pack_bits(M.reshape(-1, 128)).reshape(n, 64, 2)
    mats = adv.ge_matrices(seed=3)
    names = [k for k in mats for _ in mats[k]]
    A = np.stack([m for k in mats for m in mats[k]])
    reps = 12
    at = np.linspace(0, n - 1, reps * len(A)).round().astype(np.int64)
    rows[torch.from_numpy(at).to(dec.device)] = to_dev(np.tile(_rows_packed(A), (reps, 1, 1)).view(np.int64), dec)
    red, sw, ns = dec.osd_ge(rows)
    parts = [dec.osd_ge(rows[lo:lo + grid].contiguous()) for lo in range(0, n, grid)]
    torch.cuda.synchronize()
    pred, psw, pns = (torch.cat([p[i] for p in parts]) for i in range(3))
    assert torch.equal(ns, pns)
    full = ns >= 0
    assert torch.equal(red[full], pred[full]) and torch.equal(sw[full], psw[full])
    deficient = np.zeros(n, bool)
    deficient[at] = np.tile([k.startswith("deficient") for k in names], reps)
    nsh = ns.cpu().numpy()
    assert np.array_equal(nsh == -1, deficient)
    sel = np.union1d(stratified(n, grid, np.random.default_rng(4)), at[::3])
    Mh = M[torch.from_numpy(sel).to(dec.device)].cpu().numpy()
    redh, swh = words_np(red).reshape(n, 64, 2), sw.cpu().numpy()
    amap = dict(zip(at.tolist(), np.tile(np.arange(len(A)), reps).tolist()))
    for j, f in enumerate(sel.tolist()):
        m = A[amap[f]] if f in amap else Mh[j]
        R, rsw = c_oracle.gf2elim(m)
        if R.shape[0] < 64:
            assert nsh[f] == -1, f
            continue
        assert nsh[f] == len(rsw), f
        assert [tuple(int(v) for v in p) for p in swh[f, :nsh[f]]] == rsw, f
        assert np.array_equal(redh[f], _rows_packed(R[None])[0]), f


def _tep_eval_expected(y, cw, G, mask):
    """The NumPy restatement of test_gpu_osd.test_tep_eval_matches_oracle for one frame: (perm, hd, metric, packed cw)."""
    yp, _, Gp, pm, _ = np_oracle.swapped_info(y, cw, G)
    hard = np.where(yp > 0, 0, 1).astype(np.int64)
    e = np.array([(int(mask) >> p) & 1 for p in range(64)], dtype=np.int64)
    cand = ((hard[:64] + e) % 2).dot(Gp) % 2
    disc = (cand + hard) % 2
    orig = np.empty(128, dtype=np.int64)
    orig[pm] = cand
    return pm, disc.sum(), np_oracle.weighted_distance(disc, np.abs(yp)), pack_np(orig[None])[0]


def test_tep_eval_above_three_trips(dec):
    n = 70000
    grid = per_trip(dec, "osd_tep_eval")
    assert_trips(dec, "osd_tep_eval", n, 4)
    y, cw = device_frames(dec, n, 2.0, 13)
    perm, parity, _ = dec.osd_front(y)
    rng = np.random.default_rng(14)
    w = rng.integers(0, 7, size=n)
    bits = rng.random((n, 64)).argsort(axis=1).argsort(axis=1) < w[:, None]    # w[f] random positions per frame
    masks = np.packbits(bits.astype(np.uint8), axis=1, bitorder="little").view(np.uint64)[:, 0]
    md = to_dev(masks.view(np.int64), dec)
    out = dec.osd_tep_eval(y, perm, parity, md)
    parts = sliced(lambda lo, hi: dec.osd_tep_eval(y[lo:hi], perm[lo:hi], parity[lo:hi], md[lo:hi]), n, grid)
    torch.cuda.synchronize()
    assert_same(out, parts, ("cw", "metric", "hd"))
    sel = stratified(n, grid, np.random.default_rng(15))
    sd = torch.from_numpy(sel).to(dec.device)
    yh, cwh, ph = y[sd].cpu().numpy(), cw[sd].to(torch.uint8).cpu().numpy(), perm[sd].cpu().numpy()
    got_cw, got_m, got_hd = words_np(out["cw"][sd]), out["metric"][sd].cpu().numpy(), out["hd"][sd].cpu().numpy()
    for j in range(len(sel)):
        pm, hd, m, cwp = _tep_eval_expected(yh[j], cwh[j], dec.code.G, masks[sel[j]])
        assert np.array_equal(ph[j], pm), sel[j]
        assert got_hd[j] == hd and got_m[j].view(np.uint32) == m.view(np.uint32), sel[j]
        assert np.array_equal(got_cw[j], cwp), sel[j]


# ---------------------------------------------------------------------------------------- H-form stage
def _table(dec, blocks):
    from short_ldpc_decoding_osd_amd.ordered_statistics_decoding import _teps_from_matrix
    teps = np.concatenate([_teps_from_matrix(E) for E in blocks])
    off = np.insert(np.cumsum([len(E) for E in blocks]), 0, 0).astype(np.int32)
    return teps, off


@pytest.fixture(scope="module")
def hform(dec):
    """70 000 frames at 2.5 dB: ordering values x = NMS-4 posteriors (the stand-in for the refined LLRs), metric values
    y = channel values, labels; on the device, and the front end of the whole batch."""
    F = 70000
    y, cw = device_frames(dec, F, 2.5, 41)
    x = dec.nms(y, 4, ALPHA0)["soft"]
    lab = dec.pack_bits(cw.to(torch.int64))
    return dict(F=F, x=x, y=y, cw=cw, lab=lab, front=dec.hosd_front(x))


def test_hosd_front_above_three_trips(dec, hform):
    F, x = hform["F"], hform["x"]
    grid = per_trip(dec, "hosd_front")
    assert_trips(dec, "hosd_front", F, 3)
    parts = [dec.hosd_front(x[lo:lo + grid]) for lo in range(0, F, grid)]
    torch.cuda.synchronize()
    for i in range(4):
        assert torch.equal(hform["front"][i], torch.cat([p[i] for p in parts])), i


@pytest.mark.parametrize("form", ["runs", "work_items"])
def test_hosd_search_above_three_trips(dec, hform, form):
    """Both forms of hosd_search: the per-thread-run form (weight <= 2: the table sits in LDS once per workgroup, reused on
    every trip) and the work-item form (weight-3 TEPs: the LDS ticket is reset per frame)."""
    path = [p for p in PATH if sum(p) <= 2] if form == "runs" else PATH
    assert (max(sum(p) for p in path) == 3) == (form == "work_items")
    blocks = _blocks(path)
    teps, off = _table(dec, blocks)
    td, od = to_dev(teps, dec), to_dev(off, dec)
    F, x, y, lab, front = hform["F"], hform["x"], hform["y"], hform["lab"], hform["front"]
    grid = per_trip(dec, "hosd_search")
    assert_trips(dec, "hosd_search", F, 4)
    out = dec.hosd_search(x, y, front, td, od, label_bits=lab)
    parts = sliced(lambda lo, hi: dec.hosd_search(x[lo:hi], y[lo:hi], tuple(t[lo:hi] for t in front[:3]), td, od,
                                                  label_bits=lab[lo:hi]), F, grid)
    torch.cuda.synchronize()
    assert_same(out, parts, [k for k, v in out.items() if v is not None], form)
    sel = stratified(F, grid, np.random.default_rng(21), extra=100, tail=16)
    sd = torch.from_numpy(sel).to(dec.device)
    xh, yh, cwh = x[sd].cpu().numpy(), y[sd].cpu().numpy(), hform["cw"][sd].to(torch.uint8).cpu().numpy()
    lri, uidx, M, ns = (t[sd].cpu().numpy() for t in front)
    Mb = np.unpackbits(M.view(np.uint8).reshape(-1, 64, 8), axis=2, bitorder="little")
    bmin, barg = out["block_min"][sd].cpu().numpy(), out["block_arg"][sd].cpu().numpy()
    truth, metric, best = (out[k][sd].cpu().numpy() for k in ("truth", "metric", "best"))
    cwg = np.unpackbits(words_np(out["cw"][sd]).view(np.uint8).reshape(-1, 16), axis=1, bitorder="little")
    for j in range(len(sel)):
        r = np_oracle.hosd_frame(xh[j], yh[j], cwh[j], dec.code.H, blocks)
        tag = (form, int(sel[j]))
        assert np.array_equal(lri[j], r["lri"]) and np.array_equal(uidx[j], r["uidx"]), tag
        assert np.array_equal(Mb[j], r["M"]) and ns[j] == len(r["swaps"]), tag
        assert np.array_equal(bmin[j].view(np.uint32), r["block_min"].view(np.uint32)), tag
        assert np.array_equal(barg[j], r["block_arg"]), tag
        assert truth[j] == r["truth"] and metric[j] == r["metric"], tag
        assert best[j] == r["best_index"] and np.array_equal(cwg[j], r["codeword"]), tag


@pytest.mark.parametrize("margin", [0.9, 1.0])
def test_hosd_sliding_above_three_trips(dec, hform, margin):
    """hosd_sliding on every frame against np_oracle.sliding_window_decide (test_gpu_dlosd._check_sliding, groups 1, the
    default and nblk), and against itself in one-trip slices.  At 0.9 the frames stop at different depths."""
    F, x, y, front = hform["F"], hform["x"], hform["y"], hform["front"]
    grid = per_trip(dec, "hosd_sliding")
    assert_trips(dec, "hosd_sliding", F, 4)
    blocks = _blocks(PATH)
    win = 3
    w1, w2 = DM.stopping_fcn_weights(win)
    xh, yh, cwh = x.cpu().numpy(), y.cpu().numpy(), hform["cw"].to(torch.uint8).cpu().numpy()
    exp = _check_sliding(dec, xh, yh, cwh, blocks, win, margin, w1, w2, groups=(1, 0, len(blocks)))
    if margin < 1.0:
        assert len(np.unique(exp["deep"])) > 1
    teps, off = _table(dec, blocks)
    td, od = to_dev(teps, dec), to_dev(off, dec)
    fw = np.concatenate([w1.ravel(), w2.ravel()])
    lab = hform["lab"]
    whole = dec.hosd_sliding(x, y, front, td, od, win, margin, fw, label_bits=lab)
    parts = sliced(lambda lo, hi: dec.hosd_sliding(x[lo:hi], y[lo:hi], tuple(t[lo:hi] for t in front[:3]), td, od, win, margin,
                                                   fw, label_bits=lab[lo:hi]), F, grid)
    torch.cuda.synchronize()
    assert_same(whole, parts, [k for k, v in whole.items() if v is not None], margin)


# ---------------------------------------------------------------------------------------- pipeline and generic NMS
@pytest.fixture(scope="module")
def big_batch(dec):
    """600 001 frames at 2.5 dB generated on the device (compaction above its 8-flags-per-thread threshold)."""
    B = 600001
    y, cw = device_frames(dec, B, 2.5, 600)
    return dict(B=B, y=y, lab=dec.pack_bits(cw.to(torch.int64)), cwh=cw.to(torch.uint8).cpu().numpy(), ref={})


@pytest.mark.parametrize("keep_front", [True, False])
def test_pipeline_above_compaction_threshold(dec, big_batch, keep_front):
    from short_ldpc_decoding_osd_amd.pipeline import BatchPipeline
    B, y, lab, cwh = big_batch["B"], big_batch["y"], big_batch["lab"], big_batch["cwh"]
    assert B > COMPACT_FPT8_ABOVE
    pipe = BatchPipeline(dec, B, 10, ALPHA0, osd_order=2, keep_front=keep_front).bind(y, lab)
    pipe.run()
    torch.cuda.synchronize()
    nf = int(pipe.count.cpu()[0])
    assert_trips(dec, "osd_fused2r" if not keep_front else "osd_search2r", nf, 4)
    if keep_front:
        assert_trips(dec, "osd_front", nf, 3)
    _, fail, cnt = c_oracle.evaluate(dec.code.H, pipe.soft.cpu().numpy(), cwh)
    idx = np.flatnonzero(fail)
    c = pipe.counters().cpu().numpy()
    assert [int(v) for v in c[:5]] == [cnt[k] for k in ("frames", "frame_err", "bit_err", "undetected", "synd_fail")]
    assert np.array_equal(pipe.fail.cpu().numpy(), fail)
    assert nf == len(idx) and np.array_equal(pipe.index[:nf].cpu().numpy(), idx)
    if "osd" not in big_batch["ref"]:
        big_batch["ref"]["osd"] = c_oracle.conv_osd(dec.code.G, y[torch.from_numpy(idx).to(dec.device)].cpu().numpy(),
                                                    cwh[idx], 2)
    ref = big_batch["ref"]["osd"]
    check_conv(dict(cw=pipe.cw, best=pipe.best, metric=pipe.metric, ntep=pipe.ntep), ref, nf, keep_front)
    assert c[5] == nf and c[6] == int((~ref["correct"]).sum()) and c[7] == nf * ref["teps_size"]


def test_nms_generic_beyond_two_trips(dec):
    from short_ldpc_decoding_osd_amd import _lib
    B, T = 131072 + 5, 10
    grid = per_trip(dec, "nms_generic")
    assert_trips(dec, "nms_generic", B, 4)
    y, _ = device_frames(dec, B, 1.5, 77)
    gen = dec.nms(y, T, ALPHA0, want_traj=True, kernel=_lib.NMS_GENERIC)
    qc = dec.nms(y, T, ALPHA0, want_traj=True, kernel=_lib.NMS_QC16)
    torch.cuda.synchronize()
    assert_same(gen, qc, ("soft", "traj", "hard", "fail"))
    sel = stratified(B, grid, np.random.default_rng(78))
    sd = torch.from_numpy(sel).to(dec.device)
    soft_o, traj_o = c_oracle.nms(dec.code.H, y[sd].cpu().numpy(), T, ALPHA0, want_traj=True)
    assert np.array_equal(gen["soft"][sd].cpu().numpy().view(np.uint32), soft_o.view(np.uint32))
    assert np.array_equal(gen["traj"][:, sd].cpu().numpy().view(np.uint32), np.asarray(traj_o[1:]).view(np.uint32))


def test_nms_train_beyond_three_trips(dec):
    """nms_train_kernel at CCSDS T = 12 (two frames per workgroup, 16 384 workgroups): from the second trip on a wavefront
    builds its tape over the previous frame's.  Per-frame loss / gradient / hard / fail against one-trip slices (bits), a
    stratified sample against the float64 model and the C oracle, the batch sums against math.fsum, and the call without
    the gradient (a frame ends after its forward pass) against the full one."""
    B, T = 100000, 12
    alpha = np.array([0.669435 * (1 + 0.03 * (t % 5)) for t in range(T)], np.float32)
    w_in, w_out = 0.9, 1.1
    H = dec.code.H
    assert Z.train_waves(H, T) == 2
    grid = per_trip(dec, "nms_train")
    assert_trips(dec, "nms_train", B, 3)
    y, cw = device_frames(dec, B, 2.0, 91)
    lab = dec.pack_bits(cw.to(torch.int64))
    keys = ("loss", "grad", "hard", "fail")
    whole = dec.nms_grad(y, lab, T, alpha, w_in, w_out, want_hard=True, want_fail=True)
    parts = sliced(lambda lo, hi: {k: v for k, v in dec.nms_grad(y[lo:hi], lab[lo:hi], T, alpha, w_in, w_out, want_sums=False,
                                                              want_hard=True, want_fail=True).items() if k in keys}, B, grid)
    fwd = dec.nms_grad(y, lab, T, alpha, w_in, w_out, want_grad=False, want_sums=False, want_hard=True, want_fail=True)
    torch.cuda.synchronize()
    for k in keys:
        assert torch.equal(whole[k].view(torch.uint8), parts[k].view(torch.uint8)), k
        if k != "grad":
            assert torch.equal(whole[k].view(torch.uint8), fwd[k].view(torch.uint8)), k
    sel = stratified(B, grid, np.random.default_rng(92), extra=100, tail=32)
    sd = torch.from_numpy(sel).to(dec.device)
    yh, cwh = y[sd].cpu().numpy(), cw[sd].to(torch.uint8).cpu().numpy()
    model = grad_model(H, yh, cwh, T, alpha, w_in, w_out)
    bound = rel_bound(T)
    loss = whole["loss"][sd].cpu().numpy().astype(np.float64)
    grad = whole["grad"][sd].cpu().numpy().astype(np.float64)
    assert np.all(np.abs(loss - model["loss"]) <= bound * model["loss"] + 1e-30)
    assert np.all(np.abs(grad - model["grad"]) <= bound * model["mass"] + 1e-30)
    soft_o = c_oracle.nms(H, yh, T, alpha, w_in, w_out)
    hard_o, fail_o, _ = c_oracle.evaluate(H, soft_o, None)
    assert np.array_equal(words_np(whole["hard"][sd]), pack_np(hard_o))
    assert np.array_equal(whole["fail"][sd].cpu().numpy(), fail_o)
    ls, gs = whole["loss_sum"].cpu().numpy(), whole["grad_sum"].cpu().numpy()
    lossh, gradh = whole["loss"].cpu().numpy().astype(np.float64), whole["grad"].cpu().numpy().astype(np.float64)
    assert abs(ls[0] - math.fsum(lossh)) <= 1e-12 * abs(ls[0])
    for k in range(T + 2):
        want = math.fsum(gradh[:, k])
        assert abs(gs[k] - want) <= 1e-12 * max(abs(want), math.fsum(np.abs(gradh[:, k])))
