"""-m gpu: the (128,64) search kernels on front-end results no CCSDS frame can produce -- the generator zoo of
tests/osd_generators.py (equal, zero, all-ones and sparse rows of P', all weight inside / outside the two parity bytes the
metric prefix reads), bit for bit against the C oracle run on the zoo's own generator (checked against the NumPy
restatement by tests/test_osd_generators_host.py, which also asserts the premises of every case).

(perm, P') come from the C oracle's front end and go to ldpc_osd_search / ldpc_osd_tep_eval of a CCSDS context: those entry
points never look at the context's generator.  Out of reach for the same reason: ldpc_osd_decode, the fused order-2 kernel
and the PB front-inside route, which run the device front end on the context's generator.

Everything is compared exactly, integers equal and metrics as uint32 bit patterns, on every frame."""
import numpy as np
import pytest
import torch

from oracle import c_oracle, np_oracle
from tests import osd_generators as Z
from tests.gpu_util import pack_np, to_dev, words_np

pytestmark = pytest.mark.gpu
F32 = np.float32
CASES = [(n, m) for n in Z.NAMES for m in Z.MODES]
FRAMES = 96
FS_THRESHOLDS = [(0.1, 6.5, 30.0), (0.1, 14.5, 30.0), (0.02, 11.0, 18.0)]       # (beta, tau_e, tau_psc)
PB_ROUTES = [dict(), dict(pb_path="block"), dict(pb_path="replay")]
SMALL_BUDGETS = dict(budget_s=64, budget_m=64, budget=64, budget_l=64, budget_xl=64)
_REF = {}


@pytest.fixture(scope="module")
def dec():
    from short_ldpc_decoding_osd_amd import Code
    from short_ldpc_decoding_osd_amd.runtime import Decoder
    return Decoder(Code())


def ref(kind, c, *args, frames=None):
    """One C-oracle result per (case, search, parameters), shared by the tests and left unchanged."""
    n = len(c["y"]) if frames is None else frames
    key = (kind, c["name"], c["mode"], c.get("form", "front"), n) + args
    if key not in _REF:
        _REF[key] = getattr(c_oracle, kind)(c["G"], c["y"][:n], c["cw"][:n], *args)
    return _REF[key]


def dev(dec, c, frames=None):
    n = len(c["y"]) if frames is None else frames
    return (to_dev(np.array(c["y"]), dec), to_dev(c["perm"][:n].astype(np.uint8), dec),      # (copies: the case is read-only)
            to_dev(np.array(c["parity"][:n]).view(np.int64), dec))


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_conv(out, r, tag, sel=None):
    pick = (lambda a: a) if sel is None else (lambda a: a[sel])
    n = len(pick(r["best"]))
    assert np.array_equal(out["best"].cpu().numpy()[:n], pick(r["best"])), tag
    assert np.array_equal(words_np(out["cw"])[:n], pack_np(pick(r["codeword"]))), tag
    assert np.array_equal(u32(out["metric"].cpu().numpy()[:n]), u32(pick(r["metric"]))), tag
    assert (out["ntep"].cpu().numpy()[:n] == r["teps_size"]).all(), tag


def conv_routes(dec, c, order, **lists):
    yd, perm, parity = dev(dec, c) if not lists else lists.pop("inputs")
    routes = {"default": dec.osd_search(yd, perm, parity, dec.osd_params(order), **lists),
              "table": dec.osd_search(yd, perm, parity, dec.osd_params(order, table_scan=True), **lists)}
    if order == 2:
        routes["readlane"] = dec.osd_search(yd, perm, parity, dec.osd_params(2, readlane_scan=True), **lists)
    torch.cuda.synchronize()
    return routes


@pytest.mark.parametrize("name,mode", CASES)
def test_conventional(dec, name, mode):
    c = Z.case(name, mode, FRAMES)
    for order in (0, 1, 2, 3):
        r = ref("conv_osd", c, order)
        assert np.array_equal(r["nswaps"], c["nswaps"])
        routes = conv_routes(dec, c, order)
        for rn, o in routes.items():
            check_conv(o, r, (name, mode, order, rn))
            for k in ("cw", "metric", "best", "ntep"):
                assert torch.equal(o[k], routes["default"][k]), (order, rn, k)


def fs_best(r):
    """What ``best`` holds without the quirk: the stopping candidate's rank in visit order on a tau_e hit beyond order 0,
    the winner's rank elsewhere."""
    return np.where(r["hit"], r["num_teps"] - 1, r["best_index"])


def check_fs(out, r, quirk, tag, sel=None):
    pick = (lambda a: a) if sel is None else (lambda a: a[sel])
    n = len(pick(r["num_teps"]))
    assert np.array_equal(out["ntep"].cpu().numpy()[:n], pick(r["num_teps"])), tag
    want_cw = r["codeword_ref"] if quirk else r["codeword_hit"]
    want_m = r["metric_ref"] if quirk else r["metric_hit"]
    assert np.array_equal(words_np(out["cw"])[:n], pack_np(pick(want_cw))), tag
    assert np.array_equal(u32(out["metric"].cpu().numpy()[:n]), u32(pick(want_m))), tag
    assert np.array_equal(out["best"].cpu().numpy()[:n], pick(r["best_index"] if quirk else fs_best(r))), tag


def fs_run(dec, inputs, order, th, quirk, **lists):
    from short_ldpc_decoding_osd_amd import _lib
    beta, tau_e, tau_psc = th
    p = dec.osd_params(order, _lib.OSD_FS, fs_beta=beta, fs_tau_e=tau_e, fs_tau_psc=tau_psc, fs_reference_quirk=quirk)
    out = dec.osd_search(*inputs, p, **lists)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name,mode", CASES)
def test_fs(dec, name, mode):
    c = Z.case(name, mode, FRAMES)
    inputs = dev(dec, c)
    for order in (1, 2, 3):
        for th in FS_THRESHOLDS:
            r = ref("fs_osd", c, order, *th)
            for quirk in (1, 0):
                check_fs(fs_run(dec, inputs, order, th, quirk), r, quirk, (name, mode, order, th, quirk))


def check_pb(out, aux, r, tag, sel=None):
    pick = (lambda a: a) if sel is None else (lambda a: a[sel])
    n = len(pick(r["num_teps"]))
    a = aux.cpu().numpy()[:n]
    assert np.array_equal(out["ntep"].cpu().numpy()[:n], pick(r["num_teps"])), tag
    assert np.array_equal(a[:, 3], pick(r["stop"])) and np.array_equal(a[:, 0], pick(r["comparisons"])), tag
    assert np.array_equal(a[:, 1], pick(r["suc1"])) and np.array_equal(a[:, 2], pick(r["suc2"])), tag
    assert np.array_equal(out["best"].cpu().numpy()[:n], pick(r["best_index"])), tag
    assert np.array_equal(words_np(out["cw"])[:n], pack_np(pick(r["codeword"]))), tag
    assert np.array_equal(u32(out["metric"].cpu().numpy()[:n]), u32(pick(r["metric"]))), tag


def pb_run(dec, inputs, order, snr, kw, **lists):
    from short_ldpc_decoding_osd_amd import _lib
    aux = torch.zeros((inputs[1].shape[0], 4), dtype=torch.int32, device=dec.device)
    out = dec.osd_search(*inputs, dec.osd_params(order, _lib.OSD_PB, snr_db=snr, aux=aux, **kw), **lists)
    torch.cuda.synchronize()
    return out, aux


def pb_all_routes(dec, c, snr, tag):
    for order in (1, 2, 3):
        r = ref("pb_osd", c, order, snr)
        inputs = dev(dec, c)
        for kw in PB_ROUTES:
            out, aux = pb_run(dec, inputs, order, snr, kw)
            check_pb(out, aux, r, tag + (order, tuple(kw.values())))


@pytest.mark.parametrize("snr", [1.0, 2.5])
@pytest.mark.parametrize("name,mode", CASES)
def test_pb(dec, name, mode, snr):
    c = Z.case(name, mode, FRAMES)
    pb_all_routes(dec, c, snr, (name, mode, snr))
    if mode == "grid":                       # equal sums through the hand-over and the workgroup scan's tie rules
        prev = dec.set_pb_tuning(**SMALL_BUDGETS)
        try:
            pb_all_routes(dec, c, snr, (name, mode, snr, "budgets 64"))
        finally:
            dec.set_pb_tuning(**prev)
        assert dec.pb_tuning() == prev


def _masks(c, rng):
    """Per frame one mask of each weight 0, 1, 2, 3, 7, 64, one that selects only zero rows of P'' and one that selects only
    rows equal to another (0 where the frame has none): [8, F] uint64."""
    F = len(c["y"])
    out = np.zeros((8, F), dtype=np.uint64)
    for f in range(F):
        for i, wt in enumerate((0, 1, 2, 3, 7, 64)):
            for p in rng.choice(64, size=wt, replace=False):
                out[i, f] |= np.uint64(1) << np.uint64(p)
        rows = c["parity"][f]
        for p in np.flatnonzero(rows == 0):
            out[6, f] |= np.uint64(1) << np.uint64(p)
        vals, inv, cnt = np.unique(rows, return_inverse=True, return_counts=True)
        rep = np.flatnonzero((cnt > 1) & (vals != 0))
        if rep.size:
            for p in np.flatnonzero(inv == rep[rng.integers(rep.size)]):
                out[7, f] |= np.uint64(1) << np.uint64(p)
    return out


def check_tep_eval(dec, c, tag):
    yd, perm, parity = dev(dec, c)
    masks = _masks(c, np.random.default_rng(77))
    if c["name"] == "zero_rows":
        assert (masks[6] != 0).all()
    if c["name"] in ("equal_rows", "rank_one"):
        assert (masks[7] != 0).all()
    for row in masks:
        te = dec.osd_tep_eval(yd, perm, parity, to_dev(row.view(np.int64), dec))
        torch.cuda.synchronize()
        got_cw, got_m, got_hd = words_np(te["cw"]), te["metric"].cpu().numpy(), te["hd"].cpu().numpy()
        for f in range(len(c["y"])):
            yp, Gp, pm = c["yp"][f], c["Gp"][f].astype(np.int64), c["perm"][f]
            hard = np.where(yp > 0, 0, 1).astype(np.int64)
            e = np.array([(int(row[f]) >> p) & 1 for p in range(64)], dtype=np.int64)
            cand = ((hard[:64] + e) % 2).dot(Gp) % 2
            disc = (cand + hard) % 2
            assert got_hd[f] == disc.sum(), tag + (f,)
            assert u32(got_m[f:f + 1])[0] == u32(np_oracle.weighted_distance(disc, np.abs(yp)).reshape(1))[0], tag + (f,)
            orig = np.empty(128, dtype=np.int64)
            orig[pm] = cand
            assert np.array_equal(got_cw[f], pack_np(orig[None])[0]), tag + (f,)


@pytest.mark.parametrize("name,mode", CASES)
def test_tep_eval(dec, name, mode):
    check_tep_eval(dec, Z.case(name, mode, FRAMES), (name, mode))


@pytest.fixture(scope="module")
def teps3():
    return np_oracle.tep_matrix(64, 3)


@pytest.mark.parametrize("sorted_y", [True, False])
@pytest.mark.parametrize("name,mode", Z.DIRECT)
def test_direct_form(dec, teps3, name, mode, sorted_y):
    """perm = identity and y already primed: the pair as written, against convention_osd_main restated in NumPy on
    (y', label', [I | P']).  Sorted y' also through FS and PB against the C oracle on G = [I | P'], whose front end is then
    the identity with no exchange.  Unsorted y': the conventional search and the single-TEP evaluation only -- the FS and
    PB loops of the reference assume the order, and nothing defines their result without it."""
    c = dict(Z.direct(name, mode, sorted_y), form="sorted" if sorted_y else "unsorted")
    F = len(c["y"])
    for order, frames in ((0, F), (1, F), (2, 6), (3, 2)):
        routes = conv_routes(dec, c, order)
        for rn, o in routes.items():
            best, met, cw = o["best"].cpu().numpy(), o["metric"].cpu().numpy(), words_np(o["cw"])
            for f in range(frames):
                r = np_oracle.convention_osd(c["y"][f], c["cw"][f], c["G"], order, teps=teps3 if order == 3 else None)
                tag = (name, mode, sorted_y, order, rn, f)
                assert best[f] == r["best_index"] and u32(met[f:f + 1])[0] == u32(r["metric"].reshape(1))[0], tag
                assert np.array_equal(cw[f], pack_np(r["codeword"][None])[0]), tag
    check_tep_eval(dec, c, (name, mode, sorted_y))
    if not sorted_y:
        return
    for f in range(F):
        perm, Gp, sw = c_oracle.osd_front(c["G"], c["y"][f])
        assert np.array_equal(perm, np.arange(128)) and not sw and np.array_equal(Gp, c["G"]), f
    inputs = dev(dec, c)
    for order in (0, 1, 2, 3):
        r = ref("conv_osd", c, order)
        assert not r["nswaps"].any()
        check_conv(dec.osd_search(*inputs, dec.osd_params(order)), r, (name, mode, order))
    for order in (1, 2, 3):
        for th in FS_THRESHOLDS[:2]:
            r = ref("fs_osd", c, order, *th)
            for quirk in (1, 0):
                check_fs(fs_run(dec, inputs, order, th, quirk), r, quirk, (name, mode, order, th, quirk))
        for snr in (1.0, 2.5):
            r = ref("pb_osd", c, order, snr)
            for kw in PB_ROUTES:
                out, aux = pb_run(dec, inputs, order, snr, kw)
                check_pb(out, aux, r, (name, mode, order, snr, tuple(kw.values())))


def test_frame_list(dec):
    """equal_rows / grid through a frame list: ``index`` a shuffled subset of the frames, the device-side ``count`` smaller than
    F, perm and parity laid out by list position (perm_in[f] belongs to y[index[f]])."""
    c = Z.case("equal_rows", "grid", FRAMES)
    rng = np.random.default_rng(12)
    index = rng.permutation(FRAMES)[:80].astype(np.int32)
    n = 64
    assert not np.array_equal(index[:n], np.arange(n))
    inputs = (to_dev(np.array(c["y"]), dec), to_dev(c["perm"][index].astype(np.uint8), dec),
              to_dev(c["parity"][index].view(np.int64), dec))
    lists = dict(index=to_dev(index, dec), count=to_dev(np.array([n], np.int32), dec), F=len(index))
    sel = index[:n]
    for order in (0, 1, 2, 3):
        r = ref("conv_osd", c, order)
        for rn, o in conv_routes(dec, c, order, inputs=inputs, **lists).items():
            check_conv(o, r, (order, rn), sel)
    for order in (1, 2):
        th = FS_THRESHOLDS[1]
        r = ref("fs_osd", c, order, *th)
        for quirk in (1, 0):
            check_fs(fs_run(dec, inputs, order, th, quirk, **lists), r, quirk, (order, quirk), sel)
        r = ref("pb_osd", c, order, 1.0)
        for kw in PB_ROUTES:
            out, aux = pb_run(dec, inputs, order, 1.0, kw, **lists)
            check_pb(out, aux, r, (order, tuple(kw.values())), sel)
    masks = _masks(c, np.random.default_rng(78))[[2, 7]]
    for row in masks:
        te = dec.osd_tep_eval(*inputs, to_dev(row[index].view(np.int64), dec), index=lists["index"], count=lists["count"])
        whole = dec.osd_tep_eval(*dev(dec, c), to_dev(row.view(np.int64), dec))
        torch.cuda.synchronize()
        pick = torch.from_numpy(sel.astype(np.int64)).to(dec.device)
        for k in ("cw", "metric", "hd"):
            assert torch.equal(te[k][:n], whole[k][pick]), k
