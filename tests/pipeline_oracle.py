"""What one BatchPipeline.run() over a batch of bench.py must leave behind, from the C oracle, and the checker that
compares a pipeline's buffers with it -- shared by tests/test_gpu_graph_rotation.py and tests/test_gpu_host_threads.py.

A batch is bench.make_frames(dec, B, seed=20241020 + 1000 * i, snr_db=snr): the frames bench.py's rank 0 rotates over.
The oracle of a batch (NMS-10, the counters, the failure list) is computed once per (snr, B, i) from the frames copied to
the host and never changed afterwards; the searches over its failures are added when a test first asks for them.
Everything is compared exactly: floats by their bit patterns, integers and counters as they are."""
import concurrent.futures

import numpy as np

import bench
from oracle import c_oracle
from short_ldpc_decoding_osd_amd import _lib
from short_ldpc_decoding_osd_amd.weights import STORED_NMS1_WEIGHT, softplus32
from tests import abi_calls as A
from tests.gpu_util import pack_np, words_np
from tests.test_gpu_many_frames import check_conv
from tests.test_gpu_osd_generators import check_fs, check_pb

T = bench.T_ITERS
ALPHA = float(softplus32(STORED_NMS1_WEIGHT))
FS_DEFAULTS = (0.1, 6.5, 30.0)               # Decoder.osd_params' beta, tau_e, tau_psc, quirk on: what bench.py runs
NMS_OUT = ("soft", "hard", "fail")
LIST_OUT = ("index", "perm", "parity", "cw", "metric", "best", "ntep", "aux")       # rows 0 .. count - 1 are written
_BATCH = {}


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def workload(name):
    """(OSD order or None, algorithm id) of a bench.py workload."""
    return bench.WORKLOADS[name][0], bench.OSD_ALGO.get(name, _lib.OSD_CONVENTIONAL)


def batch(dec, snr, B, i):
    key = (float(snr), int(B), int(i), dec.device.index)
    if key not in _BATCH:
        y, labels = bench.make_frames(dec, B, seed=20241020 + 1000 * i, snr_db=snr)
        yh = y.cpu().numpy()
        cwh = dec.unpack_bits(labels).cpu().numpy().astype(np.uint8)
        soft = c_oracle.nms(dec.code.H, yh, T, ALPHA)
        hard, fail, cnt = c_oracle.evaluate(dec.code.H, soft, cwh)
        idx = np.flatnonzero(fail)
        _BATCH[key] = dict(snr=float(snr), B=int(B), i=int(i), y=y, labels=labels, soft=soft, hard=pack_np(hard), fail=fail,
                           five=[int(cnt[k]) for k in ("frames", "frame_err", "bit_err", "undetected", "synd_fail")],
                           idx=idx, yf=yh[idx], cwf=cwh[idx], refs={})
    return _BATCH[key]


def _front(G, yf):
    perm, par = np.empty((len(yf), 128), np.uint8), np.empty((len(yf), 64), np.uint64)
    for f, row in enumerate(yf):
        p, Gp, _ = c_oracle.osd_front(G, row)
        perm[f] = p
        par[f] = np.packbits(Gp[:, 64:].astype(np.uint8), axis=1, bitorder="little").view(np.uint64)[:, 0]
    return dict(perm=perm, parity=par)


def _search(dec, o, kind):
    G = dec.code.G
    if kind == "front":
        return _front(G, o["yf"])
    algo, order = kind
    if algo == _lib.OSD_PB:
        return c_oracle.pb_osd(G, o["yf"], o["cwf"], order, o["snr"])
    if algo == _lib.OSD_FS:
        return c_oracle.fs_osd(G, o["yf"], o["cwf"], order, *FS_DEFAULTS)
    return c_oracle.conv_osd(G, o["yf"], o["cwf"], order)


def prepare(dec, batches, order, algo, front):
    """The searches (and front-end results) the checks of these batches will ask for, the missing ones side by side: the C
    calls release the interpreter lock."""
    if order is None:
        return
    kinds = [(algo, order)] + (["front"] if front else [])
    todo = [(o, k) for o in batches for k in kinds if k not in o["refs"]]
    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as ex:
        for (o, k), r in zip(todo, ex.map(lambda ok: _search(dec, *ok), todo)):
            o["refs"][k] = r


def ref(dec, o, kind):
    if kind not in o["refs"]:
        o["refs"][kind] = _search(dec, o, kind)
    return o["refs"][kind]


def outputs(pipe):
    """name -> output buffer of the pipeline, the ones it has."""
    names = NMS_OUT + (("count",) + LIST_OUT if pipe.osd_order is not None else ())
    return {n: getattr(pipe, n) for n in names if getattr(pipe, n, None) is not None}


def fill_sentinels(pipe):
    for t in outputs(pipe).values():
        t.fill_(A.SENT[t.dtype])


def snapshot(pipe):
    """Host copies of every output buffer and of the counters."""
    s = {n: t.cpu() for n, t in outputs(pipe).items()}
    s["counters"] = pipe.counters().cpu()
    return s


def check(dec, s, o, order, algo, runs, tag=""):
    """Snapshot ``s`` holds exactly what ``runs`` runs of the pipeline (order, algo) over batch ``o`` leave behind."""
    assert np.array_equal(u32(s["soft"].numpy()), u32(o["soft"])), (tag, "soft")
    assert np.array_equal(words_np(s["hard"]), o["hard"]), (tag, "hard")
    assert np.array_equal(s["fail"].numpy(), o["fail"]), (tag, "fail")
    want = list(o["five"])
    if order is None:
        want += [0, 0, 0]
    else:
        nf = len(o["idx"])
        assert int(s["count"][0]) == nf, (tag, "count")
        assert np.array_equal(s["index"][:nf].numpy(), o["idx"]), (tag, "index")
        out = {k: s[k] for k in ("cw", "metric", "best", "ntep")}
        r = ref(dec, o, (algo, order))
        if algo == _lib.OSD_PB:
            check_pb(out, s["aux"], r, (tag, "pb"))
            cw, teps = r["codeword"], int(r["num_teps"].sum())
        elif algo == _lib.OSD_FS:
            check_fs(out, r, 1, (tag, "fs"))
            cw, teps = r["codeword_ref"], int(r["num_teps"].sum())
        else:
            check_conv(out, r, nf, (tag, "conv"))
            cw, teps = r["codeword"], nf * r["teps_size"]
        if "perm" in s:
            fr = ref(dec, o, "front")
            assert np.array_equal(s["perm"][:nf].numpy(), fr["perm"]), (tag, "perm")
            assert np.array_equal(words_np(s["parity"][:nf]), fr["parity"]), (tag, "parity")
        for k in LIST_OUT:
            assert k not in s or A.untouched(s[k], nf), (tag, k, "rows from count on")
        want += [nf, int((cw != o["cwf"]).any(axis=1).sum()), teps]
    assert s["counters"].tolist() == [runs * v for v in want], (tag, "counters")
