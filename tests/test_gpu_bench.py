"""-m gpu: bench.py's plain run and --dump-outputs.  A plain run prints the contract fields and none of the --full
measurements; two runs with the same arguments dump the same arrays; and the dumped arrays are what the last timed step
computed: the C oracle gives them bit for bit on the same frames (regenerated with bench.make_frames and its seed).

With 6 steps over 4 batches bench.py replays its graph once (steps 0-3) and runs steps 4 and 5 as eager calls: the step
test_plain_run_and_dumped_outputs checks is an EAGER one.  test_dumped_step_is_a_replayed_one runs 8 steps, two rotations in
one graph launch, so that the dumped step 7 (batch 3 on branch 3) comes out of the replayed graph, for the three searches and
both OSD routes; it also asserts that the timed region was the graph with parallel branches, which a failed capture
(bench.py then times eager calls and says so in the line only) would not be.

Wall time on one MI355X: 20 s for the file's 5 cases; the slowest is test_plain_run_and_dumped_outputs with its two bench.py
runs, 7.7 s; a case of test_dumped_step_is_a_replayed_one (one bench.py run) takes 2.6 to 3.9 s."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, STEPS = 20000, 6          # (more frames than bench.DUMP_FRAMES: the dump is the seeded sample)


def _bench(out_dir, *extra, steps=STEPS):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--batch", str(B), "--dump-outputs", out_dir, *extra], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def test_plain_run_and_dumped_outputs(tmp_path):
    import torch

    import bench
    from oracle import c_oracle
    from short_ldpc_decoding_osd_amd import Code
    from short_ldpc_decoding_osd_amd.runtime import Decoder
    from short_ldpc_decoding_osd_amd.weights import STORED_NMS1_WEIGHT, softplus32

    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    line = _bench(a)
    assert line["steps"] == STEPS and line["ms_per_step"] > 0 and line["value"] > 0 and line["unit"] == "frames/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f32" and line["metric"].startswith("decoded frames/sec")
    assert not {"roofline", "overlap", "cpu_baseline", "fer_vs_cpu"} & set(line)
    _bench(b)
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and {"soft.npy", "hard.npy", "fail.npy", "osd_cw.npy"} <= set(names)
    got = {n[:-4]: np.load(os.path.join(a, n)) for n in names}
    for n in names:
        assert np.array_equal(got[n[:-4]], np.load(os.path.join(b, n))), n
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 64 << 20

    # the last timed step decoded batch (STEPS - 1) % 4 of bench.py's rotation over four batches
    dec = Decoder(Code(), 0)
    y, labels = bench.make_frames(dec, B, seed=20241020 + 1000 * ((STEPS - 1) % 4))
    y, cw = y.cpu().numpy(), dec.unpack_bits(labels).cpu().numpy().astype(np.uint8)
    torch.cuda.synchronize()
    frame = got["frame"].astype(np.int64)
    assert np.array_equal(frame, bench.dump_sample(B)) and frame.size == bench.DUMP_FRAMES
    soft = c_oracle.nms(dec.code.H, y[frame], 10, float(softplus32(STORED_NMS1_WEIGHT)))
    hard, fail, _ = c_oracle.evaluate(dec.code.H, soft, cw[frame])
    assert np.array_equal(got["soft"], soft) and np.array_equal(got["hard"], hard) and np.array_equal(got["fail"], fail)
    assert got["counters"][0] == B
    osd_frame = got["osd_frame"].astype(np.int64)
    assert np.array_equal(osd_frame, frame[fail.astype(bool)])
    sub = slice(0, 400)
    ref = c_oracle.conv_osd(dec.code.G, y[osd_frame[sub]], cw[osd_frame[sub]], 2)
    assert np.array_equal(got["osd_cw"][sub], ref["codeword"]) and np.array_equal(got["osd_metric"][sub], ref["metric"])
    assert np.array_equal(got["osd_best"][sub], ref["best"])


REPLAYED_STEPS = 8           # two rotations over the four batches in one graph launch: the last step, 7, is batch 3 on branch 3
REPLAYED = [("nms10_osd2", "front+search"), ("nms10_fs2", "front+search"), ("nms10_pb3", "front+search"), ("nms10_fs2", "decode")]


@pytest.mark.parametrize("workload,route", REPLAYED, ids=[f"{w}-{r}" for w, r in REPLAYED])
def test_dumped_step_is_a_replayed_one(tmp_path, workload, route):
    import bench
    from short_ldpc_decoding_osd_amd import Code, _lib
    from short_ldpc_decoding_osd_amd.runtime import Decoder
    from tests import pipeline_oracle as PO

    line = _bench(str(tmp_path), "--workload", workload, "--osd-route", route, steps=REPLAYED_STEPS)
    assert line["steps"] == REPLAYED_STEPS and line["config"]["osd_route"] == route
    assert line["timed_region"].startswith("HIP graph replay"), line["timed_region"]
    assert line["timed_region_info"] == {"graph_steps_per_launch": 8, "graph_branches": 4, "overlapped": True}
    got = {n[:-4]: np.load(os.path.join(str(tmp_path), n)) for n in os.listdir(str(tmp_path))}

    dec = Decoder(Code(), 0)
    order, algo = PO.workload(workload)
    o = PO.batch(dec, bench.SNR_DB, B, (REPLAYED_STEPS - 1) % 4)         # (shared by the four cases)
    frame = got["frame"].astype(np.int64)
    assert np.array_equal(frame, bench.dump_sample(B)) and frame.size == bench.DUMP_FRAMES
    assert np.array_equal(got["soft"].view(np.uint32), o["soft"][frame].view(np.uint32))
    assert np.array_equal(got["hard"], np.unpackbits(o["hard"][frame].view(np.uint8), axis=1, bitorder="little"))
    assert np.array_equal(got["fail"], o["fail"][frame])
    osd_frame = got["osd_frame"].astype(np.int64)
    assert np.array_equal(osd_frame, frame[o["fail"][frame].astype(bool)])
    r = PO.ref(dec, o, (algo, order))
    if algo == _lib.OSD_PB:
        cw, metric, best, ntep = r["codeword"], r["metric"], r["best_index"], r["num_teps"]
    elif algo == _lib.OSD_FS:
        cw, metric, best, ntep = r["codeword_ref"], r["metric_ref"], r["best_index"], r["num_teps"]
    else:
        cw, metric, best, ntep = r["codeword"], r["metric"], r["best"], np.full(len(o["idx"]), r["teps_size"])
    sub = slice(0, 400)
    pos = np.searchsorted(o["idx"], osd_frame[sub])                      # the listed frames' places in the batch's failure list
    assert len(pos) == 400 and np.array_equal(o["idx"][pos], osd_frame[sub])
    assert np.array_equal(got["osd_cw"][sub], cw[pos])
    assert np.array_equal(got["osd_metric"][sub].view(np.uint32), metric[pos].view(np.uint32))
    assert np.array_equal(got["osd_best"][sub], best[pos]) and np.array_equal(got["osd_ntep"][sub], ntep[pos])
    want = o["five"] + [len(o["idx"]), int((cw != o["cwf"]).any(axis=1).sum()), int(ntep.sum())]
    assert got["counters"].tolist() == want
