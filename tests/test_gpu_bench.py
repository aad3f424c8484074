"""-m gpu: bench.py's plain run and --dump-outputs.  A plain run prints the contract fields and none of the --full
measurements; two runs with the same arguments dump the same arrays; and the dumped arrays are what the last timed step
computed: the C oracle gives them bit for bit on the same frames (regenerated with bench.make_frames and its seed)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, STEPS = 20000, 6          # (more frames than bench.DUMP_FRAMES: the dump is the seeded sample)


def _bench(out_dir, *extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", "1",
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
