"""GPU box: python tests/tools/pipeline_long_fuzz.py [minutes] -- NMS-T + conventional OSD (orders 0-3) / FS-OSD through the one-call
pipeline against the C oracle on fresh random batches until the time is up: random SNR, iteration count, scale factor, batch size,
exact zeros and ties sprinkled in, front-end results in caller buffers or not (order 2 then runs the fused front-end + scan kernel),
plus the failed-frame rows of ldpc_nms_traj_rows.  Everything bit for bit.  (The long form of tests/test_gpu_fuzz.py.)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, ROOT)
import numpy as np, torch
from oracle import c_oracle, np_oracle
from short_ldpc_decoding_osd_amd import Code, _lib
from short_ldpc_decoding_osd_amd.pipeline import BatchPipeline
from short_ldpc_decoding_osd_amd.runtime import Decoder
from tests.gpu_util import pack_np, to_dev, words_np
dec = Decoder(Code())
minutes = float(sys.argv[1]) if len(sys.argv) > 1 else 3.0
t_end = time.time() + 60 * minutes
rng = np.random.default_rng(int(time.time()))
rounds = frames_total = 0
while time.time() < t_end:
    seed = int(rng.integers(1 << 30))
    r = np.random.default_rng(seed)
    snr = float(r.choice([0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 4.0]))
    T = int(r.choice([1, 3, 7, 10, 12, 16]))
    alpha = np.float32(r.uniform(0.4, 1.0))
    algo = int(r.choice([0, 0, 0, 1]))
    order = int(r.choice([0, 1, 2, 2, 2, 3])) if algo == 0 else int(r.choice([1, 2, 2, 3]))
    B = int(r.integers(1, 900 if order == 3 else 3000))
    keep_front = bool(r.random() < 0.5)
    y, cw = np_oracle.make_frames(dec.code.G, snr, B, r)
    if r.random() < 0.4:
        y[r.integers(0, B, 5), r.integers(0, 128, 5)] = 0.0
        k = int(r.integers(0, B)); y[k, 40:44] = y[k, 7]
    if r.random() < 0.15:
        q = float(r.choice([8.0, 64.0, 1024.0])); y = (np.round(y * q) / q).astype(np.float32)
    cfg = dict(seed=seed, snr=snr, T=T, alpha=float(alpha), algo=algo, order=order, B=B, keep_front=keep_front)
    pipe = BatchPipeline(dec, B, T, alpha, osd_order=order, osd_algo=algo, keep_front=keep_front).bind(to_dev(y, dec), dec.pack_bits(to_dev(cw, dec)))
    pipe.run()
    torch.cuda.synchronize()
    soft = c_oracle.nms(dec.code.H, y, T, alpha, want_traj=True)
    traj = None
    if isinstance(soft, tuple):
        soft, traj = soft
    hard, fail, counts = c_oracle.evaluate(dec.code.H, soft, cw)
    ok = np.array_equal(pipe.soft.cpu().numpy(), soft) and np.array_equal(words_np(pipe.hard), pack_np(hard)) and np.array_equal(pipe.fail.cpu().numpy(), fail)
    idx = np.flatnonzero(fail)
    nf = int(pipe.count.cpu()[0])
    ok = ok and nf == len(idx) and np.array_equal(pipe.index[:nf].cpu().numpy(), idx)
    if ok and nf:
        if algo == 0:
            ref = c_oracle.conv_osd(dec.code.G, y[idx], cw[idx], order)
            ok = (np.array_equal(pipe.best[:nf].cpu().numpy(), ref["best"]) and np.array_equal(pipe.metric[:nf].cpu().numpy(), ref["metric"])
                  and np.array_equal(words_np(pipe.cw[:nf]), pack_np(ref["codeword"])))
        else:
            ref = c_oracle.fs_osd(dec.code.G, y[idx], cw[idx], order)
            ok = (np.array_equal(pipe.ntep[:nf].cpu().numpy(), ref["num_teps"]) and np.array_equal(words_np(pipe.cw[:nf]), pack_np(ref["codeword_ref"]))
                  and np.array_equal(pipe.metric[:nf].cpu().numpy(), ref["metric_ref"]))
        if ok and traj is not None and T > 0:
            rows = dec.nms_traj_rows(to_dev(y, dec), pipe.index, pipe.count, nf, T, alpha)      # [F, T+1, n]
            torch.cuda.synchronize()
            want = np.transpose(traj[:, idx, :], (1, 0, 2))      # (the oracle's trajectory holds T + 1 rows, row 0 = the channel values)
            ok = np.array_equal(rows.cpu().numpy(), want)
    if not ok:
        print("MISMATCH", cfg, "nf", nf, flush=True)
        sys.exit(1)
    rounds += 1; frames_total += B
    if rounds % 25 == 0:
        print(f"{rounds} rounds, {frames_total} frames exact", flush=True)
print(f"done: {rounds} rounds, {frames_total} frames, all exact")
