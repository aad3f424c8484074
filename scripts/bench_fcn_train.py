#!/usr/bin/env python3
"""Time per call of the sliding-window classifier's training kernels next to the same work written as torch ops on the same
device (unfold / sort / min for the windows; gather, matmul, softmax and autograd for the loss and gradient):

    python scripts/bench_fcn_train.py [--records 2000] [--blocks 30] [--win 5] [--batch 100] [--repeats 7] [--warmup 5]

Legs, each a HIP call and its torch counterpart, alternating (two passes), HIP events around back-to-back calls:
  windows     Decoder.fcn_windows on --records records of --blocks block minima   (ldpc_fcn_windows)
  step        Decoder.fcn_grad on --batch windows through an index                 (ldpc_fcn_grad, one training step's call)
  all         Decoder.fcn_grad over all (blocks - win + 1) * records windows, no gradient asked for (the validation pass)
and two host-clock figures that have no torch counterpart here:
  train_step  Predict_outlier_light.loss_and_grads + clip_by_norm + legacy Adam: one whole step, which ends on the host
  records     interval_boundary.query_teps_dis on one batch of --batch CCSDS frames over a 12-block decoding path: front
              end, scan of all blocks, comparison with the label's metric, compaction, the records to the host
Before timing, the torch windows and labels are checked against the kernel's bit for bit.  One JSON line per leg."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402
import torch         # noqa: E402

from short_ldpc_decoding_osd_amd import Code, globalmap as GL, interval_boundary, nn_net   # noqa: E402
from short_ldpc_decoding_osd_amd import ordered_statistics_decoding as osd_mod              # noqa: E402
from short_ldpc_decoding_osd_amd.nms_train import LegacyAdam, clip_by_norm                  # noqa: E402
from short_ldpc_decoding_osd_amd.runtime import default_decoder                             # noqa: E402

PATH = [[0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0], [1, 1, 0, 0, 0, 0], [0, 0, 0, 1, 0, 0],
        [0, 2, 0, 0, 0, 0], [0, 0, 0, 0, 1, 0], [0, 1, 1, 0, 0, 0], [0, 0, 0, 0, 0, 1], [0, 0, 2, 0, 0, 0], [1, 0, 1, 0, 0, 0]]


def torch_windows(bm, ok, win):
    R, nblk = bm.shape
    nwin = nblk - win + 1
    w = bm.unfold(1, win, 1)                                              # [R, nwin, win]
    pos = torch.arange(nwin, device=bm.device, dtype=torch.float32)[:, None, None].expand(nwin, R, 1)
    x = torch.cat([torch.sort(w, dim=2).values.permute(1, 0, 2), pos], dim=2).reshape(-1, win + 1)
    y = ((w.min(dim=2).values == bm.min(dim=1).values[:, None]) & ok[:, None]).t().reshape(-1).to(torch.uint8)
    return x.contiguous(), y.contiguous()


def torch_grad(x, y, sw, index, W1, W2, penalty, want_grad=True):
    if index is not None:
        x, y, sw = x[index.long()], y[index.long()], sw[index.long()]
    W1, W2 = W1.detach().requires_grad_(want_grad), W2.detach().requires_grad_(want_grad)
    p = torch.softmax(x @ W1 @ W2, dim=1)
    yl = y.long()
    py = p.gather(1, yl[:, None]).squeeze(1)
    pred = p[:, 0] < p[:, 1]
    pen = torch.where(pred & (yl == 0), penalty, 1.0).detach()
    loss = (-torch.log(torch.clamp(py, min=1e-30)) * pen * sw).sum()
    counts = torch.stack([(yl == pred).sum(), (yl > pred).sum(), (yl < pred).sum()])
    if not want_grad:
        return loss, counts
    return (loss, counts) + torch.autograd.grad(loss, (W1, W2))


def timed(fn, calls, repeats, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(repeats):
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / calls * 1e3)
    return out


def host_timed(fn, calls, repeats, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / calls * 1e6)
    return out


def stats(v):
    return dict(median_us=float(np.median(v)), min_us=float(min(v)), max_us=float(max(v)))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--blocks", type=int, default=30)
    ap.add_argument("--win", type=int, default=5)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args(argv)
    GL.dl_training_setting(["prog", "2.7", "2.7", str(a.batch), "12", "CCSDS_ldpc_n128_k64.alist", "NMS-1"])
    GL.set_map('sliding_win_width', a.win)
    dec = default_decoder(GL.get_map('code_parameters'))
    gen = torch.Generator(device=dec.device).manual_seed(1)
    R, nblk, win = a.records, a.blocks, a.win
    bm = (torch.rand((R, nblk), device=dec.device, generator=gen) * 20).contiguous()
    ok = torch.rand((R,), device=dec.device, generator=gen) < 0.9
    x, y, cc = dec.fcn_windows(bm, ok, win=win)
    tx, ty = torch_windows(bm, ok, win)
    assert torch.equal(x, tx) and torch.equal(y, ty), "torch windows differ from the kernel's"
    N = x.shape[0]
    ones = int(cc[1])
    sw = torch.where(y != 0, N / (2.0 * ones), N / (2.0 * (N - ones))).to(torch.float32)
    fcn = nn_net.Predict_outlier_light(win).initialize(0)
    W1, W2 = torch.from_numpy(fcn.dense1).to(dec.device), torch.from_numpy(fcn.dense2).to(dec.device)
    perm = torch.randperm(N, device=dec.device, generator=gen).to(torch.int32)
    index = perm[:a.batch].contiguous()
    common = dict(bench="fcn_train", records=R, blocks=nblk, win=win, windows=N, repeats=2 * a.repeats)
    legs = [
        ("windows", 50, lambda: dec.fcn_windows(bm, ok, win=win), lambda: torch_windows(bm, ok, win)),
        ("step", 200, lambda: dec.fcn_grad(x, y, fcn.packed(), win, 10.0, weight=sw, index=index, check_index=False),
         lambda: torch_grad(x, y, sw, index, W1, W2, 10.0)),
        ("all", 50, lambda: dec.fcn_grad(x, y, fcn.packed(), win, 10.0, weight=sw, want_grad=False),
         lambda: torch_grad(x, y, sw, None, W1, W2, 10.0, want_grad=False)),
    ]
    for name, calls, hip, tor in legs:
        us = dict(hip=[], torch=[])
        for _ in range(2):
            us["hip"] += timed(hip, calls, a.repeats, a.warmup)
            us["torch"] += timed(tor, calls, a.repeats, a.warmup)
        res = dict(common, leg=name, calls=calls, B=a.batch if name == "step" else N, hip=stats(us["hip"]), torch=stats(us["torch"]))
        res["torch_over_hip"] = res["torch"]["median_us"] / res["hip"]["median_us"]
        print(json.dumps(res), flush=True)

    # one whole training step, ending on the host
    opt = LegacyAdam(GL.optimizer_setting())
    batches = [perm[i * a.batch:(i + 1) * a.batch] for i in range(N // a.batch)]
    at = [0]

    def train_step():
        loss, grads, _, _ = fcn.loss_and_grads(x, y, sw, batches[at[0] % len(batches)], 10.0)
        opt.apply_gradients([(clip_by_norm(g, 5e2), attr, fcn.__dict__) for g, attr in zip(grads, fcn.TRAINABLE)])
        at[0] += 1
    print(json.dumps(dict(common, leg="train_step", calls=200, B=a.batch, host=stats(host_timed(train_step, 200, a.repeats, a.warmup)))),
          flush=True)

    # record generation of one batch of real frames
    GL.set_map('decoding_length', len(PATH))
    inst = osd_mod.osd(GL.get_map('code_parameters'))
    tep_info = osd_mod.generate_teps(inst, PATH)
    yb, lab = dec.gen_frames(a.batch, seed=7, snr_db=2.7)
    soft = dec.nms(yb, 12, np.float32(0.669435), want_hard=False, want_fail=False)["soft"]
    original, labels = yb.cpu().numpy(), dec.unpack_bits(lab).cpu().numpy()
    kept = interval_boundary.query_teps_dis(original, soft, labels, tep_info)[1]
    print(json.dumps(dict(common, leg="records", calls=20, B=a.batch, path_blocks=len(PATH), teps=int(tep_info[1][-1]),
                          kept=kept[0] + kept[1], undetected=kept[2],
                          host=stats(host_timed(lambda: interval_boundary.query_teps_dis(original, soft, labels, tep_info),
                                                20, a.repeats, 2)))), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
