#!/usr/bin/env python3
"""Timing of the DL-OSD stage on one GPU: NMS-T failures at 2.7 dB, collected until --frames frames, through
ldpc_dia_cnn (the bit-wise CNN), ldpc_hosd_front, ldpc_hosd_sliding (the block scan with the sliding-window early stop)
at soft_margin 0.9 and 1.0 (1.0 never stops) and ldpc_hosd_search (every block) on the same frames; then
nn_testing.Testing_OSD on both routes over a retest file of the same failures.

The networks are synthetic (no trained checkpoint ships with the project): a small random CNN and a classifier whose
logit difference grows with the window index and falls with the window's metrics, so the stop fires at a spread of depths.
The decoding path: 6-segment order patterns of total weight <= 3 with the reference's segments, by weight, the first 30
that the segments can hold.

With --pipeline-batch B: one channel batch of B frames through NMS + DL-OSD as the call sequence (with its host read of the
failure count), as the one call (ldpc_dlosd_pipeline_run) and as its captured replay.

    python scripts/bench_dlosd.py [--frames 32768] [--iters 12] [--reps 20] [--testing-frames 4096] [--kernels-only]
                                  [--pipeline-batch 131072 --capacity 4096 --repeats 5]
"""
import argparse
import itertools
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from short_ldpc_decoding_osd_amd import Code, globalmap as GL  # noqa: E402
from short_ldpc_decoding_osd_amd import data_generating, ordered_statistics_decoding as osd_mod  # noqa: E402
from short_ldpc_decoding_osd_amd.runtime import Decoder  # noqa: E402
from short_ldpc_decoding_osd_amd.weights import STORED_NMS1_WEIGHT, softplus32  # noqa: E402

HBM_PEAK = 8.0e12     # MI355X HBM3E, bytes/s


def collect_failures(dec, code, T, want, snr, seed):
    alpha = float(softplus32(STORED_NMS1_WEIGHT))
    rng = np.random.default_rng(seed)
    rows, labels, seen = [], [], 0
    while sum(len(r) for r in rows) < want:
        y, cw = data_generating.testing_data_generating(code, snr, 131072, rng=rng)
        yd = torch.from_numpy(y.astype(np.float32)).to(dec.device)
        res = dec.nms(yd, T, alpha, want_soft=False)
        idx, cnt = dec.compact(res["fail"])
        nf = int(cnt.cpu()[0])
        r = dec.nms_traj_rows(yd, idx, cnt, nf, T, alpha)
        rows.append(r[:nf].cpu().numpy())
        labels.append(cw[idx[:nf].cpu().numpy()])
        seen += len(y)
    return np.concatenate(rows)[:want], np.concatenate(labels)[:want], seen


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def path30(inst):
    _, bnd = osd_mod.secure_segment_threshold()
    size = np.diff(bnd)
    pats = sorted((p for p in itertools.product(range(4), repeat=6) if sum(p) <= 3 and all(p[i] <= size[i] for i in range(6))),
                  key=lambda p: (sum(p), p))
    return [list(p) for p in pats[:30]]


def pipeline_legs(dec, code, T, teps, off, win, fw, packed, snr, B, cap, reps, repeats):
    """One channel batch of B frames through NMS + DL-OSD three ways: the call sequence (the host reads the failure count),
    ldpc_dlosd_pipeline_run (pipeline.DlOsdPipeline, one call) and its captured replay.  Wall-clock per batch, synchronised
    after every batch; ``repeats`` measurements of ``reps`` batches each -> their minimum, median and maximum in ms."""
    from short_ldpc_decoding_osd_amd.pipeline import DlOsdPipeline
    alpha = float(softplus32(STORED_NMS1_WEIGHT))
    y, cw = data_generating.testing_data_generating(code, snr, B, rng=np.random.default_rng(5))
    yd = torch.from_numpy(y.astype(np.float32)).to(dec.device)
    lab = dec.pack_bits(torch.from_numpy(cw.astype(np.uint8)).to(dec.device))
    pipe = DlOsdPipeline(dec, B, T, alpha, teps, off, win, 0.9, fw, packed, capacity=cap).bind(yd, lab)
    nms_out = dict(soft=dec.empty((B, dec.n), torch.float32), hard=dec.empty((B, dec.words), torch.int64), fail=dec.empty((B,), torch.uint8))
    index, count = dec.empty((B,), torch.int32), dec.empty((1,), torch.int32)
    rows, xo = dec.empty((cap, T + 1, dec.n), torch.float32), dec.empty((cap, dec.n), torch.float32)
    nms_counts, final = torch.zeros(5, dtype=torch.int64, device=dec.device), torch.zeros(4, dtype=torch.int64, device=dec.device)

    def sequence():
        res = dec.nms(yd, T, alpha, out=nms_out)
        dec.eval_counts(res["hard"], lab, res["fail"], counts=nms_counts)
        dec.compact(res["fail"], index=index, count=count)
        nf = min(int(count.item()), cap)                     # the host round trip the one call does without
        if nf == 0:
            return 0
        dec.nms_traj_rows(yd, index, count, nf, T, alpha, out=rows)
        dec.dia_cnn(rows[:nf], packed, out=xo[:nf])
        sel = index[:nf].long()
        ym, labs = yd[sel], lab[sel]
        r = dec.hosd_sliding(xo[:nf], ym, dec.hosd_front(xo[:nf]), teps, off, win, 0.9, fw, label_bits=labs)
        dec.osd_merge(r["cw"], index, count, hard=res["hard"], label_bits=lab, counts=final, F=nf)
        return nf

    def measure(fn):
        fn()
        torch.cuda.synchronize()
        got = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
                torch.cuda.synchronize()
            got.append((time.perf_counter() - t0) / reps * 1e3)
        return dict(min=round(min(got), 4), median=round(float(np.median(got)), 4), max=round(max(got), 4))

    res = dict(B=B, capacity=cap, reps=reps, repeats=repeats, failures=sequence())
    res["sequence_ms"] = measure(sequence)
    res["one_call_ms"] = measure(pipe.run)
    side, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        pipe.run()
    res["replay_ms"] = measure(g.replay)
    pipe.reset_counters()
    pipe.run(timing_slot=0)
    torch.cuda.synchronize()
    res["one_call_stage_ms"] = [round(v, 4) for v in pipe.timing(0)]
    res["counters"] = pipe.counters().cpu().tolist()
    assert torch.equal(pipe.hard, nms_out["hard"]) and res["counters"][5] == res["failures"]     # the two routes agree
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32768)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--snr", type=float, default=2.7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--testing-frames", type=int, default=4096)
    ap.add_argument("--kernels-only", action="store_true", help="skip the Testing_OSD passes (profiling runs)")
    ap.add_argument("--pipeline-batch", type=int, default=0,
                    help="frames of one channel batch for the sequence / one call / captured replay legs (0: skip them)")
    ap.add_argument("--capacity", type=int, default=4096, help="rows of the pipeline's list buffers")
    ap.add_argument("--repeats", type=int, default=5, help="measurements per pipeline leg, --reps batches each")
    a = ap.parse_args()
    from tests import dlosd_model as DM
    code = Code()
    dec = Decoder(code)
    T, L, win = a.iters, a.iters + 1, 5
    for k, v in dict(code_parameters=code, num_iterations=T, segment_num=6, threshold_sum=3, decoding_length=30,
                     sliding_win_width=win, soft_margin=0.9, termination_threshold=10 ** 9, convention_path=False,
                     selected_decoder_type='NMS-1', training_snr=2.7).items():
        GL.set_map(k, v)
    inst = osd_mod.osd(code)
    path = path30(inst)
    blocks, acc = osd_mod.generate_teps(inst, path)
    teps, off = inst._device_blocks(dec, blocks)
    t0 = time.time()
    rows, labels, seen = collect_failures(dec, code, T, a.frames, a.snr, 11)
    F = len(rows)
    cnn_w = DM.random_cnn_weights(np.random.default_rng(3), L, scale=0.3)
    w1, w2 = DM.stopping_fcn_weights(win)
    fw = np.concatenate([w1.ravel(), w2.ravel()])
    rd = torch.from_numpy(rows).to(dec.device)
    yd = rd[:, 0].contiguous()
    lab = dec.pack_bits(torch.from_numpy(labels.astype(np.uint8)).to(dec.device))
    packed = DM.pack_cnn(cnn_w)
    xo = dec.dia_cnn(rd, packed)
    front = dec.hosd_front(xo)
    out = {}
    out["frames"], out["nms_frames_decoded"], out["collect_s"] = F, seen, round(time.time() - t0, 2)
    out["path_blocks"], out["path_teps"] = len(path), int(acc[-1])
    ms = timed(lambda: dec.dia_cnn(rd, packed, out=xo), a.reps)
    moved = F * (L * 128 * 4 + 128 * 4)
    out["dia_cnn_ms"] = round(ms, 4)
    out["dia_cnn_hbm_fraction"] = round(moved / (ms * 1e-3) / HBM_PEAK, 3)
    out["hosd_front_ms"] = round(timed(lambda: dec.hosd_front(xo), a.reps), 4)
    out["hosd_search_ms"] = round(timed(lambda: dec.hosd_search(xo, yd, front, teps, off, label_bits=lab, want_arg=False), a.reps), 4)
    for margin in (0.9, 1.0):
        r = dec.hosd_sliding(xo, yd, front, teps, off, win, margin, fw, label_bits=lab)
        deep = r["deep_limit"].cpu().numpy()
        tag = f"sliding_{margin}"
        out[tag + "_ms"] = round(timed(lambda: dec.hosd_sliding(xo, yd, front, teps, off, win, margin, fw, label_bits=lab), a.reps), 4)
        out[tag + "_mean_teps_evaluated"] = round(float(r["teps"].cpu().numpy().mean()), 2)
        out[tag + "_mean_reference_complexity"] = round(float(acc[deep].mean()), 2)
        out[tag + "_mean_windows"] = round(float((deep - win + 1).mean()), 3)
        out[tag + "_depths"] = {int(d): int(c) for d, c in zip(*np.unique(deep, return_counts=True))}
        out[tag + "_FER"] = round(1.0 - float(r["success"].float().mean().item()), 5)
    print(json.dumps(dict(kernels=out)), flush=True)
    if a.pipeline_batch > 0:
        print(json.dumps(dict(pipeline=pipeline_legs(dec, code, T, teps, off, win, fw, packed, a.snr, a.pipeline_batch, a.capacity,
                                                     a.reps, a.repeats))), flush=True)
    if a.kernels_only:
        return
    # ---- Testing_OSD on both routes over a retest file of the first --testing-frames failures
    from short_ldpc_decoding_osd_amd import nn_testing, read_TFdata, tf_checkpoint, tfrecord
    n = min(a.testing_frames, F)
    with tempfile.TemporaryDirectory() as d:
        path_file = os.path.join(d, "ldpc-nonzero-retest.tfrecord")
        lab_rows = np.repeat(labels[:n], L, axis=0)
        tfrecord.write_examples(path_file, rows[:n].reshape(-1, 128), lab_rows)
        names = ("cnv_one/kernel", "cnv_two/kernel", "cnv_three/kernel", "dense/kernel", "dense/bias")
        tf_checkpoint.write_checkpoint(os.path.join(d, "cnn", "ldpc-ckpt-1"),
                                       {f"myAwesomeModel/{k}/.ATTRIBUTES/VARIABLE_VALUE": v for k, v in zip(names, cnn_w)})
        tf_checkpoint.write_checkpoint(os.path.join(d, "fcn", "ldpc-ckpt-1"), {
            "myAwesomeModel/dense1/kernel/.ATTRIBUTES/VARIABLE_VALUE": w1,
            "myAwesomeModel/dense2/kernel/.ATTRIBUTES/VARIABLE_VALUE": w2})
        # the path through a pickle: the frequency order of `path` (distinct counts, descending)
        import pickle
        os.makedirs(os.path.join(d, "log", "NMS-1", "2.7-2.7dB"))
        with open(os.path.join(d, "log", "NMS-1", "2.7-2.7dB", "dist-error-pattern-model_cnn.pkl"), "wb") as fh:
            for obj in (0, 0, 0, 0, 0, {str(p): len(path) - i for i, p in enumerate(path)}):
                pickle.dump(obj, fh)
        GL.set_map('dl_training_dir', d + "/")
        restore = [[os.path.join(d, "cnn") + "/", "ldpc-ckpt", "latest"], [os.path.join(d, "fcn") + "/", "ldpc-ckpt", "latest"]]
        cwd = os.getcwd()
        os.chdir(d)
        try:
            res = {}
            for route in ("device", "host"):
                ds = read_TFdata.data_handler(128, path_file, 1024 * L)
                t1 = time.perf_counter()
                fer, log = nn_testing.Testing_OSD(a.snr, ds, restore, [True, False, False],
                                                  ['model_cnn', 'model_rnn1', 'model_rnn2'], True, route=route)
                torch.cuda.synchronize()
                el = time.perf_counter() - t1
                res[route] = dict(FER=fer, seconds=round(el, 3), frames_per_s=round(n / el, 1))
            res["frames"] = n
            res["log_tail"] = open(os.path.join(d, "log", "OSD-3-model_cnn.txt")).read().splitlines()[-6:-3]
        finally:
            os.chdir(cwd)
    print(json.dumps(dict(testing_osd=res)), flush=True)


if __name__ == "__main__":
    main()
