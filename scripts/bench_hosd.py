#!/usr/bin/env python3
"""Timing of the H-form OSD primitives (DL-OSD stage) on one GPU:
front end, block scan and the scan with the sliding-window stop over a decoding path of 6-segment order patterns.  Every
family that serves the code is timed on the same frames: the specialised kernels (ldpc_hosd_*) on (128,64), the any-shape
ones (ldpc_hosdx_*) where k, n-k <= 64 and H has n-k rows, the wide ones (ldpc_hosdw_*: k up to 127, redundant rows) and the
long ones (ldpc_hosdl_*: n up to 384, k and n-k up to 192).  The families alternate: every call is timed in two passes over
the families, and the figure is the mean of the two.

    python scripts/bench_hosd.py [--alist FILE] [--frames 32768] [--max-weight 2] [--snr 2.5] [--win 5]
"""
import argparse
import itertools
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from short_ldpc_decoding_osd_amd import Code, globalmap as GL  # noqa: E402
from short_ldpc_decoding_osd_amd import data_generating, ordered_statistics_decoding as osd_mod  # noqa: E402
from short_ldpc_decoding_osd_amd.runtime import Decoder  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32768)
    ap.add_argument("--max-weight", type=int, default=2)
    ap.add_argument("--snr", type=float, default=2.5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--alist", default=None, help="code definition (default: the CCSDS (128,64) code)")
    ap.add_argument("--win", type=int, default=5, help="window of the sliding call")
    a = ap.parse_args()
    code = Code(a.alist) if a.alist else Code()
    dec = Decoder(code)
    GL.set_map('code_parameters', code)
    GL.set_map('segment_num', 6)
    inst = osd_mod.osd(code)
    path = sorted((p for p in itertools.product(range(a.max_weight + 1), repeat=6) if sum(p) <= a.max_weight),
                  key=lambda p: (sum(p), p))
    blocks, acc = osd_mod.generate_teps(inst, [list(p) for p in path])
    teps, off = inst._device_blocks(dec, blocks)
    y, cw = data_generating.testing_data_generating(code, a.snr, a.frames, rng=np.random.default_rng(1))
    yd = torch.from_numpy(y.astype(np.float32)).to(dec.device)
    lab = dec.pack_bits(torch.from_numpy(cw.astype(np.uint8)).to(dec.device))

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            r = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps, r

    # the classifier of the sliding call: z1 - z0 = 0.35 k - 0.01 sum(window), stop at p1 > 0.9
    d = a.win + 1
    w2 = np.zeros((d, 2), np.float32)
    w2[:a.win, 1], w2[a.win, 1] = -0.01, 0.35
    fw = np.concatenate([np.eye(d, dtype=np.float32).ravel(), w2.ravel()])
    res = {"code": [dec.n, dec.k], "frames": a.frames, "blocks": len(blocks), "teps_per_frame": int(acc[-1])}
    fams = (["hosd"] if dec._hosd_fam() == "hosd" else []) + (["hosdx"] if dec.hosdx_supported else []) \
        + (["hosdw"] if dec.hosdw_supported else []) + (["hosdl"] if dec.hosdl_supported else [])
    if not fams:
        raise SystemExit(f"bench_hosd: the H-form kernels do not serve this ({dec.n},{dec.k}) code")
    times = {fam: np.zeros(3) for fam in fams}
    passes = 2
    for _ in range(passes):
        for fam in fams:
            t_front, front = timed(lambda: dec._hosd_front(fam, yd))
            t_search, out = timed(lambda: dec._hosd_search(fam, yd, yd, front, teps, off, lab, True, True))
            t_slide, sl = timed(lambda: dec._hosd_sliding(fam, yd, yd, front, teps, off, a.win, 0.9, fw, lab, 0, True))
            times[fam] += np.array([t_front, t_search, t_slide]) / passes
            hit = (out["metric"] == out["truth"]).float().mean().item()
            res.update({f"{fam}_ml_hit_rate": round(hit, 5),
                        f"{fam}_sliding_mean_depth": round(sl["deep_limit"].float().mean().item(), 3)})
    for fam in fams:
        t_front, t_search, t_slide = times[fam]
        res.update({f"{fam}_front_ms": round(t_front, 4), f"{fam}_search_ms": round(t_search, 4),
                    f"{fam}_sliding_ms": round(t_slide, 4),
                    f"{fam}_frames_per_s": round(a.frames / ((t_front + t_search) * 1e-3), 1),
                    f"{fam}_teps_per_s": round(a.frames * int(acc[-1]) / (t_search * 1e-3), 1)})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
