#!/usr/bin/env python3
"""Time per call of the device-side frame generator (Decoder.gen_frames: one launch, ldpc_gen_frames) next to the torch path
of the sweep scripts (scripts/snr_sweep.py::frames_on_device: randint -> float -> GEMM -> remainder -> randn -> multiply ->
pack_bits) on the same shapes.

    python scripts/bench_gen.py [--calls 20] [--repeats 7] [--warmup 5] [--snr 2.5]

HIP events around --calls back-to-back calls, --repeats times after --warmup calls; the two paths alternate (two passes), so
that a drift of the clocks meets both.  Printed per case: the median and the spread (min, max) over all repeats of both passes
in us per call, samples per second, and for the kernel the share of the time its 4 n + 8 ceil(n/64) bytes per frame of stores
would need at --hbm-gbs (HBM write rate assumed for that floor; a figure for orientation, the kernel is issue-bound).
Cases: CCSDS (128,64) at B = 131 072 and 1 000, the (121,80) array code, the wimax (1056,880) code at B = 16 384.
One JSON line per case.  --torch-only runs on a tree without the generator (the parent commit's yardstick)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402
import torch         # noqa: E402

from short_ldpc_decoding_osd_amd import Code              # noqa: E402
from short_ldpc_decoding_osd_amd.runtime import Decoder   # noqa: E402

CASES = [("ccsds_128_64", None, 131072), ("ccsds_128_64", None, 1000),
         ("array_121_80", "tests/golden/ArrayCode_N121_K80_r0.66.alist", 131072),
         ("wimax_1056_880", "tests/golden/wimax_1056_0.83.alist", 16384)]


def frames_on_device(dec, G, B, snr_db, gen):
    """The torch path of scripts/snr_sweep.py (G resident, as a sweep would keep it)."""
    sigma = float(np.sqrt(1.0 / (2.0 * (dec.k / dec.n) * 10.0 ** (snr_db / 10.0))))
    cw = (torch.randint(0, 2, (B, dec.k), device=dec.device, generator=gen).to(torch.float32) @ G).remainder_(2)
    y = ((1 - 2 * cw) * (1 + sigma * torch.randn((B, dec.n), device=dec.device, generator=gen))).contiguous()
    return y, dec.pack_bits(cw.to(torch.uint8))


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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--snr", type=float, default=2.5)
    ap.add_argument("--hbm-gbs", type=float, default=5000.0, help="HBM write rate assumed for the store floor, GB/s")
    ap.add_argument("--torch-only", action="store_true", help="time the torch path alone (a tree without gen_frames)")
    args = ap.parse_args(argv)
    for name, alist, B in CASES:
        dec = Decoder(Code(os.path.join(ROOT, alist)) if alist else Code(), 0)
        G = torch.from_numpy(np.asarray(dec.code.G)).to(device=dec.device, dtype=torch.float32)
        gen = torch.Generator(device=dec.device).manual_seed(1)
        legs = [("torch", lambda: frames_on_device(dec, G, B, args.snr, gen))]
        if not args.torch_only:
            out = dict(y=dec.empty((B, dec.n), torch.float32), label_bits=dec.empty((B, dec.words), torch.int64))
            frame0 = [0]

            def hip():
                dec.gen_frames(B, seed=20241020, snr_db=args.snr, frame0=frame0[0], out=out)
                frame0[0] += B
            legs.append(("hip", hip))
        us = {k: [] for k, _ in legs}
        for _ in range(2):
            for k, fn in legs:
                us[k] += timed(fn, args.calls, args.repeats, args.warmup)
        res = dict(bench="gen", code=name, n=dec.n, k=dec.k, B=B, snr_db=args.snr, calls=args.calls, repeats=2 * args.repeats)
        for k, v in us.items():
            med = float(np.median(v))
            res[k] = dict(median_us=med, min_us=min(v), max_us=max(v), samples_per_s=B * dec.n / med * 1e6)
        if "hip" in us:
            floor_us = B * (4 * dec.n + 8 * dec.words) / (args.hbm_gbs * 1e9) * 1e6
            res["hip"]["store_floor_us"] = floor_us
            res["hip"]["store_floor_share"] = floor_us / res["hip"]["median_us"]
            res["torch_over_hip"] = res["torch"]["median_us"] / res["hip"]["median_us"]
        print(json.dumps(res), flush=True)
        del dec
    return 0


if __name__ == "__main__":
    sys.exit(main())
