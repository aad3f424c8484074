#!/usr/bin/env python3
"""The one-call pipeline of the OSD families next to the calls it replaces, per batch, conventional order 2:

    (a) four calls with the host reading the failure count in between (scripts/osdx_fer.py's route): ldpc_nms_decode,
        ldpc_eval_counts, ldpc_compact, <count to the host>, ldpc_osd?_decode on that many frames
    (b) the same four calls without the host read (the decode call takes F = B and reads the count on the device); timed
        twice per pass, so that its own run-to-run spread stands next to every difference
    (c) pipeline.FamilyPipeline.run(): ldpc_family_pipeline_run, merge included
    (d) (c) replayed from a captured graph

    python scripts/bench_family_pipeline.py [--frames 32768] [--out profiles/family_pipeline/bench_family_pipeline.jsonl]

The routes alternate in one process; every figure is HIP events around --calls back-to-back batches, --repeats times, after a
warm-up.  The SNR of a code is the first of 0.5, 0.75, ... dB at which NMS-T leaves 5-25 % of the batch with a non-zero syndrome
(--snr fixes it).  Also timed alone, on the failures of the same batch: ldpc_osd_merge with counters, and ldpc_osd_counts where
it serves the code (two words per frame).  One JSON line per code."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402
import torch         # noqa: E402

from short_ldpc_decoding_osd_amd import Code   # noqa: E402
from short_ldpc_decoding_osd_amd.pipeline import FamilyPipeline   # noqa: E402
from short_ldpc_decoding_osd_amd.runtime import Decoder   # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CODES = {"ldpc_96_48": "LDPC_N96_K48_P8_set0_dmin10.alist", "array_121_80": "ArrayCode_N121_K80_r0.66.alist",
         "wl384": "wimaxlike_N384_K192_P16_set0.alist"}


def timed(fn, calls, repeats, warmup):
    """us per call of fn(): HIP events around `calls` back-to-back calls, `repeats` times after `warmup` calls."""
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


def pick_snr(dec, B, T, alpha, fixed):
    for snr in ([fixed] if fixed is not None else np.arange(0.5, 8.01, 0.25)):
        y, labels = dec.gen_frames(B, seed=7, snr_db=float(snr))
        nf = int(dec.nms(y, T, alpha, want_soft=False)["fail"].sum().item())
        if fixed is not None or 0.05 * B <= nf <= 0.25 * B:
            return float(snr), y, labels, nf
    raise SystemExit(f"no SNR up to 8 dB leaves 5-25 % failures on ({dec.n},{dec.k})")


def bench_code(name, args):
    dec = Decoder(Code(os.path.join(GOLDEN, CODES[name])), 0)
    B, T, alpha, order = args.frames, args.T, args.alpha, 2
    snr, y, labels, nf = pick_snr(dec, B, T, alpha, args.snr)
    fam = dec.osd_family()
    decode = getattr(dec, fam + "_decode")
    pdt, ptail, qtail, _ = dec._osd_layout(fam)
    e = dec.empty
    nms_out = dict(soft=None, traj=None, hard=e((B, dec.words), torch.int64), fail=e((B,), torch.uint8))
    index, count = e((B,), torch.int32), e((1,), torch.int32)
    perm, parity = e((B,) + ptail, pdt), e((B,) + qtail, torch.int64)
    out = dict(cw=e((B, dec.words), torch.int64), metric=e((B,), torch.float32), best=e((B,), torch.int32), ntep=e((B,), torch.int32))
    nms_counts = torch.zeros(5, dtype=torch.int64, device=dec.device)
    osd_counts = torch.zeros(3, dtype=torch.int64, device=dec.device)

    def four_calls(host_read):
        dec.nms(y, T, alpha, want_soft=False, out=nms_out)
        dec.eval_counts(nms_out["hard"], labels, nms_out["fail"], counts=nms_counts)
        dec.compact(nms_out["fail"], index=index, count=count)
        F = int(count.cpu()[0]) if host_read else B
        if F:
            decode(y, order, index=index, count=count, F=F, perm=perm, parity=parity, label_bits=labels, counts=osd_counts, out=out)

    pipe = FamilyPipeline(dec, B, T, alpha, osd_order=order, snr_db=snr, want_soft=False).bind(y, labels)
    pipe.run()
    four_calls(False)
    torch.cuda.synchronize()
    for key in ("cw", "metric", "best", "ntep"):          # the routes compute the same thing
        a, b = getattr(pipe, key)[:nf], out[key][:nf]
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), key
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        pipe.run()
    merge_counts = torch.zeros(4, dtype=torch.int64, device=dec.device)
    hard = nms_out["hard"].clone()
    legs = [("a_four_calls_host_read", lambda: four_calls(True)), ("b_four_calls", lambda: four_calls(False)),
            ("c_family_pipeline", pipe.run), ("b_four_calls_again", lambda: four_calls(False)), ("d_graph_replay", graph.replay),
            ("osd_merge_alone", lambda: dec.osd_merge(out["cw"], index, count, hard=hard, label_bits=labels, counts=merge_counts, F=B))]
    if dec.words == 2:
        legs.append(("osd_counts_alone", lambda: dec.osd_counts(out["cw"], labels, index=index, count=count, ntep=out["ntep"], counts=osd_counts, F=B)))
    result = dict(code=name, n=dec.n, k=dec.k, family=fam, snr_db=snr, frames=B, failures=nf, T=T, order=order, us_per_batch={})
    for _ in range(args.passes):                           # the legs alternate
        for leg, fn in legs:
            us = timed(fn, args.calls, args.repeats, args.warmup)
            result["us_per_batch"].setdefault(leg, []).append(dict(median=float(np.median(us)), min=min(us), max=max(us)))
            print(f"  {name:13s} {leg:24s} {np.median(us):9.1f} us per batch (min {min(us):.1f}, max {max(us):.1f})", flush=True)
    return result


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--codes", nargs="+", default=list(CODES), choices=list(CODES))
    ap.add_argument("--frames", type=int, default=32768)
    ap.add_argument("--T", type=int, default=10)
    ap.add_argument("--alpha", type=float, default=0.669435)
    ap.add_argument("--snr", type=float, default=None)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args(argv)
    for name in args.codes:
        line = json.dumps(bench_code(name, args))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
