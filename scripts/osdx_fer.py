"""NMS + order-p OSD (conventional, FS-OSD or PB-OSD) of any short code (1 <= k <= 64, 1 <= n-k <= 64): FER before and after the
OSD, and the two OSD kernels timed.  A high-rate code (k > 64, n <= 128, n-k <= 64) runs the same three searches through the
ldpc_osdw_* family.

    python scripts/osdx_fer.py --alist tests/golden/LDPC_N96_K48_P8_set0_dmin10.alist --snr 2.5 --frames 131072 --T 10 --order 2
    python scripts/osdx_fer.py --alist tests/golden/LDPC_N96_K48_P8_set0_dmin10.alist --snr 2.5 --frames 131072 --T 10 --order 2 \
        --osd fs --tau-e 4.5
    python scripts/osdx_fer.py --alist tests/golden/LDPC_N96_K48_P8_set0_dmin10.alist --snr 2.5 --frames 131072 --T 10 --order 3 \
        --osd pb

Frame generator -> ldpc_nms_decode -> ldpc_compact -> ldpc_osdx_decode on the failures (the reference's loop: NMS, then
convention_osd_main on the frames with a non-zero syndrome).  Times are HIP events around --calls back-to-back launches on the
failures of the whole batch, after a warm-up, --repeats times (every repeat is printed: their spread is the noise).  On a
(128,64) code the specialised osd_front_kernel and the table-scan osd_search_kernel are timed on the same frames in the same run.
--osd fs: the search is FS-OSD (ldpc_osdx_fs_decode; fs_osd, FS_OSD/fs_testing.py:129-161) with --beta, --tau-e (floor((d_min - 1) / 2)
as the reference evaluates it: required for an alist, whose d_min the script cannot know; 6.5 for the packaged CCSDS code) and
--tau-psc.  Printed then: mean and maximum TEPs per frame next to the size of the order-p table, osdx_fs_kernel timed like the other
legs and, on a (128,64) code, osd_fs_kernel through ldpc_osd_search on the same frames.
--osd pb: the search is PB-OSD (ldpc_osdx_pb_decode; pb_osd, PB_OSD/pb_testing.py:100-149), --snr doubling as the decoder's snr_db.
Printed then: mean and maximum TEPs per frame next to N_max, the shares of the three stop reasons (0 = no rule fired, 1 = the
promising rule, 2 = the success rule), osdx_pb_kernel timed like the other legs and, on a (128,64) code, ldpc_osd_search on the
same frames through the literal replay route (LDPC_OSD_F_PB_REPLAY: the same algorithm) and through the default staged route.
A code that ldpc_osdx_* refuses and ldpc_osdw_* serves (k > 64, e.g. tests/golden/ArrayCode_N121_K80_r0.66.alist) runs the
conventional search through ldpc_osdw_decode, osdw_front_kernel and osdw_search_kernel timed like the other legs.  --osd fs runs
ldpc_osdw_fs_decode there: the same line of TEPs per frame, the FER of the conventional scan of the same order on the same frames
next to it, and osdw_fs_kernel timed next to osdw_search_kernel.  --osd pb runs ldpc_osdw_pb_decode there: the same line of TEPs
per frame and stop shares, osdw_pb_kernel timed next to osdw_search_kernel of the same order and, with --tau-e, osdw_fs_kernel
on the same frames.  On a code both families serve, the conventional run also times the osdw kernels on the same frames in the
same run, alternating with the osdx kernels, the --osd fs run times osdw_fs_kernel alternating with osdx_fs_kernel and the
--osd pb run osdw_pb_kernel alternating with osdx_pb_kernel.
A code that neither older family serves and ldpc_osdl_* does (n <= 384, k <= 192, n-k <= 192, e.g.
tests/golden/wimaxlike_N384_K192_P16_set0.alist, or any code with n <= 128 and n-k > 64) runs the conventional search through
ldpc_osdl_decode, osdl_front_kernel and osdl_search_kernel timed like the other legs.  --osd fs runs ldpc_osdl_fs_decode there:
the line of TEPs per frame, the FER of the conventional scan of the same order on the same frames next to it, and osdl_fs_kernel
timed next to osdl_search_kernel.  --osd pb runs ldpc_osdl_pb_decode there: the line of TEPs per frame next to N_max and the
stop shares, osdl_pb_kernel timed next to osdl_search_kernel of the same order and, with --tau-e, osdl_fs_kernel on the same
frames.  On a code that ldpc_osdw_* serves as well the conventional run also times the osdl kernels on the same frames,
alternating; on a code an older family serves the --osd fs run asserts that ldpc_osdl_fs_decode gives the same outputs and
times osdl_fs_kernel alternating with the older family's FS kernel, and the --osd pb run does the same with
ldpc_osdl_pb_decode and osdl_pb_kernel.
The conventional run also times the one-TEP kernel (osdx_ / osdw_ / osdl_tep_eval_kernel) of every family it runs, on the same
front-end results: every frame evaluates the TEP that flips MRB positions 0 and k - 1.
--oracle N times the C oracle's front end (oracle/c_oracle.osd_front, one core) on the first N failures and prints its frames/s.
--gen hip draws the frames with the library's counter-based generator (Decoder.gen_frames: frames 0 .. --frames - 1 of the set
--seed, one launch) instead of the torch ops; the JSON line says which.
--pipeline makes the same run through ONE call as well (pipeline.FamilyPipeline, ldpc_family_pipeline_run: NMS, counters,
compaction, the family's OSD and ldpc_osd_merge) and asserts that its outputs and counters equal those of the four calls above;
it prints the bit error rate before and after the OSD codewords are merged into the NMS decisions.
One JSON line at the end."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402
import torch         # noqa: E402

from short_ldpc_decoding_osd_amd import Code, _lib              # noqa: E402
from short_ldpc_decoding_osd_amd.runtime import Decoder, _ptr   # noqa: E402


def make_frames(dec, B, seed, snr_db):
    """Synthetic frames on the device (data_generating.py:13-51): y = (1 - 2c)(1 + sigma N(0,1)), packed labels."""
    g = torch.Generator(device=dec.device).manual_seed(seed)
    G = torch.from_numpy(np.asarray(dec.code.G)).to(device=dec.device, dtype=torch.float32)
    sigma = float(np.sqrt(1.0 / (2.0 * (dec.k / dec.n) * 10.0 ** (snr_db / 10.0))))
    y = torch.empty((B, dec.n), dtype=torch.float32, device=dec.device)
    labels = torch.empty((B, dec.words), dtype=torch.int64, device=dec.device)
    for s in range(0, B, 1 << 16):
        e = min(B, s + (1 << 16))
        msg = torch.randint(0, 2, (e - s, dec.k), device=dec.device, generator=g).to(torch.float32)
        cw = (msg @ G).remainder_(2)
        y[s:e] = (1 - 2 * cw) * (1 + sigma * torch.randn((e - s, dec.n), device=dec.device, generator=g))
        labels[s:e] = dec.pack_bits(cw.to(torch.uint8))
    return y, labels


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


def pipeline_check(dec, args, y, labels, res, nms_counts, index, nf, out, osd_counts, aux):
    """--pipeline: NMS, counters, compaction, OSD and the merge through ldpc_family_pipeline_run, against the four calls of
    this script: every output of the listed frames and the counters, exactly; then the merged decisions and the bit error
    rates the merge's counters give."""
    from short_ldpc_decoding_osd_amd.pipeline import FamilyPipeline
    from short_ldpc_decoding_osd_amd.sharding import combine_fer
    kw = dict(fs_beta=args.beta, fs_tau_e=args.tau_e, fs_tau_psc=args.tau_psc) if args.osd == "fs" else {}
    pipe = FamilyPipeline(dec, y.shape[0], args.T, args.alpha, osd_order=args.order, snr_db=args.snr,
                          osd_algo={"conv": _lib.OSD_CONVENTIONAL, "fs": _lib.OSD_FS, "pb": _lib.OSD_PB}[args.osd], **kw).bind(y, labels)
    pipe.run()
    torch.cuda.synchronize()

    def same(a, b):
        return torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    assert int(pipe.count.item()) == nf and same(pipe.index[:nf], index[:nf]), "failure list"
    assert same(pipe.soft, res["soft"]) and same(pipe.fail, res["fail"]), "NMS outputs"
    for key in ("perm", "parity", "cw", "metric", "best", "ntep"):
        assert same(getattr(pipe, key)[:nf], out[key][:nf]), key
    assert aux is None or same(pipe.aux[:nf], aux[:nf]), "aux"
    c = pipe.counters().cpu().tolist()
    assert c[:5] == nms_counts.cpu().tolist() and c[5:8] == osd_counts.cpu().tolist(), "counters"
    merged = res["hard"].clone()
    merged[index[:nf].long()] = out["cw"][:nf]
    assert same(pipe.hard, merged), "merged decisions"
    assert c[8] == nf and c[9] == c[6]
    rates = combine_fer(c, n=dec.n)
    print(f"  --pipeline: one call (family {pipe.family}) gives the outputs and counters of the four calls; "
          f"BER {rates['ber_nms']:.3e} after NMS, {rates['ber_end_to_end']:.3e} after the merge", flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--alist", default=None, help="alist file of the code (default: the packaged CCSDS (128,64) code)")
    ap.add_argument("--snr", type=float, default=2.5)
    ap.add_argument("--frames", type=int, default=131072)
    ap.add_argument("--T", type=int, default=10)
    ap.add_argument("--alpha", type=float, default=0.669435, help="effective check normaliser of NMS-1")
    ap.add_argument("--order", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--gen", choices=("torch", "hip"), default="torch", help="frame source: torch ops, or the library's generator")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--osd", choices=("conv", "fs", "pb"), default="conv",
                    help="the search: the conventional table scan, FS-OSD, or PB-OSD")
    ap.add_argument("--beta", type=float, default=0.1, help="FS-OSD: beta of the lower bound (Main_FS_OSD.py:20)")
    ap.add_argument("--tau-e", type=float, default=None, help="FS-OSD: the stop threshold on the Hamming distance")
    ap.add_argument("--tau-psc", type=float, default=30.0, help="FS-OSD: tau_psc (FS_OSD/globalmap.py:50)")
    ap.add_argument("--oracle", type=int, default=0, help="time the C oracle's front end on this many of the failures (one core)")
    ap.add_argument("--pipeline", action="store_true",
                    help="the same run through ONE call as well (pipeline.FamilyPipeline); its outputs must equal those of the four calls")
    args = ap.parse_args(argv)
    fs, pb = args.osd == "fs", args.osd == "pb"
    if fs and args.tau_e is None:
        if args.alist:
            ap.error("--osd fs needs --tau-e for an alist code (there is no default d_min)")
        args.tau_e = 6.5

    dec = Decoder(Code(args.alist) if args.alist else Code(), 0)
    wide = dec.osdw_supported and not dec.osdx_supported     # k > 64: the high-rate family
    long_ = dec.osdl_supported and not dec.osdx_supported and not dec.osdw_supported     # n > 128 or n-k > 64: the long / low-rate family
    if not dec.osdx_supported and not dec.osdw_supported and not dec.osdl_supported:
        raise SystemExit(f"osdx_fer: the OSD kernels serve n <= 384, 1 <= k <= 192 and 1 <= n-k <= 192; this code is ({dec.n},{dec.k})")
    B = args.frames
    y, labels = dec.gen_frames(B, seed=args.seed, snr_db=args.snr) if args.gen == "hip" else make_frames(dec, B, args.seed, args.snr)
    res = dec.nms(y, args.T, args.alpha)
    nms_counts = dec.eval_counts(res["hard"], labels, res["fail"])
    index, count = dec.compact(res["fail"])
    torch.cuda.synchronize()
    nf = int(count.cpu()[0])
    idx = index[:max(nf, 1)].contiguous()
    counts = torch.zeros(3, dtype=torch.int64, device=dec.device)
    if fs:
        fsp = dec.osd_params(args.order, _lib.OSD_FS, fs_beta=args.beta, fs_tau_e=args.tau_e, fs_tau_psc=args.tau_psc)
        fs_decode = dec.osdw_fs_decode if wide else dec.osdl_fs_decode if long_ else dec.osdx_fs_decode
        out = fs_decode(y, fsp, index=idx, count=count, label_bits=labels, counts=counts)
    elif pb:
        aux = torch.zeros((idx.shape[0], 4), dtype=torch.int32, device=dec.device)
        pbp = dec.osd_params(args.order, _lib.OSD_PB, snr_db=args.snr, aux=aux)
        pb_decode = dec.osdw_pb_decode if wide else dec.osdl_pb_decode if long_ else dec.osdx_pb_decode
        out = pb_decode(y, pbp, index=idx, count=count, label_bits=labels, counts=counts)
    elif wide:
        out = dec.osdw_decode(y, args.order, index=idx, count=count, label_bits=labels, counts=counts)
    elif long_:
        out = dec.osdl_decode(y, args.order, index=idx, count=count, label_bits=labels, counts=counts)
    else:
        out = dec.osdx_decode(y, args.order, index=idx, count=count, label_bits=labels, counts=counts)
    torch.cuda.synchronize()
    if args.pipeline:
        pipeline_check(dec, args, y, labels, res, nms_counts, index, nf, out, counts, aux if pb else None)
    nc = nms_counts.cpu().tolist()
    oc = counts.cpu().tolist()
    # a frame is wrong after the stage if NMS left an undetected error (zero syndrome: never listed) or the OSD missed it
    fer_nms = nc[1] / B
    fer_osd = (nc[3] + oc[1]) / B
    print(f"({dec.n},{dec.k}) {args.snr} dB, {B} frames, NMS-{args.T}: FER {fer_nms:.3e} ({nc[1]} wrong, {nf} with a non-zero syndrome, "
          f"{nc[3]} undetected)", flush=True)
    result = dict(n=dec.n, k=dec.k, snr_db=args.snr, frames=B, T=args.T, order=args.order, failures=nf, fer_nms=fer_nms, fer_osd=fer_osd,
                  gen=args.gen, kernels={})
    if fs:
        table = sum(math.comb(dec.k, w) for w in range(args.order + 1))
        ntep = out["ntep"][:nf].to(torch.float64)
        mean, most = (float(ntep.mean()), int(ntep.max())) if nf else (0.0, 0)
        print(f"  order-{args.order} FS-OSD (beta {args.beta}, tau_e {args.tau_e}, tau_psc {args.tau_psc}) on the {nf} failures: FER {fer_osd:.3e} "
              f"({oc[1]} still wrong); TEPs per frame: mean {mean:.1f}, max {most}, table {table}", flush=True)
        result.update(osd="fs", beta=args.beta, tau_e=args.tau_e, tau_psc=args.tau_psc, teps_mean=mean, teps_max=most, teps_table=table)
        if wide or long_:                                    # the full scan of the same order on the same frames
            cc = torch.zeros(3, dtype=torch.int64, device=dec.device)
            outc = (dec.osdw_decode if wide else dec.osdl_decode)(y, args.order, index=idx, count=count, label_bits=labels, counts=cc)
            torch.cuda.synchronize()
            fer_conv = (nc[3] + cc.cpu().tolist()[1]) / B
            print(f"  order-{args.order} conventional scan on the same failures: FER {fer_conv:.3e} ({cc.cpu().tolist()[1]} still wrong, "
                  f"{table} TEPs per frame)", flush=True)
            result.update(fer_conv=fer_conv)
    elif pb:
        table = sum(math.comb(dec.k, w) for w in range(args.order + 1))
        ntep = out["ntep"][:nf].to(torch.float64)
        mean, most = (float(ntep.mean()), int(ntep.max())) if nf else (0.0, 0)
        stops = [int((aux[:nf, 3] == r).sum()) / max(nf, 1) for r in range(3)]
        print(f"  order-{args.order} PB-OSD (snr_db {args.snr}) on the {nf} failures: FER {fer_osd:.3e} ({oc[1]} still wrong); TEPs per frame: "
              f"mean {mean:.1f}, max {most}, N_max {table}; stops: none {stops[0]:.3f}, promising {stops[1]:.3f}, success {stops[2]:.3f}",
              flush=True)
        result.update(osd="pb", teps_mean=mean, teps_max=most, teps_table=table, stop_shares=stops)
    else:
        print(f"  order-{args.order} OSD on the {nf} failures: FER {fer_osd:.3e} ({oc[1]} still wrong, {oc[2] // max(oc[0], 1)} TEPs per frame)",
              flush=True)
    if nf == 0:
        print(json.dumps(result), flush=True)
        return 0
    front = (out["perm"], out["parity"], None)
    legs = [("osdx_front_kernel", lambda: dec.osdx_front(y, index=idx, count=count, out=front)),
            ("osdx_search_kernel", lambda: dec.osdx_search(y, out["perm"], out["parity"], args.order, index=idx, count=count, out=out))]
    if wide:
        legs = [("osdw_front_kernel", lambda: dec.osdw_front(y, index=idx, count=count, out=front)),
                ("osdw_search_kernel", lambda: dec.osdw_search(y, out["perm"], out["parity"], args.order, index=idx, count=count, out=out))]
    elif long_:
        legs = [("osdl_front_kernel", lambda: dec.osdl_front(y, index=idx, count=count, out=front)),
                ("osdl_search_kernel", lambda: dec.osdl_search(y, out["perm"], out["parity"], args.order, index=idx, count=count, out=out))]
    legs_l = []
    if not fs and not pb and dec.osdw_supported and dec.osdl_supported:   # the osdl kernels on the same frames, alternating
        outl = dec.osdl_decode(y, args.order, index=idx, count=count)
        frontl = (outl["perm"], outl["parity"], None)
        for key in ("cw", "metric", "best", "ntep"):
            assert torch.equal(outl[key][:nf], out[key][:nf]), key
        legs_l = [("osdl_front_kernel", lambda: dec.osdl_front(y, index=idx, count=count, out=frontl)),
                  ("osdl_search_kernel", lambda: dec.osdl_search(y, outl["perm"], outl["parity"], args.order, index=idx, count=count, out=outl))]
    if not wide and not fs and not pb and dec.osdw_supported:       # both families serve the code: the osdw kernels on the same frames
        outw = dec.osdw_decode(y, args.order, index=idx, count=count)
        frontw = (outw["perm"], outw["parity"], None)
        legs += [("osdw_front_kernel", lambda: dec.osdw_front(y, index=idx, count=count, out=frontw)),
                 ("osdw_search_kernel", lambda: dec.osdw_search(y, outw["perm"], outw["parity"], args.order, index=idx, count=count, out=outw))]
    if fs and wide:
        legs[1] = ("osdw_fs_kernel", lambda: dec.osdw_fs_search(y, out["perm"], out["parity"], fsp, index=idx, count=count, out=out))
        legs.append(("osdw_search_kernel", lambda: dec.osdw_search(y, out["perm"], out["parity"], args.order, index=idx, count=count, out=outc)))
    elif fs and long_:
        legs[1] = ("osdl_fs_kernel", lambda: dec.osdl_fs_search(y, out["perm"], out["parity"], fsp, index=idx, count=count, out=out))
        legs.append(("osdl_search_kernel", lambda: dec.osdl_search(y, out["perm"], out["parity"], args.order, index=idx, count=count, out=outc)))
    elif fs:
        legs[1] = ("osdx_fs_kernel", lambda: dec.osdx_fs_search(y, out["perm"], out["parity"], fsp, index=idx, count=count, out=out))
        if dec.osdw_supported:                           # both families serve the code: osdw_fs_kernel on the same frames
            outw = dec.osdw_fs_decode(y, fsp, index=idx, count=count)
            legs.append(("osdw_fs_kernel", lambda: dec.osdw_fs_search(y, outw["perm"], outw["parity"], fsp, index=idx, count=count, out=outw)))
        if (dec.n, dec.k) == (128, 64):                  # the specialised kernel on the same front-end results, in the same run
            out2 = dec.osd_search(y, out["perm"], out["parity"], fsp, index=idx, count=count)
            legs.append(("osd_fs_kernel", lambda: dec.osd_search(y, out["perm"], out["parity"], fsp, index=idx, count=count, out=out2)))
    elif pb and wide:
        legs[1] = ("osdw_pb_kernel", lambda: dec.osdw_pb_search(y, out["perm"], out["parity"], pbp, index=idx, count=count, out=out))
        outc = dec.osdw_search(y, out["perm"], out["parity"], args.order, index=idx, count=count)
        legs.append(("osdw_search_kernel", lambda: dec.osdw_search(y, out["perm"], out["parity"], args.order, index=idx, count=count, out=outc)))
        if args.tau_e is not None:                       # FS-OSD of the same order on the same frames
            fsp = dec.osd_params(args.order, _lib.OSD_FS, fs_beta=args.beta, fs_tau_e=args.tau_e, fs_tau_psc=args.tau_psc)
            outf = dec.osdw_fs_search(y, out["perm"], out["parity"], fsp, index=idx, count=count)
            legs.append(("osdw_fs_kernel", lambda: dec.osdw_fs_search(y, out["perm"], out["parity"], fsp, index=idx, count=count, out=outf)))
    elif pb and long_:
        legs[1] = ("osdl_pb_kernel", lambda: dec.osdl_pb_search(y, out["perm"], out["parity"], pbp, index=idx, count=count, out=out))
        outc = dec.osdl_search(y, out["perm"], out["parity"], args.order, index=idx, count=count)
        legs.append(("osdl_search_kernel", lambda: dec.osdl_search(y, out["perm"], out["parity"], args.order, index=idx, count=count, out=outc)))
        if args.tau_e is not None:                       # FS-OSD of the same order on the same frames
            fsp = dec.osd_params(args.order, _lib.OSD_FS, fs_beta=args.beta, fs_tau_e=args.tau_e, fs_tau_psc=args.tau_psc)
            outf = dec.osdl_fs_search(y, out["perm"], out["parity"], fsp, index=idx, count=count)
            legs.append(("osdl_fs_kernel", lambda: dec.osdl_fs_search(y, out["perm"], out["parity"], fsp, index=idx, count=count, out=outf)))
    elif pb:
        legs[1] = ("osdx_pb_kernel", lambda: dec.osdx_pb_search(y, out["perm"], out["parity"], pbp, index=idx, count=count, out=out))
        if dec.osdw_supported:                           # both families serve the code: osdw_pb_kernel on the same frames
            outw = dec.osdw_pb_decode(y, dec.osd_params(args.order, _lib.OSD_PB, snr_db=args.snr), index=idx, count=count)
            pbw = dec.osd_params(args.order, _lib.OSD_PB, snr_db=args.snr)
            legs.append(("osdw_pb_kernel", lambda: dec.osdw_pb_search(y, outw["perm"], outw["parity"], pbw, index=idx, count=count, out=outw)))
        if (dec.n, dec.k) == (128, 64):                  # the specialised routes on the same front-end results, in the same run
            for name, path in (("osd_search(PB replay)", "replay"), ("osd_search(PB staged)", None)):
                pr = dec.osd_params(args.order, _lib.OSD_PB, snr_db=args.snr, pb_path=path)
                o2 = dec.osd_search(y, out["perm"], out["parity"], pr, index=idx, count=count)
                legs.append((name, lambda pr=pr, o2=o2: dec.osd_search(y, out["perm"], out["parity"], pr, index=idx, count=count, out=o2)))
    elif (dec.n, dec.k) == (128, 64):                      # the specialised kernels on the same frames, in the same run
        p = dec.osd_params(args.order, table_scan=True)
        perm2, par2, ns2 = dec.osd_front(y, index=idx, count=count)
        out2 = dec.osd_search(y, perm2, par2, p, index=idx, count=count)
        legs += [("osd_front_kernel", lambda: dec.osd_front(y, index=idx, count=count, out=(perm2, par2, ns2))),
                 ("osd_search_kernel(table)", lambda: dec.osd_search(y, perm2, par2, p, index=idx, count=count, out=out2))]
    if fs and not long_ and dec.osdl_supported:            # an older family serves the code: osdl_fs_kernel on the same frames, alternating
        outl = dec.osdl_fs_decode(y, fsp, index=idx, count=count)
        for key in ("cw", "metric", "best", "ntep"):
            assert torch.equal(outl[key][:nf], out[key][:nf]), key
        legs_l = [("osdl_fs_kernel", lambda: dec.osdl_fs_search(y, outl["perm"], outl["parity"], fsp, index=idx, count=count, out=outl))]
    if pb and not long_ and dec.osdl_supported:            # an older family serves the code: osdl_pb_kernel on the same frames, alternating
        auxl = torch.zeros_like(aux)
        pbl = dec.osd_params(args.order, _lib.OSD_PB, snr_db=args.snr, aux=auxl)
        outl = dec.osdl_pb_decode(y, pbl, index=idx, count=count)
        torch.cuda.synchronize()
        for key in ("cw", "metric", "best", "ntep"):
            assert torch.equal(outl[key][:nf], out[key][:nf]), key
        assert torch.equal(auxl[:nf], aux[:nf]), "aux"
        legs_l = [("osdl_pb_kernel", lambda: dec.osdl_pb_search(y, outl["perm"], outl["parity"], pbl, index=idx, count=count, out=outl))]
    legs += legs_l
    if not fs and not pb:                                # the one-TEP kernel of every family in the run: each frame flips MRB positions 0 and k - 1
        def tep_mask(words):
            m = np.zeros((idx.shape[0], words), np.uint64)
            for p in {0, dec.k - 1}:
                m[:, p // 64] |= np.uint64(1) << np.uint64(p % 64)
            return torch.from_numpy(m.view(np.int64)).to(dec.device)
        fronts = {"osdl" if long_ else "osdw" if wide else "osdx": (out["perm"], out["parity"])}
        if not wide and not long_ and dec.osdw_supported:
            fronts["osdw"] = (outw["perm"], outw["parity"])
        if legs_l:
            fronts["osdl"] = (outl["perm"], outl["parity"])
        for fam, (fperm, fparity) in fronts.items():
            mask = tep_mask({"osdx": 1, "osdw": 2, "osdl": (dec.k + 63) // 64}[fam])
            mask = mask[:, 0].contiguous() if fam == "osdx" else mask
            res = getattr(dec, fam + "_tep_eval")(y, fperm, fparity, mask, index=idx, count=count)
            targs = tuple(_ptr(t) for t in (y, idx, count)) + (idx.shape[0],) + tuple(
                _ptr(t) for t in (fperm, fparity, mask, res["cw"], res["metric"], res["hd"]))
            # (Decoder.*_tep_eval allocates its outputs on every call; the timed leg calls the library function on those of one call)
            legs.append((fam + "_tep_eval_kernel", lambda fam=fam, targs=targs: dec._osd_call(fam, "tep_eval", *targs)))
    if args.oracle > 0:
        import time
        from oracle import c_oracle
        Gn = np.asarray(dec.code.G)
        yo = y[idx[:min(nf, args.oracle)].long()].cpu().numpy()
        c_oracle.osd_front(Gn, yo[0])
        t0 = time.perf_counter()
        for row in yo:
            c_oracle.osd_front(Gn, row)
        dt = time.perf_counter() - t0
        result["oracle_front_frames_per_s"] = len(yo) / dt
        print(f"  C oracle front end, one core: {len(yo)} frames in {dt:.3f} s, {len(yo) / dt:.1f} frames/s", flush=True)
    for _ in range(2):                                   # the legs alternate: two passes over all of them
        for name, fn in legs:
            us = timed(fn, args.calls, args.repeats, args.warmup)
            med = float(np.median(us))
            result["kernels"].setdefault(name, []).append(dict(us_per_call=us, median_us=med, frames_per_s=nf / med * 1e6))
            print(f"  {name:26s} {med:9.1f} us per call (min {min(us):.1f}, max {max(us):.1f}), {nf / med:8.2f} M frames/s", flush=True)
    print(json.dumps(result), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
