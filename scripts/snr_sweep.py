#!/usr/bin/env python3
"""BASELINE config 5: SNR sweep of (learned-)NMS + PB-OSD (or FS / conventional OSD) with frames sharded
across the GPUs of a node and ONE RCCL all-reduce of the counters per SNR point.

    python scripts/snr_sweep.py --snr 1.0 3.5 6 --frames 1048576 --osd pb --order 3
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 scripts/snr_sweep.py ...

Prints one JSON line per SNR point (rank 0): FER_NMS, FER_OSD|fail, their product (what the reference's
recipe multiplies by hand, `Training and Testing recipe.txt:18`), end-to-end FER, mean TEPs, frames/s.
The reference sweeps 2.0-3.0 dB with order 3 and stops each point at 100 OSD failures, checked after every FRAME
(PB_OSD/globalmap.py:42-43, pb_testing.py:159-174: `fail_sum`, OSD failures only).  `--stop-errors N` is the sharded form
of that rule and is NOT line-for-line comparable with the reference's logs: it counts END-TO-END errors (OSD failures +
NMS errors the syndrome did not flag) and checks the threshold after every MACRO-BATCH (one 64-byte all-reduce each, every
rank leaves on the same macro-batch), so a point overshoots by up to one macro-batch of `--batch` x world frames -- use a
small `--batch` with it; the JSON line says so (`stop_rule`).  By default every point decodes the requested number of frames.
`--cpu-check` decodes a bounded sample of every point with the CPU port (oracle/ldpc_oracle.c, the checker) on rank 0 and
prints `fer_vs_cpu` beside the GPU figures: +-5 % judged when both sides hold >= 1600 frame errors, else "not judged".
`--gen hip` draws the frames with the library's counter-based generator (`Decoder.gen_frames`, one launch per batch) instead
of the torch ops: the seed belongs to the SNR point and every batch starts at its first GLOBAL frame number, so a point
decodes the same frames for every world size, `--batch` and `--streams`; the JSON line says `"gen": "hip"`.
`--alist FILE` sweeps another code, any that a G-form OSD family serves (ldpc_osdx_*, ldpc_osdw_*, ldpc_osdl_*: up to
(384,192)), through `pipeline.FamilyPipeline` with every other option unchanged; the JSON line then names the family and adds
the bit error rates before and after the OSD codewords are merged into the NMS decisions (`ber_nms`, `ber_end_to_end`).
`--cpu-check` there: the CPU port's NMS serves every shape, its OSD batch calls serve (128,64) only, so the conventional OSD of
another shape goes through the NumPy port frame by frame (a smaller sample in the same time) and FS / PB are not judged.

    python scripts/snr_sweep.py --alist tests/golden/LDPC_N96_K48_P8_set0_dmin10.alist --osd conv --order 2 --cpu-check

`--osd dl --training DIR [--alist FILE]` sweeps NMS + the DL-OSD stage on `pipeline.DlOsdPipeline` (one call per batch, any code
an H-form family serves), with the networks and the decoding path taken exactly as `scripts/run_dl_osd.py` takes them: the CNN
and classifier checkpoints under DIR/ckpts/, the dist-error-pattern pickle under DIR/log/ (or `--convention-path`), `--no-dia`
for DIA = False, `--type` for the decoder type in those paths.  `--capacity` sizes the per-failure buffers (frames beyond it
stay NMS failures; the JSON line's `left_out` counts them).  Every other option works as on the other legs (`--gen hip`,
`--streams`, multi-rank, `--stop-errors`: undetected + merged wrong).  The JSON line carries the 15 counters' rates: `fer_end_to_end`,
`ber_nms`, `ber_end_to_end`, `fer_dl_given_fail`, `mean_windows`, `mean_complexity`, `mean_teps`.  `--cpu-check` there: the
failures of the point's last batch on rank 0 (at most `--cpu-frames`) go through the host route `osd.sliding_osd` -- block minima
on the device, the window loop and the classifier on the host -- and `dl_vs_host` holds both sides' (S, F, windows, complexity).

    python scripts/snr_sweep.py --osd dl --training DIR --snr 2.0 3.0 3 --iters 12 --capacity 16384 --cpu-check
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from short_ldpc_decoding_osd_amd import Code, _lib  # noqa: E402
from short_ldpc_decoding_osd_amd.pipeline import BatchPipeline, DlOsdPipeline, FamilyPipeline  # noqa: E402
from short_ldpc_decoding_osd_amd.runtime import Decoder  # noqa: E402
from short_ldpc_decoding_osd_amd.sharding import combine_fer, end_to_end_errors, rank_seed, shard_range, sweep_point  # noqa: E402
from short_ldpc_decoding_osd_amd.weights import softplus32  # noqa: E402

ALGOS = {"conv": _lib.OSD_CONVENTIONAL, "fs": _lib.OSD_FS, "pb": _lib.OSD_PB}


def frames_on_device(dec, B, snr_db, gen):
    G = torch.from_numpy(dec.code.G).to(device=dec.device, dtype=torch.float32)
    sigma = float(np.sqrt(1.0 / (2.0 * (dec.k / dec.n) * 10.0 ** (snr_db / 10.0))))
    cw = (torch.randint(0, 2, (B, dec.k), device=dec.device, generator=gen).to(torch.float32) @ G).remainder_(2)
    y = ((1 - 2 * cw) * (1 + sigma * torch.randn((B, dec.n), device=dec.device, generator=gen))).contiguous()
    return y, dec.pack_bits(cw.to(torch.uint8))


def cpu_counts_any_shape(G, H, y, cw, alpha, order, iters, teps):
    """bench.cpu_counts for a code that is not (128,64), conventional OSD: NMS and the counters by the C port, which serve every
    shape, then the NumPy port of the front end and the order-p scan on every syndrome failure.  Same int64[5]."""
    from oracle import c_oracle, np_oracle
    soft = c_oracle.nms(H, y, iters, alpha)
    _, fail, cnt = c_oracle.evaluate(H, soft, cw)
    wrong = int(cnt["synd_fail"])
    if order is not None:
        wrong = 0
        for f in np.flatnonzero(fail):
            yp, labp, Gp, _, _ = np_oracle.swapped_info(y[f], cw[f], G)
            wrong += not np_oracle.convention_osd(yp, labp, Gp, order, teps)["correct"]
    return np.array([y.shape[0], cnt["frame_err"], cnt["undetected"], cnt["synd_fail"], wrong], dtype=np.int64)


def cpu_check(code, alpha, args, snr, gpu_errors, gpu_frames):
    """The same SNR point through the CPU port on a bounded sample (all host cores of this rank's share): FER of both
    sides and the +-5 % judgement of BASELINE.json's north_star (>= 1600 frame errors on both sides, else not judged)."""
    import concurrent.futures

    import bench
    from oracle import np_oracle
    algo = ALGOS[args.osd]
    if args.alist and (code.G.shape != (64, 128)):
        if args.order is not None and algo != _lib.OSD_CONVENTIONAL:
            return {"judged": False, "within_5_percent": "not judged",
                    "reason": "the CPU port's FS-OSD and PB-OSD serve (128,64) only; --osd conv is checked on every shape"}
        teps = np_oracle.tep_matrix(code.G.shape[0], args.order) if args.order is not None else None

        def counts(G, H, y, cw, alpha, order, algo, snr, iters):
            return cpu_counts_any_shape(G, H, y, cw, alpha, order, iters, teps)
    else:
        counts = bench.cpu_counts
    rng = np.random.default_rng(20241020 + int(round(snr * 100)))
    cores = bench.host_cores()
    probe = 200
    y, cw = np_oracle.make_frames(code.G, snr, probe, rng)
    t0 = time.perf_counter()
    counts(code.G, code.H, y, cw, alpha, args.order, algo, snr, args.iters)
    per = int(max(100, min(200000, probe / (time.perf_counter() - t0) * args.cpu_seconds)))
    y, cw = np_oracle.make_frames(code.G, snr, per * cores, rng)
    with concurrent.futures.ThreadPoolExecutor(max_workers=cores) as ex:
        c = sum(ex.map(lambda i: counts(code.G, code.H, y[i * per:(i + 1) * per], cw[i * per:(i + 1) * per], alpha,
                                                  args.order, algo, snr, args.iters), range(cores)))
    ec = int(c[4] + c[2]) if args.order is not None else int(c[1])
    fg, fc = gpu_errors / max(gpu_frames, 1), ec / max(int(c[0]), 1)
    enough = gpu_errors >= 1600 and ec >= 1600
    rel = fg / fc - 1.0 if fc > 0 else float("nan")
    return {"gpu_fer_end_to_end": fg, "cpu_fer_end_to_end": fc, "cpu_frames": int(c[0]), "cpu_frame_errors": ec, "gpu_frame_errors": int(gpu_errors),
            "fer_rel_diff_vs_cpu": rel, "two_sigma_of_rel_diff": 2.0 * float(np.sqrt(1.0 / max(gpu_errors, 1) + 1.0 / max(ec, 1))),
            "judged": bool(enough), "within_5_percent": bool(abs(rel) <= 0.05) if enough else "not judged"}


def dl_setup(args):
    """The DL-OSD stage's settings, networks and decoding path, as scripts/run_dl_osd.py and nn_testing.Testing_OSD take them
    -> dict(dec, inst, fcn, nn, blocks, acc, teps, off, win, margin, path)."""
    from short_ldpc_decoding_osd_amd import globalmap as GL
    from short_ldpc_decoding_osd_amd import nn_testing as NT
    from short_ldpc_decoding_osd_amd import ordered_statistics_decoding as OSD
    GL.global_setting(["prog", args.snr[0], args.snr[1], args.snr[2], str(args.batch), str(args.iters),
                       args.alist or "CCSDS_ldpc_n128_k64.alist", args.type], stage="DL")
    GL.set_map('dl_training_dir', os.path.join(os.path.abspath(args.training), ""))
    GL.set_map('convention_path', args.convention_path)
    indicator_list, prefix_list = [True, False, False], ['model_cnn', 'model_rnn1', 'model_rnn2']
    restore_list = [GL.logistic_setting_model(indicator_list, prefix_list), GL.set_predict_model(True)]
    dia = not args.no_dia
    inst = OSD.osd(GL.get_map('code_parameters'))
    query = NT.query_convention_path if args.convention_path else NT.query_decoding_path
    path, _ = query(indicator_list, prefix_list, dia)
    blocks, acc = OSD.generate_teps(inst, path)
    nn, fcn = NT.NN_gen(restore_list, indicator_list) if dia else (None, NT.load_fcn(restore_list[1]))
    dec = OSD._dec()                                            # (the host route of --cpu-check decodes on this context too)
    teps, off = inst._device_blocks(dec, blocks)
    return dict(dec=dec, inst=inst, fcn=fcn, nn=nn, blocks=blocks, acc=np.asarray(acc, dtype=np.int64), teps=teps, off=off,
                win=GL.get_map('sliding_win_width'), margin=GL.get_map('soft_margin'), path=path)


def dl_cpu_check(dl, pipe, limit):
    """The failures that ``pipe`` holds (its last batch; at most ``limit``) through the host route osd.sliding_osd, beside what the
    one call made of the same frames: (success, failure, windows, complexity) of both sides."""
    dec, win = pipe.dec, dl["win"]
    F = min(int(pipe.count.item()), pipe.capacity, int(limit))
    if F == 0:
        return {"frames": 0, "agree": "not judged"}
    L = pipe.T + 1
    metric = pipe.metric_llr[:F].cpu().numpy()
    if pipe.rows is not None:
        input_list, ordering = pipe.rows[:F].cpu().numpy().reshape(F * L, dec.n), pipe.order_llr[:F].cpu().numpy()
    else:                                                       # DIA = False: only row 0 of a trajectory is read
        input_list, ordering = np.zeros((F * L, dec.n), dtype=np.float32), metric
        input_list[0::L] = metric
    labels = dec.unpack_bits(pipe.list_labels[:F].contiguous()).cpu().numpy()
    host = dl["inst"].sliding_osd(dl["fcn"], input_list, ordering, labels, (dl["blocks"], dl["acc"]))
    deep, ok = pipe.deep_limit[:F].cpu().numpy().astype(np.int64), pipe.success[:F].cpu().numpy().astype(bool)
    device = (int(ok.sum()), int((~ok).sum()), int((deep - win + 1).sum()), int(dl["acc"][deep].sum()))
    return {"frames": F, "host": [int(v) for v in host], "device": list(device), "agree": tuple(int(v) for v in host) == device}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--snr", nargs=3, default=["1.0", "3.5", "6"], metavar=("LO", "HI", "NUM"))
    ap.add_argument("--frames", type=int, default=1 << 20, help="frames per SNR point, all ranks together")
    ap.add_argument("--batch", type=int, default=131072, help="frames per device batch")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--osd", choices=sorted(ALGOS) + ["dl"], default="pb")
    ap.add_argument("--training", default=None, help="--osd dl: the training stage's directory (ckpts/, log/), as run_dl_osd.py takes it")
    ap.add_argument("--type", default="NMS-1", help="--osd dl: the decoder type in the training directory's paths")
    ap.add_argument("--no-dia", action="store_true", help="--osd dl: no CNN, the ordering values are the channel values")
    ap.add_argument("--convention-path", action="store_true", help="--osd dl: the conventional decoding path instead of the pickle's")
    ap.add_argument("--capacity", type=int, default=0, help="--osd dl: rows of the per-failure buffers (0: the batch size)")
    ap.add_argument("--cpu-frames", type=int, default=256, help="--osd dl --cpu-check: failures that go through the host route")
    ap.add_argument("--order", type=int, default=3)
    ap.add_argument("--weight", type=float, default=-0.048, help="stored (pre-softplus) NMS-1 weight")
    ap.add_argument("--values", default=None, help="par/values.txt of the training stage (overrides --weight)")
    ap.add_argument("--stop-errors", type=int, default=0,
                    help="end an SNR point once this many end-to-end frame errors were seen over all ranks (the reference's "
                         "termination_num_threshlod, PB_OSD/globalmap.py:43: 100); 0 = decode --frames frames")
    ap.add_argument("--resident", action="store_true",
                    help="generate a point's frames BEFORE its timed region (inputs resident in HBM when it starts, bench.py's contract) "
                         "instead of one batch ahead inside it: the figure is then `frames_per_s_resident_inputs`")
    ap.add_argument("--cpu-check", action="store_true",
                    help="rank 0: decode a bounded sample of every SNR point with the CPU port too and print fer_vs_cpu")
    ap.add_argument("--cpu-seconds", type=float, default=10.0, help="--cpu-check: CPU time budget per SNR point")
    ap.add_argument("--gen", choices=("torch", "hip"), default="torch",
                    help="frame source: torch ops with one torch generator per rank (the frames depend on the layout), or the "
                         "library's counter-based generator (frame i of a point is the same for every layout)")
    ap.add_argument("--streams", type=int, default=3,
                    help="decode streams: consecutive batches rotate over them, so the tail of one batch's search kernels "
                         "(a few long searches on an emptying chip) overlaps the next batches' decoding (scratch is per stream; "
                         "PB-3 sweep, 2 / 3 / 4 streams: 1.99 / 2.04 / 2.00 x 10^7 frames/s at 1.0 dB, 7.5 / 7.8 / 7.5 x 10^7 at 2.0 dB)")
    ap.add_argument("--alist", default=None,
                    help="alist file of another code: the sweep runs on pipeline.FamilyPipeline (any code a G-form OSD family serves)")
    args = ap.parse_args()

    world, rank, local = (int(os.environ.get(k, d)) for k, d in (("WORLD_SIZE", 1), ("RANK", 0), ("LOCAL_RANK", 0)))
    torch.cuda.set_device(local)
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local))
    stored = args.weight
    if args.values:
        from short_ldpc_decoding_osd_amd import weights
        _, v = weights.parse_values_txt(args.values)
        stored = float([x for k, x in v.items() if "check" in k][0][0])
    alpha = float(softplus32(stored))                           # softplus, ms_test.py:207-208
    dl = None
    if args.osd == "dl":
        if not args.training:
            ap.error("--osd dl needs --training DIR")
        dl = dl_setup(args)
        dec = dl["dec"]
    else:
        dec = Decoder(Code(args.alist) if args.alist else Code(), local)

    def make_pipe(B, snr):
        """The pipeline object of a batch size: the (128,64) one, or with --alist the one on the OSD families."""
        if dl:
            return DlOsdPipeline(dec, B, args.iters, alpha, dl["teps"], dl["off"], dl["win"], dl["margin"], dl["fcn"].packed(),
                                 dl["nn"].packed() if dl["nn"] is not None else None, capacity=min(B, args.capacity) if args.capacity else None,
                                 want_soft=False)
        if args.alist:
            return FamilyPipeline(dec, B, args.iters, alpha, osd_order=args.order, osd_algo=ALGOS[args.osd], snr_db=snr, want_soft=False)
        return BatchPipeline(dec, B, args.iters, alpha, osd_order=args.order, osd_algo=ALGOS[args.osd], snr_db=snr,
                             want_soft=False, keep_front=False)
    lo, hi = shard_range(args.frames, rank, world)
    mine = hi - lo
    gen = torch.Generator(device=dec.device).manual_seed(rank_seed(20241020, rank))
    # the next batch's frames are generated on a second stream while the current batch is decoded (one batch ahead)
    main_stream, gen_stream = torch.cuda.current_stream(), torch.cuda.Stream()
    dstreams = [main_stream] + [torch.cuda.Stream() for _ in range(1, max(1, args.streams))]
    # warm-up with a full-size batch on every stream: the library's workspaces (OSD front-end results, PB-OSD lists / tables)
    # and torch's per-stream memory pools (hipMalloc synchronises) are sized before the first timed point
    with torch.cuda.stream(gen_stream):
        yw, lw = frames_on_device(dec, min(args.batch, max(mine, 1)), float(args.snr[0]), torch.Generator(device=dec.device).manual_seed(1))
    torch.cuda.synchronize()
    for st in dstreams:
        with torch.cuda.stream(st):
            if args.order is not None and not args.alist and not dl:      # (the families have no library workspace)
                dec.osd_reserve_stream(min(args.batch, max(mine, 1)), dec.osd_params(args.order, ALGOS[args.osd], snr_db=float(args.snr[0])))
            warm = make_pipe(yw.shape[0], float(args.snr[0])).bind(yw, lw)
            warm.run()
    torch.cuda.synchronize()
    with_osd = args.order is not None or dl is not None
    max_batches = -(-shard_range(args.frames, 0, world)[1] // args.batch)       # rank 0 owns the largest shard

    def produce(B, snr, st, k):
        """Batch k of this rank's share of the point."""
        with torch.cuda.stream(gen_stream):          # (no wait on the decode streams: the generator depends on nothing there)
            if args.gen == "hip":
                y, lab = dec.gen_frames(B, seed=20241020 + int(round(snr * 100)), snr_db=snr, frame0=lo + k * args.batch)
            else:
                y, lab = frames_on_device(dec, B, snr, gen)
            ev = torch.cuda.Event()
            ev.record(gen_stream)
        for t in (y, lab):
            t.record_stream(st)                      # (allocated on gen_stream, consumed on a decode stream)
        return y, lab, ev

    for snr in np.linspace(float(args.snr[0]), float(args.snr[1]), int(args.snr[2])):
        snr = round(float(snr), 2)
        sizes = [min(args.batch, mine - k * args.batch) for k in range(max_batches) if mine - k * args.batch > 0]
        if args.resident:
            ahead = [produce(b, snr, dstreams[k % len(dstreams)], k) for k, b in enumerate(sizes)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if not args.resident:
            ahead = [produce(sizes[0], snr, dstreams[0], 0)] if sizes else []
        taken = [0]
        last = [None]  # the pipeline object of the last batch decoded (--osd dl --cpu-check reads its buffers)
        pool = {}      # (stream number, batch size) -> pipeline object of this point: its output buffers are made once, not per batch

        def decode_batch(B, snr=snr):
            y, lab, ev = ahead.pop(0)
            st = dstreams[taken[0] % len(dstreams)]
            taken[0] += 1
            if taken[0] < len(sizes) and not args.resident:
                ahead.append(produce(sizes[taken[0]], snr, dstreams[taken[0] % len(dstreams)], taken[0]))
            assert y.shape[0] == B
            with torch.cuda.stream(st):
                st.wait_event(ev)
                key = ((taken[0] - 1) % len(dstreams), B)
                pipe = pool.get(key)
                if pipe is None:
                    pipe = pool[key] = make_pipe(B, snr)
                else:
                    pipe.reset_counters()
                pipe.bind(y, lab).run()
                last[0] = pipe
                c = pipe.counters().clone()      # (the object's own counters are zeroed for its next batch on this stream)
                done_ev = torch.cuda.Event()
                done_ev.record(st)
            if st is not main_stream:
                c.record_stream(main_stream)
                main_stream.wait_event(done_ev)      # (the counters are summed on the main stream; the NEXT batch is already enqueued on the other)
            return c

        total, ran = sweep_point(decode_batch, mine, args.batch, max_batches, args.stop_errors, with_osd, device=dec.device,
                                 width=15 if dl else 12 if args.alist else 8)   # the point's exchange step(s)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if rank == 0:
            c = total.cpu().numpy()
            out = combine_fer(c, n=dec.n)
            if args.alist or dl:
                out.update(code=[dec.n, dec.k], family=warm.family)
            if dl:
                out.update(path_blocks=len(dl["path"]), path_teps=int(dl["acc"][-1]), win=dl["win"], soft_margin=dl["margin"],
                           dia=dl["nn"] is not None, capacity=warm.capacity)
            out.update(snr_db=snr, osd=args.osd, order=args.order, alpha=alpha, n_gpus=world, macro_batches=ran, gen=args.gen,
                       stop_errors=args.stop_errors, **{"frames_per_s_resident_inputs" if args.resident else "frames_per_s_incl_generation": int(c[0]) / dt},
                       stop_rule=("end-to-end errors >= %d, checked per macro-batch of %d x %d frames" % (args.stop_errors, args.batch, world)) if args.stop_errors else "none: every frame decoded")
            if args.cpu_check and dl:
                out["dl_vs_host"] = dl_cpu_check(dl, last[0], args.cpu_frames) if last[0] is not None else {"frames": 0, "agree": "not judged"}
            elif args.cpu_check:
                out["fer_vs_cpu"] = cpu_check(dec.code, alpha, args, snr, end_to_end_errors(c, with_osd), int(c[0]))
            print(json.dumps(out), flush=True)
        if args.cpu_check:
            # (the device idled for the seconds of the CPU check: a point lasts 20-40 ms and would be timed on a chip that is still
            #  raising its clocks -- 4.5 instead of 5.7 x 10^7 frames/s at 1.5 dB; steady state is what the metric asks for)
            tw = time.perf_counter()
            while time.perf_counter() - tw < 0.4:
                with torch.cuda.stream(dstreams[-1]):
                    for _ in range(4):
                        warm.run()
                torch.cuda.synchronize()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
