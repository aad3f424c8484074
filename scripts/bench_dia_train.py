#!/usr/bin/env python3
"""Time per ldpc_dia_cnn_grad call next to ldpc_dia_cnn on the same rows (L = 13, CCSDS (128,64)) at F = 100 (the
reference's batch) and F = 32768, with the rows' bytes over the time of each call, and one full training step at F = 100:
call, synchronisation (the gradient comes to the host), clip and Adam on the host.  One JSON line per F; times in
microseconds as [median, min, max] of 7 repeats."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from short_ldpc_decoding_osd_amd import Code, nn_net  # noqa: E402
from short_ldpc_decoding_osd_amd import globalmap as GL  # noqa: E402
from short_ldpc_decoding_osd_amd.nms_train import ExponentialDecay, LegacyAdam, clip_by_norm  # noqa: E402
from short_ldpc_decoding_osd_amd.runtime import default_decoder  # noqa: E402


def timed(fn, n):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def spread(fns, n, repeats=7):
    """{name: [median, min, max]} in microseconds per call: device events around n back-to-back calls, ``repeats`` times
    after a warm-up, the candidates alternating."""
    for fn in fns.values():
        for _ in range(5):
            fn()
    got = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            got[k].append(timed(fn, n))
    return {k: [round(sorted(v)[len(v) // 2], 2), round(min(v), 2), round(max(v), 2)] for k, v in got.items()}


def main():
    L = 13
    code = Code()
    GL.set_map('code_parameters', code)
    GL.set_map('num_iterations', L - 1)
    dec = default_decoder(code)
    nn = nn_net.conv_bitwise().initialize(0)
    g = torch.Generator(device=dec.device).manual_seed(1)
    for F in (100, 32768):
        n_rep = 200 if F < 10000 else 20
        rows = (torch.randn((F, L, dec.n), device=dec.device, generator=g) * 3).contiguous()
        labels = torch.randint(0, 2, (F, dec.n), device=dec.device, generator=g, dtype=torch.int64)
        lab = dec.pack_bits(labels)
        w = nn.packed()
        out = dec.dia_cnn(rows, w)
        row = dict(F=F, L=L, rows_MB=rows.numel() * 4 / 1e6)
        row.update(spread({"grad_us": lambda: dec.dia_cnn_grad(rows, lab, w),
                           "grad_with_out_us": lambda: dec.dia_cnn_grad(rows, lab, w, want_out=True),
                           "forward_us": lambda: dec.dia_cnn(rows, w, out=out)}, n_rep))
        row["grad_over_forward"] = row["grad_us"][0] / row["forward_us"][0]
        row["grad_rows_GBps"] = rows.numel() * 4 / row["grad_us"][0] / 1e3
        row["forward_rows_GBps"] = rows.numel() * 4 / row["forward_us"][0] / 1e3
        if F == 100:      # a full step as Training_NN takes it (host wall clock: the step ends on the host)
            opt = LegacyAdam(ExponentialDecay(0.001, 500, 0.95))

            def step():
                _, grads = nn.loss_and_grads(rows, labels)
                opt.apply_gradients([(clip_by_norm(gr, 5e2), a, nn.__dict__) for gr, a in zip(grads, nn.TRAINABLE)])
            for _ in range(10):
                step()
            steps = []
            for _ in range(7):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n_rep):
                    step()
                steps.append((time.perf_counter() - t0) / n_rep * 1e6)
            row["train_step_us"] = [round(sorted(steps)[3], 2), round(min(steps), 2), round(max(steps), 2)]
        print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)


if __name__ == "__main__":
    main()
