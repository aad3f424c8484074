#!/usr/bin/env python3
"""Time per ldpc_nms_train_grad call (forward + backward + batch sums) at B in {100, 4096, 131072}, T = 12, CCSDS (128,64),
next to ldpc_nms_decode's generic and QC16 kernels at the same B.  One JSON line per B (microseconds per call)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from short_ldpc_decoding_osd_amd import Code  # noqa: E402
from short_ldpc_decoding_osd_amd.runtime import Decoder  # noqa: E402


def timed(fn, n):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def main():
    dec = Decoder(Code(), 0)
    T = 12
    alpha = np.full(T, 0.669435, np.float32)
    g = torch.Generator(device=dec.device).manual_seed(1)
    for B in (100, 4096, 131072):
        n_rep = 200 if B < 100000 else 20
        y = (1.0 + 0.8 * torch.randn((B, dec.n), device=dec.device, generator=g)).contiguous()
        lab = torch.zeros((B, dec.words), dtype=torch.int64, device=dec.device)   # all-zero codeword, BPSK +1
        out = dec.nms_grad(y, lab, T, alpha)
        dout = dec.nms(y, T, alpha, want_soft=True, want_hard=False, want_fail=False, kernel=1)
        row = dict(B=B, T=T,
                   train_grad_us=timed(lambda: dec.nms_grad(y, lab, T, alpha, out=out), n_rep),
                   train_grad_no_sums_us=timed(lambda: dec.nms_grad(y, lab, T, alpha, want_sums=False, out=dict(out, loss_sum=None, grad_sum=None)), n_rep),
                   nms_generic_us=timed(lambda: dec.nms(y, T, alpha, want_hard=False, want_fail=False, kernel=1, out=dout), n_rep),
                   nms_qc16_us=timed(lambda: dec.nms(y, T, alpha, want_hard=False, want_fail=False, kernel=2, out=dout), n_rep))
        row["train_over_generic"] = row["train_grad_us"] / row["nms_generic_us"]
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
