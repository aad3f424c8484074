"""GPU box: python tests/tools/pb_big_batches.py -- PB-OSD order 3 against the C oracle on ~12 000 failing frames per SNR (lists long enough
for the chunk kernel's tail rule, under several of its settings), every run twice: where a search is handed on depends on timing, the
results must not.  (~80 s, most of it the oracle.)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, ROOT)
import numpy as np, torch
from oracle import c_oracle, np_oracle
from short_ldpc_decoding_osd_amd import Code, _lib
from short_ldpc_decoding_osd_amd.runtime import Decoder
from tests.test_gpu_osd_pb import _check, _failures
dec = Decoder(Code())
for snr, frames, tuning in ((1.5, 22000, {}), (2.0, 30000, dict(late_pct=60)), (1.0, 14000, dict(late_pct=100, late_div=64)), (2.5, 60000, dict(late_min=0, late_pct=100))):
    t0 = time.time()
    y, cw = _failures(dec, snr, frames, seed=int(snr * 100) + 3)
    y, cw = y[:12000], cw[:12000]
    prev = dec.set_pb_tuning(**tuning)
    for rep in range(2):
        _check(dec, y, cw, 3, snr, None)
    dec.set_pb_tuning(**prev)
    print(f"snr {snr}: {y.shape[0]} failing frames, tuning {tuning}: exact twice ({time.time() - t0:.0f} s)", flush=True)
