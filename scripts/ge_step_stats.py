#!/usr/bin/env python3
"""Step statistics of the OSD front end's elimination on real NMS syndrome failures, counted on the host (no GPU):
frames as bench.py's CPU baseline draws them (np_oracle.make_frames, seed 20241020, 2.5 dB), NMS-10 by the C oracle, and for
every syndrome failure the step pattern of tests/ge_steps.py, whose elimination is checked against the C oracle's.

    python scripts/ge_step_stats.py [frames]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import c_oracle, np_oracle                                            # noqa: E402
from short_ldpc_decoding_osd_amd.weights import STORED_NMS1_WEIGHT, softplus32    # noqa: E402
from tests import ge_steps as S                                                    # noqa: E402

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 8000
code = np_oracle.Code(os.path.join(os.path.dirname(__file__), "..", "short_ldpc_decoding_osd_amd", "data", "CCSDS_ldpc_n128_k64.alist"))
G, H = np.asarray(code.G), np.asarray(code.H)
y, cw = np_oracle.make_frames(G, 2.5, frames, np.random.default_rng(20241020))
soft = c_oracle.nms(H, y, 10, float(softplus32(STORED_NMS1_WEIGHT)))
fail = np.flatnonzero(c_oracle.evaluate(H, soft, cw)[1])
steps = triv = stale = barred = rex = known = 0
first = []
for f in fail:
    M, _ = S.sorted_matrix(G, y[f])
    p = S.pattern(M)
    assert p["col_exchanges"] == c_oracle.osd_front(G, y[f])[2]
    steps += 64
    triv += len(p["trivial"]); stale += len(p["stale"]); barred += len(p["barred"])
    rex += len(p["row_exchange"]); known += len(p["known"])
    first.append(p["col_exchanges"][0][0] if p["col_exchanges"] else 64)
first = np.array(first)
print(f"frames {frames}, syndrome failures {len(fail)} ({len(fail) / frames:.4f})")
print(f"trivial steps        {triv / steps:.4f} of the steps ({triv / len(fail):.2f} per frame)")
print(f"stale notes          {stale / steps:.4f}   barred by an earlier column exchange {barred / steps:.4f}")
print(f"row exchanges        {rex / steps:.4f} of the steps ({rex / len(fail):.2f} per frame), map entry known in {known / max(rex, 1):.4f} of them")
print(f"column exchange      {np.mean(first < 64):.4f} of the frames; first at step: median {np.median(first[first < 64]):.0f}, "
      f"before step 48 in {np.mean(first < 48):.4f} of the frames")
