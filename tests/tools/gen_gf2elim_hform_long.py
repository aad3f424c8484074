"""Writes tests/golden/gf2elim_hform_long.npz: the reference's own GF(2) elimination (``fill_matrix_info.Code.gf2elim``, the
routine that DL_OSD_Testing_serial/ordered_statistics_decoding.py:222-257 repeats) on ascending-|x| column orders of long
parity-check matrices -- the pin for the 192-row, three-word elimination of ldpc_hosdl_front.

    python tests/tools/gen_gf2elim_hform_long.py <directory of the reference's fill_matrix_info.py>

Two sets (prefix g_ / r_):
  g_  32 orders of the (384,192) H of tests/golden/wimaxlike_N384_K192_P16_set0.alist, 16 at each of two SNRs
  r_  16 orders of a 192-row H of rank 150 on n = 300 (``hosdw_model.redundant(150, 300, "random_dense", 192, "first")``, stored as
      r_H): the routine deletes all-zero rows, here while more than 128 rows are left
Per set: x [F,n] f32 (the values whose magnitudes order the columns), order [F,n] i16 (stable ascending argsort of |x|),
swaps [F,S,2] i16 and nswaps [F] (the recorded column exchanges), M [F,m,ceil(k/8)] u8 (columns m..n-1 of the reduced matrix,
bits packed little-endian along the row).  Neither this tool's output nor any test reads the reference afterwards.
"""
import contextlib
import io
import os
import sys

sys.dont_write_bytecode = True

import numpy as np   # noqa: E402

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)

from oracle import np_oracle          # noqa: E402
from tests import hosdw_model as WM   # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
ALIST = os.path.join(GOLDEN, "wimaxlike_N384_K192_P16_set0.alist")


def eliminate(ref_code, H, x):
    n = H.shape[1]
    order = np.argsort(np.abs(x), axis=1, kind="stable")
    M_out, swaps, ns = [], [], []
    for f in range(len(x)):
        R, rec = ref_code.gf2elim(np.array(H[:, order[f]], dtype=np.int64))
        m = R.shape[0]
        assert np.array_equal(R[:, :m], np.eye(m, dtype=np.int64))
        M_out.append(np.packbits(R[:, m:].astype(np.uint8), axis=1, bitorder="little"))
        swaps.append(rec)
        ns.append(len(rec))
    S = max(max(ns), 1)
    sw = np.full((len(x), S, 2), -1, np.int16)
    for f, rec in enumerate(swaps):
        for t, (a, b) in enumerate(rec):
            sw[f, t] = (a, b)
    assert n < 32768
    return dict(x=x, order=order.astype(np.int16), swaps=sw, nswaps=np.array(ns, np.int16), M=np.stack(M_out))


def main():
    sys.path.insert(0, sys.argv[1])
    import fill_matrix_info as ref   # the reference's own module
    with contextlib.redirect_stdout(io.StringIO()):
        ref_code = ref.Code(ALIST)
    c = np_oracle.Code(ALIST)
    assert np.array_equal(np.asarray(ref_code.H), c.H)
    out = {}
    xs = []
    for i, snr in enumerate((1.5, 3.0)):
        xs.append(np.asarray(np_oracle.make_frames(c.G, snr, 16, np.random.default_rng(384192 + i))[0], np.float32))
    for key, v in eliminate(ref_code, c.H, np.concatenate(xs)).items():
        out["g_" + key] = v
    H, G = WM.redundant(150, 300, "random_dense", 192, "first")
    x = np.asarray(np_oracle.make_frames(G, 2.0, 16, np.random.default_rng(300150))[0], np.float32)
    for key, v in eliminate(ref_code, np.asarray(H), x).items():
        out["r_" + key] = v
    out["r_H"] = np.asarray(H, np.uint8)
    assert out["r_M"].shape[1] == 150 and out["g_M"].shape[1] == 192
    path = os.path.join(GOLDEN, "gf2elim_hform_long.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; exchanges g mean %.1f max %d, r mean %.1f max %d"
          % (out["g_nswaps"].mean(), out["g_nswaps"].max(), out["r_nswaps"].mean(), out["r_nswaps"].max()))


if __name__ == "__main__":
    main()
