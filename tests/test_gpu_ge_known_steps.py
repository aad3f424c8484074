"""-m gpu: the elimination of the OSD front end (ge_columns, csrc/ldpc_wave.h) on inputs built around its steps of known outcome,
bit for bit against the C oracle: `perm`, the rows of P' and the exchange count through ldpc_osd_front, the order-2 result
through ldpc_osd_search and ldpc_osd_decode (the fused kernel), one FS and one PB search, the H-form front end, and ldpc_osd_ge.

Two short cuts were built for these steps (profiles/ge_known/README.md): a row exchange takes the row-map entry of position i as
the constant 63 - i while no earlier exchange has moved a row there (kept), and a step whose pivot column is an untouched unit
vector skips the pivot search (measured slower, not kept).  The cases are the ones either short cut can get wrong, so they stay
whichever is in the kernel.  They come from tests/ge_steps.py; tests/test_ge_known_steps_inputs.py checks on the host that each
shows the step pattern it is named for, and the premises are asserted here again from the oracle's exchange records.

  units_first / units_last        64 trivial steps / none
  alternating                     unit and dense columns in turn: trivial steps and stale unit columns mixed
  units_descending                e_63 ... e_0: 32 row exchanges, every one with a known map entry (a reversal exchanges each pair
                                  once: no order makes all 64 steps exchange, the last step never can)
  units_rotated                   e_1 ... e_63, e_0: 63 row exchanges, `moved` fills, only step 0 has a known entry
  units_ascending                 no row exchange at all
  stale_unit                      a dense column takes row k, then e_k follows: no longer a unit column when its step comes
  first_exchange_31/32/47/63      the first column exchange at that step, unit columns behind it
  ldpc_osd_ge matrices            the first exchange at step 0, 1, 31, 32, 47, 63 -- steps 0 and 1 need a zero / a repeated
                                  column, which G of the CCSDS code does not have, so these go through ldpc_osd_ge -- each with a
                                  second exchange at step 63 that takes its column from the parity half
  all_equal, all_zero, one_flt_max, denormals   the edge sets of tests/test_gpu_osd_trim.py, built again here"""
import numpy as np
import pytest
import torch

from oracle import c_oracle, np_oracle
from tests import ge_steps as S
from tests import osd_generators as Z
from tests.gpu_util import pack_np, to_dev, words_np
from tests.test_gpu_osd_generators import check_fs, check_pb, fs_run, pb_run

pytestmark = pytest.mark.gpu
F32 = np.float32
FLT_MAX = np.finfo(F32).max
_CACHE = {}


@pytest.fixture(scope="module")
def dec():
    from short_ldpc_decoding_osd_amd import Code
    from short_ldpc_decoding_osd_amd.runtime import Decoder
    return Decoder(Code())


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def natural(dec):
    """300 frames at 2.5 dB with the oracle's front end and order-2 result: computed once, shared, left unchanged."""
    if "natural" not in _CACHE:
        y, cw = np_oracle.make_frames(dec.code.G, 2.5, 300, np.random.default_rng(7401))
        _CACHE["natural"] = (y, cw, Z.front(dec.code.G, y), c_oracle.conv_osd(dec.code.G, y, cw, 2))
    return _CACHE["natural"]


def check_front(dec, yd, front):
    perm, Gp, ns = front
    dperm, dparity, dns = dec.osd_front(yd)
    torch.cuda.synchronize()
    assert np.array_equal(dperm.cpu().numpy().astype(np.int32), perm)
    assert np.array_equal(words_np(dparity), Z.pack_rows(Gp[:, :, 64:]))
    assert np.array_equal(dns.cpu().numpy(), ns)
    return dperm, dparity


def check_result(out, r, n, tag):
    assert np.array_equal(out["best"].cpu().numpy(), r["best"][:n]), tag
    assert np.array_equal(words_np(out["cw"]), pack_np(r["codeword"][:n])), tag
    assert np.array_equal(u32(out["metric"].cpu().numpy()), u32(r["metric"][:n])), tag
    assert (out["ntep"].cpu().numpy() == 2081).all(), tag


def check_both_routes(dec, y, front, r, tag):
    """ldpc_osd_front against the oracle's front end, then front + ldpc_osd_search and ldpc_osd_decode (osd_fused2r_kernel, which
    runs the front end itself) against the oracle's order-2 result."""
    n = len(y)
    yd = to_dev(y, dec)
    dperm, dparity = check_front(dec, yd, tuple(a[:n] for a in front))
    scan = dec.osd_search(yd, dperm, dparity, dec.osd_params(2))
    fused = dec.osd_decode(yd, 2)
    torch.cuda.synchronize()
    check_result(scan, r, n, tag + ("search",))
    check_result(fused, r, n, tag + ("fused",))


@pytest.mark.parametrize("frames", [1, 2, 65, 300])
def test_frame_counts(dec, frames):
    y, cw, front, r = natural(dec)
    check_both_routes(dec, np.array(y[:frames]), front, r, (frames,))


# -------------------------------------------------------------------------------------------------------- crafted cases
def case_sets(dec):
    if "cases" in _CACHE:
        return _CACHE["cases"]
    G, H = np.asarray(dec.code.G), np.asarray(dec.code.H)
    y, cw, _, _ = natural(dec)
    sets = {name: (ys, cw[:len(ys)]) for name, ys in S.crafted_frames(G, H, y).items()}
    rng = np.random.default_rng(7402)
    sign = np.where(np.signbit(y), F32(-1.0), F32(1.0))
    sets["all_equal"] = (sign[:4] * F32(1.0), cw[:4])
    sets["all_zero"] = (np.concatenate([np.zeros((1, 128), F32), -np.zeros((1, 128), F32), (sign[:2] * F32(0.0))]), cw[:4])
    big = (y[:8] * F32(1e-3)).astype(F32)
    for f in range(8):
        big[f, (0, 63, 64, 127, 17, 90, 5, 100)[f]] = FLT_MAX if f % 2 else -FLT_MAX
    sets["one_flt_max"] = (big, cw[:8])
    den = rng.integers(1, 40, size=(8, 128)).astype(np.uint32).view(F32)             # 1..39 units of 2^-149, many ties
    sets["denormals"] = ((sign[:8] * den).astype(F32), cw[:8])
    out = {}
    for name, (ys, cs) in sets.items():
        ys = np.ascontiguousarray(ys, dtype=F32)
        out[name] = (ys, cs, Z.front(G, ys), c_oracle.conv_osd(G, ys, cs, 2))
    _CACHE["cases"] = out
    return out


EDGES = ("all_equal", "all_zero", "one_flt_max", "denormals")


@pytest.mark.parametrize("name", sorted(S.EXPECT) + list(EDGES))
def test_crafted_cases(dec, name):
    G = np.asarray(dec.code.G)
    y, cw, front, r = case_sets(dec)[name]
    # the premises, from the oracle and the inputs alone
    if name in S.EXPECT:
        for row in y:
            M, _ = S.sorted_matrix(G, row)
            p = S.pattern(M)
            assert p["col_exchanges"] == c_oracle.osd_front(G, row)[2]
            S.check_expectation(name, p)
    elif name == "all_equal":
        assert (np.abs(y) == 1.0).all()
    elif name == "all_zero":
        assert (y == 0).all() and np.signbit(y).any() and not np.signbit(y).all()
    elif name == "one_flt_max":
        assert ((np.abs(y) == FLT_MAX).sum(axis=1) == 1).all() and np.isfinite(r["metric"]).all()
    elif name == "denormals":
        assert (np.abs(y) < np.finfo(F32).tiny).all() and (y != 0).all()
    check_both_routes(dec, y, front, r, (name,))


def _rows_packed(M):
    return np.packbits(M.astype(np.uint8), axis=2, bitorder="little").view(np.uint64).reshape(M.shape[0], 64, 2)


def test_exchange_steps_through_osd_ge(dec):
    """First column exchange at step 0, 1, 31, 32, 47 and 63, unit columns behind it, a second exchange from the parity half."""
    mats = S.ge_matrices()
    M = np.stack([mats[t] for t in S.GE_STEPS])
    red, swaps, ns = dec.osd_ge(to_dev(_rows_packed(M).view(np.int64), dec))
    torch.cuda.synchronize()
    red, sw, ns = words_np(red).reshape(-1, 64, 2), swaps.cpu().numpy(), ns.cpu().numpy()
    for i, t in enumerate(S.GE_STEPS):
        p = S.pattern(M[i])
        S.check_ge_matrix(t, p)
        R, rsw = c_oracle.gf2elim(M[i])
        assert rsw == p["col_exchanges"] and ns[i] == len(rsw), t
        assert [tuple(int(v) for v in q) for q in sw[i, :ns[i]]] == rsw, t
        assert np.array_equal(red[i], _rows_packed(R[None])[0]), t


# -------------------------------------------------------------------------------------------------------- FS, PB, H form
def _mixed64(dec):
    """64 frames: three of every crafted order and natural ones to fill."""
    sets = case_sets(dec)
    y, cw, _, _ = natural(dec)
    ys = np.concatenate([sets[n][0] for n in sorted(S.EXPECT)] + [y])[:64]
    cs = np.concatenate([sets[n][1] for n in sorted(S.EXPECT)] + [cw])[:64]
    return np.ascontiguousarray(ys), cs


def test_fs_and_pb_search(dec):
    G = dec.code.G
    y, cw = _mixed64(dec)
    yd = to_dev(y, dec)
    dperm, dparity = check_front(dec, yd, Z.front(G, y))
    th = (0.1, 6.5, 30.0)
    check_fs(fs_run(dec, (yd, dperm, dparity), 2, th, 1), c_oracle.fs_osd(G, y, cw, 2, *th), 1, ("fs",))
    out, aux = pb_run(dec, (yd, dperm, dparity), 2, 2.5, {})
    check_pb(out, aux, c_oracle.pb_osd(G, y, cw, 2, 2.5), ("pb",))


def test_hform_front(dec):
    """ldpc_hosd_front at 64 frames against the oracle's elimination of H in ascending order (hosd_identify_mrb on
    c_oracle.gf2elim).  H has no unit column (column weights 3 and 5): every step searches its pivot; the row exchanges are the
    same code as in the G form."""
    H = np.asarray(dec.code.H)
    assert not (H.sum(axis=0) == 1).any()
    y, _ = _mixed64(dec)
    lri, uidx, M, ns = (t.cpu().numpy() for t in dec.hosd_front(to_dev(y, dec)))
    Mb = np.unpackbits(M.view(np.uint8).reshape(-1, 64, 8), axis=2, bitorder="little")
    for f, row in enumerate(y):
        order = np_oracle.hosd_reorder(row)
        R, sw = c_oracle.gf2elim(H[:, order])
        idx = np.arange(128)
        for a, b in sw:
            idx[a], idx[b] = idx[b], idx[a]
        srt = np.argsort(idx[64:], kind="stable")
        assert np.array_equal(lri[f], order), f
        assert ns[f] == len(sw), f
        assert np.array_equal(uidx[f], np.concatenate([idx[:64], idx[64:][srt]])), f
        assert np.array_equal(Mb[f], R[:, 64:][:, srt]), f
