"""-m gpu: ldpc_nms_decode against the definition of min-sum decoding -- no oracle in the loop.

On a cycle-free Tanner graph (tests/nms_definition.py) with alpha = 1, unit weights and T = the graph's diameter in check hops,
every soft value equals the difference of two constrained minima over all codewords, within n u sum |y_j|, and the hard
decisions are the ML codeword.  On the graphs of tests/nms_graphs.py the generic kernel is an odd function of its input: on
y (-1)^c for a codeword c the soft values change sign bit for bit and the hard decisions come out XOR c."""
import numpy as np
import pytest
import torch

from oracle import c_oracle
from tests import nms_definition as N
from tests import nms_graphs as Z
from tests import osd_definition as D
from tests.gpu_util import pack_np, to_dev, words_np

pytestmark = pytest.mark.gpu
CASES = {"tree13": N.tree13, "forest70": N.forest70}
_decs = {}


def forest_decoder(name):
    from short_ldpc_decoding_osd_amd import Code
    from short_ldpc_decoding_osd_amd.runtime import Decoder
    if name not in _decs:
        _decs[name] = Decoder(Code(H=CASES[name]()))
    return _decs[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_min_sum_on_a_forest_is_the_definition(name):
    from short_ldpc_decoding_osd_amd import _lib
    H = CASES[name]()
    m, n = H.shape
    assert N.is_forest(H)
    T = N.diameter(H)
    dec = forest_decoder(name)
    assert (dec.n, dec.k) == (n, n - m)
    book = N.codebook(H)
    y = N.frames(H, 200)
    # the premise, on the CPU oracle and never on the kernel: an iteration fewer misses the bound
    assert (np.abs(c_oracle.nms(H, y, T - 1, 1.0) - N.exact_soft(book, y)[0]) > N.bound(y)).any()
    yd = to_dev(y, dec)
    for kernel in (_lib.NMS_AUTO, _lib.NMS_GENERIC):
        res = dec.nms(yd, T, 1.0, kernel=kernel)
        torch.cuda.synchronize()
        hard = np.unpackbits(words_np(res["hard"]).view(np.uint8), axis=1, bitorder="little")[:, :n]
        decided, diff, bound = N.check(H, y, res["soft"].cpu().numpy(), hard, res["fail"].cpu().numpy(), book)
        print(f"[definition] kernel NMS {name} T={T} selection {kernel}: frames {len(y)}, decided {decided}, "
              f"worst soft difference {diff:.3g} (bound {bound:.3g})")
        assert decided >= 150


@pytest.mark.parametrize("name", ["array_121_60", "ldpc_96_48", "wimax_1056", "thin", "wide"])
def test_generic_kernel_is_an_odd_function(name):
    from short_ldpc_decoding_osd_amd import _lib
    from tests.test_gpu_nms_graphs import decoder
    dec = decoder(name)
    assert dec.nms_kernel == _lib.NMS_GENERIC
    G = np.asarray(Z.graph(name)[1], dtype=np.int64)
    y, _ = Z.frames(name, 2.0, 65, 17)
    assert (y != 0).all()
    alpha = np.array([0.7, 0.8, 0.65, 0.9, 0.75], np.float32)
    base = dec.nms(to_dev(y, dec), 5, alpha, 0.85, 1.2)
    torch.cuda.synchronize()
    soft, hard = base["soft"].cpu().numpy(), words_np(base["hard"])
    assert (soft != 0).all()                                  # a soft value of 0 is a hard 1 under either sign
    for seed in (1, 2):
        c = np.random.default_rng(seed).integers(0, 2, G.shape[0]).dot(G) % 2
        assert c.any()
        got = dec.nms(to_dev(D.flip(y, c), dec), 5, alpha, 0.85, 1.2)
        torch.cuda.synchronize()
        assert np.array_equal(D.flip(soft, c).view(np.uint32), got["soft"].cpu().numpy().view(np.uint32)), seed
        assert np.array_equal(hard ^ pack_np(c[None, :].astype(np.uint8)), words_np(got["hard"])), seed
        assert torch.equal(base["fail"], got["fail"]), seed
