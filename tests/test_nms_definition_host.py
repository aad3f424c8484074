"""CPU: the premises of tests/test_gpu_nms_definition.py on the C oracle -- the two graphs are forests of the stated shape, the
oracle's min-sum reaches the definition after diameter iterations and misses it after one fewer."""
import numpy as np
import pytest

from oracle import c_oracle
from tests import nms_definition as N

CASES = {"tree13": N.tree13, "forest70": N.forest70}


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_min_sum_is_exact_on_a_forest(name):
    H = CASES[name]()
    m, n = H.shape
    assert N.is_forest(H) and (H.sum(axis=0) == 1).any()
    if name == "tree13":
        assert sorted(set(H.sum(axis=1))) == [3, 4] and sorted(set(H.sum(axis=0))) == [1, 2, 3] and N.diameter(H) == 4
    else:
        assert n > 64 and n - m <= 16 and H.sum(axis=1).max() >= 9
    T = N.diameter(H)
    assert 1 < T <= 64
    book = N.codebook(H)
    assert len(book) == 1 << (n - m)
    y = N.frames(H, 200)
    for t in (T, T + 3):
        soft = c_oracle.nms(H, y, t, 1.0)
        hard, fail, _ = c_oracle.evaluate(H, soft, None)
        decided, diff, bound = N.check(H, y, soft, hard, fail, book)
        print(f"[definition] c_oracle NMS {name} T={t}: frames 200, decided {decided}, worst soft difference {diff:.3g} (bound {bound:.3g})")
        assert decided >= 150
    short = c_oracle.nms(H, y, T - 1, 1.0)
    assert (np.abs(short - N.exact_soft(book, y)[0]) > N.bound(y)).any()       # an iteration fewer is not enough


def test_a_cycle_is_no_forest():
    H = N.tree13()
    H[4, 0] = 1
    assert not N.is_forest(H)
