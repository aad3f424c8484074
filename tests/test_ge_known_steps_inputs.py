"""The crafted inputs of tests/test_gpu_ge_known_steps.py, checked on the host: every input is valid only if the C oracle's own
elimination shows the step pattern the case is named for (trivial steps, row exchanges, step of the first column exchange).
tests/ge_steps.py replays the elimination with the bookkeeping of the short cuts (profiles/ge_known/README.md); its reduced matrix and exchange list must be the
oracle's, so the counts describe the oracle's elimination."""
import numpy as np
import pytest

from oracle import c_oracle, np_oracle
from tests import ge_steps as S


@pytest.fixture(scope="module")
def natural(np_code):
    return np_oracle.make_frames(np_code.G, 2.5, 40, np.random.default_rng(7410))


def _replay_is_oracle(M, p, front=None):
    R, sw = c_oracle.gf2elim(M)
    assert R.shape[0] == 64 and not p["deficient"]
    assert sw == p["col_exchanges"]
    assert np.array_equal(R, p["reduced"])
    if front is not None:
        assert front[2] == sw


@pytest.mark.parametrize("name", sorted(S.EXPECT))
def test_crafted_order_has_its_pattern(np_code, natural, name):
    G, H = np.asarray(np_code.G), np.asarray(np_code.H)
    frames = S.crafted_frames(G, H, natural[0])[name]
    want = S.orders(G, H)[name]
    for y in frames:
        M, order = S.sorted_matrix(G, y)
        assert np.array_equal(order, want)                    # the magnitudes put the columns where the case wants them
        p = S.pattern(M)
        _replay_is_oracle(M, p, c_oracle.osd_front(G, y))
        S.check_expectation(name, p)


@pytest.mark.parametrize("t", S.GE_STEPS)
def test_exchange_matrix_has_its_pattern(t):
    M = S.ge_matrices()[t]
    p = S.pattern(M)
    _replay_is_oracle(M, p)
    S.check_ge_matrix(t, p)


def test_replay_is_the_oracle_on_natural_frames(np_code, natural):
    """and the step statistics of ordinary frames stay what the short cuts were sized for: a good share of trivial steps, column
    exchanges late."""
    G = np.asarray(np_code.G)
    triv, first = [], []
    for y in natural[0]:
        M, _ = S.sorted_matrix(G, y)
        p = S.pattern(M)
        _replay_is_oracle(M, p, c_oracle.osd_front(G, y))
        triv.append(len(p["trivial"]))
        first.append(p["col_exchanges"][0][0] if p["col_exchanges"] else 64)
    assert np.mean(triv) > 8 and np.median(first) >= 48
