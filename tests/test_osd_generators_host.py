"""CPU: the C oracle against the NumPy restatement on the generator zoo of tests/osd_generators.py, before the GPU tests
trust it there (until now the two were only pinned to each other on the CCSDS generator), and the premises of the zoo --
computed from the oracle's own outputs, so that no case passes by being empty.  Everything is compared exactly: integers
equal, metrics as uint32 bit patterns.

PB-OSD has no bit-deterministic NumPy form, so here the C oracle's PB search is held to invariants only.  The one about the
visit order (never worse than the best of the TEPs visited for certain) cannot name the order among equal reliability
sums, which the reference leaves to its list; on the grid cases, where most sums tie, it says little.  That the PB tie
rules are followed exactly rests on the comparison of the kernels with the C oracle (tests/test_gpu_osd_generators.py)."""
import itertools

import numpy as np
import pytest

from oracle import c_oracle, np_oracle
from tests import osd_generators as Z

F32 = np.float32
CASES = [(n, m) for n in Z.NAMES for m in Z.MODES]
FRAMES = 96                      # the frames of a case (tests/test_gpu_osd_generators.py runs the same ones)
FS_THRESHOLDS = [(0.1, 6.5, 30.0), (0.1, 14.5, 30.0), (0.02, 11.0, 18.0)]       # (beta, tau_e, tau_psc)
PB_SNRS = (1.0, 2.5)
PB3_HOST_FRAMES = {("zero_rows", "grid"): 8}    # a full scan of 43 745 TEPs per frame (0.1 s each in the C oracle): a sample here
# the NumPy conventional search at order 3 takes about a second per frame: one frame per generator and magnitude mode
ORDER3_FRAMES = {(n, m): 1 for n in Z.NAMES for m in Z.MODES}


_REF = {}


def ref(kind, c, n, *args):
    """One C-oracle result per (case, search, frames, parameters), shared by the tests and left unchanged."""
    key = (kind, c["name"], c["mode"], n) + args
    if key not in _REF:
        _REF[key] = getattr(c_oracle, kind)(c["G"], c["y"][:n], c["cw"][:n], *args)
    return _REF[key]


def bits(a):
    return np.asarray(a, dtype=F32).view(np.uint32)


def to_orig(perm, primed_bits):
    out = np.empty(128, dtype=np.int64)
    out[perm] = primed_bits
    return out


def check_matrix(name):
    """H with H G^T = 0 for G = [I | P'][:, pi^-1]: [P'^T | I] with its columns moved the same way."""
    H = np.empty((64, 128), np.int64)
    H[:, Z.pi(name)] = np.concatenate([Z.parity(name).T, np.eye(64, dtype=np.int64)], axis=1)
    return H


def test_rows_cost_is_the_per_row_loop():
    rng = np.random.default_rng(1)
    w = np.abs(rng.normal(1.0, 0.7, size=128)).astype(F32)
    disc = rng.integers(0, 2, size=(300, 128))
    disc[0], disc[1] = 0, 1
    got = np_oracle.weighted_distance_rows(disc, w, 64)
    want = np.array([np_oracle.weighted_distance(d, w) for d in disc], dtype=F32)
    assert np.array_equal(bits(got), bits(want))
    for n, k in ((128, 64), (121, 60), (96, 48), (40, 16), (24, 10), (9, 1)):      # tails of 0..7 bits, k != n / 2
        got = np_oracle.weighted_distance_rows(disc[:, :n], w[:n], k)
        want = np.array([np_oracle._weighted_distance_k(d, w[:n], k) for d in disc[:, :n]], dtype=F32)
        assert np.array_equal(bits(got), bits(want)), (n, k)


@pytest.mark.parametrize("name", Z.NAMES)
def test_generators_are_what_they_say(name):
    P, G = Z.parity(name), Z.generator(name)
    assert G.shape == (64, 128) and np.array_equal(G[:, Z.pi(name)], Z.systematic(name))
    assert not (check_matrix(name).dot(G.T) % 2).any()
    wt = P.sum(axis=1)
    if name == "zero_rows":
        assert np.flatnonzero(wt == 0).tolist() == list(Z.ZERO_ROWS)
    if name == "equal_rows":
        assert all(np.array_equal(P[2 * i], P[2 * i + 1]) for i in range(32))
        assert len(np.unique(P[list(Z.EQUAL_GROUP)], axis=0)) == 1 and len(np.unique(P, axis=0)) == 29
    if name == "ones_row":
        assert wt[0] == 64 and np.array_equal(P[32:63] ^ P[1:32], np.ones((31, 64), np.int64))
    if name == "identity":
        assert np.array_equal(P, np.eye(64, dtype=np.int64))
    if name == "sparse":
        assert wt.min() == 1 and wt.max() == 3
    if name == "low_bytes":
        assert not P[:, 16:].any() and wt.min() >= 1 and np.array_equal(np.sort(Z.pi(name)[Z.zero_columns(name)]), np.arange(80, 128))
    if name == "high_bytes":
        assert not P[:, :16].any() and wt.min() >= 1 and np.array_equal(np.sort(Z.pi(name)[Z.zero_columns(name)]), np.arange(16))
    if name == "rank_one":
        assert len(np.unique(P[wt > 0], axis=0)) == 1 and 8 <= (wt == 0).sum() <= 56


@pytest.mark.parametrize("name,mode", CASES)
def test_front_end(name, mode):
    c = Z.case(name, mode, FRAMES)
    H = check_matrix(name)
    eye = np.eye(64, dtype=np.int64)
    for f in range(FRAMES):
        perm, Gp = c["perm"][f], c["Gp"][f]
        assert np.array_equal(Gp[:, :64], eye), f
        assert np.array_equal(np.sort(perm), np.arange(128)), f
        back = np.empty((64, 128), np.int64)
        back[:, perm] = Gp                                     # row r of Gp in original bit order
        assert not (H.dot(back.T) % 2).any(), f                # ... is a codeword of G
    for f in range(6):
        yp, lp, Gp, perm, sw = np_oracle.swapped_info(c["y"][f], c["cw"][f], c["G"])
        permc, Gpc, swc = c_oracle.osd_front(c["G"], c["y"][f])
        assert np.array_equal(perm, permc) and np.array_equal(Gp, Gpc) and sw == swc, f
        assert np.array_equal(bits(yp), bits(c["yp"][f])), f


def test_direct_form_needs_no_front_end():
    for name, mode in Z.DIRECT:
        d = Z.direct(name, mode, True)
        assert (np.diff(np.abs(d["y"]), axis=1) <= 0).all()
        for f in range(len(d["y"])):
            perm, Gp, sw = c_oracle.osd_front(d["G"], d["y"][f])
            assert np.array_equal(perm, np.arange(128)) and not sw and np.array_equal(Gp, d["G"]), (name, f)
        u = Z.direct(name, mode, False)
        assert (np.diff(np.abs(u["y"][:, :64]), axis=1) > 0).any()


@pytest.fixture(scope="module")
def teps3():
    return np_oracle.tep_matrix(64, 3)


@pytest.mark.parametrize("name,mode", CASES)
def test_conventional_c_vs_numpy(name, mode, teps3):
    c = Z.case(name, mode, FRAMES)
    for order, frames in ((0, 4), (1, 4), (2, 4), (3, ORDER3_FRAMES[name, mode])):
        res = c_oracle.conv_osd(c["G"], c["y"][:frames], c["cw"][:frames], order)
        for f in range(frames):
            perm = c["perm"][f]
            r = np_oracle.convention_osd(c["yp"][f], c["cw"][f][perm], c["Gp"][f].astype(np.int64), order,
                                         teps=teps3 if order == 3 else None)
            assert r["best_index"] == res["best"][f] and bits(r["metric"]) == bits(res["metric"][f]), (order, f)
            assert np.array_equal(to_orig(perm, r["codeword"]), res["codeword"][f]), (order, f)
            assert r["teps_size"] == res["teps_size"] and r["correct"] == res["correct"][f], (order, f)


@pytest.mark.parametrize("name,mode", CASES)
def test_fs_c_vs_numpy(name, mode):
    c = Z.case(name, mode, FRAMES)
    frames = 4
    for order, (beta, tau_e, tau_psc) in itertools.product((1, 2), FS_THRESHOLDS[:2]):
        res = c_oracle.fs_osd(c["G"], c["y"][:frames], c["cw"][:frames], order, beta, tau_e, tau_psc)
        for f in range(frames):
            perm = c["perm"][f]
            o = np_oracle.fs_osd_frame(c["yp"][f], c["cw"][f][perm], c["Gp"][f].astype(np.int64), order, beta, tau_e, tau_psc)
            tag = (order, tau_e, f)
            assert o["num_teps"] == res["num_teps"][f], tag
            assert bits(o["metric_ref"]) == bits(res["metric_ref"][f]), tag
            assert np.array_equal(to_orig(perm, o["codeword_ref"]), res["codeword_ref"][f]), tag
            assert (o["codeword_hit"] is not None) == bool(res["hit"][f]), tag
            if res["hit"][f]:
                assert bits(o["metric_hit"]) == bits(res["metric_hit"][f]), tag
                assert np.array_equal(to_orig(perm, o["codeword_hit"]), res["codeword_hit"][f]), tag
            else:
                assert bits(res["metric_hit"][f]) == bits(res["metric_ref"][f]), tag
                assert np.array_equal(res["codeword_hit"][f], res["codeword_ref"][f]), tag


def _supports(order):
    return [s for w in range(1, order + 1) for s in itertools.combinations(range(64), w)]


SUPPORTS = {o: _supports(o) for o in (1, 2)}
TEPS = {o: np.array([[p in s for p in range(64)] for s in SUPPORTS[o]], dtype=np.int64) for o in (1, 2)}


def _surely_visited_min(yp, Gp, order, num_teps):
    """The smallest metric among the order-0 candidate and the TEPs that PB-OSD has visited for certain after
    ``num_teps - 1`` pops: the frontier pops in non-decreasing order of the reliability sum (a child never has a smaller
    sum than its parent on descending |y'|), so every TEP whose sum is strictly below the (num_teps - 1)-th smallest sum
    is among them, however the ties were ordered."""
    w = np.abs(yp)
    hard = np.where(yp > 0, 0, 1).astype(np.int64)
    sums = np.zeros(len(SUPPORTS[order]), F32)
    for i, s in enumerate(SUPPORTS[order]):
        acc = w[s[0]]
        for p in s[1:]:
            acc = F32(acc + w[p])
        sums[i] = acc
    pops = num_teps - 1
    E = np.zeros((1, 64), np.int64)
    if pops >= 1:
        sure = sums < np.sort(sums)[pops - 1]
        E = np.concatenate([E, TEPS[order][sure]])
    cand = ((E + hard[None, :64]) % 2).dot(Gp) % 2
    return np_oracle.weighted_distance_rows((cand + hard[None]) % 2, w, 64).min()


@pytest.mark.parametrize("name,mode", CASES)
def test_pb_invariants(name, mode):
    """np_oracle.pb_osd_frame is not bit-deterministic (its docstring), so the C oracle's PB-OSD is held to its own
    invariants on the zoo."""
    c = Z.case(name, mode, FRAMES)
    H = check_matrix(name)
    hard = np.where(c["yp"] > 0, 0, 1).astype(np.int64)
    for order, snr in itertools.product((1, 2, 3), PB_SNRS):
        n = PB3_HOST_FRAMES.get((name, mode), FRAMES) if order == 3 else FRAMES
        res = ref("pb_osd", c, n, order, snr)
        nmax = 1 + 64 + (2016 if order > 1 else 0) + (41664 if order > 2 else 0)
        assert not (H.dot(res["codeword"].T) % 2).any(), (order, snr)
        assert (res["num_teps"] <= nmax).all() and (res["num_teps"] >= 1).all()
        assert ((res["stop"] == 0) == (res["num_teps"] == nmax)).all()
        assert (res["best_index"] <= res["num_teps"]).all() and ((res["stop"] != 2) | (res["best_index"] == res["num_teps"])).all()
        for f in range(n):
            disc = (res["codeword"][f][c["perm"][f]] + hard[f]) % 2
            assert bits(np_oracle.weighted_distance(disc, np.abs(c["yp"][f]))) == bits(res["metric"][f]), (order, snr, f)
        if order <= 2:
            for f in range(0, FRAMES, 4):
                floor = _surely_visited_min(c["yp"][f], c["Gp"][f].astype(np.int64), order, int(res["num_teps"][f]))
                assert res["metric"][f] <= floor, (order, snr, f)


# ------------------------------------------------------------------------------------------------------ premises
@pytest.mark.parametrize("name", ["equal_rows", "rank_one", "zero_rows"])
def test_premise_first_minimum_decides(name):
    """grid mode: in at least a quarter of the frames two or more of the 65 order-1 TEPs attain the minimum metric."""
    c = Z.case(name, "grid", FRAMES)
    ties = int(Z.tie_frames(c).sum())
    s = Z.structure(c)
    print(f"{name}: {ties} of {FRAMES} frames tie at the order-1 minimum; zero rows {s['zero'].min()}-{s['zero'].max()}, "
          f"repeated rows {s['dup'].min()}-{s['dup'].max()}")
    assert 4 * ties >= FRAMES
    if name == "zero_rows":
        assert (s["zero"] == 8).all()
        assert (c["parity"][:, :8] == 0).any() and (c["parity"][:, 56:] == 0).any()     # at high and at low MRB positions
    if name == "equal_rows":
        assert (s["dup"] >= 6).all()
    if name == "rank_one":
        assert (s["kinds"] <= 2).all()


@pytest.mark.parametrize("name", ["low_bytes", "high_bytes"])
@pytest.mark.parametrize("mode", Z.MODES)
def test_premise_prefix(name, mode):
    """From P'' and y': low_bytes -- the prefix (MRB sum + parity bytes 0-1) of every TEP is its full metric; high_bytes --
    it is its MRB sum.  Checked on the metrics themselves for the 65 order-1 TEPs of a few frames."""
    c = Z.case(name, mode, FRAMES)
    assert Z.prefix_premise(c).all()
    E = np_oracle.tep_matrix(64, 1)
    for f in range(0, FRAMES, 12):
        yp, Gp = c["yp"][f], c["Gp"][f].astype(np.int64)
        hard = np.where(yp > 0, 0, 1).astype(np.int64)
        disc = (((E + hard[None, :64]) % 2).dot(Gp) % 2 + hard[None]) % 2
        w = np.abs(yp)
        full = np_oracle.weighted_distance_rows(disc, w, 64)
        cut = disc.copy()
        cut[:, 80:] = 0
        prefix = np_oracle.weighted_distance_rows(cut, w, 64)
        cut[:, 64:] = 0
        mrb = np_oracle.weighted_distance_rows(cut, w, 64)
        assert np.array_equal(bits(prefix), bits(full if name == "low_bytes" else mrb)), f
        assert name == "low_bytes" or (full > mrb).any()


def test_premises_across_the_zoo():
    """FS: hits and no hits; num_teps = 1 (order-0 stop); the lower-bound break after a class, which is num_teps = 1 + 64
    at order >= 2 and 1 + 64 + 2016 at order 3 (at order 1 / 2 those are the full scans); a stop strictly inside a class.
    PB: stop reasons 1 and 2, and 0 at order >= 2 (order 1 runs out of TEPs trivially); a grid frame beyond 64 TEPs (a
    search handed on under the 64-TEP budgets).  Conventional order 2: a frame with >= 5 full survivor batches of the
    rotation scan."""
    from tests.test_gpu_osd2_scan import stage1_model
    fs_hit = fs_nohit = 0
    inside, stops, handed = 0, set(), 0
    fs_counts = {(o, v): 0 for o in (1, 2, 3) for v in (1, 65, 2081)}
    pb_full = {1: 0, 2: 0, 3: 0}
    for name, mode in CASES:
        c = Z.case(name, mode, FRAMES)
        line = f"{name:13s}{mode:6s}"
        for order, (beta, tau_e, tau_psc) in itertools.product((1, 2, 3), FS_THRESHOLDS):
            r = c_oracle.fs_osd(c["G"], c["y"], c["cw"], order, beta, tau_e, tau_psc)
            fs_hit += int(r["hit"].sum())
            fs_nohit += int((~r["hit"]).sum())
            for v in (1, 65, 2081):
                fs_counts[order, v] += int((~r["hit"] & (r["num_teps"] == v)).sum())
            inside += int((r["hit"] & ~np.isin(r["num_teps"], (1, 65, 2081, 43745))).sum())
            if (tau_e, order) in ((6.5, 2), (14.5, 2)):
                line += f" FS2 tau_e {tau_e}: {int(r['hit'].sum())} hits;"
        for order, snr in itertools.product((1, 2, 3), PB_SNRS):
            n = PB3_HOST_FRAMES.get((name, mode), FRAMES) if order == 3 else FRAMES
            r = ref("pb_osd", c, n, order, snr)
            stops |= set(r["stop"].tolist())
            pb_full[order] += int((r["stop"] == 0).sum())
            if mode == "grid":
                handed += int((r["num_teps"] > 64).sum())
            if order == 3:
                line += f" PB3 {snr} dB stops {np.bincount(r['stop'], minlength=3).tolist()};"
        print(line)
    print("FS frames without a hit, (order, num_teps): count", fs_counts, "; hits inside a class", inside)
    print("PB frames that ran out of TEPs, by order", pb_full)
    assert fs_hit > 0 and fs_nohit > 0 and inside > 0
    assert fs_counts[2, 1] > 0 and fs_counts[2, 65] > 0 and fs_counts[3, 65] > 0 and fs_counts[3, 2081] > 0
    assert stops == {0, 1, 2} and pb_full[2] > 0 and pb_full[3] > 0 and handed > 0
    batches = {}
    for name in ("sparse", "identity"):
        c = Z.case(name, "grid", FRAMES)
        batches[name] = stage1_model(c["G"], c["y"][:8])[:, 0]
    print("full survivor batches, first 8 frames:", {k: v.tolist() for k, v in batches.items()})
    assert max(v.max() for v in batches.values()) >= 5
