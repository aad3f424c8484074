"""CPU: the definition checkers of tests/osd_definition.py reject every mutant of a correct result, and the CPU models (the C
oracle, np_oracle.hosd_frame, the family models) satisfy the definitions on the codes and input kinds that
tests/test_gpu_osd_definition.py puts before the kernels."""
import numpy as np
import pytest

from oracle import c_oracle, np_oracle
from tests import osd_adversary, osdx_fs_model, osdx_model, osdx_pb_model
from tests import osd_definition as D
from tests import osd_definition_cases as C
from tests import osd_family as OF


# ---------------------------------------------------------------------------------------------------------------------
# sensitivity: a checker that accepts a mutant is a bug
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def correct():
    """CCSDS, 40 frames at 1.0 dB: the C oracle's front end and order-2 result of each, accepted by the checkers."""
    H, G = osdx_model.graph("ccsds")
    y, _ = osdx_model.frames("ccsds", 1.0, 40, 1)
    fronts = [c_oracle.osd_front(G, row) for row in y]
    conv = c_oracle.conv_osd(G, y, None, 2)
    frames = []
    for f, (perm, Gp, sw) in enumerate(fronts):
        D.front_g(H, y[f], perm, Gp[:, 64:], len(sw))
        frames.append(D.GFrame(H, y[f], perm, Gp[:, 64:]))
        D.search(frames[f], 2, conv["codeword"][f], conv["metric"][f], conv["teps_size"])
    return dict(H=H, G=G, y=y, fronts=fronts, conv=conv, frames=frames)


def rejected(criteria, call, *args, **kw):
    with pytest.raises(D.Violation) as e:
        call(*args, **kw)
    assert e.value.criterion in criteria, (e.value.criterion, str(e.value))


def systematic_on(G, info):
    """The generator of the code of G that is the identity on the columns ``info`` (an information set, in this order), by
    Gauss-Jordan elimination -- the test's own, the checkers hold none."""
    M = np.array(G, dtype=np.int64) % 2
    for r, c in enumerate(info):
        piv = r + int(np.flatnonzero(M[r:, c])[0])
        M[[r, piv]] = M[[piv, r]]
        hit = np.flatnonzero(M[:, c])
        hit = hit[hit != r]
        M[hit] ^= M[r]
    return M


def test_front_mutants_are_rejected(correct):
    H, G, y = correct["H"], correct["G"], correct["y"]
    k = 64
    swapped = 0
    for f, (perm, Gp, sw) in enumerate(correct["fronts"]):
        P = Gp[:, k:].copy()
        rng = np.random.default_rng(f)
        # two MRB entries swapped: alone, and with their rows of P'
        i, j = sorted(rng.choice(k, 2, replace=False))
        p2 = perm.copy()
        p2[[i, j]] = p2[[j, i]]
        rejected("b", D.front_g, H, y[f], p2, P)
        P2 = P.copy()
        P2[[i, j]] = P2[[j, i]]
        rejected("b", D.front_g, H, y[f], p2, P2)
        # one bit of P' flipped
        P2 = P.copy()
        P2[rng.integers(k), rng.integers(k)] ^= 1
        rejected("c", D.front_g, H, y[f], perm, P2)
        # the parity part out of order: two entries and their columns of P' exchanged, every row is still a codeword
        i, j = sorted(rng.choice(k, 2, replace=False))
        p2, P2 = perm.copy(), P.copy()
        p2[[k + i, k + j]] = p2[[k + j, k + i]]
        P2[:, [i, j]] = P2[:, [j, i]]
        rejected("b", D.front_g, H, y[f], p2, P2)
        # a valid information set that is not the greedy one: MRB position r leaves for a parity position c that depends on
        # it, so a more reliable column that depends on the basis stays in the parity part; P' recomputed for that set
        r, c = np.argwhere(P == 1)[rng.integers(int(P.sum()))]
        rho = D.rank_desc(y[f])[0]
        info = np.array(sorted(set(perm[:k].tolist()) - {int(perm[r])} | {int(perm[k + c])}, key=lambda i: rho[i]))
        rest = np.array(sorted(set(range(128)) - set(info.tolist()), key=lambda i: rho[i]))
        p2 = np.concatenate([info, rest])
        Gs = systematic_on(G, info)[:, p2]
        assert np.array_equal(Gs[:, :k], np.eye(k, dtype=np.int64))
        rejected("d", D.front_g, H, y[f], p2, Gs[:, k:])
        # nswaps: zero where columns were exchanged, non-zero where none was
        rejected(("nswaps",), D.front_g, H, y[f], perm, P, 0 if sw else 2)
        swapped += bool(sw)
    assert 0 < swapped < len(y)                               # premise: frames with and without an exchange


def test_search_mutants_are_rejected(correct):
    y, conv = correct["y"], correct["conv"]
    n = 128
    g = D.gamma(n)
    second = outside = 0
    for f, fr in enumerate(correct["frames"]):
        cw, metric = conv["codeword"][f], conv["metric"][f]
        # the metric off by 4 gamma, either way
        rejected(("metric",), D.search, fr, 2, cw, np.float32(metric * (1 + 4 * g)), 2081)
        rejected(("metric",), D.search, fr, 2, cw, np.float32(metric * (1 - 4 * g)), 2081)
        rejected(("ntep",), D.search, fr, 2, cw, metric, 2080)
        # no codeword
        bad = cw.copy()
        bad[7] ^= 1
        rejected(("codeword",), D.search, fr, 2, bad, metric, 2081)
        # the second best of the set, where it is further away than the bound
        E = D.patterns(64, 2)
        m64 = fr.order_metrics(2)
        a, b = np.argsort(m64)[:2]
        if m64[a] > 0 and (m64[b] - m64[a]) / m64[a] > D.gap_bound(n):
            rejected(("optimum", "argmin"), D.search, fr, 2, fr.codeword(E[b]), np.float32(m64[b]), 2081)
            second += 1
        # a codeword outside the order-p set: the order-2 winner with two flips, held to order 1
        e = cw[fr.perm][:64] ^ fr.hard[:64]
        if e.sum() == 2:
            rejected(("member",), D.search, fr, 1, cw, metric, 65)
            rejected(("member",), D.pruned, fr, 1, cw, metric)
            outside += 1
    assert second >= 20 and outside >= 3                     # premise: the mutants existed


def test_the_hard_decision_rule_at_zero_is_held(correct):
    """y >= 0 read as a 0 on frames that hold exact zeros in the MRB: the mutant's candidates are centred on other hard
    decisions, so its winner lies outside the order-p set of the definition."""
    H, G = correct["H"], correct["G"]
    y = C.kinds("ccsds")["zeros"][::3]                       # the frames with more than n - k zeros
    caught = 0
    for row in y:
        perm, Gp, _ = c_oracle.osd_front(G, row)
        fr = D.GFrame(H, row, perm, Gp[:, 64:])
        assert (row[perm[:64]] == 0).any()                    # premise: a zero in the MRB
        mutant = D.GFrame(H, row, perm, Gp[:, 64:])
        mutant.hard = np.where(row[perm] >= 0, 0, 1).astype(np.int64)
        m = mutant.metrics(D.patterns(64, 1))
        b = int(np.argmin(m))
        rejected(("member",), D.search, fr, 1, mutant.codeword(D.patterns(64, 1)[b]), np.float32(m[b]), 65, exact=True)
        caught += 1
    assert caught >= 3


def test_h_form_mutants_are_rejected():
    H, G = osdx_model.graph("ccsds")
    y, _ = osdx_model.frames("ccsds", 1.0, 12, 2)
    swapped = 0
    for f, row in enumerate(y):
        r = np_oracle.hosd_frame(row, row, None, H, [])
        lri, uidx, M = r["lri"], r["uidx"], r["M"]
        D.front_h(G, row, lri, uidx, M)
        rng = np.random.default_rng(f)
        m = 64
        l2 = lri.copy()
        l2[[3, 4]] = l2[[4, 3]]
        rejected(("sort",), D.front_h, G, row, l2, uidx, M)
        i, j = sorted(rng.choice(64, 2, replace=False))
        u2, M2 = uidx.copy(), M.copy()
        u2[[m + i, m + j]] = u2[[m + j, m + i]]
        M2[:, [i, j]] = M2[:, [j, i]]
        rejected("b", D.front_h, G, row, lri, u2, M2)
        M2 = M.copy()
        M2[rng.integers(64), rng.integers(64)] ^= 1
        rejected("c", D.front_h, G, row, lri, uidx, M2)
        # not the least reliable basis: LRB position r leaves for an MRB position that depends on it
        rr, c = np.argwhere(M == 1)[rng.integers(int(M.sum()))]
        lrb = [int(v) for v in uidx[:m]]
        lrb[rr] = int(uidx[m + c])
        mrb = sorted(set(range(128)) - set(lrb))
        u2 = np.array(lrb + mrb)
        Hs = systematic_on(H, lri[u2][:m])[:, lri[u2]]
        rejected("d", D.front_h, G, row, lri, u2, Hs[:, m:])
        swapped += bool(r["swaps"])
    assert swapped


# ---------------------------------------------------------------------------------------------------------------------
# the models against the definition
# ---------------------------------------------------------------------------------------------------------------------
def test_c_oracle_on_ccsds_satisfies_the_definitions():
    H, G = osdx_model.graph("ccsds")
    tallies = {}
    for kind, y in C.kinds("ccsds").items():
        fronts = [c_oracle.osd_front(G, row) for row in y]
        ns = np.array([len(s[2]) for s in fronts])
        if kind == "natural":
            assert ns.max() >= 3
        frames = []
        for f, (perm, Gp, sw) in enumerate(fronts):
            D.front_g(H, y[f], perm, Gp[:, 64:], len(sw))
            frames.append(D.GFrame(H, y[f], perm, Gp[:, 64:]))
        for order in (0, 1, 2):
            conv = c_oracle.conv_osd(G, y, None, order)
            t = tallies.setdefault(order, D.Tally(f"c_oracle ccsds order {order}"))
            for f, fr in enumerate(frames):
                t.add(D.search(fr, order, conv["codeword"][f], conv["metric"][f], conv["teps_size"], exact=kind in C.EXACT))
        fs = c_oracle.fs_osd(G, y, None, 2)
        pb = c_oracle.pb_osd(G, y, None, 2, 1.0)
        for f, fr in enumerate(frames):
            D.pruned(fr, 2, fs["codeword_ref"][f], fs["metric_ref"][f])
            D.pruned(fr, 2, fs["codeword_hit"][f], fs["metric_hit"][f])
            D.pruned(fr, 2, pb["codeword"][f], pb["metric"][f], full=pb["stop"][f] == 0)
    for t in tallies.values():
        t.done()


@pytest.mark.parametrize("case", C.G_CASES, ids=C.case_id)
def test_family_models_satisfy_the_definitions(case):
    fam = OF.FAMILIES[case[0]]
    G = C.graph(case[1])[1]

    def front_fn(y):
        return OF.front_oracle(G, y, fam)

    def scan_fn(y, order, front):
        with np.errstate(over="ignore"):
            return [("model", osdx_model.scan_oracle(G, y, order, front))]
    C.check_g_case(case, front_fn, scan_fn, "model")


PB_SETS = [("array_121_60", 0), ("short", 0), ("short", 1), ("ccsds", 0), ("ldpc_96_48", 1)]    # the first four hold full scans


def test_fs_and_pb_models_satisfy_the_inequalities():
    """osdx_fs_model / osdx_pb_model serve every family: their results (FS on ldpc_96_48, PB on four codes) are codewords of the order-p set with a
    true metric, not below the optimum; a PB frame that no rule stopped reaches it."""
    H, G = osdx_model.graph("ldpc_96_48")
    y, _, front, batch, order, sets, results = osdx_fs_model.parity_case("ldpc_96_48")
    frames = C.check_fronts(OF.OSDX, H, 48, y[:48], front[0][:48], front[1][:48], front[2][:48])
    for res in results:
        for key in ("ref", "hit"):
            cw = C.unpack_cw(res["cw_" + key], 96)
            for f, fr in enumerate(frames):
                D.pruned(fr, order, cw[f], res["metric_" + key][f])
    full = 0
    for name, i in PB_SETS:
        H, G = osdx_model.graph(name)
        k, n = G.shape
        y, _, front, order, _, res = osdx_pb_model.case(name, i)
        frames = C.check_fronts(OF.OSDX, H, k, y, front[0], front[1], front[2])
        cw = C.unpack_cw(res["cw"], n)
        for f, fr in enumerate(frames):
            stop0 = res["aux"][f, 3] == 0
            D.pruned(fr, order, cw[f], res["metric"][f], full=stop0)
            full += int(stop0)
    assert full >= 5                                          # premise: full scans are among the frames


@pytest.mark.parametrize("name,which", [("ccsds", "hosd"), ("ldpc_96_48", "hosdx"), ("array_121_60", "hosdw"), ("s200_100", "hosdl")])
def test_h_form_models_satisfy_the_definitions(name, which):
    """np_oracle.hosd_frame, hosdx_model.hosdx_frame and hosdw_model.hosdw_frame (the model of ldpc_hosdl_* as well) on natural, dependent-sets-first, quantised and zero frames:
    the front-end criteria, and the block scan on the blocks of all patterns of weight 0, 1 and 2."""
    from tests import hosdw_model, hosdx_model
    H, G = C.graph(name)
    k, n = G.shape
    assert (H.shape[0] > n - k) == (name == "array_121_60")   # 66 rows of rank 61
    model = dict(hosd=np_oracle.hosd_frame, hosdx=hosdx_model.hosdx_frame, hosdw=hosdw_model.hosdw_frame,
                 hosdl=hosdw_model.hosdw_frame)[which]
    nat = np_oracle.make_frames(G, 1.0, 12, np.random.default_rng(3))[0]
    sets = dict(natural=nat, dependent=osd_adversary.h_form_frames(G, H, nat[:4], 5),
                ties=osd_adversary.h_form_frames(G, H, nat[4:8], 6, ties=True), quantised=C.quantise(nat),
                zeros=C.with_zeros(C.quantise(nat[:6]), k, 8))
    E = D.patterns(k, 2)
    w = E.sum(axis=1)
    blocks = [np.asarray(E[w == t], dtype=np.int64) for t in (0, 1, 2)]
    swaps = 0
    for kind, ys in sets.items():
        for row in ys:
            r = model(row, row, None, H, blocks)
            D.front_h(G, row, r["lri"], r["uidx"], r["M"])
            fr = D.HFrame(G, row, row, r["lri"], r["uidx"], r["M"])
            assert not (H.dot(r["codeword"]) % 2).any()
            D.block_scan(fr, blocks, r["block_min"], r["metric"], r["codeword"], exact=kind in ("quantised", "zeros"))
            swaps = max(swaps, len(r["swaps"]))
    assert swaps >= 3


@pytest.mark.parametrize("famname,code", C.PRUNED)
def test_pruned_inputs_of_the_gpu_test(famname, code):
    """The FS / PB inputs of tests/test_gpu_osd_definition.py on the models: the inequalities on the family's own code, and
    on the shared (128,64) set the premise that at least 5 frames are full scans, which reach the optimum."""
    fam = OF.FAMILIES[famname]
    H, G = C.graph(code)
    k, n = G.shape
    y = C.pruned_frames(code)
    front = OF.front_oracle(G, y, fam)
    frames = C.check_fronts(fam, H, k, y, front[0], front[1], front[2])
    res = osdx_pb_model.pb(y, front[0], front[3], 2, C.PB_SNR_DB)
    C.check_pruned(frames, n, 2, res, res["aux"][:, 3] == 0)
    batch = osdx_fs_model.Batch(y, front[0], front[3])
    for s in C.FS_SETS:
        r = batch.fs(2, *s)
        for key in ("ref", "hit"):
            C.check_pruned(frames, n, 2, dict(cw=r["cw_" + key], metric=r["metric_" + key]))
    H, G = C.graph("ccsds")
    y, _, _, order, snr_db, res = osdx_pb_model.case(*C.PB_FULL)
    assert (order, snr_db) == (2, C.PB_SNR_DB)
    front = OF.front_oracle(G, y, fam)
    frames = C.check_fronts(fam, H, 64, y, front[0], front[1], front[2])
    assert C.check_pruned(frames, 128, 2, res, res["aux"][:, 3] == 0) >= 5
