"""-m gpu: the form bench.py times, against the C oracle on every branch.  bench.py's timed region replays ONE captured HIP
graph in which the distinct batches run as BatchPipeline.run() chains on parallel capture streams that fork from and join
into a side stream, for up to eight rotations per launch.  Kernels of different batches then overlap: they share the
context, each chain has the workspace of its own capture stream, and the PB-OSD control words are cleared inside the graph.

``captured_rotation`` restates run_rank's rotation (a closure that cannot be imported).  A case captures it, fills every
output buffer of every pipe with sentinels, replays, and compares ALL pipes with the oracle of tests/pipeline_oracle.py:
soft / hard / fail, count and index, cw / metric / best / ntep, the PB aux columns, perm / parity where the pipe keeps
them, sentinels from row ``count`` on, and the eight counters (rotations x one step).  Then three replays with no
synchronisation in between, and one replay after batches 0 and 2 changed places in the input buffers.  The cases: every
workload and OSD route on four branches; the graph shapes from one chain to 4 branches x 8 rotations and five batches on
four branches; conventional order 2 at an SNR at which every batch has more failures than the front end's grid, so that
the persistent front kernel makes a second trip while the other branches run.  One test tampers with the outputs of a
passing case to show that the checker notices one bit in any buffer.

Wall time on one MI355X: 12 s for the file's 23 cases, the oracle included; the slowest case takes 3.3 s
(test_front_end_second_trip_beside_other_branches[front+search], which computes the oracle of the 1.0 dB batches), the first
case 2.8 s (the oracle of the 2.5 dB batches), every other case less than 1 s."""
import pytest
import torch

from tests import pipeline_oracle as PO

pytestmark = pytest.mark.gpu
SNR, B = 2.5, 12000
# Conventional order 2 with every failure list longer than front_grid() (csrc/ldpc_internal.h: 32 workgroups per CU, 8192
# on the 256 CUs of an MI355X): 1.0 dB and the smallest batch, in multiples of 1000, at which the C oracle lists more than
# 8192 failures in each of the four batches -- 8376, 8318, 8250 and 8299 of 10 000 (of 9000: 7526, 7499, 7440, 7466).
LOW_SNR, LOW_B = 1.0, 10000


@pytest.fixture(scope="module")
def dec():
    from short_ldpc_decoding_osd_amd import Code
    from short_ldpc_decoding_osd_amd.runtime import Decoder
    return Decoder(Code())


class Case:
    """Pipes over the batches 0 .. nb - 1 and the captured rotation, built as bench.py builds them."""

    def __init__(self, dec, name, keep_front, nbr, rpg, nb=4, snr=SNR, frames=B):
        from short_ldpc_decoding_osd_amd.pipeline import BatchPipeline
        self.dec, self.rpg = dec, rpg
        self.order, self.algo = PO.workload(name)
        self.batches = [PO.batch(dec, snr, frames, i) for i in range(nb)]
        PO.prepare(dec, self.batches, self.order, self.algo, keep_front)
        self.pipes = [BatchPipeline(dec, frames, PO.T, PO.ALPHA, osd_order=self.order, osd_algo=self.algo, snr_db=snr,
                                    keep_front=keep_front).bind(o["y"].clone(), o["labels"].clone()) for o in self.batches]
        torch.cuda.synchronize()
        self.graph, self.streams = captured_rotation(dec, self.pipes, nbr, rpg, frames, self.order)

    def clear(self):
        for p in self.pipes:
            PO.fill_sentinels(p)
            p.reset_counters()

    def check(self, expect, runs, tag):
        torch.cuda.synchronize()
        for i, (p, o) in enumerate(zip(self.pipes, expect)):
            PO.check(self.dec, PO.snapshot(p), o, self.order, self.algo, runs, (tag, "pipe", i))

    def close(self):
        """The graph goes first, then the capture streams' workspaces (include/ldpc_osd.h, 'Captured graphs'): a later case
        may get the same streams from torch's pool."""
        torch.cuda.synchronize()
        self.graph = None
        for st in self.streams:
            self.dec.osd_release_stream(st)


def captured_rotation(dec, pipes, nbr, rpg, frames, order):
    """bench.py run_rank, the lines between ``side = torch.cuda.Stream()`` and ``graph = g`` (543-574): one side stream plus
    nbr - 1 branch streams; every capture stream's OSD workspace is sized and one eager rotation runs on the capture streams;
    then ``rpg`` rotations are captured, batch i on branch i mod nbr, between a fork from and a join into the side stream."""
    side = torch.cuda.Stream()
    branch = [side] + [torch.cuda.Stream() for _ in range(1, nbr)]

    def rotation(reps=1):
        for st in branch[1:]:
            st.wait_stream(side)                 # fork
        for _ in range(reps):
            for i, p in enumerate(pipes):
                with torch.cuda.stream(branch[i % nbr]):
                    p.run()
        for st in branch[1:]:
            side.wait_stream(st)                 # join

    with torch.cuda.stream(side):
        for st in branch:
            with torch.cuda.stream(st):
                if order is not None:
                    dec.osd_reserve_stream(frames, pipes[0]._p.osd)
        rotation()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        rotation(rpg)
    return g, branch


def run_case(dec, name, keep_front, nbr, rpg, nb=4, snr=SNR, frames=B, min_count=None):
    tag = (name, "front+search" if keep_front else "decode", nbr, rpg, nb, snr)
    c = Case(dec, name, keep_front, nbr, rpg, nb, snr, frames)
    try:
        for o in c.batches:
            if min_count is None:               # (tests/test_properties: 0.20 < FER < 0.31 at 2.5 dB)
                assert 0.20 * frames < len(o["idx"]) < 0.31 * frames, (tag, o["i"], len(o["idx"]))
            else:
                assert len(o["idx"]) > min_count, (tag, o["i"], len(o["idx"]), min_count)
        c.clear()
        c.graph.replay()
        c.check(c.batches, rpg, tag + ("one replay",))
        c.clear()
        for _ in range(3):                      # no synchronisation in between
            c.graph.replay()
        c.check(c.batches, 3 * rpg, tag + ("three replays",))
        # batches 0 and 2 change places in the input buffers: the replay follows the buffers' contents
        expect = list(c.batches)
        expect[0], expect[2] = expect[2], expect[0]
        for p, o in ((c.pipes[0], expect[0]), (c.pipes[2], expect[2])):
            p._y.copy_(o["y"])
            p._labels.copy_(o["labels"])
        c.clear()
        c.graph.replay()
        c.check(expect, rpg, tag + ("batches 0 and 2 exchanged",))
    finally:
        c.close()


ROUTES = [("nms10", True), ("nms10_osd0", True), ("nms10_osd2", True), ("nms10_osd2", False), ("nms10_fs2", True),
          ("nms10_fs2", False), ("nms10_pb3", True), ("nms10_pb3", False)]


@pytest.mark.parametrize("name,keep_front", ROUTES, ids=[f"{n}-{'front+search' if k else 'decode'}" for n, k in ROUTES])
def test_every_workload_and_route(dec, name, keep_front):
    run_case(dec, name, keep_front, nbr=4, rpg=2)


@pytest.mark.parametrize("nbr,rpg,nb", [(1, 1, 4), (2, 1, 4), (3, 2, 4), (4, 1, 4), (4, 8, 4), (4, 1, 5)],
                         ids=lambda v: str(v))
@pytest.mark.parametrize("name,keep_front", [("nms10_osd2", True), ("nms10_pb3", False)], ids=["osd2-front+search", "pb3-decode"])
def test_graph_shapes(dec, name, keep_front, nbr, rpg, nb):
    """From one chain to 4 branches x 8 rotations; with five batches branch 0 carries two of them in one rotation."""
    run_case(dec, name, keep_front, nbr, rpg, nb)


@pytest.mark.parametrize("keep_front", [True, False], ids=["front+search", "decode"])
def test_front_end_second_trip_beside_other_branches(dec, keep_front):
    grid = torch.cuda.get_device_properties(dec.device).multi_processor_count * 32        # front_grid(), csrc/ldpc_internal.h
    run_case(dec, "nms10_osd2", keep_front, nbr=4, rpg=2, snr=LOW_SNR, frames=LOW_B, min_count=grid)


def _flip(t, row):
    t[row:row + 1].view(torch.uint8).view(-1)[0] ^= 1


def test_the_checker_bites(dec):
    """Tampered copies of a passing case's outputs (PB-OSD front+search: the pipe has every buffer): one bit in each buffer
    in turn, in the last pipe -- in a listed row and, for the list buffers, in the last row, which still holds its sentinel --
    ``count`` off by one either way, and 1 added to each counter.  Only tensors are tampered with; no kernel runs again."""
    c = Case(dec, "nms10_pb3", True, nbr=4, rpg=2)
    try:
        c.clear()
        c.graph.replay()
        torch.cuda.synchronize()
        o = c.batches[-1]
        good = PO.snapshot(c.pipes[-1])
    finally:
        c.close()
    args = (o, c.order, c.algo, c.rpg)
    PO.check(dec, good, *args)
    assert set(good) == set(PO.NMS_OUT + ("count",) + PO.LIST_OUT + ("counters",))
    nf = len(o["idx"])
    tampered = []
    for name in PO.NMS_OUT + PO.LIST_OUT:
        for row in (nf // 2,) + ((B - 1,) if name in PO.LIST_OUT else ()):
            bad = dict(good, **{name: good[name].clone()})
            _flip(bad[name], row)
            tampered.append(((name, row), bad))
    for d in (-1, 1):
        tampered.append((("count", d), dict(good, count=good["count"] + d)))
    for k in range(8):
        cnt = good["counters"].clone()
        cnt[k] += 1
        tampered.append((("counters", k), dict(good, counters=cnt)))
    for what, bad in tampered:
        with pytest.raises(AssertionError):
            PO.check(dec, bad, *args)
            pytest.fail(f"the checker accepted a tampered {what}")
    PO.check(dec, good, *args)                  # the snapshot itself was never changed
