"""-m gpu: decode calls on different streams of ONE context from SEVERAL host threads (include/ldpc_osd.h, ldpc_ctx_create:
"from one host thread or several ... for every algorithm").  Four threads, each with its own stream and its own
BatchPipeline through ldpc_osd_decode (keep_front=False: the front end goes into the stream's workspace) on a distinct
batch of its own size.  A barrier precedes the first call of every thread, so that the workspaces are created under the
context's mutex at the same moment; eight runs per thread follow without further barriers.  Every pipe's outputs and
counters are exact against the C oracle (tests/pipeline_oracle.py).  ldpc_last_error is thread-local: a refused call in one
thread leaves its message there and nowhere else.

Wall time on one MI355X: 5 s for the file's 5 cases; the slowest case takes 1.6 s
(test_four_host_threads_one_context[conventional], which computes the NMS oracle of the four batches)."""
import threading

import pytest
import torch

from tests import abi_calls as A
from tests import pipeline_oracle as PO

pytestmark = pytest.mark.gpu
SNR, THREADS, RUNS = 2.5, 4, 8
CONV, FS, PB = ("nms10_osd2", "nms10_fs2", "nms10_pb3")
CASES = {"conventional": (CONV,) * 4, "fs": (FS,) * 4, "pb": (PB,) * 4, "mixed": (CONV, FS, PB, PB)}


@pytest.fixture(scope="module")
def dec():
    from short_ldpc_decoding_osd_amd import Code
    from short_ldpc_decoding_osd_amd.runtime import Decoder
    return Decoder(Code())


def frames_of(t):
    return 6000 - 500 * t          # workspaces of different sizes


def run_threads(dec, names, refuse_in=None):
    """Thread t decodes batch t RUNS times with workload names[t]; returns the messages ldpc_last_error gave in each thread:
    after every successful run, and (thread ``refuse_in``) after a refused ldpc_compact between its runs."""
    from short_ldpc_decoding_osd_amd.pipeline import BatchPipeline
    specs = [PO.workload(n) for n in names]
    batches = [PO.batch(dec, SNR, frames_of(t), t) for t in range(THREADS)]
    pipes = []
    for (order, algo), o in zip(specs, batches):
        PO.prepare(dec, [o], order, algo, front=False)
        pipes.append(BatchPipeline(dec, o["B"], PO.T, PO.ALPHA, osd_order=order, osd_algo=algo, snr_db=SNR,
                                   keep_front=False).bind(o["y"].clone(), o["labels"].clone()))
    for p in pipes:
        PO.fill_sentinels(p)
        p.reset_counters()
    torch.cuda.synchronize()
    barrier = threading.Barrier(THREADS)
    errors, after_ok, after_refused = [], [[] for _ in pipes], []

    def work(t):
        try:
            torch.cuda.set_device(dec.device)
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                barrier.wait(timeout=120)
                for _ in range(RUNS):
                    pipes[t].run()
                    after_ok[t].append(dec.L.ldpc_last_error().decode())
                    if t == refuse_in:
                        rc = dec.L.ldpc_compact(dec._ctx, None, -1, None, None, dec._stream())
                        after_refused.append((rc, dec.L.ldpc_last_error().decode()))
            st.synchronize()
        except BaseException as exc:   # noqa: BLE001
            barrier.abort()
            errors.append((t, exc))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(THREADS)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    if errors:                     # (the cause first: the other threads only saw the barrier break)
        raise sorted(errors, key=lambda te: isinstance(te[1], threading.BrokenBarrierError))[0][1]
    torch.cuda.synchronize()
    for t, (p, o) in enumerate(zip(pipes, batches)):
        PO.check(dec, PO.snapshot(p), o, *specs[t], RUNS, (names[t], "thread", t))
    return after_ok, after_refused


@pytest.mark.parametrize("case", list(CASES))
def test_four_host_threads_one_context(dec, case):
    run_threads(dec, CASES[case])


def test_last_error_is_thread_local(dec):
    after_ok, after_refused = run_threads(dec, CASES["mixed"], refuse_in=1)
    assert len(after_refused) == RUNS
    for rc, msg in after_refused:
        assert rc == A.E_ARG and "ldpc_compact" in msg, (rc, msg)
    for t, msgs in enumerate(after_ok):
        assert len(msgs) == RUNS
        if t != 1:
            assert not any("ldpc_compact" in m for m in msgs), (t, msgs)
