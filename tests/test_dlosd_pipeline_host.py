"""CPU: what the DL-OSD pipeline adds outside the device -- sharding.sweep_point(width=15) and combine_fer on 15 counters under
gloo (world_size 2, one rank with an empty shard), the unchanged meaning of widths 8 and 12, the layout of ldpc_dlosd_pipeline
in the header against the binding's ctypes mirror, compiled with the host compiler, and the refusals of
ldpc_dlosd_pipeline_run in the stand-alone sanitizer program (its own main, nothing preloaded)."""
import ctypes as C
import os
import re
import shutil
import socket
import subprocess
import sys

import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# counters of one macro-batch ([0] is the batch's frame count): 5 NMS, 6 stage, 4 merge
PER_BATCH = [0, 3, 40, 1, 2, 2, 1, 1, 9, 700, 850, 2, 1, 9, 25]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, total, batch, stop_errors, width, out):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from short_ldpc_decoding_osd_amd.sharding import shard_range, sweep_point
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    lo, hi = shard_range(total, rank, world)

    def decode_batch(B):
        return torch.tensor([B] + PER_BATCH[1:width], dtype=torch.int64)

    max_batches = -(-shard_range(total, 0, world)[1] // batch)
    try:
        red, ran = sweep_point(decode_batch, hi - lo, batch, max_batches, stop_errors, with_osd=True, device=torch.device("cpu"),
                               width=width)
        out.put((rank, ran, red.tolist()))
    except Exception as exc:                                # (reported, not raised: the parent asserts on it)
        out.put((rank, -1, repr(exc)))
    dist.barrier()
    dist.destroy_process_group()


def _run(total, batch, stop_errors, width):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, total, batch, stop_errors, width, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return got


@pytest.mark.parametrize("total,stop_errors", [(1, 0), (1, 1), (70, 0), (70, 5)])
def test_sweep_point_carries_fifteen_counters(total, stop_errors):
    """total = 1: rank 1 owns no frame and contributes fifteen zeros; total = 70, 35 per rank in batches of 10: four
    macro-batches, or as many as reach the stop rule, which at width 15 reads undetected [3] + merged wrong [12]: 1 + 1 per
    batch and rank (the stage's own failure counter [7] and the width-8 position [6] hold 1 as well, the frames through the
    stage [5] hold 2: a rule that read another position would still stop here, so [6] is told apart below)."""
    (_, ran0, red0), (_, ran1, red1) = _run(total, 10, stop_errors, 15)
    assert ran0 == ran1 and red0 == red1 and len(red0) == 15
    if total == 1:
        calls = 1
        assert ran0 == 1 and red0[0] == 1
    elif stop_errors:
        calls = 4                                             # 2 ranks x 2 errors per macro-batch: 4, then 8 >= 5
        assert ran0 == 2 and red0[0] == 40
    else:
        calls = 8
        assert ran0 == 4 and red0[0] == 70
    assert red0[1:] == [calls * v for v in PER_BATCH[1:]]


def test_stop_rule_positions():
    from short_ldpc_decoding_osd_amd.sharding import end_to_end_errors
    c15 = list(range(100, 115))
    assert end_to_end_errors(c15, True) == c15[3] + c15[12] and end_to_end_errors(c15, False) == c15[1]
    assert end_to_end_errors(c15[:12], True) == c15[3] + c15[6] == end_to_end_errors(c15[:8], True)


@pytest.mark.parametrize("width", [8, 12])
def test_other_widths_are_unchanged(width):
    (_, ran0, red0), (_, _, red1) = _run(1, 10, 0, width)
    assert red0 == red1 == [1] + PER_BATCH[1:width] and ran0 == 1
    from short_ldpc_decoding_osd_amd.sharding import combine_fer
    c8 = [1000, 120, 900, 4, 110, 110, 30, 220000]
    c12 = c8 + [110, 30, 260, 700]
    r8, r12 = combine_fer(c8), combine_fer(c12, n=96)
    assert r8 == {"frames": 1000, "fer_nms": 0.12, "synd_fail_rate": 0.11, "undetected": 4, "fer_osd_given_fail": 30 / 110,
                  "fer_product": 0.11 * (30 / 110), "fer_end_to_end": 34 / 1000, "mean_teps": 2000.0}
    assert r12 == dict(r8, bit_err_end_to_end=460, ber_nms=900 / 96000, ber_end_to_end=460 / 96000)


def test_combine_fer_on_fifteen_counters():
    from short_ldpc_decoding_osd_amd.sharding import combine_fer
    #      frames ferr  berr und synd | staged S   F  windows complexity teps | merged wrong after before
    c15 = [1000, 120, 900, 4, 110, 110, 85, 25, 330, 55000, 66000, 110, 24, 260, 700]
    r = combine_fer(c15, n=96)
    assert r == {"frames": 1000, "fer_nms": 0.12, "synd_fail_rate": 0.11, "undetected": 4, "stage_frames": 110, "left_out": 0,
                 "fer_dl_given_fail": 25 / 110, "mean_windows": 3.0, "mean_complexity": 500.0, "mean_teps": 600.0,
                 "fer_end_to_end": 28 / 1000, "bit_err_end_to_end": 900 - 700 + 260, "ber_nms": 900 / 96000,
                 "ber_end_to_end": 460 / 96000}
    assert "ber_nms" not in combine_fer(c15) and combine_fer(c15)["bit_err_end_to_end"] == 460
    # a capacity below the failures, and a point without failures
    assert combine_fer(c15[:5] + [100] + c15[6:])["left_out"] == 10
    quiet = combine_fer([1000, 0, 0, 0, 0] + [0] * 10, n=96)
    assert quiet["fer_end_to_end"] == 0.0 and quiet["ber_end_to_end"] == 0.0 and "mean_windows" not in quiet


LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "ldpc_osd.h"
#define M(name) printf("%s %zu\n", #name, offsetof(ldpc_dlosd_pipeline, name));
int main(void)
{
    printf("sizeof %zu\n", sizeof(ldpc_dlosd_pipeline));
    printf("families %d %d %d %d %d\n", LDPC_HOSD_FAMILY_AUTO, LDPC_HOSD_FAMILY_128, LDPC_HOSD_FAMILY_X, LDPC_HOSD_FAMILY_W,
           LDPC_HOSD_FAMILY_L);
    MEMBERS
    return 0;
}
"""
TYPES = r"^(const|float|double|uint64_t|uint8_t|int64_t|int32_t|void)+"


def test_header_and_binding_agree_on_the_dlosd_pipeline(tmp_path):
    from short_ldpc_decoding_osd_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ldpc_osd.h")).read()
    body = re.search(r"typedef struct ldpc_dlosd_pipeline \{(.*?)\} ldpc_dlosd_pipeline;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"[\s\*]", "", n) for decl in body.split(";") if decl.strip() for n in decl.strip().split(" ", 1)[1].split(",")]
    # (declarations such as `const float *d_llr` and `int32_t *d_best, *d_teps_evaluated`: the last word of each declarator)
    names = [re.sub(TYPES, "", n) for n in names]
    assert names == [f for f, _ in _lib.DlOsdPipeline._fields_]
    assert _lib.HOSD_FAMILIES == {"hosd": 1, "hosdx": 2, "hosdw": 3, "hosdl": 4} and _lib.HOSD_FAMILY_AUTO == 0
    assert "ldpc_dlosd_pipeline_run" in _lib.SYMBOLS
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler builds the oracle, so one is there"
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C.replace("MEMBERS", "\n    ".join(f"M({n})" for n in names)))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    lines = dict(line.split(" ", 1) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(lines.pop("sizeof")) == C.sizeof(_lib.DlOsdPipeline)
    assert lines.pop("families") == "0 1 2 3 4"
    assert {k: int(v) for k, v in lines.items()} == {f: getattr(_lib.DlOsdPipeline, f).offset for f, _ in _lib.DlOsdPipeline._fields_}


def test_refusals_in_the_sanitizer_program():
    """The stand-alone program of the sanitizer build (contexts made by hand, no device, nothing preloaded) runs the validation
    of ldpc_dlosd_pipeline_run -- every refusal, its text and the family each code resolves to -- under
    -fsanitize=address,undefined and exits 0 when every expectation holds."""
    from short_ldpc_decoding_osd_amd import build
    src = open(os.path.join(build.CSRC, "ldpc_sanitizer_main.cpp")).read()
    assert src.count("expect(ldpc_dlosd_pipeline_run(") >= 25     # the checks are there to pass
    build.build_asan()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([build.ASAN_MAIN], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0 and "ok: 0 failure(s)" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
