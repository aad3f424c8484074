"""CPU: what the family pipeline adds outside the device -- sharding.sweep_point(width=12) and combine_fer on 12 counters under
gloo (world_size 2, one rank with an empty shard: its zero tensor must have the width of the others' counters), and the
layout of ldpc_family_pipeline in the header against the binding's ctypes mirror, compiled with the host compiler."""
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
PER_BATCH = [0, 3, 40, 1, 2, 2, 1, 90, 2, 1, 9, 25]      # counters of one macro-batch; [0] is the batch's frame count


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
def test_sweep_point_carries_twelve_counters(total, stop_errors):
    """total = 1: rank 1 owns no frame and contributes twelve zeros; total = 70, 35 per rank in batches of 10: four
    macro-batches, or as many as reach the stop rule, which reads the first eight counters: 1 undetected + 1 OSD failure per
    batch and rank."""
    (_, ran0, red0), (_, ran1, red1) = _run(total, 10, stop_errors, 12)
    assert ran0 == ran1 and red0 == red1 and len(red0) == 12
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


def test_default_width_is_unchanged():
    (_, ran0, red0), (_, _, red1) = _run(1, 10, 0, 8)
    assert red0 == red1 == [1] + PER_BATCH[1:8] and ran0 == 1


def test_combine_fer_on_twelve_counters():
    from short_ldpc_decoding_osd_amd.sharding import combine_fer
    c8 = [1000, 120, 900, 4, 110, 110, 30, 220000]
    c12 = c8 + [110, 30, 260, 700]
    old, new = combine_fer(c8), combine_fer(c12, n=96)
    assert {k: new[k] for k in old} == old                                   # the eight mean what they meant
    assert set(new) - set(old) == {"bit_err_end_to_end", "ber_nms", "ber_end_to_end"}
    assert new["bit_err_end_to_end"] == 900 - 700 + 260
    assert new["ber_nms"] == 900 / (1000 * 96) and new["ber_end_to_end"] == 460 / (1000 * 96)
    assert "ber_nms" not in combine_fer(c12) and combine_fer(c12)["bit_err_end_to_end"] == 460
    assert "bit_err_end_to_end" not in combine_fer(c8, n=96)


LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "ldpc_osd.h"
#define M(name) printf("%s %zu\n", #name, offsetof(ldpc_family_pipeline, name));
int main(void)
{
    printf("sizeof %zu\n", sizeof(ldpc_family_pipeline));
    printf("families %d %d %d %d\n", LDPC_OSD_FAMILY_AUTO, LDPC_OSD_FAMILY_X, LDPC_OSD_FAMILY_W, LDPC_OSD_FAMILY_L);
    MEMBERS
    return 0;
}
"""


def test_header_and_binding_agree_on_the_family_pipeline(tmp_path):
    from short_ldpc_decoding_osd_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ldpc_osd.h")).read()
    body = re.search(r"typedef struct ldpc_family_pipeline \{(.*?)\} ldpc_family_pipeline;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"[\s\*]", "", n) for decl in body.split(";") if decl.strip() for n in decl.strip().split(" ", 1)[1].split(",")]
    names = [n.split(" ")[-1] for n in names]
    # (declarations such as `const float *d_llr` and `int32_t *d_best, *d_ntep`: the last word of each declarator)
    names = [re.sub(r"^(const|float|uint64_t|uint8_t|int64_t|int32_t|void|ldpc_osd_params)+", "", n) for n in names]
    assert names == [f for f, _ in _lib.FamilyPipeline._fields_]
    assert _lib.OSD_FAMILIES == {"osdx": 1, "osdw": 2, "osdl": 3} and _lib.OSD_FAMILY_AUTO == 0
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a C compiler builds the oracle, so one is there"
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C.replace("MEMBERS", "\n    ".join(f"M({n})" for n in names)))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    lines = dict(line.split(" ", 1) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(lines.pop("sizeof")) == C.sizeof(_lib.FamilyPipeline)
    assert lines.pop("families") == "0 1 2 3"
    assert {k: int(v) for k, v in lines.items()} == {f: getattr(_lib.FamilyPipeline, f).offset for f, _ in _lib.FamilyPipeline._fields_}
