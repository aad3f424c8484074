"""Builds libldpcosd.so in-tree with hipcc for gfx950 (MI355X).  No GPU is needed to build.

    python -m short_ldpc_decoding_osd_amd.build [--force]
    python -m short_ldpc_decoding_osd_amd.build --asan [--run]

--asan: CPU sanitizer build ("race detection / sanitizers"): the library's HOST code (csrc/ldpc_host.cpp: alist
parser, G construction, GF(2) elimination, TEP tables, CRC-32C) and the C oracle under -fsanitize=address,undefined, as
libldpcosd_asan.so / oracle/_build/libldpc_oracle_asan.so; --run then runs the host-side test files against them
(LDPC_OSD_LIB / LDPC_ORACLE_LIB select the libraries, the sanitizer runtime is preloaded).  The host-side validation of
ldpc_osd_merge, ldpc_family_pipeline_run (csrc/ldpc_family_check.h) and ldpc_dlosd_pipeline_run (csrc/ldpc_dlosd_check.h) is part
of that library, and --run first runs a
stand-alone program on it (csrc/ldpc_sanitizer_main.cpp: contexts made by hand, no device, nothing preloaded).  Device code is never
sanitized: GPU AddressSanitizer runs are not available on this pool.
"""
from __future__ import annotations

import concurrent.futures
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(CSRC, "_obj")
LIB = os.path.join(HERE, "libldpcosd.so")
SOURCES = ["ldpc_host.cpp", "ldpc_api.hip", "ldpc_nms.hip", "ldpc_nms_train.hip", "ldpc_util.hip", "ldpc_osd.hip",
           "ldpc_osd_pb.hip", "ldpc_osdx.hip", "ldpc_osdw.hip", "ldpc_osdl.hip", "ldpc_osdl_fs.hip", "ldpc_osdl_pb.hip",
           "ldpc_hosd.hip", "ldpc_hosdl.hip", "ldpc_dia.hip", "ldpc_gen.hip"]
# -ffp-contract=off: the float order of the NMS / OSD metric is part of the contract (no FMA fusion)
# -fno-slp-vectorize: packed v_pk_add_f32 is no faster than two v_add_f32 on gfx950 and blocks the
#                      fusion of the DPP rotations into their consumers
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
         "-fno-slp-vectorize", "-Wall", "-Wno-unused-function"]


def _hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    raise RuntimeError("hipcc not found")


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    os.makedirs(OBJ, exist_ok=True)
    hipcc = _hipcc()
    headers = [os.path.join(CSRC, h) for h in sorted(os.listdir(CSRC)) if h.endswith(".h")]      # every header: a new one cannot be forgotten
    headers.append(os.path.join(HERE, "..", "include", "ldpc_osd.h"))
    jobs = []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(OBJ, os.path.splitext(src)[0] + ".o")
        if force or _stale(o, [s] + headers):
            jobs.append([hipcc, "-x", "hip", "-c", s, "-o", o] + FLAGS)

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode:
            raise RuntimeError("hipcc failed:\n" + " ".join(cmd) + "\n" + p.stdout + p.stderr)
        return p.stderr

    with concurrent.futures.ThreadPoolExecutor(max_workers=4) as ex:
        for warn in ex.map(run, jobs):
            if warn and verbose:
                print(warn)
    objs = [os.path.join(OBJ, os.path.splitext(s)[0] + ".o") for s in SOURCES]
    if force or jobs or _stale(LIB, objs):
        run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs)
    return LIB


ASAN_LIB = os.path.join(HERE, "libldpcosd_asan.so")
ASAN_MAIN = os.path.join(OBJ, "ldpc_sanitizer_main")
ASAN_TESTS = ["tests/test_cabi.py", "tests/test_hosd_host.py", "tests/test_tfrecord.py", "tests/test_weights.py", "tests/test_oracle_golden.py"]


def build_asan(verbose=False):
    """Host-only sanitizer build of the library and the oracle; returns (library, oracle library, sanitizer runtime)."""
    root = os.path.dirname(HERE)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
    cmd = ["g++", "-std=c++17", "-fPIC", "-shared", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"] + san + [
        os.path.join(CSRC, "ldpc_host.cpp"), os.path.join(CSRC, "ldpc_sanitizer_stubs.cpp"), os.path.join(CSRC, "ldpc_sanitizer_checks.cpp"),
        "-o", ASAN_LIB, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"]
    # the stand-alone driver of the validation in ldpc_sanitizer_checks.cpp, linked against that library
    os.makedirs(OBJ, exist_ok=True)
    cmd_main = ["g++", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"] + san + [
        os.path.join(CSRC, "ldpc_sanitizer_main.cpp"), ASAN_LIB, "-o", ASAN_MAIN, "-Wl,-rpath," + HERE, "-Wl,-rpath,/opt/rocm/lib"]
    oracle_so = os.path.join(root, "oracle", "_build", "libldpc_oracle_asan.so")
    os.makedirs(os.path.dirname(oracle_so), exist_ok=True)
    cmd2 = ["gcc", "-std=c11", "-fPIC", "-shared", "-Wall", "-Wextra", "-ffp-contract=off", "-fno-fast-math"] + san + [
        os.path.join(root, "oracle", "ldpc_oracle.c"), "-o", oracle_so, "-lm"]
    for c in (cmd, cmd2, cmd_main):
        if verbose:
            print(" ".join(c), flush=True)
        p = subprocess.run(c, capture_output=True, text=True)
        if p.returncode:
            raise RuntimeError("sanitizer build failed:\n" + " ".join(c) + "\n" + p.stdout + p.stderr)
    rt = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    return ASAN_LIB, oracle_so, rt


def run_asan_tests(extra=()):
    """pytest over the host-side test files with the sanitized libraries; returns the subprocess result."""
    lib, oracle_so, rt = build_asan()
    root = os.path.dirname(HERE)
    alone = subprocess.run([ASAN_MAIN], cwd=root, capture_output=True, text=True,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    if alone.returncode:
        return alone
    env = dict(os.environ, LDPC_OSD_LIB=lib, LDPC_ORACLE_LIB=oracle_so, LD_PRELOAD=rt,
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    return subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "not gpu", "-p", "no:cacheprovider"] + ASAN_TESTS + list(extra),
                          cwd=root, env=env, capture_output=True, text=True)


if __name__ == "__main__":
    if "--asan" in sys.argv:
        print(build_asan(verbose=True))
        if "--run" in sys.argv:
            r = run_asan_tests()
            print(r.stdout[-3000:], r.stderr[-3000:])
            sys.exit(r.returncode)
    else:
        print(build(force="--force" in sys.argv, verbose=True))
