#!/usr/bin/env python3
"""Are the kernels of two source trees the same code?  Compiles the named .hip files of both trees to gfx950 assembly with the
build's flags (`hipcc --cuda-device-only -S`, plus `-Rpass-analysis=kernel-resource-usage`), and compares every function of the
first tree with the function of the same demangled name in the second, instruction by instruction: labels are renumbered
per function, mangled names are masked (a kernel that became a template instantiation has another mangled name and lands in a
COMDAT section of its own; an empty template argument list `<>` is dropped from the name), comments are dropped.  No GPU.

    git worktree add /tmp/parent HEAD~1
    python scripts/compare_kernel_asm.py /tmp/parent . ldpc_hosd.hip ldpc_hosdl.hip ldpc_dia.hip [--resources]

Prints one line per function of the first tree -- IDENTICAL, or DIFFERS with both instruction counts, or MISSING -- and the
functions only the second tree has; with --resources also VGPRs / LDS bytes / scratch bytes of every kernel of both trees.
Exit status 1 if a function differs or is missing."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from short_ldpc_decoding_osd_amd import build as B  # noqa: E402


def compile_asm(tree, name, out):
    src = os.path.join(tree, "short_ldpc_decoding_osd_amd", "csrc", name)
    flags = [f for f in B.FLAGS if f != "-Wall"]
    r = subprocess.run([B._hipcc(), "-x", "hip", "--cuda-device-only", "-S", src, "-o", out, "-Rpass-analysis=kernel-resource-usage"] + flags,
                       capture_output=True, text=True)
    if r.returncode:
        raise SystemExit(f"hipcc failed on {src}:\n{r.stderr[-3000:]}")
    return r.stderr


def functions(path):
    """mangled name -> the instruction lines of the function, normalised."""
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        s = line.split(";")[0].rstrip()
        if not s.strip() or s.lstrip().startswith(".section") or s.strip() == ".text":
            continue                                           # (where the function is placed is not its code)
        s = re.sub(r"\.LBB\d+_", ".LBB_", s)
        body.append(re.sub(r"_Z\w+", "SYM", s))
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return {n: re.sub(r"^void ", "", d).split("(")[0].replace("<>", "") for n, d in zip(names, r)}


def resources(remarks):
    out, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
        for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("first")
    ap.add_argument("second")
    ap.add_argument("files", nargs="+")
    ap.add_argument("--resources", action="store_true")
    a = ap.parse_args()
    bad = 0
    with tempfile.TemporaryDirectory() as d:
        for name in a.files:
            asm = [os.path.join(d, f"{i}_{name}.s") for i in (1, 2)]
            rem = [compile_asm(tree, name, out) for tree, out in zip((a.first, a.second), asm)]
            f1, f2 = functions(asm[0]), functions(asm[1])
            d1, d2 = demangle(list(f1)), demangle(list(f2))
            by_name = {}
            for k, v in d2.items():
                by_name.setdefault(v, []).append(k)
            for k, v in d1.items():
                cands = by_name.get(v, [])
                if any(f2[c] == f1[k] for c in cands):
                    verdict = "IDENTICAL"
                elif cands:
                    verdict, bad = f"DIFFERS (second: {[len(f2[c]) for c in cands]} instructions)", bad + 1
                else:
                    verdict, bad = "MISSING in the second tree", bad + 1
                print(f"{name}: {v:60s} {len(f1[k]):6d} instructions  {verdict}")
            for v in sorted(set(d2.values()) - set(d1.values())):
                print(f"{name}: {v:60s} only in the second tree")
            if a.resources:
                for tag, r, dm in (("first", resources(rem[0]), d1), ("second", resources(rem[1]), d2)):
                    for k, v in r.items():
                        if k in dm:
                            print(f"{name}: {tag:6s} {dm[k]:60s} VGPRs {v.get('vgprs')}  LDS {v.get('lds')}  scratch {v.get('scratch')}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
