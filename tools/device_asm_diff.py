#!/usr/bin/env python3
"""Device-assembly equality of two source trees: the check of a host-only change to ofasys_amd/csrc.

    tools/device_asm_diff.py <tree A> <tree B> [file.hip ...]     # e.g. a `git worktree` of the parent commit, and `.`

Compiles every file of the Makefile's SRCS (and DBG_SRCS again with -DOFA_DEBUG_SWITCHES) in both trees to device assembly
(--cuda-device-only -S, the Makefile's flags), replaces the translation-unit hash __hip_cuid_<hex> by a fixed token and compares the
texts for equality -- it inspects no instruction.  Prints one line per file and exits non-zero on any difference.  CPU only."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor


def make_vars(tree):
    text = open(os.path.join(tree, "ofasys_amd/csrc/Makefile")).read()
    var = lambda name: re.search(r"^%s\s*\??=\s*(.*)$" % name, text, re.M).group(1)
    flags = var("CXXFLAGS").replace("$(ARCH)", var("ARCH")).split()
    return os.environ.get("HIPCC", var("HIPCC")), flags, var("SRCS").split(), [s + ".hip" for s in var("DBG_SRCS").split()]


def device_asm(job):
    tree, src, extra, out = job
    hipcc, flags, _, _ = make_vars(tree)
    subprocess.run([hipcc, *flags, *extra, "--cuda-device-only", "-S", src, "-o", out], cwd=os.path.join(tree, "ofasys_amd/csrc"), check=True)
    return re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", open(out).read())


def chunks(asm):
    """{symbol: text} per global symbol, plus the code-object metadata as a sorted list of its per-kernel entries"""
    code, _, meta = asm.partition(".amdgpu_metadata")
    parts = re.split(r"^\s*\.globl\s+(\S+).*\n", code, flags=re.M)
    by_sym = dict(zip(parts[1::2], parts[2::2]))
    by_sym[".head"] = parts[0]
    by_sym[".metadata"] = sorted(re.split(r"^  - (?=\.agpr_count|\.args)", meta, flags=re.M))
    return by_sym


def verdict(a, b):
    if a == b:
        return "identical"
    ca, cb = chunks(a), chunks(b)
    if ca == cb:
        return "DIFFERENT: every kernel symbol identical, only their emission order differs"
    sym = next((s for s in ca if ca[s] != cb.get(s)), None) or next(s for s in cb if s not in ca)
    return "DIFFERENT: first differing kernel symbol %s" % sym


def main():
    tree_a, tree_b = (os.path.abspath(t) for t in sys.argv[1:3])
    _, _, srcs, dbg = make_vars(tree_b)
    variants = [(s, []) for s in srcs] + [(s, ["-DOFA_DEBUG_SWITCHES"]) for s in dbg]
    variants = [v for v in variants if not sys.argv[3:] or v[0] in sys.argv[3:]]      # optional: only the named sources
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
        jobs = [(t, s, x, os.path.join(tmp, "%d_%d.s" % (i, k))) for i, (s, x) in enumerate(variants) for k, t in enumerate((tree_a, tree_b))]
        asm = list(pool.map(device_asm, jobs))
    results = [verdict(asm[2 * i], asm[2 * i + 1]) for i in range(len(variants))]
    for (s, x), r in zip(variants, results):
        print("%-44s %s" % (" ".join([s] + x), r))
    bad = sum(r != "identical" for r in results)
    print("%d of %d device assemblies differ" % (bad, len(results)) if bad else "all %d device assemblies identical" % len(results))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
