#!/usr/bin/env python3
"""Compare the gfx950 assembly of .hip files between two source trees, as text.

  tools/compare_device_asm.py OLD_TREE NEW_TREE [file.hip ...] [--jobs N] [--keep DIR]

Each tree is a checkout of this repository.  Every named file of accelerating-genomics_amd/csrc (default: the ten banded
translation units, agx_sw_band*_kernel.hip) is compiled in both trees with the HIPFLAGS of that tree's Makefile plus
`--cuda-device-only -S`, which needs no GPU.  The two outputs are compared line for line after the `__hip_cuid_*` symbol lines are
dropped (they hash the source text).  Prints one markdown table row per file -- lines, differing lines -- and the first few
differing lines of a file that differs; exits 1 if any file differs.
"""
import argparse
import concurrent.futures
import difflib
import glob
import os
import re
import subprocess
import sys
import tempfile

PKG = "accelerating-genomics_amd"


def hipflags(tree):
    """HIPCC and HIPFLAGS as the tree's Makefile sets them, $(ARCH) and $(INC) expanded"""
    text = open(os.path.join(tree, PKG, "Makefile")).read()
    var = {k: v.strip() for k, v in re.findall(r"^(\w+)\s*[:?]?=\s*(.*)$", text, re.M)}
    flags = var["HIPFLAGS"].replace("$(ARCH)", var["ARCH"]).replace("$(INC)", os.path.join(tree, "include"))
    return os.environ.get("HIPCC", var["HIPCC"]), flags.split()


def assembly(tree, name, out):
    hipcc, flags = hipflags(tree)
    cmd = [hipcc] + flags + ["--cuda-device-only", "-S", os.path.join(tree, PKG, "csrc", name), "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode:
        sys.exit("%s\n%s" % (" ".join(cmd), r.stdout))
    return [l for l in open(out).read().splitlines() if "__hip_cuid_" not in l]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("files", nargs="*")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--keep", help="leave the .s files in this directory")
    a = ap.parse_args()
    old, new = os.path.abspath(a.old), os.path.abspath(a.new)
    files = a.files or sorted(os.path.basename(p) for p in glob.glob(os.path.join(new, PKG, "csrc", "agx_sw_band*_kernel.hip")))
    tmp = a.keep or tempfile.mkdtemp(prefix="device_asm_")
    os.makedirs(tmp, exist_ok=True)
    with concurrent.futures.ThreadPoolExecutor(a.jobs) as pool:
        jobs = {(f, side): pool.submit(assembly, tree, f, os.path.join(tmp, "%s.%s.s" % (f, side)))
                for f in files for side, tree in (("old", old), ("new", new))}
    print("| file | lines old | lines new | differing lines |")
    print("|---|---|---|---|")
    differ = 0
    for f in files:
        x, y = jobs[(f, "old")].result(), jobs[(f, "new")].result()
        delta = [l for l in difflib.unified_diff(x, y, "old/" + f, "new/" + f, lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---")]
        print("| `%s` | %d | %d | %d |" % (f, len(x), len(y), len(delta)))
        if delta:
            differ += 1
            print("\n".join("    " + l for l in delta[:20]), file=sys.stderr)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
