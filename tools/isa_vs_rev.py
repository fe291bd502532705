#!/usr/bin/env python3
"""Which kernels of a translation unit of csrc/ moved, and by how much?  A REPORT, not a gate: what holds a change of shared kernel text to the
parent is the bits (parity tests), the resources (tools/kru.sh) and the time on the GPU ("One text per step"); a kernel listed here with
a count that moved by much more than half a percent is more than scheduling, and the two listings are to be read.  Compiles csrc/FILE.hip (default:
riesz.hip) of a git revision (default: HEAD~1), against that revision's headers, and of the working tree to gfx950 assembly with the flags of the
Makefile's rule for that file, and compares the instruction streams kernel by kernel, labels and symbol names stripped.  riesz.hip only: the kernels
the revision has are compared with their mask-0 instantiations here (k_rz_split -> k_rz_split<TK_FMA>, k_rz_phase<E> -> k_rz_phase<E, false, false>,
...; the instantiations without the portable functions of LVM_RZ_PORTABLE_TRIG -- last template argument false -- stand for the kernels of a
revision from before that argument).  Needs hipcc, no GPU.
usage: tools/isa_vs_rev.py [FILE.hip] [REV]; exit status 1 when a kernel differs or is missing."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC_REL = "live-video-magnification_amd/csrc"
CSRC = os.path.join(ROOT, *CSRC_REL.split("/"))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt", "--cuda-device-only", "-S"]
NOSLP = ("laplace.hip", "riesz.hip")          # the Makefile's NOSLP_<file> = -fno-slp-vectorize


def kernels(asm):
    out = {}
    for m in re.finditer(r"^(_ZN3lvm\w+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:", open(asm).read(), re.S | re.M):
        body = []
        for line in m.group(2).split("\n"):
            line = line.split(";")[0].strip()
            if line and not line.startswith(".") and not line.endswith(":"):
                body.append(re.sub(r"_ZN3lvm\w+", "SYM", re.sub(r"\.LBB\d+_\d+", "L", line)))
        out[m.group(1)] = body
    names = list(out)
    plain = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.strip().split("\n")
    return {re.sub(r"^void ", "", p.replace("(anonymous namespace)::", "").split("(")[0]): out[n] for n, p in zip(names, plain)}


def portable_off(name):
    """the name an instantiation without the portable functions (LVM_RZ_PORTABLE_TRIG: the last template argument, false) had before that argument existed"""
    name = re.sub(r"(k_rz_phase4?)<(\w+), (\w+), (\w+), false>", r"\1<\2, \3, \4>", name)
    return re.sub(r"(k_rz_blur_\w+)<(\w+), (\w+), false>", r"\1<\2, \3>", name)


def default_name(name):
    """the name a mask-0 instantiation of the working tree had before the kinds became template arguments"""
    name = name.replace("k_rz_split<0>", "k_rz_split")
    name = portable_off(name)
    name = re.sub(r"(k_rz_phase4?)<(\w+), false, false>", r"\1<\2>", name)
    name = re.sub(r"(k_rz_blur_\w+)<(\w+), false>", r"\1<\2>", name)
    name = re.sub(r"k_rz_collapse<(\w+), 0>", r"k_rz_collapse<\1>", name)
    return re.sub(r"(k_rz_final<.*), false>$", r"\1>", name)


def main():
    args = sys.argv[1:]
    src = args.pop(0) if args and args[0].endswith(".hip") else "riesz.hip"
    rev = args[0] if args else "HEAD~1"
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = FLAGS + (["-fno-slp-vectorize"] if src in NOSLP else [])
    with tempfile.TemporaryDirectory() as tmp:
        # the revision's translation unit with every header of its csrc/ and the public header beside it (an #include "..." looks there first)
        listed = subprocess.run(["git", "-C", ROOT, "ls-tree", "--name-only", rev, CSRC_REL + "/"], capture_output=True, text=True, check=True).stdout.split()
        for rel in [r for r in listed if r.endswith(".h")] + [CSRC_REL + "/" + src, "include/lvm_hip.h"]:
            with open(os.path.join(tmp, os.path.basename(rel)), "wb") as f:
                f.write(subprocess.run(["git", "-C", ROOT, "show", "%s:%s" % (rev, rel)], capture_output=True, check=True).stdout)
        subprocess.check_call([hipcc] + flags + ["-I" + tmp, "-o", os.path.join(tmp, "rev.s"), os.path.join(tmp, src)])
        subprocess.check_call([hipcc] + flags + ["-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o", os.path.join(tmp, "tree.s"), os.path.join(CSRC, src)])
        old, new = kernels(os.path.join(tmp, "rev.s")), kernels(os.path.join(tmp, "tree.s"))
    if src == "riesz.hip":
        # (a revision that already has the kinds as template arguments: the names as they are, or without the portable-functions argument)
        new = {**{default_name(k): v for k, v in new.items()}, **{portable_off(k): v for k, v in new.items()}, **new}
    if src == "laplace.hip":
        # (a revision from before the block walk was always 2 x 2: k_lap_up_rows<2, D, HC> there is k_lap_up_rows<D, HC> here)
        new = {**{k.replace("k_lap_up_rows<", "k_lap_up_rows<2, "): v for k, v in new.items()}, **new}
    bad = [k for k in old if old[k] != new.get(k)]
    for k in bad:
        print("%s: %s" % ("MISSING" if k not in new else "DIFFERS (%d -> %d instructions)" % (len(old[k]), len(new[k])), k))
    print("%s: %d of %d kernels of %s have identical instruction streams in the working tree (%d kernels there)" % (src, len(old) - len(bad), len(old), rev, len(new)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
