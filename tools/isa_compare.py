#!/usr/bin/env python3
"""Kernel-by-kernel comparison of the gfx950 code of two builds of libpveenv.so: which kernels have the same instruction stream,
which differ, which exist in one build only.  Branch targets and PC-relative constants are masked (they move when other code
moves); everything else must match instruction for instruction.  Used to show that a change leaves existing kernels untouched.
  python tools/isa_compare.py OLD.so NEW.so [--show KERNEL_SUBSTRING]"""
import argparse
import difflib
import os
import re
import subprocess
import tempfile

LLVM = "/opt/rocm/llvm/bin"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
MASKED = ("s_branch", "s_cbranch", "s_getpc", "s_add_u32", "s_addc_u32")


def disassemble(lib, tmp):
    base = os.path.join(tmp, os.path.basename(lib))
    subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, base + ".fatbin"])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=" + TARGET,
                           "--input=" + base + ".fatbin", "--output=" + base + ".co", "--unbundle"])
    return subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", base + ".co"],
                          stdout=subprocess.PIPE, text=True, check=True).stdout


def kernels(text):
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None:
            continue
        ins = re.sub(r"//.*$", "", re.sub(r"^\s*[0-9a-f]+:\s*", "", line)).strip()
        if not ins or ins == "...":              # (padding between functions)
            continue
        ins = re.sub(r"<[^>]*>", "<L>", ins)
        if ins.startswith(MASKED):
            ins = re.sub(r"0x[0-9a-f]+|\b\d+\b", "X", ins)
        out[cur].append(ins)
    return out


def demangle(names):
    res = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True).stdout.split("\n")
    return dict(zip(names, (re.sub(r"\(.*", "", n) for n in res)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--show", default=None, help="print the instruction diff of the kernels whose name contains this")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        ko, kn = kernels(disassemble(a.old, tmp)), kernels(disassemble(a.new, tmp))
    dm = demangle(sorted(set(ko) | set(kn)))
    # kernels are paired by their demangled name without the parameter list: a change of a parameter TYPE (another mangled
    # symbol for the same template instantiation) is not a removed and a new kernel
    ko, kn = {dm[k]: v for k, v in ko.items()}, {dm[k]: v for k, v in kn.items()}
    dm = {k: k for k in set(ko) | set(kn)}
    same = [k for k in ko if k in kn and ko[k] == kn[k]]
    diff = [k for k in ko if k in kn and ko[k] != kn[k]]
    for k in diff:
        print("DIFFERENT  %-70s %6d -> %6d instructions" % (dm[k][:70], len(ko[k]), len(kn[k])))
        if a.show and a.show in dm[k]:
            print("\n".join(difflib.unified_diff(ko[k], kn[k], lineterm="", n=1)))
    for k in ko:
        if k not in kn:
            print("REMOVED    %s" % dm[k])
    for k in kn:
        if k not in ko:
            print("NEW        %s" % dm[k])
    print("%d kernels of the old build: %d identical, %d different, %d removed; %d new" %
          (len(ko), len(same), len(diff), sum(k not in kn for k in ko), sum(k not in ko for k in kn)))
