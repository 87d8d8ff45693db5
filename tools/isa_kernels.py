#!/usr/bin/env python3
"""Per-kernel comparison of two device assembly files, for a refactor that renames or reorders the kernels of one file (tools/isa_equal.sh
compares whole files, so it reports such a file as different even when every kernel's code is the same).

    KEEP=/tmp/asm tools/isa_equal.sh <rev>                                   # keeps <rev>'s and the tree's assembly under /tmp/asm/{old,new}
    tools/isa_kernels.py /tmp/asm/old/attention.s /tmp/asm/new/attention.s

Each file is split at its kernel symbols (the code up to .Lfunc_end, then the kernel descriptor and resource comments up to the next
section).  What is normalised before two kernels are compared: the kernel's own mangled name, the per-function number in local labels
(.LBB12_3), comments, the per-compile __hip_cuid symbol.  A kernel of the new file is "identical" when some kernel of the old file has the same
normalised text (its name is printed, so a renamed instantiation shows up as a pair); every other kernel is listed with the register,
scratch and LDS figures of its descriptor in both files.  Exit status 1 if any kernel has no identical partner."""
import hashlib
import re
import shutil
import subprocess
import sys

FIGURES = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "private_segment_fixed_size", "group_segment_fixed_size")


def kernels(path):
    lines = open(path).read().split("\n")
    out, i = {}, 0
    while i < len(lines):
        m = re.match(r"\s*\.globl\s+(\S+)", lines[i])
        if m and any(re.match(r"\s*\.type\s+" + re.escape(m.group(1)) + ",@function", ln) for ln in lines[i:i + 4]):
            j = i
            while not re.match(r"\.Lfunc_end\d+:", lines[j]):
                j += 1
            while j < len(lines) and not re.match(r"\s*(\.section\s+\.text|\.amdgpu_metadata|\.section\s+\.AMDGPU\.gpr|\.type\s+__hip_cuid)", lines[j]):
                j += 1
            out[m.group(1)] = lines[i:j]
            i = j - 1
        i += 1
    return out


def normalised(name, body):
    t = "\n".join(body).replace(name, "KERNEL")
    t = re.sub(r"\.LBB\d+_", ".LBB_", t)
    t = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", t)
    t = re.sub(r"__hip_cuid_[0-9a-fX]+", "__hip_cuid_X", t)
    return re.sub(r"\s*;.*", "", t)


def figures(body):
    f = {}
    for ln in body:
        m = re.match(r"\s*\.amdhsa_(\w+)\s+(\S+)", ln)
        if m and m.group(1) in FIGURES:
            f[m.group(1)] = m.group(2)
    return " ".join(f"{k}={f.get(k, '?')}" for k in FIGURES)


def demangled(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {n: o.replace("(anonymous namespace)::", "") for n, o in zip(names, out)}


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    names = demangled(list(old) + list(new))
    by_text = {}
    for n, b in old.items():
        by_text.setdefault(hashlib.sha1(normalised(n, b).encode()).hexdigest(), []).append(n)
    matched, differing = set(), 0
    for n, b in new.items():
        partners = by_text.get(hashlib.sha1(normalised(n, b).encode()).hexdigest())
        if partners:
            partner = n if n in partners else partners[0]      # the kernel of the same name (same template arguments) where it is one of them
            matched.add(partner)
            print(f"identical  {names[n]}  ==  {names[partner]}")
        else:
            differing += 1
            print(f"DIFFERS    {names[n]}\n           new: {figures(b)}")
    for n, b in old.items():
        if n not in matched:
            print(f"unmatched  {names[n]} (old)\n           old: {figures(b)}")
    same_name = sum(1 for n in new if n in matched)
    print(f"# {len(new) - differing} of {len(new)} kernels identical to a kernel of {sys.argv[1]} ({same_name} to the one of the same name); "
          f"{len(old) - len(matched)} of its {len(old)} kernels have no partner")
    sys.exit(1 if differing else 0)


if __name__ == "__main__":
    main()
