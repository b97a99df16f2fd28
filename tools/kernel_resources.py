#!/usr/bin/env python3
"""Per-kernel resources of two builds of the code object, side by side: was a refactor of the kernels' text a refactor of
their code?

    make -C gorder_amd/csrc asm          # in each tree: build/resource_usage.txt and build/*gfx950.s
    tools/kernel_resources.py BEFORE/build AFTER/build [family ...] > profiles/NAME.txt

For every kernel (keyed by mangled symbol): codeLenInByte, TotalNumSgprs, NumVgprs, NumAgprs, ScratchSize and LDSByteSize
from the `; Kernel info:` block of the .s, occupancy and the spill counts from the remarks, and a hash of the kernel's
instructions (labels renumbered).  The two tables of the named families (all kernels without names) are printed whole, then
their differences, then every kernel outside the families whose instructions changed.  Exit status 1 if a column that must
not change (VGPRs, AGPRs, scratch, VGPR spills, LDS, occupancy) did, or a kernel outside the families changed at all.
"""
import glob
import hashlib
import os
import re
import sys

COLUMNS = ("code", "sgpr", "vgpr", "agpr", "scratch", "lds", "occ", "sspill", "vspill", "hash")
MUST_MATCH = ("vgpr", "agpr", "scratch", "vspill", "lds", "occ")
INFO = {"codeLenInByte": "code", "TotalNumSgprs": "sgpr", "NumVgprs": "vgpr", "NumAgprs": "agpr", "ScratchSize": "scratch",
        "LDSByteSize": "lds"}
REMARK = {"Occupancy [waves/SIMD]": "occ", "SGPRs Spill": "sspill", "VGPRs Spill": "vspill"}


def body_hash(lines):
    """Hash of a function's instructions with its local labels renumbered in the order in which they first appear (their
    numbers follow the order in which the compiler made the blocks, which is not part of the code)."""
    seen = {}
    text = re.sub(r"\.L(?:BB|tmp|JTI)\d+_\d+", lambda m: seen.setdefault(m.group(0), f".L{len(seen)}"), "\n".join(lines))
    return hashlib.sha1(text.encode()).hexdigest()[:12]


def read_build(build):
    kernels, bodies = {}, {}
    (asm,) = glob.glob(os.path.join(build, "*gfx950.s"))
    name, body, in_info = None, None, False
    with open(asm) as f:
        for line in f:
            # a function's instructions end at the first of: the section of its kernel descriptor, the descriptor, .Lfunc_end
            if body and (line.startswith(".Lfunc_end") or re.match(r"\s*\.(section|amdhsa_kernel)\b", line)):
                bodies[body[0]] = body_hash(body[1])
                body = None
            m = re.match(r"\s*\.amdhsa_kernel (\S+)", line)
            if m:
                name = m.group(1)
                if name not in bodies:
                    sys.exit(f"{asm}: no instructions found for kernel {name}")
                kernels[name] = {"hash": bodies[name]}
                continue
            m = re.match(r"(_Z\w+|k_\w+):\s", line)
            if m:                                   # a function's entry label: its instructions follow
                body = (m.group(1), [])
                continue
            if body:
                text = line.split(";")[0].strip()
                if text:
                    body[1].append(text)
                continue
            if line.startswith("; Kernel info:"):
                in_info = True
                continue
            if in_info:
                m = re.match(r"; (\w+)\s*[:=]\s*(\d+)", line)
                if m and m.group(1) in INFO and name in kernels:
                    kernels[name][INFO[m.group(1)]] = int(m.group(2))
                if line.startswith("; COMPUTE_PGM") or not line.startswith(";"):
                    in_info = False
    name = None
    with open(os.path.join(build, "resource_usage.txt")) as f:
        for line in f:
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = m.group(1)
                continue
            m = re.search(r":\s+([A-Za-z /\[\]]+): (\d+) \[-Rpass-analysis", line)
            if m and m.group(1) in REMARK and name in kernels:
                kernels[name][REMARK[m.group(1)]] = int(m.group(2))
    return kernels


def family_of(symbol, families):
    m = re.match(r"_ZN\d+_GLOBAL__N_1(\d+)", symbol)
    if not m:
        return None
    start = m.end()
    base = symbol[start:start + int(m.group(1))]
    return base if base in families else None


def table(title, kernels, names):
    print(f"== {title}: {len(names)} kernels")
    print(" ".join(f"{c:>7}" for c in COLUMNS[:-1]) + "  " + f"{'hash':12}  symbol")
    for n in names:
        k = kernels[n]
        print(" ".join(f"{k.get(c, '-'):>7}" for c in COLUMNS[:-1]) + "  " + f"{k.get('hash', '-'):12}  {n}")
    print()


def main():
    before, after = read_build(sys.argv[1]), read_build(sys.argv[2])
    families = sys.argv[3:]
    if sorted(before) != sorted(after):
        print("the two builds do not hold the same kernels:", sorted(set(before) ^ set(after)))
        return 1
    inside = sorted(n for n in before if not families or family_of(n, families))
    outside = sorted(n for n in before if n not in inside)
    print(f"{len(before)} kernels in the code object, {len(inside)} of them in the families: {' '.join(families) or '(all)'}")
    print("columns: codeLenInByte, TotalNumSgprs, NumVgprs, NumAgprs, ScratchSize, LDSByteSize (static), occupancy, SGPR spills,"
          " VGPR spills, hash of the instructions\n")
    table("before", before, inside)
    table("after", after, inside)
    bad = 0
    print("== differences inside the families (before -> after)")
    n_same = 0
    for n in inside:
        diff = [c for c in COLUMNS if before[n].get(c) != after[n].get(c)]
        if not diff:
            n_same += 1
            continue
        bad += any(c in MUST_MATCH for c in diff)
        print("  " + ", ".join(f"{c} {before[n].get(c)} -> {after[n].get(c)}" for c in diff) + f"  {n}")
    print(f"  ({n_same} of {len(inside)} identical in every column, the instructions included)\n")
    print("== kernels outside the families whose instructions or resources changed")
    changed = [n for n in outside if before[n] != after[n]]
    for n in changed:
        print("  " + n)
    print(f"  ({len(outside) - len(changed)} of {len(outside)} identical)")
    return 1 if bad or changed else 0


if __name__ == "__main__":
    sys.exit(main())
