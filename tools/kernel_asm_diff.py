#!/usr/bin/env python3
"""kernel_asm_diff.py A.s B.s — compare two gfx950 assembly listings of the kernel translation unit, kernel by kernel.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -o A.s alaz_amd/csrc/servicegraph.hip

Per kernel: `identical`, `reordered` (the same instructions in another order) or `different`, with both instruction counts and
next_free_vgpr / next_free_sgpr / private_segment_fixed_size of the .amdhsa block.  Comment lines, the numbers of local labels and
the __hip_cuid_* symbol are ignored.  Exit status 1 when a kernel exists on one side only."""
import re
import sys
from collections import Counter

RES = ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size")


def kernels(path):
    """{name: (instructions, resources)} — the lines between a kernel's label and its .amdhsa_kernel block, and that block's fields"""
    out, name, body, res, in_res = {}, None, [], {}, False
    for raw in open(path):
        line = raw.split(";")[0].strip()
        if not line or "__hip_cuid_" in line:
            continue
        m = re.match(r"^([A-Za-z_]\w*):$", line)
        if m and not in_res:
            name, body, res = m.group(1), [], {}
        elif line.startswith(".amdhsa_kernel "):
            in_res = True
        elif line == ".end_amdhsa_kernel":
            if name: out[name] = (body, res)
            name, in_res = None, False
        elif in_res:
            f = line.split()
            if f[0][len(".amdhsa_"):] in RES: res[f[0][len(".amdhsa_"):]] = f[1]
        elif name and not line.startswith("."):
            body.append(re.sub(r"\.LBB\d+_\d+", ".LBB", line))
        elif name and re.match(r"^\.LBB\d+_\d+:$", line):
            body.append(".LBB:")
    return out


def main(a_path, b_path):
    a, b = kernels(a_path), kernels(b_path)
    tally = Counter()
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print(f"{'only in ' + (a_path if name in a else b_path):<10}  {name}"); tally["one side only"] += 1
            continue
        (ia, ra), (ib, rb) = a[name], b[name]
        verdict = "identical" if ia == ib else "reordered" if Counter(ia) == Counter(ib) else "different"
        tally[verdict] += 1
        if verdict != "identical" or ra != rb:
            na, nb = (sum(1 for x in i if x != ".LBB:") for i in (ia, ib))
            print(f"{verdict:<10} insns {na} -> {nb}  " + "  ".join(f"{k} {ra.get(k)} -> {rb.get(k)}" for k in RES) + f"  {name}")
    print(f"{len(a)} / {len(b)} kernels: " + ", ".join(f"{n} {v}" for v, n in sorted(tally.items())))
    return 1 if tally["one side only"] else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
