#!/usr/bin/env python3
"""asm_load_waits.py [listing.s ...] — a census of global loads that are waited for as soon as they are issued.

A load costs its latency once per WAIT, not once per load: a kernel that issues twenty loads and then waits pays one round trip, one
that waits behind each pays twenty.  hipcc puts a load that sits under a condition of its own (a bounds test, a range test) into a
basic block of its own and retires it there, so the source's "eight loads in flight" can compile to eight dependent round trips
(sg_k4.h's gather met the same).  This tool makes that visible without a GPU.

Without arguments it compiles the kernel translation unit to gfx950 assembly as tools/check_asm_loads.py does (about 100 s); with
arguments it reads listings made by

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -o X.s alaz_amd/csrc/servicegraph.hip

Per kernel: the global loads (global_load_*; atomics and LDS-DMA are none) and how many of them are DRAINED AT ONCE: followed, within
two instructions, by an s_waitcnt whose vmcnt is 0 — nothing else was issued behind it that the wait could overlap with.  Labels,
directives and comments are no instructions.  Kernels without a drained load are left out unless --all is given; --kernel SUBSTR
keeps the kernels whose (mangled or demangled) name contains SUBSTR.

events(text) is the parsed form the tests use: {kernel: [("load", mnemonic) | ("wait", n) | ("label", name), ...]} in program order,
waits being the s_waitcnt that name vmcnt, n their count."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "alaz_amd", "csrc", "servicegraph.hip")
NEAR = 2                                   # a wait this many instructions behind the load, or nearer, drains it "at once"


def compile_listing(out, src=SRC):
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                           "-Wno-unused-value", "-Wno-unused-command-line-argument", "-o", out, src], stderr=subprocess.DEVNULL)
    return out


def instructions(text):
    """{kernel: [instruction or 'label:' lines]} — what lies between a kernel's label and its s_endpgm / .amdhsa_kernel block"""
    out, name = {}, None
    for raw in text.split("\n"):
        line = raw.split(";")[0].strip()
        if not line:
            continue
        m = re.match(r"^([A-Za-z_]\w*):$", line)
        if m and not line.startswith(".L"):
            name = m.group(1)
            if name.startswith("__hip_cuid_"):
                name = None
            else:
                out[name] = []
            continue
        if name is None:
            continue
        if line.startswith(".amdhsa_kernel") or line.startswith(".section") or line.startswith(".rodata"):
            name = None
            continue
        if re.match(r"^\.LBB\d+_\d+:$", line):
            out[name].append(line)
        elif not line.startswith("."):
            out[name].append(line)
    return {k: v for k, v in out.items() if any(i.startswith("s_endpgm") for i in v)}


def is_load(ins):
    return ins.startswith("global_load_") and not ins.startswith("global_load_lds")


def vmcnt(ins):
    """the vmcnt of an s_waitcnt, None when it names none"""
    if not ins.startswith("s_waitcnt"):
        return None
    m = re.search(r"vmcnt\((\d+)\)", ins)
    return int(m.group(1)) if m else None


def events(text):
    ev = {}
    for k, body in instructions(text).items():
        e = []
        for ins in body:
            if ins.endswith(":"):
                e.append(("label", ins[:-1]))
            elif is_load(ins):
                e.append(("load", ins.split()[0]))
            elif vmcnt(ins) is not None:
                e.append(("wait", vmcnt(ins)))
        ev[k] = e
    return ev


def census(text):
    """{kernel: (loads, drained at once)}"""
    out = {}
    for k, body in instructions(text).items():
        ins = [i for i in body if not i.endswith(":")]
        loads = [n for n, i in enumerate(ins) if is_load(i)]
        drained = sum(1 for n in loads if any(vmcnt(j) == 0 for j in ins[n + 1:n + 1 + NEAR]))
        out[k] = (len(loads), drained)
    return out


def demangle(names):
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not filt:
        return {n: n for n in names}
    try:
        r = subprocess.run([filt], input="\n".join(names) + "\n", capture_output=True, text=True, timeout=60)
        got = r.stdout.splitlines()
        if r.returncode == 0 and len(got) == len(names):
            return {n: re.sub(r"\(.*$", "", g) for n, g in zip(names, got)}
    except (OSError, subprocess.SubprocessError):
        pass
    return {n: n for n in names}


def table(text, show_all=False, only=None):
    c = census(text)
    nice = demangle(sorted(c))
    rows = [(nice[k], k, n, d) for k, (n, d) in c.items() if (show_all or d) and (not only or only in k or only in nice[k])]
    rows.sort(key=lambda r: (-r[3], -r[2], r[0]))
    w = max([len(r[0]) for r in rows] + [6])
    lines = [f"{'kernel':<{w}}  loads  drained at once"] + [f"{r[0]:<{w}}  {r[2]:>5}  {r[3]:>5}" for r in rows]
    lines.append(f"{len(c)} kernels, {sum(n for n, _ in c.values())} global loads, {sum(d for _, d in c.values())} drained at once")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("listings", nargs="*")
    ap.add_argument("--all", action="store_true", help="also the kernels without a drained load")
    ap.add_argument("--kernel", help="only kernels whose name contains this")
    a = ap.parse_args()
    if a.listings:
        for p in a.listings:
            print(f"# {os.path.basename(p)}")
            print(table(open(p).read(), a.all, a.kernel))
    else:
        with tempfile.TemporaryDirectory() as td:
            print(table(open(compile_listing(os.path.join(td, "sg.s"))).read(), a.all, a.kernel))
    return 0


if __name__ == "__main__":
    sys.exit(main())
