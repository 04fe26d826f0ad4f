#!/usr/bin/env python3
"""asm_diff.py OLD.s NEW.s: two gfx950 assembly listings of kernels.hip (hipcc --cuda-device-only -S), compared per kernel symbol.

Prints, for every kernel, whether the instruction streams are identical after label renaming, the instruction-count delta, and
any difference in the resource figures of its .amdhsa_kernel block (registers, LDS, scratch, accum_offset).  Exit status 1 if
the symbol sets differ.  For refactors that must not change the device code.
"""
import re
import subprocess
import sys

FIGURES = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size", "accum_offset")


def parse(path):
    kernels, figures, cur, body = {}, {}, None, []
    label = re.compile(r"\.?L[A-Za-z_]*\d+(_\d+)?")
    for line in open(path):
        t = line.split(";")[0].strip()
        m = re.match(r"\.amdhsa_kernel (\S+)", t)
        if m:
            desc = m.group(1)
            figures[desc] = {}
            continue
        m = re.match(r"\.amdhsa_(\w+) (\S+)", t)
        if m and m.group(1) in FIGURES:
            figures[desc][m.group(1)] = m.group(2)
            continue
        m = re.match(r"(_Z\w+):$", t)
        if m:
            cur, body = m.group(1), []
            kernels[cur] = body
            continue
        if cur is None or not t:
            continue
        if t.startswith(".Lfunc_end"):
            cur = None
            continue
        if t.startswith(".") and not t.endswith(":"):
            continue  # directives
        body.append(label.sub("L", t))
    return {k: v for k, v in kernels.items() if k in figures}, figures


def main():
    old, fo = parse(sys.argv[1])
    new, fn = parse(sys.argv[2])
    if set(old) != set(new):
        print("symbol sets differ:", sorted(set(old) ^ set(new)))
        return 1
    names = subprocess.run(["c++filt"], input="\n".join(sorted(old)), capture_output=True, text=True).stdout.split("\n")
    same = 0
    for sym, name in zip(sorted(old), names):
        count = lambda b: sum(1 for t in b if not t.endswith(":"))
        ident = old[sym] == new[sym]
        same += ident
        figs = [f"{k} {fo[sym].get(k)} -> {fn[sym].get(k)}" for k in FIGURES if fo[sym].get(k) != fn[sym].get(k)]
        name = re.sub(r"^void mij::|\(.*$", "", name)
        print(f"{'identical' if ident else 'differs  '} {count(new[sym]) - count(old[sym]):+5d} of {count(old[sym]):6d}  {name}" + ("  " + "; ".join(figs) if figs else ""))
    print(f"{same} of {len(old)} kernels identical")
    return 0


if __name__ == "__main__":
    sys.exit(main())
