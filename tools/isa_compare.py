"""Do two builds of libmijpeg.so hold the same machine code for the kernels both have?

    python tools/isa_compare.py OLD/libmijpeg.so NEW/libmijpeg.so [--kernels REGEX] [--appended Lb0E] [--mask-pcrel]

Disassembles the gfx950 code objects of both libraries (llvm-objdump, addresses and encodings left out, comments stripped) and
compares, kernel by kernel, the instruction lists.  --appended: the mangled spelling of template arguments the NEW build has
behind the OLD ones (a flavour added as a defaulted last template parameter: `Lb0E` is `false`), so that the old name finds its
new twin.  --mask-pcrel: the literal of the s_add_u32 behind an s_getpc_b64 -- the distance from the kernel to a constant table in
.rodata, which moves whenever the code object gains or loses a kernel -- is left out of the comparison.  Prints one line per kernel and the totals; exit status 1 when something differs.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_isa_guard import OBJDUMP, gfx950_code_objects  # noqa: E402


def kernels(path, mask_pcrel=False):
    out = {}
    for co in gfx950_code_objects(path):
        with tempfile.NamedTemporaryFile(suffix=".co", delete=False) as f:
            f.write(co)
        asm = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "--no-leading-addr", f.name], capture_output=True, text=True, check=True).stdout
        os.unlink(f.name)
        cur = None
        for ln in asm.splitlines():
            m = re.match(r"^[0-9a-f]* ?<(\S+)>:", ln)
            if m:
                cur = out.setdefault(m.group(1), [])
            elif cur is not None and ln.strip():
                ins = re.sub(r"//.*", "", ln).strip()
                if ins == "...":  # (llvm-objdump's mark for zero padding between two symbols: layout, not an instruction)
                    continue
                if mask_pcrel and cur and cur[-1].startswith("s_getpc_b64") and ins.startswith("s_add_u32"):
                    ins = re.sub(r"0x[0-9a-f]+$", "<pc-relative>", ins)
                cur.append(ins)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--kernels", default=r"fused(420p|420|422|444|1)_kernel")
    ap.add_argument("--appended", default="")
    ap.add_argument("--mask-pcrel", action="store_true")
    args = ap.parse_args()
    a, b = kernels(args.old, args.mask_pcrel), kernels(args.new, args.mask_pcrel)
    same = different = missing = 0
    for name in sorted(a):
        if not re.search(args.kernels, name):
            continue
        twin = re.sub(r"(I(?:L[bi]\d+E)+)(EEv)", lambda m: m.group(1) + args.appended + m.group(2), name, count=1) if args.appended else name
        if twin not in b:
            missing += 1
            print(f"missing    {name}")
        elif a[name] == b[twin]:
            same += 1
            print(f"identical  {len(a[name]):6d} instructions  {name}")
        else:
            different += 1
            print(f"DIFFERENT  {len(a[name]):6d} / {len(b[twin]):6d} instructions  {name}")
    print(f"identical {same}, different {different}, missing {missing}")
    return 1 if different or missing else 0


if __name__ == "__main__":
    sys.exit(main())
