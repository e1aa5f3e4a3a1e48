#!/usr/bin/env python
"""Compare the gfx950 kernels of two builds, kernel by kernel:
    python tools/kernel_diff.py [--match SUBSTRING ...] OLD NEW
OLD and NEW are two assembly files (`hipcc --cuda-device-only -S`) or two built libraries (their code objects are
disassembled with llvm-objdump; addresses the linker resolved relative to the program counter are masked).  Every kernel
is reduced to its instruction text (comments, directives, labels of the assembler's bookkeeping and blank lines dropped)
and reported as SAME or DIFF with the instruction counts of both sides;
kernels that only one side has are reported as ONLY-OLD / ONLY-NEW.  Exit status 1 when anything differs.  This is a text
comparison: it tells whether a refactor left a kernel alone, not what the difference means."""
import glob
import os
import re
import subprocess
import sys
import tempfile
from typing import Dict, List

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")


def _demangle(names: List[str]) -> List[str]:
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return [re.sub(r"^void ", "", re.sub(r"\(.*", "", n)) for n in out[:len(names)]]


def kernels_of_asm(text: str) -> Dict[str, List[str]]:
    """Kernel name -> instruction lines of an assembly file: a function runs from its label to `.Lfunc_end`."""
    out, name, body = {}, None, []
    for line in text.split("\n"):
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and not m.group(1).startswith(".L"):
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name], name = body, None
            continue
        code = line.split(";")[0].strip()
        if code and not code.startswith("."):      # directives; local labels (`.LBB0_1:`) go with them, branches keep their targets
            body.append(re.sub(r"\s+", " ", code))
    return out


def kernels_of_library(path: str) -> Dict[str, List[str]]:
    """Kernel name -> instruction lines of the gfx950 code objects bundled in a library."""
    out: Dict[str, List[str]] = {}
    with tempfile.TemporaryDirectory() as tmp:
        link = os.path.join(tmp, os.path.basename(path))
        os.symlink(os.path.abspath(path), link)
        subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", link], cwd=tmp, capture_output=True)
        for co in sorted(glob.glob(os.path.join(tmp, "*gfx950*"))):
            dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], capture_output=True, text=True).stdout
            name = None
            for line in dis.split("\n"):
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    name = m.group(1)
                    out.setdefault(name, [])
                    continue
                code = re.sub(r"\s+", " ", line.split("//")[0].strip())
                if not name or not code or code == "..." or code.startswith("Disassembly"):     # ("...": alignment padding)
                    continue
                # an address the linker resolved relative to the program counter moves with everything linked around the kernel
                if out[name] and out[name][-1].startswith("s_getpc_b64") and code.startswith("s_add_u32"):
                    code = re.sub(r"0x[0-9a-f]+$", "<pc-relative>", code)
                out[name].append(code)
    return out


def kernels_of(path: str) -> Dict[str, List[str]]:
    with open(path, "rb") as f:
        is_elf = f.read(4) == b"\x7fELF"
    raw = kernels_of_library(path) if is_elf else kernels_of_asm(open(path).read())
    names = list(raw)
    return {d: raw[n] for n, d in zip(names, _demangle(names))}


def main() -> int:
    args, match = sys.argv[1:], []
    while "--match" in args:
        i = args.index("--match")
        match.append(args[i + 1])
        del args[i:i + 2]
    if len(args) != 2:
        raise SystemExit(__doc__)
    old, new = kernels_of(args[0]), kernels_of(args[1])
    differs = False
    for name in sorted(set(old) | set(new)):
        if match and not any(k in name for k in match):
            continue
        if name not in new or name not in old:
            verdict, differs = ("ONLY-OLD" if name in old else "ONLY-NEW"), True
        else:
            verdict = "SAME" if old[name] == new[name] else "DIFF"
            differs |= verdict == "DIFF"
        print(f"{verdict:8s} {len(old.get(name, [])):6d} {len(new.get(name, [])):6d}  {name}")
    return 1 if differs else 0


if __name__ == "__main__":
    sys.exit(main())
