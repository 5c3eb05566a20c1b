#!/usr/bin/env python3
"""Do two builds of the library carry the same machine code?  Per kernel, from the code objects themselves.

    python tools/isa_diff.py OLD/libmgx.so NEW/libmgx.so [--filter SUBSTR ...] [--show]

Disassembles every gfx950 code object of both libraries (`llvm-objdump -d --no-show-raw-insn`, as tests/test_kernel_budget.py
does), splits the listing by kernel symbol and compares the instruction streams.  Addresses, the `<symbol+offset>` the disassembler
prints behind a branch target, every comment and the padding behind a kernel's last instruction are dropped first: they move with
everything else in the object.  One line per kernel -- `same` with the instruction count, or `DIFFERENT` with both counts (--show: the unified diff) --
and exit status 1 if any kernel differs or exists on one side only.  A refactor that must not touch the kernels says so with this.
"""
from __future__ import annotations

import difflib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as kr  # noqa: E402

SYM = re.compile(r"^[0-9a-f]+ <(.+)>:$")


def demangle(names: list[str]) -> list[str]:
    for tool in (os.path.join(kr.LLVM_BIN, "llvm-cxxfilt"), "c++filt"):
        try:
            res = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
        except OSError:
            continue
        if len(res) == len(names):
            return res
    return names


def streams(lib: str) -> dict[str, list[str]]:
    """{demangled kernel or function symbol: its normalised instructions}"""
    out: dict[str, list[str]] = {}
    for elf in kr.code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".elf") as fh:
            fh.write(elf)
            fh.flush()
            txt = subprocess.check_output([os.path.join(kr.LLVM_BIN, "llvm-objdump"), "-d", "--no-show-raw-insn", fh.name], text=True)
        cur = None
        for line in txt.splitlines():
            m = SYM.match(line.strip())
            if m:
                cur = out.setdefault(m.group(1), [])
                continue
            if cur is None or not line.strip() or line.startswith("Disassembly"):
                continue
            ins = line.split("//")[0]                                # (the comment holds the address)
            ins = re.sub(r"<[^>]*>", "", ins)                        # (branch targets by symbol + offset)
            ins = " ".join(ins.split())
            if ins:
                cur.append(ins)
    for ins in out.values():                                         # (the padding up to the next symbol is not the kernel's)
        while ins and ins[-1] != "s_endpgm" and (ins[-1] == "..." or ins[-1].startswith(("s_nop", "s_code_end"))):
            ins.pop()
    names = list(out)
    return dict(zip(demangle(names), (out[n] for n in names)))


def main() -> int:
    argv = sys.argv[1:]
    show = "--show" in argv
    flt = [argv[i + 1] for i, a in enumerate(argv) if a == "--filter"]
    libs = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] != "--filter")]
    old, new = streams(libs[0]), streams(libs[1])
    bad = 0
    for name in sorted(set(old) | set(new)):
        if flt and not any(f in name for f in flt):
            continue
        short = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        if name not in old or name not in new:
            print(f"ONLY IN {'OLD' if name in old else 'NEW'}  {short}")
            bad += 1
        elif old[name] == new[name]:
            print(f"same       {len(new[name]):6d} instructions  {short}")
        else:
            print(f"DIFFERENT  {len(old[name]):6d} -> {len(new[name]):6d} instructions  {short}")
            bad += 1
            if show:
                print("\n".join(difflib.unified_diff(old[name], new[name], "old", "new", lineterm="", n=2)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
